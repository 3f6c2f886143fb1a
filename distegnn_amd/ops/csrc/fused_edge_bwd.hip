// Fused backward of the FastEGNN edge block (gfx950).
//
// Recomputes the forward chain tile-by-tile (checkpoint style) and emits
// every per-edge gradient in ONE kernel. See fused_edge.hip for the chain;
// the python side finishes with three split-K wgrad GEMMs and CSR segment
// sums (ops/__init__.py _FusedEdgeBlockFn.backward); the bias column sums
// are taken here. Two modes: per edge (EB_PLAIN) stores ein and
// dh_row / dh_col; the default, EB_LIN below, leaves dh and the h-columns of
// dW1 to per-node sums of dz1 and emits none of the three.
//
// Occupancy design (PMC-driven, same as the forward): weights are read
// from GLOBAL padded/transposed copies (L2-resident) instead of LDS, and
// activation/derivative tiles are consolidated into PRE-ACTIVATION tiles
// (silu / silu' computed on the fly) that are overwritten in place by the
// dz chain: LDS drops from 158 KB (1 block/CU, 65% SQ_WAIT_ANY) to
// ~53 KB, and the dein product is split into 3 register passes to stay
// under the 2-waves/SIMD VGPR budget.
//
//   dp   = dtrans . cdu            dcdu = p * dtrans
//   dz3  = (dp w3v) silu'(z3)      dw3v += sum dp s3
//   dz2  = (dmsg_n[row] + dz3 W3) silu'(z2)
//   dz1  = (dz2 W2) silu'(z1)
//   dein = dz1 W1 -> dh_i, dh_j, dr2
//   dcd  = (normalize ? dcdu/(|d|+eps) : dcdu) + 2 d dr2

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

namespace {

constexpr int EA = 2;
constexpr int TILE = 64;
constexpr int THREADS = 256;

// per-H derived dimensions (H=64 reproduces the tuned round-1 constants:
// K_IN 131, K_PAD 160, K_STRIDE 168, K_OUT 144, H_STRIDE 72)
template <int H>
struct EDB {
  static constexpr int K_IN = 2 * H + 1 + EA;
  static constexpr int K_PAD = (K_IN + 31) / 32 * 32;
  static constexpr int K_STRIDE = K_PAD + 8;
  static constexpr int K_OUT = (K_IN + 15) / 16 * 16;  // ein cols (dW1 GEMM)
  static constexpr int H_STRIDE = H + 8;
  static constexpr int NT = H / 16;
  static constexpr int HP = H / 8;
  static constexpr int NTK = K_OUT / 16;               // dein n-tiles
};

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float silu_(float x) {
  return x / (1.f + __expf(-x));
}
__device__ __forceinline__ float dsilu_(float x) {
  float s = 1.f / (1.f + __expf(-x));
  return s * (1.f + x * (1.f - s));
}

template <int H>
struct Smem {
  int in_tile;  // [TILE][K_STRIDE] bf16  (ein, later dein)
  int z1;       // [TILE][H_STRIDE] bf16  (pre-act; overwritten by dz1)
  int z2;       // (overwritten by dz2)
  int z3;       // (overwritten by dz3)
  int diff;     // [TILE][4] f32
  int scal;     // [TILE][4] f32 (p, dp/dr2, -, -)
  int bias;     // [4*H] f32
  int wpart;    // [H] f32
  int gbacc;    // [3*H] f32 (block-local gb1/gb2/gb3 column sums)
  int rows;     // [TILE] i32 (edge row indices, staged once per tile)
  int cols;     // [TILE] i32
  int total;
};

template <int H>
__host__ __device__ constexpr Smem<H> smem_layout() {
  Smem<H> L{};
  int o = 0;
  L.in_tile = o; o += TILE * EDB<H>::K_STRIDE * 2;
  L.z1 = o; o += TILE * EDB<H>::H_STRIDE * 2;
  L.z2 = o; o += TILE * EDB<H>::H_STRIDE * 2;
  L.z3 = o; o += TILE * EDB<H>::H_STRIDE * 2;
  L.diff = o; o += TILE * 4 * 4;
  L.scal = o; o += TILE * 4 * 4;
  L.bias = o; o += 4 * H * 4;
  L.wpart = o; o += H * 4;
  L.gbacc = o; o += 3 * H * 4;
  L.rows = o; o += TILE * 4;
  L.cols = o; o += TILE * 4;
  L.total = o;
  return L;
}

__device__ __forceinline__ bf16x8 lds8(const char* smem, int off) {
  return *reinterpret_cast<const bf16x8*>(smem + off);
}
__device__ __forceinline__ bf16x8 g8(const bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
// Launder a pointer so the compiler cannot hoist its loads across phases:
// without this, LICM pre-loads EVERY phase's weight fragments into
// registers across the tile loop (measured 256 VGPR + 170 AGPR -> 1
// wave/SIMD).
__device__ __forceinline__ const bf16* opaque(const bf16* p) {
  asm volatile("" : "+v"(p));
  return p;
}
// read 8 bf16 pre-activations from LDS and apply silu -> bf16x8
__device__ __forceinline__ bf16x8 lds8_silu(const char* smem, int off) {
  bf16x8 z = lds8(smem, off);
  bf16x8 r;
#pragma unroll
  for (int u = 0; u < 8; ++u) r[u] = (__bf16)silu_((float)z[u]);
  return r;
}

// A from LDS (optionally through silu), B from global [64][wk] k-contig.
template <int KSTEPS, bool SILU_A, int NT>
__device__ __forceinline__ void mm_g(const char* smem, int a_off,
                                     int a_stride,
                                     const bf16* __restrict__ w, int wk,
                                     int lane, f32x4 (&acc)[NT]) {
__builtin_amdgcn_s_setprio(1);
  #pragma unroll
  for (int kk = 0; kk < KSTEPS; ++kk) {
    int k = kk * 32 + (lane >> 4) * 8;
    bf16x8 a = SILU_A ? lds8_silu(smem, a_off + (lane & 15) * a_stride + k * 2)
                      : lds8(smem, a_off + (lane & 15) * a_stride + k * 2);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bf16x8 b = g8(w + (nt * 16 + (lane & 15)) * wk + k);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
    }
  }
  __builtin_amdgcn_s_setprio(0);
}

// EB_LIN: the first layer is linear in ein and ein is a gather of node
// rows, so dh and the h-columns of dW1 follow from per-node sums of dz1
// (S_row, S_col; see docs/KERNELS.md). This mode stores neither ein nor
// dh_row/dh_col and computes only the dein n-tile that holds column 2H
// (dr2, which dcd needs). The three dW1 columns that are per-edge (r2 and
// the two edge attributes) are formed here, in the column loop that sums
// gb1: dz1 times the bf16 values in columns 2H..2H+2 of in_tile, summed
// over a wave's 16 rows in a fixed order and stored as one partial row per
// (tile, wave). The host folds the partial rows with a deterministic sum,
// so dW1 is bit-identical run to run (no atomics on a weight gradient).
enum EdgeBwdMode { EB_PLAIN = 0, EB_LIN = 1 };

template <int H, int MODE>
__global__ __launch_bounds__(THREADS,
                             (MODE == EB_LIN && H == 32) ? 4
                             : (H <= 64 ? 3 : 1))
void fused_edge_bwd(
    const bf16* __restrict__ h, const float* __restrict__ coord,
    const float* __restrict__ eattr, const long* __restrict__ row,
    const long* __restrict__ col,
    const bf16* __restrict__ dmsg_n,     // [N,64]
    const float* __restrict__ dtrans_n,  // [N,3]
    const bf16* __restrict__ w1p,   // [64][K_PAD]
    const bf16* __restrict__ w1tp,  // [K_OUT][64] (W1^T rows padded)
    const bf16* __restrict__ w2, const bf16* __restrict__ w2t,
    const bf16* __restrict__ w3, const bf16* __restrict__ w3t,
    const float* __restrict__ b1, const float* __restrict__ b2,
    const float* __restrict__ b3, const float* __restrict__ w3v,
    bf16* __restrict__ ein_out, bf16* __restrict__ t1_out,
    bf16* __restrict__ msg_out, bf16* __restrict__ dz1_out,
    bf16* __restrict__ dz2_out, bf16* __restrict__ dz3_out,
    bf16* __restrict__ dhr_out, bf16* __restrict__ dhc_out,
    float* __restrict__ dcd_out, float* __restrict__ dw3v_out,
    float* __restrict__ gb_out,  // [3*H]: gb1 | gb2 | gb3 column sums
    float* __restrict__ tail_out,  // LIN: dW1 tail partials [4*ntile][3*H]
    long m, int normalize, float eps) {
  constexpr bool LIN = MODE == EB_LIN;
  constexpr int K_IN = EDB<H>::K_IN;
  constexpr int K_PAD = EDB<H>::K_PAD;
  constexpr int K_STRIDE = EDB<H>::K_STRIDE;
  constexpr int K_OUT = EDB<H>::K_OUT;
  constexpr int H_STRIDE = EDB<H>::H_STRIDE;
  constexpr int NT = EDB<H>::NT;
  constexpr int HP = EDB<H>::HP;
  constexpr int NTK = EDB<H>::NTK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr Smem<H> L = smem_layout<H>();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  float* biases = reinterpret_cast<float*>(smem + L.bias);
  float* wpart = reinterpret_cast<float*>(smem + L.wpart);
  float* gbacc = reinterpret_cast<float*>(smem + L.gbacc);
  for (int i = tid; i < H; i += THREADS) {
    biases[i] = b1[i];
    biases[H + i] = b2[i];
    biases[2 * H + i] = b3[i];
    biases[3 * H + i] = w3v[i];
    wpart[i] = 0.f;
    gbacc[i] = 0.f;
    gbacc[H + i] = 0.f;
    gbacc[2 * H + i] = 0.f;
  }
  __syncthreads();  // biases/accumulators initialized by wave 0

  // Wave-per-subtile execution: every phase below reads and writes ONLY
  // its own wave's 16 rows of each LDS tile (and its own 16 entries of
  // rows/cols/diff/scal), so the tile loop needs NO barriers in either
  // mode — 12 independent waves per CU instead of 3 barrier-convoyed
  // 4-wave groups (PMC showed 62% SQ_WAIT_ANY dominated by the 14
  // sync-separated phases). The block-wide wpart/gbacc sums are LDS
  // atomics, flushed after the one barrier that follows the loop.
  // XCD-aware tile remap (same as fused_edge_fwd): contiguous tile
  // ranges per XCD keep each XCD's row gathers inside its 4 MiB L2.
  const long ntile = (m + TILE - 1) / TILE;
  const long tq = ntile >> 3, tr = ntile & 7;
  for (long vt = blockIdx.x; vt < ntile; vt += gridDim.x) {
    const long xcd = vt & 7, ti = vt >> 3;
    const long tile =
        (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + ti;
    long e0 = tile * TILE;
    int nedge = (int)((m - e0 < (long)TILE) ? (m - e0) : (long)TILE);
    int* rws = reinterpret_cast<int*>(smem + L.rows);
    int* cls = reinterpret_cast<int*>(smem + L.cols);
    if (lane < 16) {
      int e = wave * 16 + lane;
      rws[e] = e < nedge ? (int)row[e0 + e] : 0;
      cls[e] = e < nedge ? (int)col[e0 + e] : 0;
    }

    // ---- stage ein (wave-local rows) ----
    for (int idx = lane; idx < 16 * 2 * HP; idx += 64) {
      int e = wave * 16 + idx / (2 * HP), piece = idx % (2 * HP);
      char* dst = smem + L.in_tile + e * K_STRIDE * 2;
      int c8 = (piece % HP) * 8;
      bf16x8 v = {};
      if (e < nedge) {
        long src = piece < HP ? rws[e] : cls[e];
        v = g8(h + src * H + c8);
      }
      *reinterpret_cast<bf16x8*>(dst + (piece < HP ? c8 : H + c8) * 2) = v;
    }
    if (lane < 16) {
      int e = wave * 16 + lane;
      char* dst = smem + L.in_tile + e * K_STRIDE * 2;
      float* dptr = reinterpret_cast<float*>(smem + L.diff) + e * 4;
      float dx = 0, dy = 0, dz = 0, r2 = 0, a0 = 0, a1 = 0;
      if (e < nedge) {
        long ge = e0 + e;
        long i = rws[e], j = cls[e];
        dx = coord[i * 3] - coord[j * 3];
        dy = coord[i * 3 + 1] - coord[j * 3 + 1];
        dz = coord[i * 3 + 2] - coord[j * 3 + 2];
        r2 = dx * dx + dy * dy + dz * dz;
        a0 = eattr[ge * EA];
        a1 = eattr[ge * EA + 1];
      }
      dptr[0] = dx; dptr[1] = dy; dptr[2] = dz; dptr[3] = r2;
      __bf16* brow = reinterpret_cast<__bf16*>(dst);
      brow[2 * H] = (__bf16)r2;
      brow[2 * H + 1] = (__bf16)a0;
      brow[2 * H + 2] = (__bf16)a1;
#pragma unroll
      for (int k = K_IN; k < K_PAD; ++k) brow[k] = (__bf16)0.f;
    }
    // ein -> global (only the split-K wgrad path consumes it)
    if constexpr (!LIN) {
      for (int idx = lane; idx < 16 * (K_OUT / 8); idx += 64) {
        int e = wave * 16 + idx / (K_OUT / 8);
        if (e >= nedge) continue;
        int c8 = (idx % (K_OUT / 8)) * 8;
        *reinterpret_cast<bf16x8*>(ein_out + (e0 + e) * K_OUT + c8) =
            lds8(smem, L.in_tile + (e * K_STRIDE + c8) * 2);
      }
    }

    // ---- recompute: z1, z2, z3 (pre-activations) ----
    {
      f32x4 acc[NT] = {};
      mm_g<K_PAD / 32, false, NT>(smem, L.in_tile + wave * 16 * K_STRIDE * 2,
                              K_STRIDE * 2, opaque(w1p), K_PAD, lane, acc);
      __bf16* z1 = reinterpret_cast<__bf16*>(smem + L.z1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int e = wave * 16 + (lane >> 4) * 4 + r;
          z1[e * H_STRIDE + c] = (__bf16)(acc[nt][r] + biases[c]);
        }
      }
    }
    // t1 = silu(z1) -> global (coalesced, wave-local rows)
    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = wave * 16 + idx / HP;
      if (e >= nedge) continue;
      int c8 = (idx % HP) * 8;
      *reinterpret_cast<bf16x8*>(t1_out + (e0 + e) * H + c8) =
          lds8_silu(smem, L.z1 + (e * H_STRIDE + c8) * 2);
    }
    {
      f32x4 acc[NT] = {};
      mm_g<H / 32, true, NT>(smem, L.z1 + wave * 16 * H_STRIDE * 2, H_STRIDE * 2,
                    opaque(w2), H, lane, acc);
      __bf16* z2 = reinterpret_cast<__bf16*>(smem + L.z2);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int e = wave * 16 + (lane >> 4) * 4 + r;
          z2[e * H_STRIDE + c] = (__bf16)(acc[nt][r] + biases[H + c]);
        }
      }
    }
    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = wave * 16 + idx / HP;
      if (e >= nedge) continue;
      int c8 = (idx % HP) * 8;
      *reinterpret_cast<bf16x8*>(msg_out + (e0 + e) * H + c8) =
          lds8_silu(smem, L.z2 + (e * H_STRIDE + c8) * 2);
    }
    {
      f32x4 acc[NT] = {};
      mm_g<H / 32, true, NT>(smem, L.z2 + wave * 16 * H_STRIDE * 2, H_STRIDE * 2,
                    opaque(w3), H, lane, acc);
      __bf16* z3 = reinterpret_cast<__bf16*>(smem + L.z3);
      float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + (lane & 15);
        float wv = biases[3 * H + c];
        float bb = biases[2 * H + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = acc[nt][r] + bb;
          z3[((wave * 16 + (lane >> 4) * 4 + r)) * H_STRIDE + c] = (__bf16)z;
          part[r] += silu_(z) * wv;
        }
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[r] += __shfl_xor(part[r], off, 64);
      if ((lane & 15) == 0) {
        float* sc = reinterpret_cast<float*>(smem + L.scal);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sc[(wave * 16 + (lane >> 4) * 4 + r) * 4] = part[r];  // p
      }
    }

    // ---- head backward: dp; dw3v partial; dz3 overwrites z3 ----
    if (lane < 16) {
      int e = wave * 16 + lane;
      float* sc = reinterpret_cast<float*>(smem + L.scal) + e * 4;
      const float* dptr = reinterpret_cast<float*>(smem + L.diff) + e * 4;
      float dp = 0.f;
      if (e < nedge) {
        long i = rws[e];
        float inv = normalize ? 1.f / (sqrtf(dptr[3]) + eps) : 1.f;
        dp = (dtrans_n[i * 3] * dptr[0] + dtrans_n[i * 3 + 1] * dptr[1] +
              dtrans_n[i * 3 + 2] * dptr[2]) * inv;
      }
      sc[1] = dp;
    }
#pragma unroll
    for (int c = tid & 63; c < H; c += 64) {
      // lane covers column(s) c over its wave's 16 edges: dw3v partial +
      // dz3 in place
      int estart = (tid >> 6) * 16;
      float acc_w = 0.f, acc_b3 = 0.f;
      float wv = biases[3 * H + c];
      __bf16* z3 = reinterpret_cast<__bf16*>(smem + L.z3);
      const float* sc = reinterpret_cast<const float*>(smem + L.scal);
      for (int e = estart; e < estart + 16; ++e) {
        float z = (float)z3[e * H_STRIDE + c];
        float dp = sc[e * 4 + 1];
        acc_w += dp * silu_(z);
        float d3 = dp * wv * dsilu_(z);
        acc_b3 += d3;
        z3[e * H_STRIDE + c] = (__bf16)d3;
      }
      atomicAdd(&wpart[c], acc_w);
      atomicAdd(&gbacc[2 * H + c], acc_b3);
    }
    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = wave * 16 + idx / HP;
      if (e >= nedge) continue;
      int c8 = (idx % HP) * 8;
      *reinterpret_cast<bf16x8*>(dz3_out + (e0 + e) * H + c8) =
          lds8(smem, L.z3 + (e * H_STRIDE + c8) * 2);
    }

    // ---- dz2 = (dmsg_n[row] + dz3 @ W3) silu'(z2), overwrite z2 ----
    {
      f32x4 acc[NT] = {};
      mm_g<H / 32, false, NT>(smem, L.z3 + wave * 16 * H_STRIDE * 2, H_STRIDE * 2,
                     opaque(w3t), H, lane, acc);
      // z3 consumed: reuse its tile to stage dmsg_n[row] COALESCED
      // (the C-layout merge otherwise issues 16 scattered 2 B loads/lane)
      for (int idx = lane; idx < 16 * HP; idx += 64) {
        int e = wave * 16 + idx / HP;
        int c8 = (idx % HP) * 8;
        bf16x8 v = {};
        if (e < nedge) v = g8(dmsg_n + (long)rws[e] * H + c8);
        *reinterpret_cast<bf16x8*>(smem + L.z3 + (e * H_STRIDE + c8) * 2) = v;
      }
      __bf16* z2 = reinterpret_cast<__bf16*>(smem + L.z2);
      const __bf16* dmsg_t = reinterpret_cast<const __bf16*>(smem + L.z3);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int e = wave * 16 + (lane >> 4) * 4 + r;
          float up = (float)dmsg_t[e * H_STRIDE + c];
          float z = (float)z2[e * H_STRIDE + c];
          z2[e * H_STRIDE + c] = (__bf16)((acc[nt][r] + up) * dsilu_(z));
        }
      }
    }
    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = wave * 16 + idx / HP;
      if (e >= nedge) continue;
      int c8 = (idx % HP) * 8;
      *reinterpret_cast<bf16x8*>(dz2_out + (e0 + e) * H + c8) =
          lds8(smem, L.z2 + (e * H_STRIDE + c8) * 2);
    }
#pragma unroll
    for (int c = tid & 63; c < H; c += 64) {
      int estart = (tid >> 6) * 16;
      const __bf16* z2 = reinterpret_cast<const __bf16*>(smem + L.z2);
      float acc_b = 0.f;
      for (int e = estart; e < estart + 16; ++e)
        acc_b += (float)z2[e * H_STRIDE + c];
      atomicAdd(&gbacc[H + c], acc_b);
    }

    // ---- dz1 = (dz2 @ W2) silu'(z1), overwrite z1 ----
    {
      f32x4 acc[NT] = {};
      mm_g<H / 32, false, NT>(smem, L.z2 + wave * 16 * H_STRIDE * 2, H_STRIDE * 2,
                     opaque(w2t), H, lane, acc);
      __bf16* z1 = reinterpret_cast<__bf16*>(smem + L.z1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int e = wave * 16 + (lane >> 4) * 4 + r;
          float z = (float)z1[e * H_STRIDE + c];
          z1[e * H_STRIDE + c] = (__bf16)(acc[nt][r] * dsilu_(z));
        }
      }
    }
    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = wave * 16 + idx / HP;
      if (e >= nedge) continue;
      int c8 = (idx % HP) * 8;
      *reinterpret_cast<bf16x8*>(dz1_out + (e0 + e) * H + c8) =
          lds8(smem, L.z1 + (e * H_STRIDE + c8) * 2);
    }
#pragma unroll
    for (int c = tid & 63; c < H; c += 64) {
      int estart = (tid >> 6) * 16;
      const __bf16* z1 = reinterpret_cast<const __bf16*>(smem + L.z1);
      float acc_b = 0.f;
      for (int e = estart; e < estart + 16; ++e)
        acc_b += (float)z1[e * H_STRIDE + c];
      atomicAdd(&gbacc[c], acc_b);
    }

    // ---- dein = dz1 @ W1 in register passes of <=3 n-tiles ----
    // pass outputs land in in_tile (ein no longer needed). NTK 16-col
    // tiles (9 at H=64) processed 3 per pass to bound live accumulators.
    if constexpr (LIN) {
      // only the n-tile that holds column 2H, in the k order of the full
      // product below: dr2 is bit-equal. Nothing goes back into in_tile.
      constexpr int T2H = 2 * H / 16;
      const bf16* w1tp_ = opaque(w1tp);
      f32x4 acc = {};
#pragma unroll
      for (int kk = 0; kk < H / 32; ++kk) {
        int k = kk * 32 + (lane >> 4) * 8;
        bf16x8 a = lds8(smem, L.z1 + (wave * 16 + (lane & 15)) * H_STRIDE * 2
                                  + k * 2);
        bf16x8 b = g8(w1tp_ + (T2H * 16 + (lane & 15)) * H + k);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      }
      if ((lane & 15) == 0) {
        float* sc = reinterpret_cast<float*>(smem + L.scal);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sc[(wave * 16 + (lane >> 4) * 4 + r) * 4 + 2] = acc[r];  // dr2
      }
      // dW1 tail: z1 holds dz1 and in_tile still holds ein, whose columns
      // 2H..2H+2 are the bf16 r2/attr the first layer read (zero on padded
      // rows, as is dz1), so each product is exact in fp32. Lane c sums
      // column c over its wave's 16 rows in order; every (tile, wave)
      // writes its whole partial row.
      float* tl = tail_out +
                  ((e0 >> 6) * 4 + __builtin_amdgcn_readfirstlane(wave)) *
                      (3 * H);
#pragma unroll
      for (int c = lane; c < H; c += 64) {
        const __bf16* z1 = reinterpret_cast<const __bf16*>(smem + L.z1);
        const __bf16* ein = reinterpret_cast<const __bf16*>(smem + L.in_tile);
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        // four rows per trip: a full unroll holds 64 LDS reads in flight
#pragma unroll 4
        for (int e = wave * 16; e < wave * 16 + 16; ++e) {
          float d = (float)z1[e * H_STRIDE + c];
          t0 += d * (float)ein[e * K_STRIDE + 2 * H];
          t1 += d * (float)ein[e * K_STRIDE + 2 * H + 1];
          t2 += d * (float)ein[e * K_STRIDE + 2 * H + 2];
        }
        tl[c * 3] = t0;
        tl[c * 3 + 1] = t1;
        tl[c * 3 + 2] = t2;
      }
    } else {
#pragma unroll
      for (int pass = 0; pass * 3 < NTK; ++pass) {
        const bf16* w1tp_ = opaque(w1tp);
        f32x4 acc[3] = {};
#pragma unroll
        for (int kk = 0; kk < H / 32; ++kk) {
          int k = kk * 32 + (lane >> 4) * 8;
          bf16x8 a = lds8(smem, L.z1 + (wave * 16 + (lane & 15)) * H_STRIDE * 2
                                    + k * 2);
#pragma unroll
          for (int nt = 0; nt < 3; ++nt) {
            if (pass * 3 + nt >= NTK) break;
            int gc = (pass * 3 + nt) * 16 + (lane & 15);
            bf16x8 b = g8(w1tp_ + gc * H + k);
            acc[nt] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt], 0, 0, 0);
          }
        }
        __bf16* dein = reinterpret_cast<__bf16*>(smem + L.in_tile);
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) {
          if (pass * 3 + nt >= NTK) break;
          int c = (pass * 3 + nt) * 16 + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int e = wave * 16 + (lane >> 4) * 4 + r;
            dein[e * K_STRIDE + c] = (__bf16)acc[nt][r];
            if (c == 2 * H) {
              float* sc = reinterpret_cast<float*>(smem + L.scal);
              sc[e * 4 + 2] = acc[nt][r];  // dr2 (fp32, before bf16 rounding)
            }
          }
        }
      }
    }
    // dh_row / dh_col -> global (coalesced, wave-local rows)
    if constexpr (!LIN) {
      for (int idx = lane; idx < 16 * HP; idx += 64) {
        int e = wave * 16 + idx / HP;
        if (e >= nedge) continue;
        int c8 = (idx % HP) * 8;
        *reinterpret_cast<bf16x8*>(dhr_out + (e0 + e) * H + c8) =
            lds8(smem, L.in_tile + (e * K_STRIDE + c8) * 2);
        *reinterpret_cast<bf16x8*>(dhc_out + (e0 + e) * H + c8) =
            lds8(smem, L.in_tile + (e * K_STRIDE + H + c8) * 2);
      }
    }
    // dcd (wave-local rows)
    if (lane < 16 && wave * 16 + lane < nedge) {
      int e = wave * 16 + lane;
      long ge = e0 + e;
      const float* dptr = reinterpret_cast<float*>(smem + L.diff) + e * 4;
      const float* sc = reinterpret_cast<float*>(smem + L.scal) + e * 4;
      long i = rws[e];
      float tx = dtrans_n[i * 3], ty = dtrans_n[i * 3 + 1],
            tz = dtrans_n[i * 3 + 2];
      float p = sc[0], dr2 = sc[2];
      float inv = normalize ? 1.f / (sqrtf(dptr[3]) + eps) : 1.f;
      dcd_out[ge * 3] = p * tx * inv + 2.f * dptr[0] * dr2;
      dcd_out[ge * 3 + 1] = p * ty * inv + 2.f * dptr[1] * dr2;
      dcd_out[ge * 3 + 2] = p * tz * inv + 2.f * dptr[2] * dr2;
    }
  }
  __syncthreads();
  for (int c = tid; c < H; c += THREADS) atomicAdd(&dw3v_out[c], wpart[c]);
  for (int c = tid; c < 3 * H; c += THREADS) atomicAdd(&gb_out[c], gbacc[c]);
}

}  // namespace

template <int H, int MODE>
static std::vector<torch::Tensor> fused_edge_backward_impl(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor dmsg_n,
    torch::Tensor dtrans_n, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped) {
  constexpr bool LIN = MODE == EB_LIN;
  long m = row.numel();
  constexpr int K_IN = EDB<H>::K_IN;
  constexpr int K_PAD = EDB<H>::K_PAD;
  constexpr int K_OUT = EDB<H>::K_OUT;
  auto bopt = h.options();
  auto fopt = coord.options().dtype(torch::kFloat);
  auto ein = torch::empty({LIN ? 0 : m, (long)K_OUT}, bopt);
  auto t1 = torch::empty({m, (long)H}, bopt);
  auto msg = torch::empty({m, (long)H}, bopt);
  auto dz1 = torch::empty({m, (long)H}, bopt);
  auto dz2 = torch::empty({m, (long)H}, bopt);
  auto dz3 = torch::empty({m, (long)H}, bopt);
  auto dhr = torch::empty({LIN ? 0 : m, (long)H}, bopt);
  auto dhc = torch::empty({LIN ? 0 : m, (long)H}, bopt);
  auto dcd = torch::empty({m, 3}, fopt);
  torch::Tensor dw3v, gb, tail_part;
  if (LIN) {
    // one fill for the two atomically accumulated outputs
    auto acc = torch::zeros({4 * (long)H}, fopt);
    dw3v = acc.narrow(0, 0, H);
    gb = acc.narrow(0, H, 3 * H);
    // one partial row of the dW1 tail per (tile, wave); the kernel writes
    // every row
    tail_part = torch::empty({4 * ((m + TILE - 1) / TILE), 3 * (long)H}, fopt);
  } else {
    dw3v = torch::zeros({(long)H}, fopt);
    gb = torch::zeros({3 * (long)H}, fopt);
  }
  if (m == 0) {
    if (LIN)
      return {t1, msg, dz1, dz2, dz3, dcd, dw3v, gb,
              torch::zeros({(long)H, 3}, fopt)};
    return {ein, t1, msg, dz1, dz2, dz3, dhr, dhc, dcd, dw3v, gb};
  }
  auto stream = at::hip::getCurrentHIPStream();
  constexpr Smem<H> L = smem_layout<H>();
  long tiles = (m + TILE - 1) / TILE;
  int blocks = (int)std::min<long>(tiles, 16384);
  auto hc = h.contiguous();
  auto cc = coord.contiguous().to(torch::kFloat);
  auto ec = eattr.contiguous().to(torch::kFloat);
  auto dmn = dmsg_n.contiguous();
  auto dtn = dtrans_n.contiguous().to(torch::kFloat);
  torch::Tensor w1p, w1tp, w2c, w2tc, w3c, w3tc, b1c, b2c, b3c, w3vc;
  if (!prepped.empty()) {
    TORCH_CHECK(prepped.size() == 10, "edge bwd prepped wants 10 tensors");
    w1p = prepped[0]; w1tp = prepped[1]; w2c = prepped[2];
    w2tc = prepped[3]; w3c = prepped[4]; w3tc = prepped[5];
    b1c = prepped[6]; b2c = prepped[7]; b3c = prepped[8]; w3vc = prepped[9];
    TORCH_CHECK(w1p.size(1) == K_PAD && w1tp.size(0) == K_OUT,
                "prepped w1p/w1tp must be padded");
  } else {
    // the kernel reads the weights as bf16: anything else would be
    // reinterpreted, not converted
    TORCH_CHECK(w1.scalar_type() == torch::kBFloat16 &&
                    w2.scalar_type() == torch::kBFloat16 &&
                    w3.scalar_type() == torch::kBFloat16,
                "fused_edge_backward: w1/w2/w3 must be bf16 when no prepped "
                "weights are passed");
    auto w1c = w1.contiguous();
    w1p = torch::constant_pad_nd(w1c, {0, K_PAD - K_IN});
    w1tp = torch::constant_pad_nd(w1c.t().contiguous(),
                                  {0, 0, 0, K_OUT - K_IN});
    w2c = w2.contiguous();
    w2tc = w2c.t().contiguous();
    w3c = w3.contiguous();
    w3tc = w3c.t().contiguous();
    b1c = b1.contiguous().to(torch::kFloat);
    b2c = b2.contiguous().to(torch::kFloat);
    b3c = b3.contiguous().to(torch::kFloat);
    w3vc = w3v.contiguous().to(torch::kFloat);
  }
  fused_edge_bwd<H, MODE><<<blocks, THREADS, L.total, stream>>>(
      reinterpret_cast<const bf16*>(hc.data_ptr()), cc.data_ptr<float>(),
      ec.data_ptr<float>(), row.contiguous().data_ptr<long>(),
      col.contiguous().data_ptr<long>(),
      reinterpret_cast<const bf16*>(dmn.data_ptr()), dtn.data_ptr<float>(),
      reinterpret_cast<const bf16*>(w1p.data_ptr()),
      reinterpret_cast<const bf16*>(w1tp.data_ptr()),
      reinterpret_cast<const bf16*>(w2c.data_ptr()),
      reinterpret_cast<const bf16*>(w2tc.data_ptr()),
      reinterpret_cast<const bf16*>(w3c.data_ptr()),
      reinterpret_cast<const bf16*>(w3tc.data_ptr()), b1c.data_ptr<float>(),
      b2c.data_ptr<float>(), b3c.data_ptr<float>(), w3vc.data_ptr<float>(),
      reinterpret_cast<bf16*>(ein.data_ptr()),
      reinterpret_cast<bf16*>(t1.data_ptr()),
      reinterpret_cast<bf16*>(msg.data_ptr()),
      reinterpret_cast<bf16*>(dz1.data_ptr()),
      reinterpret_cast<bf16*>(dz2.data_ptr()),
      reinterpret_cast<bf16*>(dz3.data_ptr()),
      reinterpret_cast<bf16*>(dhr.data_ptr()),
      reinterpret_cast<bf16*>(dhc.data_ptr()), dcd.data_ptr<float>(),
      dw3v.data_ptr<float>(), gb.data_ptr<float>(),
      LIN ? tail_part.data_ptr<float>() : nullptr, m, normalize ? 1 : 0,
      (float)eps);
  if (LIN) {
    // aten's sum is deterministic: a fixed fold over the partial rows
    auto gw1_tail = tail_part.sum(0).view({(long)H, 3});
    return {t1, msg, dz1, dz2, dz3, dcd, dw3v, gb, gw1_tail};
  }
  return {ein, t1, msg, dz1, dz2, dz3, dhr, dhc, dcd, dw3v, gb};
}

std::vector<torch::Tensor> fused_edge_backward(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor dmsg_n,
    torch::Tensor dtrans_n, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped) {
  long hdim = h.size(1);
  TORCH_CHECK(hdim == 32 || hdim == 64 || hdim == 128,
              "fused edge backward supports hidden_nf in {32, 64, 128}");
  if (hdim == 32)
    return fused_edge_backward_impl<32, EB_PLAIN>(
        h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3,
        b3, w3v, normalize, eps, std::move(prepped));
  if (hdim == 128)
    return fused_edge_backward_impl<128, EB_PLAIN>(
        h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3,
        b3, w3v, normalize, eps, std::move(prepped));
  return fused_edge_backward_impl<64, EB_PLAIN>(
      h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3, b3,
      w3v, normalize, eps, std::move(prepped));
}

// node-sum variant (EB_LIN): returns {t1, msg, dz1, dz2, dz3, dcd, dw3v, gb,
// gw1_tail [H,3] f32}. No ein, dh_row or dh_col: the caller takes dh and
// the h-columns of dW1 from the per-node sums of dz1.
std::vector<torch::Tensor> fused_edge_backward_lin(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor dmsg_n,
    torch::Tensor dtrans_n, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped) {
  long hdim = h.size(1);
  TORCH_CHECK(hdim == 32 || hdim == 64 || hdim == 128,
              "fused edge backward supports hidden_nf in {32, 64, 128}");
  if (hdim == 32)
    return fused_edge_backward_impl<32, EB_LIN>(
        h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3,
        b3, w3v, normalize, eps, std::move(prepped));
  if (hdim == 128)
    return fused_edge_backward_impl<128, EB_LIN>(
        h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3,
        b3, w3v, normalize, eps, std::move(prepped));
  return fused_edge_backward_impl<64, EB_LIN>(
      h, coord, eattr, row, col, dmsg_n, dtrans_n, w1, b1, w2, b2, w3, b3,
      w3v, normalize, eps, std::move(prepped));
}
