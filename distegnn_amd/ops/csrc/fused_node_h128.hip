// Fused node block at hidden_nf = 128: the kernels of fused_node.hip with
// the weights left in global memory.
//
// At H = 128 the weights no longer fit in LDS beside a tile (fused_node.hip
// would need 229 KB forward, 382 KB backward), so they stay in global
// memory, where all of them (172 KB forward, 337 KB backward) sit in one
// XCD's L2, and every wave reads its B fragments from there. What makes
// that affordable is the mapping: the four waves of a block split the 128
// OUTPUT COLUMNS (32 each, two 16-column MFMA tiles) and every wave walks
// all four 16-row subtiles of the 64-row tile, so a B fragment is loaded
// once per block and tile and used for 64 rows, and a block reads each
// weight matrix exactly once per tile (with the row split of fused_node.hip
// it would be four times). The fragments of K step kk + 2 are loaded before
// the MFMAs of step kk.
//
// The input tile [h | agg_e | agg_v | attr | 0] is shared by the four
// waves, so the phases of a tile are separated by block barriers (four per
// tile forward, seven backward); two blocks are resident per CU and cover
// each other's barriers. The three H-wide column blocks of the tile are
// recycled as staging areas once the first GEMM has read them:
//
//   forward   R1 <- t1, R2 <- h + out
//   backward  R0 <- dzv, R1 <- t1, R2 <- dz1, then R0 <- dh, R1 <- dagg_e,
//             R2 <- dagg_v
//
// Semantics, rounding points and outputs are those of fused_node.hip. The
// column sums are kept per lane for the wave's 32 columns; a block writes
// ONE partial row (every wave its own columns), folded by the host's sum.
// phiv needs the 128-column dot product, which is folded over the four
// waves through LDS in a fixed order. No atomics anywhere.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "fused_node_h128.h"

namespace {

constexpr int H = 128;
constexpr int TILE = 64;               // rows per block and trip
constexpr int MS = TILE / 16;          // 16-row subtiles, all walked by a wave
constexpr int WN = 2;                  // 16-column tiles per wave
constexpr int THREADS = 256;
constexpr int GRID_CAP = 512;          // 256 CUs x 2 resident blocks
constexpr int HS = H + 8;              // bank-padded strides (elements)
constexpr int AHEAD = 2;               // K steps of B fragments in flight

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float rb(float v) { return (float)(__bf16)v; }
__device__ __forceinline__ float sigm(float x) {
  return 1.f / (1.f + __expf(-x));
}

template <int A, bool VEL_ONLY>
struct Cfg {
  static constexpr int K1 = 3 * H + A;
  static constexpr int KP = (K1 + 31) / 32 * 32;
  static constexpr int KS = KP + 8;
  static constexpr int XS_FWD = VEL_ONLY ? HS : KS;
  // vel-only backward: h and one H-wide staging block
  static constexpr int XS_BWD = VEL_ONLY ? 2 * H + 8 : KS;
  static constexpr int PW = 4 * H + H * A + 1;  // partial-row width
};

// Between the 16-row subtiles of an epilogue. Left alone the scheduler
// interleaves the exponentials and divisions of all 32 values of a lane
// and runs out of registers; this keeps it to one subtile (8) at a time.
#define SUBTILE_FENCE() __builtin_amdgcn_sched_barrier(0)

// The value is computed where this stands. Without it the compiler sinks
// an epilogue to the first use of its results, past the next GEMM, and
// keeps the accumulators (and z and the sigmoid instead of silu') alive.
#define PIN(v) asm volatile("" : "+v"(v))

// acc[m][j] += a[m*16 + row][K] * b[(nt0 + j)*16 + n][K]^T, K = 32*KSTEPS.
// a is the block's LDS tile, b a row-major global matrix of row stride
// b_stride (elements, a multiple of 8).
template <int KSTEPS>
__device__ __forceinline__ void mma_cols(const __bf16* a, int a_stride,
                                         const bf16* __restrict__ b,
                                         int b_stride, int nt0, int lane,
                                         f32x4 (&acc)[MS][WN]) {
  const int r = lane & 15, kb = (lane >> 4) * 8;
  const __bf16* bl = reinterpret_cast<const __bf16*>(b) +
                     (long)(nt0 * 16 + r) * b_stride + kb;
  const __bf16* al = a + r * a_stride + kb;
  // The weights do not change over the tile loop, so the compiler would
  // lift the first loads of all seven walks out of it and keep (spill) 112
  // registers of fragments. An empty asm on the pointer keeps them here.
  asm volatile("" : "+v"(bl));
  // q[0] is the step in use, q[1..AHEAD] are in flight. The loop is kept
  // rolled: unrolled, the compiler hoists every load of the walk and
  // spills.
  bf16x8 q[AHEAD + 1][WN];
#pragma unroll
  for (int d = 0; d < AHEAD; ++d)
#pragma unroll
    for (int j = 0; j < WN; ++j)
      q[d][j] = *reinterpret_cast<const bf16x8*>(
          bl + (long)j * 16 * b_stride + (d < KSTEPS ? d : 0) * 32);
#pragma unroll
  for (int j = 0; j < WN; ++j) q[AHEAD][j] = q[AHEAD - 1][j];
#pragma unroll 1
  for (int kk = 0; kk < KSTEPS; ++kk) {
    if (kk + AHEAD < KSTEPS) {
#pragma unroll
      for (int j = 0; j < WN; ++j)
        q[AHEAD][j] = *reinterpret_cast<const bf16x8*>(
            bl + (long)j * 16 * b_stride + (kk + AHEAD) * 32);
    }
#pragma unroll
    for (int m = 0; m < MS; ++m) {
      bf16x8 av =
          *reinterpret_cast<const bf16x8*>(al + m * 16 * a_stride + kk * 32);
#pragma unroll
      for (int j = 0; j < WN; ++j)
        acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, q[0][j],
                                                            acc[m][j], 0, 0,
                                                            0);
    }
#pragma unroll
    for (int d = 0; d < AHEAD; ++d)
#pragma unroll
      for (int j = 0; j < WN; ++j) q[d][j] = q[d + 1][j];
  }
}

// Tile copies: thread tid moves 16 bytes of rows tid/16 + 16 i, i = 0..3.
// Addresses are one per-thread offset plus constants, off a base that is
// uniform over the block, so that the compiler keeps four offsets for all
// tensors and not a 64-bit pointer per tensor and row.
//
// 64 rows x H of a global [n, H] tensor -> tile columns [col0, +H); rows
// past nrow are zero
__device__ __forceinline__ void load_tile(__bf16* tile, int stride, int col0,
                                          const bf16* src, long row0,
                                          int nrow, int tid) {
  const bf16* base = src + row0 * H;
  const int r0 = tid >> 4, c8 = (tid & 15) * 8;
  __bf16* tl = tile + r0 * stride + c8;
#pragma unroll
  for (int i = 0; i < TILE / 16; ++i) {
    bf16x8 v = {};
    if (r0 + i * 16 < nrow)
      v = *reinterpret_cast<const bf16x8*>(
          base + (unsigned)(r0 * H + c8 + i * 16 * H));
    *reinterpret_cast<bf16x8*>(tl + i * 16 * stride + col0) = v;
  }
}

// tile columns [col0, +H) -> the first nrow of 64 rows of a global [n, H]
__device__ __forceinline__ void store_tile(const __bf16* tile, int stride,
                                           int col0, bf16* dst, long row0,
                                           int nrow, int tid) {
  bf16* base = dst + row0 * H;
  const int r0 = tid >> 4, c8 = (tid & 15) * 8;
  const __bf16* tl = tile + r0 * stride + c8;
#pragma unroll
  for (int i = 0; i < TILE / 16; ++i) {
    if (r0 + i * 16 < nrow)
      *reinterpret_cast<bf16x8*>(base +
                                 (unsigned)(r0 * H + c8 + i * 16 * H)) =
          *reinterpret_cast<const bf16x8*>(tl + i * 16 * stride + col0);
  }
}

template <int A>
__device__ __forceinline__ void load_attr(__bf16* tile, int stride,
                                          const bf16* attr, long row0,
                                          int nrow, int tid) {
  if constexpr (A > 0) {
    for (int idx = tid; idx < TILE * A; idx += THREADS) {
      int r = idx / A, a = idx % A;
      tile[r * stride + 3 * H + a] =
          r < nrow ? ((const __bf16*)attr)[(row0 + r) * A + a] : (__bf16)0.f;
    }
  }
}

// this lane's accumulator values -> tile columns [col0, +H)
__device__ __forceinline__ void put_cols(__bf16* tile, int stride, int col0,
                                         int nt0, int lane,
                                         const float (&v)[MS][WN][4]) {
  __bf16* tl = tile + (lane >> 4) * 4 * stride + nt0 * 16 + (lane & 15);
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tl[(m * 16 + r) * stride + col0 + j * 16] = (__bf16)v[m][j][r];
}

// ---------------------------------------------------------------- forward
template <int A, bool VEL_ONLY>
__global__ __launch_bounds__(THREADS, 2) void fused_node_h128_fwd_kernel(
    const bf16* __restrict__ h, const bf16* __restrict__ agg_e,
    const bf16* __restrict__ agg_v, const bf16* __restrict__ attr,
    const bf16* __restrict__ w1p,   // [H][KP] zero-padded columns
    const bf16* __restrict__ b1, const bf16* __restrict__ w2,
    const bf16* __restrict__ b2, const bf16* __restrict__ wv1,
    const bf16* __restrict__ bv1, const bf16* __restrict__ wv2,
    const bf16* __restrict__ bv2, bf16* __restrict__ h_out,
    float* __restrict__ phiv, long n) {
  using C = Cfg<A, VEL_ONLY>;
  constexpr int XS = C::XS_FWD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = lane & 15, rg = (lane >> 4) * 4;
  const int nt0 = wave * WN;

  __bf16* x = reinterpret_cast<__bf16*>(smem);
  float* fb = reinterpret_cast<float*>(x + TILE * XS);
  float* pp = fb + 4 * H + 4;   // [4 waves][64 rows] partial phiv

  for (int i = tid; i < H; i += THREADS) {
    fb[i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b1)[i];
    fb[H + i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b2)[i];
    fb[2 * H + i] = (float)((const __bf16*)bv1)[i];
    fb[3 * H + i] = (float)((const __bf16*)wv2)[i];
  }
  if (tid == 0) fb[4 * H] = (float)((const __bf16*)bv2)[0];
  // pad columns of the input tile stay zero for the whole kernel
  if constexpr (!VEL_ONLY) {
    constexpr int PADC = XS - C::K1;
    for (int idx = tid; idx < TILE * PADC; idx += THREADS) {
      int r = idx / PADC, c = C::K1 + idx % PADC;
      x[r * XS + c] = (__bf16)0.f;
    }
  }

  const long ntile = (n + TILE - 1) / TILE;
  for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long row0 = t * TILE;
    const long left = n - row0;
    const int nrow = left >= TILE ? TILE : (int)left;

    load_tile(x, XS, 0, h, row0, nrow, tid);
    if constexpr (!VEL_ONLY) {
      load_tile(x, XS, H, agg_e, row0, nrow, tid);
      load_tile(x, XS, 2 * H, agg_v, row0, nrow, tid);
      load_attr<A>(x, XS, attr, row0, nrow, tid);
    }
    __syncthreads();

    // ---- vel chain: this wave's 32 columns of the phiv dot product ----
    {
      f32x4 acc[MS][WN] = {};
      mma_cols<H / 32>(x, XS, wv1, H, nt0, lane, acc);
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          int c = (nt0 + j) * 16 + cl;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float zv = rb(acc[m][j][r] + fb[2 * H + c]);
            float tv = rb(zv * sigm(zv));
            p[r] += tv * fb[3 * H + c];
          }
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] += __shfl_xor(p[r], off, 64);
        if (cl == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) pp[wave * TILE + m * 16 + rg + r] = p[r];
        }
      }
    }

    if constexpr (!VEL_ONLY) {
      // ---- node chain ----
      float t1[MS][WN][4];
      {
        f32x4 acc[MS][WN] = {};
        mma_cols<C::KP / 32>(x, XS, w1p, C::KP, nt0, lane, acc);
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
          for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float z = rb(acc[m][j][r] + fb[(nt0 + j) * 16 + cl]);
              t1[m][j][r] = z * sigm(z);
            }
      }
      __syncthreads();  // every wave has read the input tile: R1 <- t1
      put_cols(x, XS, H, nt0, lane, t1);
      __syncthreads();
      f32x4 acc2[MS][WN] = {};
      mma_cols<H / 32>(x + H, XS, w2, H, nt0, lane, acc2);
      // R2 <- h + out (nobody reads R2 after the first GEMM)
#pragma unroll
      for (int m = 0; m < MS; ++m)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          int c = (nt0 + j) * 16 + cl;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = m * 16 + rg + r;
            float o = rb(acc2[m][j][r] + fb[H + c]);
            float hv = (float)x[row * XS + c];
            x[row * XS + 2 * H + c] = (__bf16)(hv + o);
          }
        }
      __syncthreads();
      store_tile(x, XS, 2 * H, h_out, row0, nrow, tid);
    } else {
      __syncthreads();
    }
    // fold the four waves' column quarters in a fixed order
    if (tid < nrow)
      phiv[row0 + tid] = rb(((pp[tid] + pp[TILE + tid]) + pp[2 * TILE + tid]) +
                            pp[3 * TILE + tid] + fb[4 * H]);
    __syncthreads();  // tile and pp reads done before the next trip
  }
}

// --------------------------------------------------------------- backward
template <int A, bool VEL_ONLY>
__global__ __launch_bounds__(THREADS, 2) void fused_node_h128_bwd_kernel(
    const bf16* __restrict__ dh_out, const float* __restrict__ dphiv,
    const bf16* __restrict__ h, const bf16* __restrict__ agg_e,
    const bf16* __restrict__ agg_v, const bf16* __restrict__ attr,
    const bf16* __restrict__ w1p,   // [H][KP]
    const bf16* __restrict__ w1t,   // [K1][H]; the first 3H rows are read
    const bf16* __restrict__ b1, const bf16* __restrict__ w2t,
    const bf16* __restrict__ wv1, const bf16* __restrict__ wv1t,
    const bf16* __restrict__ bv1, const bf16* __restrict__ wv2,
    bf16* __restrict__ dh, bf16* __restrict__ dagg_e,
    bf16* __restrict__ dagg_v, bf16* __restrict__ dz1_out,
    bf16* __restrict__ t1_out, bf16* __restrict__ dzv_out,
    float* __restrict__ parts,  // [gridDim.x][PW]
    long n) {
  using C = Cfg<A, VEL_ONLY>;
  constexpr int XS = C::XS_BWD;
  constexpr int AA = A > 0 ? A : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid0 = threadIdx.x, wave = tid0 >> 6;
  const int nt0 = wave * WN;

  __bf16* x = reinterpret_cast<__bf16*>(smem);
  __bf16* g = x + TILE * XS;   // dh_out tile (not vel-only)
  float* fb = reinterpret_cast<float*>(g + (VEL_ONLY ? 0 : TILE * HS));
  float* dps = fb + 3 * H;     // [64] bf16-rounded dphiv of the tile
  // vel-only keeps h in columns [0, H) and stages in [H, 2H)
  constexpr int S0 = VEL_ONLY ? H : 0;

  for (int i = tid0; i < H; i += THREADS) {
    fb[i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b1)[i];
    fb[H + i] = (float)((const __bf16*)bv1)[i];
    fb[2 * H + i] = (float)((const __bf16*)wv2)[i];
  }
  if constexpr (!VEL_ONLY) {
    constexpr int PADC = XS - C::K1;
    for (int idx = tid0; idx < TILE * PADC; idx += THREADS) {
      int r = idx / PADC, c = C::K1 + idx % PADC;
      x[r * XS + c] = (__bf16)0.f;
    }
  }

  // column-sum accumulators, live across the tile loop (C layout: this
  // lane's rows rg..rg+3 of every subtile, column (nt0 + j)*16 + cl)
  float gb1[WN] = {}, gb2[WN] = {}, gbv1[WN] = {}, gwv2[WN] = {};
  float tail[WN][AA] = {};
  float gbv2 = 0.f;   // wave 0: lane l sums row l of every tile

  const long ntile = (n + TILE - 1) / TILE;
  for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long row0 = t * TILE;
    const long left = n - row0;
    const int nrow = left >= TILE ? TILE : (int)left;
    // The thread index passes through an empty asm once per trip: every
    // LDS and global address below is then computed where it is used. As
    // loop invariants the compiler kept well over a hundred of them in
    // registers across the trip and spilled.
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, cl = lane & 15, rg = (lane >> 4) * 4;
    // this lane's origin in the accumulator layout (row rg, column
    // nt0*16 + cl): every access below is one of these plus a constant
    __bf16* xl = x + rg * XS + nt0 * 16 + cl;
    const __bf16* gl = g + rg * HS + nt0 * 16 + cl;
    const __bf16* xa = x + rg * XS + 3 * H;   // attribute columns
    const float* fbl = fb + nt0 * 16 + cl;
    const float* dpl = dps + rg;

    load_tile(x, XS, 0, h, row0, nrow, tid);
    if constexpr (!VEL_ONLY) {
      load_tile(x, XS, H, agg_e, row0, nrow, tid);
      load_tile(x, XS, 2 * H, agg_v, row0, nrow, tid);
      load_attr<A>(x, XS, attr, row0, nrow, tid);
      load_tile(g, HS, 0, dh_out, row0, nrow, tid);
    }
    if (tid < TILE) dps[tid] = tid < nrow ? rb(dphiv[row0 + tid]) : 0.f;
    __syncthreads();
    if (wave == 0) gbv2 += dps[lane];

    // ---- recompute both pre-activations from the input tile (the vel
    // chain first: it leaves 32 live values, the node chain 64) ----
    float t1[MS][WN][4], ds1[MS][WN][4], dzv[MS][WN][4];
    {
      f32x4 acc[MS][WN] = {};
      mma_cols<H / 32>(x, XS, wv1, H, nt0, lane, acc);
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        SUBTILE_FENCE();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dp = dpl[m * 16 + r];
#pragma unroll
          for (int j = 0; j < WN; ++j) {
            float z = rb(acc[m][j][r] + fbl[H + j * 16]);
            float sg = sigm(z);
            float tv = rb(z * sg);
            float dtv = rb(dp * fbl[2 * H + j * 16]);
            float d = rb(dtv * (sg * (1.f + z * (1.f - sg))));
            dzv[m][j][r] = d;
            PIN(dzv[m][j][r]);
            gbv1[j] += d;
            gwv2[j] += dp * tv;
            PIN(gbv1[j]);   // the sums too: else the terms are kept
            PIN(gwv2[j]);   // (spilled) and added at the end of the trip
          }
        }
      }
    }
    if constexpr (!VEL_ONLY) {
      f32x4 acc[MS][WN] = {};
      mma_cols<C::KP / 32>(x, XS, w1p, C::KP, nt0, lane, acc);
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        SUBTILE_FENCE();
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float z = rb(acc[m][j][r] + fbl[j * 16]);
            float sg = sigm(z);
            t1[m][j][r] = rb(z * sg);
            ds1[m][j][r] = sg * (1.f + z * (1.f - sg));
            PIN(t1[m][j][r]);
            PIN(ds1[m][j][r]);
          }
      }
    }
    __syncthreads();  // input tile consumed by every wave: columns recycle

    // ---- R0 <- dzv, R1 <- t1 ----
    put_cols(x, XS, S0, nt0, lane, dzv);
    if constexpr (!VEL_ONLY) put_cols(x, XS, H, nt0, lane, t1);
    __syncthreads();
    store_tile(x, XS, S0, dzv_out, row0, nrow, tid);

    if constexpr (VEL_ONLY) {
      f32x4 adh[MS][WN] = {};
      mma_cols<H / 32>(x + S0, XS, wv1t, H, nt0, lane, adh);
      // h's columns are free since the barrier after the recompute
#pragma unroll
      for (int m = 0; m < MS; ++m)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            xl[(m * 16 + r) * XS + j * 16] = (__bf16)adh[m][j][r];
      __syncthreads();
      store_tile(x, XS, 0, dh, row0, nrow, tid);
    } else {
      store_tile(x, XS, H, t1_out, row0, nrow, tid);
      // ---- dt1 = dh_out W2, dz1 = dt1 * silu'(z1): R2 <- dz1 ----
      {
        f32x4 acc2[MS][WN] = {};
        mma_cols<H / 32>(g, HS, w2t, H, nt0, lane, acc2);
#pragma unroll
        for (int m = 0; m < MS; ++m) {
          SUBTILE_FENCE();
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = m * 16 + r;   // past the lane's origin
            float at[AA];
            if constexpr (A > 0) {
#pragma unroll
              for (int a = 0; a < A; ++a) at[a] = (float)xa[row * XS + a];
            }
#pragma unroll
            for (int j = 0; j < WN; ++j) {
              float d = rb(rb(acc2[m][j][r]) * ds1[m][j][r]);
              gb1[j] += d;
              gb2[j] += (float)gl[row * HS + j * 16];
              PIN(gb1[j]);
              PIN(gb2[j]);
              if constexpr (A > 0) {
#pragma unroll
                for (int a = 0; a < A; ++a) {
                  tail[j][a] += d * at[a];
                  PIN(tail[j][a]);
                }
              }
              xl[row * XS + 2 * H + j * 16] = (__bf16)d;
            }
          }
        }
      }
      __syncthreads();  // dz1 complete; the t1 rows are stored
      store_tile(x, XS, 2 * H, dz1_out, row0, nrow, tid);
      // ---- dh = dh_out + dzv Wv1 + dz1 W1[:, :H] (R0 and R2 are read by
      // every wave until the next barrier: dh waits in registers) ----
      f32x4 adh[MS][WN] = {};
      mma_cols<H / 32>(x, XS, wv1t, H, nt0, lane, adh);
      mma_cols<H / 32>(x + 2 * H, XS, w1t, H, nt0, lane, adh);
      // ---- dagg_e, dagg_v = dz1 W1[:, H:3H], one H-wide block each ----
      {
        f32x4 ad[MS][WN] = {};
        mma_cols<H / 32>(x + 2 * H, XS, w1t + (long)H * H, H, nt0, lane, ad);
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
          for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              xl[(m * 16 + r) * XS + H + j * 16] =                 // R1 <- dagg_e
                  (__bf16)ad[m][j][r];
      }
      f32x4 adv[MS][WN] = {};
      mma_cols<H / 32>(x + 2 * H, XS, w1t + (long)2 * H * H, H, nt0, lane,
                       adv);
      __syncthreads();  // dzv and dz1 read by every wave: R0 <- dh, R2 <- dagg_v
#pragma unroll
      for (int m = 0; m < MS; ++m)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            xl[(m * 16 + r) * XS + j * 16] =
                (__bf16)(adh[m][j][r] +
                         (float)gl[(m * 16 + r) * HS + j * 16]);
            xl[(m * 16 + r) * XS + 2 * H + j * 16] = (__bf16)adv[m][j][r];
          }
      __syncthreads();
      store_tile(x, XS, 0, dh, row0, nrow, tid);
      store_tile(x, XS, H, dagg_e, row0, nrow, tid);
      store_tile(x, XS, 2 * H, dagg_v, row0, nrow, tid);
    }
    __syncthreads();  // tile reads done before the next trip's loads
  }

  // fold the 4 row groups of the wave; lanes 0..15 hold the sums of the
  // wave's columns. Every column of the block's row has one writer.
  const int lane = tid0 & 63;
  float* prow = parts + (long)blockIdx.x * C::PW;
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    float v[4 + AA] = {gb1[j], gb2[j], gbv1[j], gwv2[j]};
#pragma unroll
    for (int a = 0; a < AA; ++a) v[4 + a] = tail[j][a];
#pragma unroll
    for (int i = 0; i < 4 + AA; ++i) {
      v[i] += __shfl_xor(v[i], 16, 64);
      v[i] += __shfl_xor(v[i], 32, 64);
    }
    if (lane < 16) {
      int c = (nt0 + j) * 16 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) prow[i * H + c] = v[i];
#pragma unroll
      for (int a = 0; a < A; ++a) prow[4 * H + c * A + a] = v[4 + a];
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) gbv2 += __shfl_xor(gbv2, off, 64);
    if (lane == 0) prow[4 * H + H * A] = gbv2;
  }
}

template <int A, bool VEL_ONLY>
size_t fwd_smem() {
  using C = Cfg<A, VEL_ONLY>;
  return (size_t)TILE * C::XS_FWD * 2 + (4 * H + 4 + 4 * TILE) * 4;
}

template <int A, bool VEL_ONLY>
size_t bwd_smem() {
  using C = Cfg<A, VEL_ONLY>;
  size_t e = (size_t)TILE * C::XS_BWD + (VEL_ONLY ? 0 : TILE * HS);
  return e * 2 + (3 * H + TILE) * 4;
}

const bf16* bp(const torch::Tensor& t) {
  return reinterpret_cast<const bf16*>(t.data_ptr());
}
bf16* bpm(torch::Tensor& t) { return reinterpret_cast<bf16*>(t.data_ptr()); }

int grid_for(long n) {
  return (int)std::min<long>((n + TILE - 1) / TILE, GRID_CAP);
}

template <typename K>
void allow_lds(K kern, size_t sm) {
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sm));
}

}  // namespace

#define NODE128_CASES(M)                                                    \
  if (vel_only) {                                                           \
    M(0, true);                                                             \
  } else {                                                                  \
    switch (a) {                                                            \
      case 0: M(0, false); break;                                           \
      case 1: M(1, false); break;                                           \
      case 2: M(2, false); break;                                           \
      case 3: M(3, false); break;                                           \
      case 4: M(4, false); break;                                           \
      case 5: M(5, false); break;                                           \
      case 6: M(6, false); break;                                           \
      case 7: M(7, false); break;                                           \
      case 8: M(8, false); break;                                           \
      default: TORCH_CHECK(false, "fused_node: node_attr_nf > 8");          \
    }                                                                       \
  }

void fused_node_h128_forward(const torch::Tensor& h,
                             const torch::Tensor& agg_e,
                             const torch::Tensor& agg_v,
                             const c10::optional<torch::Tensor>& attr, int a,
                             const std::vector<torch::Tensor>& prepped,
                             bool vel_only, torch::Tensor& h_out,
                             torch::Tensor& phiv) {
  const long n = h.size(0);
  TORCH_CHECK(h.size(1) == H && n > 0, "fused_node_h128: [N > 0, 128] input");
  auto stream = at::hip::getCurrentHIPStream();
  const bf16* attr_p = a > 0 && !vel_only ? bp(*attr) : nullptr;
  const int blocks = grid_for(n);
#define NODE128_FWD(AAv, VO)                                                \
  do {                                                                      \
    auto kern = fused_node_h128_fwd_kernel<AAv, VO>;                        \
    size_t sm = fwd_smem<AAv, VO>();                                        \
    static bool lds_set = false;                                            \
    if (!lds_set) {                                                         \
      allow_lds(kern, sm);                                                  \
      lds_set = true;                                                       \
    }                                                                       \
    kern<<<blocks, THREADS, sm, stream>>>(                                  \
        bp(h), bp(agg_e), bp(agg_v), attr_p, bp(prepped[0]),                \
        bp(prepped[1]), bp(prepped[2]), bp(prepped[3]), bp(prepped[4]),     \
        bp(prepped[5]), bp(prepped[6]), bp(prepped[7]), bpm(h_out),         \
        phiv.data_ptr<float>(), n);                                         \
    HIP_CHECK(hipGetLastError());                                           \
  } while (0)
  NODE128_CASES(NODE128_FWD)
#undef NODE128_FWD
}

torch::Tensor fused_node_h128_backward(
    const torch::Tensor& dh_out, const torch::Tensor& dphiv,
    const torch::Tensor& h, const torch::Tensor& agg_e,
    const torch::Tensor& agg_v, const c10::optional<torch::Tensor>& attr,
    int a, const std::vector<torch::Tensor>& prepped, bool vel_only,
    torch::Tensor& dh, torch::Tensor& dagg_e, torch::Tensor& dagg_v,
    torch::Tensor& dz1, torch::Tensor& t1, torch::Tensor& dzv) {
  const long n = h.size(0);
  TORCH_CHECK(h.size(1) == H && n > 0, "fused_node_h128: [N > 0, 128] input");
  auto stream = at::hip::getCurrentHIPStream();
  const bf16* attr_p = a > 0 && !vel_only ? bp(*attr) : nullptr;
  const int blocks = grid_for(n);
  const long pw = 4 * H + (long)H * (vel_only ? 0 : a) + 1;
  auto parts =
      torch::empty({(long)blocks, pw}, h.options().dtype(torch::kFloat));
#define NODE128_BWD(AAv, VO)                                                \
  do {                                                                      \
    auto kern = fused_node_h128_bwd_kernel<AAv, VO>;                        \
    size_t sm = bwd_smem<AAv, VO>();                                        \
    static bool lds_set = false;                                            \
    if (!lds_set) {                                                         \
      allow_lds(kern, sm);                                                  \
      lds_set = true;                                                       \
    }                                                                       \
    kern<<<blocks, THREADS, sm, stream>>>(                                  \
        bp(dh_out), dphiv.data_ptr<float>(), bp(h), bp(agg_e), bp(agg_v),   \
        attr_p, bp(prepped[0]), bp(prepped[1]), bp(prepped[2]),             \
        bp(prepped[3]), bp(prepped[4]), bp(prepped[5]), bp(prepped[6]),     \
        bp(prepped[7]), bpm(dh), bpm(dagg_e), bpm(dagg_v), bpm(dz1),        \
        bpm(t1), bpm(dzv), parts.data_ptr<float>(), n);                     \
    HIP_CHECK(hipGetLastError());                                           \
  } while (0)
  NODE128_CASES(NODE128_BWD)
#undef NODE128_BWD
  return parts;
}
