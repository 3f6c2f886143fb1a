// Fused node block: phi_h (node_mlp + residual) and phi_v (coord_mlp_vel)
// of one FastEGNN layer in one forward and one backward kernel.
//
//   node chain  z1 = [h | agg_e | agg_v | attr] W1^T + b1, t1 = silu(z1),
//               out = t1 W2^T + b2, h_out = h + out
//   vel chain   zv = h Wv1^T + bv1, tv = silu(zv), phiv = tv . wv2 + bv2
//
// The composition this replaces ran ~25 launches per layer (cat, four
// tall_linear forwards, silus, residual add; mirrored backward with column
// sums and slice copies), each re-reading or re-writing an [N, H] tensor.
// Here the input tile is assembled in LDS from its four sources, every
// intermediate stays in registers/LDS, and the backward recomputes z1/zv
// from the inputs (nothing else is saved).
//
// Mapping: 64-row tiles, 4 waves, one wave per 16-row subtile. Every phase
// reads and writes only its own wave's LDS rows, so there is no block
// barrier inside the tile loop (only wave-level fences). Weights are
// staged to LDS once per block; the grid is capped and blocks walk tiles.
// mfma_f32_16x16x32_bf16 throughout; operand/accumulator lane orders are
// those of tall_linear.hip. The bf16 rounding points of the composition
// are kept: z1, t1, out, h + out, zv, tv, phiv (forward), dt1, dz1, dtv,
// dzv (backward).
//
// Bias / head / attribute-column gradients are accumulated in registers
// over the tiles a wave walks and written once per (block, wave) as a
// partial row; the host folds the rows with one deterministic sum.
//
// Instantiated for H in {32, 64}. At H = 128 the weights do not fit in LDS;
// the entry points below hand that width to fused_node_h128.hip.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "fused_node_h128.h"

namespace {

constexpr int TILE = 64;
constexpr int THREADS = 256;
constexpr int NUM_CU = 256;            // grid cap: blocks walk tiles past it
constexpr size_t LDS_PER_CU = 160 * 1024;

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float rb(float v) { return (float)(__bf16)v; }
__device__ __forceinline__ float sigm(float x) {
  return 1.f / (1.f + __expf(-x));
}

// Orders one wave's LDS writes before its later LDS reads (other lanes'
// data); no other wave touches the same rows.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int H, int A, bool VEL_ONLY>
struct NodeCfg {
  static constexpr int NT = H / 16;
  static constexpr int K1 = 3 * H + A;
  static constexpr int KP = (K1 + 31) / 32 * 32;
  static constexpr int HS = H + 8;   // bank-padded strides (elements)
  static constexpr int KS = KP + 8;
  // per-wave input tile: [h | agg_e | agg_v | attr | 0]; vel-only keeps h
  // and one H-wide scratch block
  static constexpr int XS = VEL_ONLY ? 2 * H + 8 : KS;
  static constexpr int PW = 4 * H + H * A + 1;  // partial-row width
};

// acc[nt] += a_tile[16 rows][K] * b[nt*16 + n][K]^T for K = 32 * ksteps
template <int NT>
__device__ __forceinline__ void mma_tile(const __bf16* a, int a_stride,
                                         const __bf16* b, int b_stride,
                                         int ksteps, int lane,
                                         f32x4 (&acc)[NT]) {
  const int r = lane & 15, kb = (lane >> 4) * 8;
  for (int kk = 0; kk < ksteps; ++kk) {
    bf16x8 av =
        *reinterpret_cast<const bf16x8*>(a + r * a_stride + kk * 32 + kb);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bf16x8 bv = *reinterpret_cast<const bf16x8*>(
          b + (nt * 16 + r) * b_stride + kk * 32 + kb);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[nt], 0,
                                                        0, 0);
    }
  }
}

// stage a [rows][cols] bf16 matrix (cols % 8 == 0, 16-B aligned rows)
__device__ __forceinline__ void stage_w(__bf16* dst, int dst_stride,
                                        const bf16* src, int rows, int cols,
                                        int tid) {
  const int c8n = cols / 8;
  for (int idx = tid; idx < rows * c8n; idx += THREADS) {
    int r = idx / c8n, c8 = (idx % c8n) * 8;
    *reinterpret_cast<bf16x8*>(dst + r * dst_stride + c8) =
        *reinterpret_cast<const bf16x8*>(src + (long)r * cols + c8);
  }
}

// 16 rows x H of one global [n, H] tensor -> wave tile columns [col0, +H)
template <int H>
__device__ __forceinline__ void load_rows(__bf16* tile, int stride, int col0,
                                          const bf16* src, long row0,
                                          int nrow, int lane) {
  constexpr int C8 = H / 8;
#pragma unroll
  for (int idx = lane; idx < 16 * C8; idx += 64) {
    int r = idx / C8, c8 = (idx % C8) * 8;
    bf16x8 v = {};
    if (r < nrow)
      v = *reinterpret_cast<const bf16x8*>(src + (row0 + r) * H + c8);
    *reinterpret_cast<bf16x8*>(tile + r * stride + col0 + c8) = v;
  }
}

// wave tile columns [col0, +H) -> 16 rows of a global [n, H] tensor
template <int H>
__device__ __forceinline__ void store_rows(const __bf16* tile, int stride,
                                           int col0, bf16* dst, long row0,
                                           int nrow, int lane) {
  constexpr int C8 = H / 8;
#pragma unroll
  for (int idx = lane; idx < 16 * C8; idx += 64) {
    int r = idx / C8, c8 = (idx % C8) * 8;
    if (r < nrow)
      *reinterpret_cast<bf16x8*>(dst + (row0 + r) * H + c8) =
          *reinterpret_cast<const bf16x8*>(tile + r * stride + col0 + c8);
  }
}

template <int H, int A>
__device__ __forceinline__ void load_attr(__bf16* tile, int stride,
                                          const bf16* attr, long row0,
                                          int nrow, int lane) {
  if constexpr (A > 0) {
    for (int idx = lane; idx < 16 * A; idx += 64) {
      int r = idx / A, a = idx % A;
      tile[r * stride + 3 * H + a] =
          r < nrow ? ((const __bf16*)attr)[(row0 + r) * A + a] : (__bf16)0.f;
    }
  }
}

// ---------------------------------------------------------------- forward
template <int H, int A, bool VEL_ONLY>
__global__ __launch_bounds__(THREADS) void fused_node_fwd_kernel(
    const bf16* __restrict__ h, const bf16* __restrict__ agg_e,
    const bf16* __restrict__ agg_v, const bf16* __restrict__ attr,
    const bf16* __restrict__ w1p,   // [H][KP] zero-padded columns
    const bf16* __restrict__ b1, const bf16* __restrict__ w2,
    const bf16* __restrict__ b2, const bf16* __restrict__ wv1,
    const bf16* __restrict__ bv1, const bf16* __restrict__ wv2,
    const bf16* __restrict__ bv2, bf16* __restrict__ h_out,
    float* __restrict__ phiv, long n) {
  using C = NodeCfg<H, A, VEL_ONLY>;
  constexpr int NT = C::NT, HS = C::HS, KS = C::KS, XS = C::XS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = lane & 15, rg = (lane >> 4) * 4;

  __bf16* wv1s = reinterpret_cast<__bf16*>(smem);
  __bf16* w1s = wv1s + H * HS;
  __bf16* w2s = w1s + (VEL_ONLY ? 0 : H * KS);
  __bf16* xall = w2s + (VEL_ONLY ? 0 : H * HS);
  float* fb = reinterpret_cast<float*>(xall + 4 * 16 * XS);
  __bf16* x = xall + wave * 16 * XS;

  stage_w(wv1s, HS, wv1, H, H, tid);
  if constexpr (!VEL_ONLY) {
    stage_w(w1s, KS, w1p, H, C::KP, tid);
    stage_w(w2s, HS, w2, H, H, tid);
  }
  for (int i = tid; i < H; i += THREADS) {
    fb[i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b1)[i];
    fb[H + i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b2)[i];
    fb[2 * H + i] = (float)((const __bf16*)bv1)[i];
    fb[3 * H + i] = (float)((const __bf16*)wv2)[i];
  }
  if (tid == 0) fb[4 * H] = (float)((const __bf16*)bv2)[0];
  // pad columns of the input tile stay zero for the whole kernel
  if constexpr (!VEL_ONLY) {
    for (int idx = lane; idx < 16 * (KS - C::K1); idx += 64) {
      int r = idx / (KS - C::K1), c = C::K1 + idx % (KS - C::K1);
      x[r * XS + c] = (__bf16)0.f;
    }
  }
  __syncthreads();

  const long ntile = (n + TILE - 1) / TILE;
  for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long row0 = t * TILE + wave * 16;
    long left = n - row0;
    const int nrow = left >= 16 ? 16 : (left > 0 ? (int)left : 0);

    load_rows<H>(x, XS, 0, h, row0, nrow, lane);
    if constexpr (!VEL_ONLY) {
      load_rows<H>(x, XS, H, agg_e, row0, nrow, lane);
      load_rows<H>(x, XS, 2 * H, agg_v, row0, nrow, lane);
      load_attr<H, A>(x, XS, attr, row0, nrow, lane);
    }
    wave_sync();

    // ---- vel chain: phiv ----
    {
      f32x4 acc[NT] = {};
      mma_tile<NT>(x, XS, wv1s, HS, H / 32, lane, acc);
      float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float zv = rb(acc[nt][r] + fb[2 * H + c]);
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
        for (int r = 0; r < 4; ++r)
          if (rg + r < nrow) phiv[row0 + rg + r] = rb(p[r] + fb[4 * H]);
      }
    }

    if constexpr (!VEL_ONLY) {
      // ---- node chain ----
      f32x4 acc[NT] = {};
      mma_tile<NT>(x, XS, w1s, KS, C::KP / 32, lane, acc);
      wave_sync();  // all reads of the agg_e columns done: reuse as t1
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = rb(acc[nt][r] + fb[c]);
          x[(rg + r) * XS + H + c] = (__bf16)(z * sigm(z));
        }
      }
      wave_sync();
      f32x4 acc2[NT] = {};
      mma_tile<NT>(x + H, XS, w2s, HS, H / 32, lane, acc2);
      wave_sync();
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float o = rb(acc2[nt][r] + fb[H + c]);
          float hv = (float)x[(rg + r) * XS + c];
          x[(rg + r) * XS + H + c] = (__bf16)(hv + o);
        }
      }
      wave_sync();
      store_rows<H>(x, XS, H, h_out, row0, nrow, lane);
    }
    wave_sync();  // tile reads done before the next trip's loads
  }
}

// --------------------------------------------------------------- backward
template <int H, int A, bool VEL_ONLY>
__global__ __launch_bounds__(THREADS) void fused_node_bwd_kernel(
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
    float* __restrict__ parts,  // [gridDim.x * 4][PW]
    long n) {
  using C = NodeCfg<H, A, VEL_ONLY>;
  constexpr int NT = C::NT, HS = C::HS, KS = C::KS, XS = C::XS;
  constexpr int AA = A > 0 ? A : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cl = lane & 15, rg = (lane >> 4) * 4;

  __bf16* wv1s = reinterpret_cast<__bf16*>(smem);
  __bf16* wv1ts = wv1s + H * HS;
  __bf16* w1s = wv1ts + H * HS;
  __bf16* w1ts = w1s + (VEL_ONLY ? 0 : H * KS);
  __bf16* w2ts = w1ts + (VEL_ONLY ? 0 : 3 * H * HS);
  __bf16* xall = w2ts + (VEL_ONLY ? 0 : H * HS);
  __bf16* gall = xall + 4 * 16 * XS;
  float* fb = reinterpret_cast<float*>(gall + (VEL_ONLY ? 0 : 4 * 16 * HS));
  __bf16* x = xall + wave * 16 * XS;
  __bf16* g = gall + wave * 16 * HS;   // dh_out tile (not vel-only)
  __bf16* s = x + (VEL_ONLY ? H : 0);  // scratch: dzv / t1 / dz1 as A tile
  __bf16* o = x + H;                   // output staging (not vel-only)

  stage_w(wv1s, HS, wv1, H, H, tid);
  stage_w(wv1ts, HS, wv1t, H, H, tid);
  if constexpr (!VEL_ONLY) {
    stage_w(w1s, KS, w1p, H, C::KP, tid);
    stage_w(w1ts, HS, w1t, 3 * H, H, tid);
    stage_w(w2ts, HS, w2t, H, H, tid);
  }
  for (int i = tid; i < H; i += THREADS) {
    fb[i] = VEL_ONLY ? 0.f : (float)((const __bf16*)b1)[i];
    fb[H + i] = (float)((const __bf16*)bv1)[i];
    fb[2 * H + i] = (float)((const __bf16*)wv2)[i];
  }
  if constexpr (!VEL_ONLY) {
    for (int idx = lane; idx < 16 * (KS - C::K1); idx += 64) {
      int r = idx / (KS - C::K1), c = C::K1 + idx % (KS - C::K1);
      x[r * XS + c] = (__bf16)0.f;
    }
  }
  __syncthreads();

  // column-sum accumulators, live across the tile loop (C layout: this
  // lane's 4 rows of column nt*16 + cl)
  float gb1[NT] = {}, gb2[NT] = {}, gbv1[NT] = {}, gwv2[NT] = {};
  float tail[NT][AA] = {};
  float gbv2 = 0.f;

  const long ntile = (n + TILE - 1) / TILE;
  for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long row0 = t * TILE + wave * 16;
    long left = n - row0;
    const int nrow = left >= 16 ? 16 : (left > 0 ? (int)left : 0);

    load_rows<H>(x, XS, 0, h, row0, nrow, lane);
    if constexpr (!VEL_ONLY) {
      load_rows<H>(x, XS, H, agg_e, row0, nrow, lane);
      load_rows<H>(x, XS, 2 * H, agg_v, row0, nrow, lane);
      load_attr<H, A>(x, XS, attr, row0, nrow, lane);
      load_rows<H>(g, HS, 0, dh_out, row0, nrow, lane);
    }
    float dp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dp[r] = rg + r < nrow ? rb(dphiv[row0 + rg + r]) : 0.f;
    if (cl == 0) gbv2 += dp[0] + dp[1] + dp[2] + dp[3];
    wave_sync();

    // ---- recompute both pre-activations from the input tile ----
    float t1[NT][4], ds1[NT][4], dzv[NT][4];
    if constexpr (!VEL_ONLY) {
      f32x4 acc[NT] = {};
      mma_tile<NT>(x, XS, w1s, KS, C::KP / 32, lane, acc);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = rb(acc[nt][r] + fb[nt * 16 + cl]);
          float sg = sigm(z);
          t1[nt][r] = rb(z * sg);
          ds1[nt][r] = sg * (1.f + z * (1.f - sg));
        }
    }
    {
      f32x4 acc[NT] = {};
      mma_tile<NT>(x, XS, wv1s, HS, H / 32, lane, acc);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = rb(acc[nt][r] + fb[H + c]);
          float sg = sigm(z);
          float tv = rb(z * sg);
          float dtv = rb(dp[r] * fb[2 * H + c]);
          float d = rb(dtv * (sg * (1.f + z * (1.f - sg))));
          dzv[nt][r] = d;
          gbv1[nt] += d;
          gwv2[nt] += dp[r] * tv;
        }
      }
    }
    // attribute columns of dW1 need attr after the tile is recycled
    float at[4][AA];
    if constexpr (!VEL_ONLY && A > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int a = 0; a < A; ++a)
          at[r][a] = (float)x[(rg + r) * XS + 3 * H + a];
    }
    wave_sync();  // input tile consumed: its columns become scratch

    // ---- dzv: store, and start dh with dzv Wv1 ----
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[(rg + r) * XS + nt * 16 + cl] = (__bf16)dzv[nt][r];
    wave_sync();
    store_rows<H>(s, XS, 0, dzv_out, row0, nrow, lane);
    f32x4 adh[NT] = {};
    mma_tile<NT>(s, XS, wv1ts, HS, H / 32, lane, adh);
    wave_sync();

    if constexpr (VEL_ONLY) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s[(rg + r) * XS + nt * 16 + cl] = (__bf16)adh[nt][r];
      wave_sync();
      store_rows<H>(s, XS, 0, dh, row0, nrow, lane);
    } else {
      // ---- t1 out (operand of dW2) ----
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s[(rg + r) * XS + nt * 16 + cl] = (__bf16)t1[nt][r];
      wave_sync();
      store_rows<H>(s, XS, 0, t1_out, row0, nrow, lane);
      // ---- dt1 = dh_out W2, dz1 = dt1 * silu'(z1) ----
      f32x4 acc2[NT] = {};
      mma_tile<NT>(g, HS, w2ts, HS, H / 32, lane, acc2);
      wave_sync();  // t1 rows stored before dz1 overwrites them
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float d = rb(rb(acc2[nt][r]) * ds1[nt][r]);
          gb1[nt] += d;
          gb2[nt] += (float)g[(rg + r) * HS + c];
          if constexpr (A > 0) {
#pragma unroll
            for (int a = 0; a < A; ++a) tail[nt][a] += d * at[r][a];
          }
          s[(rg + r) * XS + c] = (__bf16)d;
        }
      }
      wave_sync();
      store_rows<H>(s, XS, 0, dz1_out, row0, nrow, lane);
      // ---- din = dz1 W1, first 3H columns, one H-wide block at a time
      mma_tile<NT>(s, XS, w1ts, HS, H / 32, lane, adh);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        int c = nt * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o[(rg + r) * XS + c] =
              (__bf16)(adh[nt][r] + (float)g[(rg + r) * HS + c]);
      }
      wave_sync();
      store_rows<H>(o, XS, 0, dh, row0, nrow, lane);
#pragma unroll
      for (int blk = 1; blk < 3; ++blk) {
        f32x4 ad[NT] = {};
        mma_tile<NT>(s, XS, w1ts + blk * H * HS, HS, H / 32, lane, ad);
        wave_sync();  // previous block's rows stored
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            o[(rg + r) * XS + nt * 16 + cl] = (__bf16)ad[nt][r];
        wave_sync();
        store_rows<H>(o, XS, 0, blk == 1 ? dagg_e : dagg_v, row0, nrow,
                      lane);
      }
    }
    wave_sync();  // tile reads done before the next trip's loads
  }

  // fold the 4 row groups of the wave; lanes 0..15 hold the column sums
  float* prow = parts + ((long)blockIdx.x * 4 + wave) * C::PW;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    float v[4 + AA] = {gb1[nt], gb2[nt], gbv1[nt], gwv2[nt]};
#pragma unroll
    for (int a = 0; a < AA; ++a) v[4 + a] = tail[nt][a];
#pragma unroll
    for (int i = 0; i < 4 + AA; ++i) {
      v[i] += __shfl_xor(v[i], 16, 64);
      v[i] += __shfl_xor(v[i], 32, 64);
    }
    if (lane < 16) {
      int c = nt * 16 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) prow[i * H + c] = v[i];
#pragma unroll
      for (int a = 0; a < A; ++a) prow[4 * H + c * A + a] = v[4 + a];
    }
  }
  gbv2 += __shfl_xor(gbv2, 16, 64);
  gbv2 += __shfl_xor(gbv2, 32, 64);
  if (lane == 0) prow[4 * H + H * A] = gbv2;
}

template <int H, int A, bool VEL_ONLY>
size_t fwd_smem() {
  using C = NodeCfg<H, A, VEL_ONLY>;
  size_t e = (size_t)H * C::HS + 4 * 16 * C::XS;
  if (!VEL_ONLY) e += (size_t)H * C::KS + H * C::HS;
  return e * 2 + (4 * H + 4) * 4;
}

template <int H, int A, bool VEL_ONLY>
size_t bwd_smem() {
  using C = NodeCfg<H, A, VEL_ONLY>;
  size_t e = (size_t)2 * H * C::HS + 4 * 16 * C::XS;
  if (!VEL_ONLY)
    e += (size_t)H * C::KS + 3 * H * C::HS + H * C::HS + 4 * 16 * C::HS;
  return e * 2 + (3 * H + 4) * 4;
}

const bf16* bp(const torch::Tensor& t) {
  return reinterpret_cast<const bf16*>(t.data_ptr());
}
bf16* bpm(torch::Tensor& t) { return reinterpret_cast<bf16*>(t.data_ptr()); }

void check_bf16(const torch::Tensor& t, long rows, long cols,
                const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.is_contiguous() && t.dim() == 2 && t.size(0) == rows &&
                  t.size(1) == cols,
              name, " must be a contiguous CUDA bf16 [", rows, ", ", cols,
              "] tensor");
}

// one or two resident blocks per CU, as the LDS footprint allows
int grid_for(long n, size_t smem) {
  long tiles = (n + TILE - 1) / TILE;
  long per_cu = smem * 2 <= LDS_PER_CU ? 2 : 1;
  return (int)std::min<long>(tiles, NUM_CU * per_cu);
}

}  // namespace

// prepped (all bf16): w1 column-padded [H, roundup32(3H+A)], b1, w2, b2,
// wv1, bv1, wv2 [1,H], bv2 [1]. vel_only reads only the last four.
std::vector<torch::Tensor> fused_node_forward(
    torch::Tensor h, torch::Tensor agg_e, torch::Tensor agg_v,
    c10::optional<torch::Tensor> attr, std::vector<torch::Tensor> prepped,
    bool vel_only) {
  const long n = h.size(0);
  const int hd = (int)h.size(1);
  const int a = attr.has_value() ? (int)attr->size(1) : 0;
  check_bf16(h, n, hd, "h");
  TORCH_CHECK(prepped.size() == 8, "fused_node_forward: 8 prepped tensors");
  if (!vel_only) {
    check_bf16(agg_e, n, hd, "agg_e");
    check_bf16(agg_v, n, hd, "agg_v");
    if (a > 0) check_bf16(*attr, n, a, "attr");
    check_bf16(prepped[0], hd, (3 * hd + a + 31) / 32 * 32, "w1 (padded)");
    check_bf16(prepped[2], hd, hd, "w2");
    TORCH_CHECK(prepped[1].numel() == hd && prepped[3].numel() == hd,
                "bias size");
  }
  check_bf16(prepped[4], hd, hd, "wv1");
  TORCH_CHECK(prepped[5].numel() == hd && prepped[6].numel() == hd &&
                  prepped[7].numel() == 1,
              "vel head sizes");
  for (auto& t : prepped)
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                    t.is_contiguous(),
                "prepped weights must be contiguous CUDA bf16");
  auto h_out = vel_only ? torch::empty({0, (long)hd}, h.options())
                        : torch::empty({n, (long)hd}, h.options());
  auto phiv = torch::empty({n, 1}, h.options().dtype(torch::kFloat));
  if (n == 0) return {h_out, phiv};
  if (hd == 128) {  // weights read from L2: fused_node_h128.hip
    TORCH_CHECK(a <= 8, "fused_node: node_attr_nf > 8");
    fused_node_h128_forward(h, agg_e, agg_v, attr, a, prepped, vel_only,
                            h_out, phiv);
    return {h_out, phiv};
  }
  auto stream = at::hip::getCurrentHIPStream();
  const bf16* attr_p = a > 0 ? bp(*attr) : nullptr;

#define NODE_FWD(HH, AAv, VO)                                               \
  do {                                                                      \
    auto kern = fused_node_fwd_kernel<HH, AAv, VO>;                         \
    size_t sm = fwd_smem<HH, AAv, VO>();                                    \
    static bool lds_set = false;                                            \
    if (!lds_set) {                                                         \
      HIP_CHECK(hipFuncSetAttribute(                                        \
          reinterpret_cast<const void*>(kern),                              \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));            \
      lds_set = true;                                                       \
    }                                                                       \
    const int blocks = grid_for(n, sm);                                     \
    kern<<<blocks, THREADS, sm, stream>>>(                                  \
        bp(h), bp(agg_e), bp(agg_v), attr_p, bp(prepped[0]),                \
        bp(prepped[1]), bp(prepped[2]), bp(prepped[3]), bp(prepped[4]),     \
        bp(prepped[5]), bp(prepped[6]), bp(prepped[7]), bpm(h_out),         \
        phiv.data_ptr<float>(), n);                                         \
    HIP_CHECK(hipGetLastError());                                           \
  } while (0)
#define NODE_FWD_A(HH, AAv)                                                 \
  case AAv:                                                                 \
    NODE_FWD(HH, AAv, false);                                               \
    break;
#define NODE_FWD_H(HH)                                                      \
  case HH:                                                                  \
    if (vel_only) {                                                         \
      NODE_FWD(HH, 0, true);                                                \
    } else {                                                                \
      switch (a) {                                                          \
        NODE_FWD_A(HH, 0) NODE_FWD_A(HH, 1) NODE_FWD_A(HH, 2)               \
        NODE_FWD_A(HH, 3) NODE_FWD_A(HH, 4) NODE_FWD_A(HH, 5)               \
        NODE_FWD_A(HH, 6) NODE_FWD_A(HH, 7) NODE_FWD_A(HH, 8)               \
        default: TORCH_CHECK(false, "fused_node: node_attr_nf > 8");        \
      }                                                                     \
    }                                                                       \
    break;
  switch (hd) {
    NODE_FWD_H(32)
    NODE_FWD_H(64)
    default: TORCH_CHECK(false, "fused_node: hidden_nf must be 32, 64 or 128");
  }
#undef NODE_FWD_H
#undef NODE_FWD_A
#undef NODE_FWD
  return {h_out, phiv};
}

// prepped (all bf16): w1 column-padded, w1^T [3H+A, H], b1, w2^T, wv1,
// wv1^T, bv1, wv2. Returns dh, dagg_e, dagg_v, dz1, t1, dzv (bf16 [N,H];
// only dh and dzv are filled in vel-only mode) and the fp32 partial rows
// [blocks*4, 4H + H*A + 1] = gb1 | gb2 | gbv1 | gwv2 | dW1 attr columns |
// gbv2, to be summed over dim 0 (one row per block at H = 128).
std::vector<torch::Tensor> fused_node_backward(
    torch::Tensor dh_out, torch::Tensor dphiv, torch::Tensor h,
    torch::Tensor agg_e, torch::Tensor agg_v,
    c10::optional<torch::Tensor> attr, std::vector<torch::Tensor> prepped,
    bool vel_only) {
  const long n = h.size(0);
  const int hd = (int)h.size(1);
  const int a = attr.has_value() ? (int)attr->size(1) : 0;
  check_bf16(h, n, hd, "h");
  TORCH_CHECK(dphiv.is_cuda() && dphiv.scalar_type() == torch::kFloat &&
                  dphiv.is_contiguous() && dphiv.numel() == n,
              "dphiv must be a contiguous CUDA fp32 [N, 1] tensor");
  TORCH_CHECK(prepped.size() == 8, "fused_node_backward: 8 prepped tensors");
  if (!vel_only) {
    check_bf16(dh_out, n, hd, "dh_out");
    check_bf16(agg_e, n, hd, "agg_e");
    check_bf16(agg_v, n, hd, "agg_v");
    if (a > 0) check_bf16(*attr, n, a, "attr");
    check_bf16(prepped[0], hd, (3 * hd + a + 31) / 32 * 32, "w1 (padded)");
    check_bf16(prepped[1], 3 * hd + a, hd, "w1^T");
    check_bf16(prepped[3], hd, hd, "w2^T");
    TORCH_CHECK(prepped[2].numel() == hd, "bias size");
  }
  check_bf16(prepped[4], hd, hd, "wv1");
  check_bf16(prepped[5], hd, hd, "wv1^T");
  TORCH_CHECK(prepped[6].numel() == hd && prepped[7].numel() == hd,
              "vel head sizes");
  for (auto& t : prepped)
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                    t.is_contiguous(),
                "prepped weights must be contiguous CUDA bf16");
  const long nf = vel_only ? 0 : n;
  auto opt = h.options();
  auto dh = torch::empty({n, (long)hd}, opt);
  auto dagg_e = torch::empty({nf, (long)hd}, opt);
  auto dagg_v = torch::empty({nf, (long)hd}, opt);
  auto dz1 = torch::empty({nf, (long)hd}, opt);
  auto t1 = torch::empty({nf, (long)hd}, opt);
  auto dzv = torch::empty({n, (long)hd}, opt);
  const long pw = 4 * hd + (long)hd * (vel_only ? 0 : a) + 1;
  torch::Tensor parts;
  if (n == 0) {
    parts = torch::zeros({0, pw}, opt.dtype(torch::kFloat));
    return {dh, dagg_e, dagg_v, dz1, t1, dzv, parts};
  }
  if (hd == 128) {  // weights read from L2: fused_node_h128.hip
    TORCH_CHECK(a <= 8, "fused_node: node_attr_nf > 8");
    parts = fused_node_h128_backward(dh_out, dphiv, h, agg_e, agg_v, attr, a,
                                     prepped, vel_only, dh, dagg_e, dagg_v,
                                     dz1, t1, dzv);
    return {dh, dagg_e, dagg_v, dz1, t1, dzv, parts};
  }
  auto stream = at::hip::getCurrentHIPStream();
  const bf16* attr_p = a > 0 ? bp(*attr) : nullptr;

#define NODE_BWD(HH, AAv, VO)                                               \
  do {                                                                      \
    auto kern = fused_node_bwd_kernel<HH, AAv, VO>;                         \
    size_t sm = bwd_smem<HH, AAv, VO>();                                    \
    static bool lds_set = false;                                            \
    if (!lds_set) {                                                         \
      HIP_CHECK(hipFuncSetAttribute(                                        \
          reinterpret_cast<const void*>(kern),                              \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));            \
      lds_set = true;                                                       \
    }                                                                       \
    const int blocks = grid_for(n, sm);                                     \
    parts = torch::empty({(long)blocks * 4, pw}, opt.dtype(torch::kFloat)); \
    kern<<<blocks, THREADS, sm, stream>>>(                                  \
        bp(dh_out), dphiv.data_ptr<float>(), bp(h), bp(agg_e), bp(agg_v),   \
        attr_p, bp(prepped[0]), bp(prepped[1]), bp(prepped[2]),             \
        bp(prepped[3]), bp(prepped[4]), bp(prepped[5]), bp(prepped[6]),     \
        bp(prepped[7]), bpm(dh), bpm(dagg_e), bpm(dagg_v), bpm(dz1),        \
        bpm(t1), bpm(dzv), parts.data_ptr<float>(), n);                     \
    HIP_CHECK(hipGetLastError());                                           \
  } while (0)
#define NODE_BWD_A(HH, AAv)                                                 \
  case AAv:                                                                 \
    NODE_BWD(HH, AAv, false);                                               \
    break;
#define NODE_BWD_H(HH)                                                      \
  case HH:                                                                  \
    if (vel_only) {                                                         \
      NODE_BWD(HH, 0, true);                                                \
    } else {                                                                \
      switch (a) {                                                          \
        NODE_BWD_A(HH, 0) NODE_BWD_A(HH, 1) NODE_BWD_A(HH, 2)               \
        NODE_BWD_A(HH, 3) NODE_BWD_A(HH, 4) NODE_BWD_A(HH, 5)               \
        NODE_BWD_A(HH, 6) NODE_BWD_A(HH, 7) NODE_BWD_A(HH, 8)               \
        default: TORCH_CHECK(false, "fused_node: node_attr_nf > 8");        \
      }                                                                     \
    }                                                                       \
    break;
  switch (hd) {
    NODE_BWD_H(32)
    NODE_BWD_H(64)
    default: TORCH_CHECK(false, "fused_node: hidden_nf must be 32, 64 or 128");
  }
#undef NODE_BWD_H
#undef NODE_BWD_A
#undef NODE_BWD
  return {dh, dagg_e, dagg_v, dz1, t1, dzv, parts};
}
