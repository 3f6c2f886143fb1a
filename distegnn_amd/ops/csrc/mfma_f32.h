// Shared pieces of the forward-only fp32 fused blocks (fused_edge_f32.hip,
// fused_virtual_f32.hip): geometry, the f32-in / f32-accumulate MFMA GEMM
// and its epilogues.
//
// v_mfma_f32_16x16x4_f32 takes ONE float per lane and operand:
//   A[i = l&15][k = l>>4],  B[k = l>>4][j = l&15],  D rows (l>>4)*4 + r,
//   column l&15 (the C/D map of the bf16 16x16 form).
// It is bit-for-bit an f32 fmaf chain over k. A 16-wide k-step is four
// MFMAs: lane group g = l>>4 loads the float4 at k = 16*kk + 4*g from its
// LDS row (A) and from its weight row (B) and feeds element j to the j-th
// MFMA. Within a k-step the k order is thereby permuted (j-major instead of
// g-major), identically in A and B, so every product meets its partner and
// the sum holds the same terms.
//
// One LDS tile serves the whole chain. A wave owns 16 rows of it and no
// other wave touches them (no barriers in the tile loop). Row layout, in
// floats, K_STRIDE apart:
//   [0, 2H)       gathered features        -> GEMM1 input
//   [2H, K_PAD)   scalar tail, zero padded -> GEMM1 input
//   [0, H)        t1   (written after GEMM1 has read the whole row)
//   [H, 2H)       msg  (written after GEMM2 has read t1)
// K_STRIDE = K_PAD + 4 and K_PAD = 2H + 16, so K_STRIDE = 20 (mod 32): the
// 16 rows of a float4 fragment read start 80 bytes apart modulo the 256-byte
// bank span and cover all 64 banks once. The node block (fused_node_f32.hip)
// has three H-wide input blocks, K_PAD = 3H + 16, and its own column order;
// its stride 3H + 20 has the same residue.
#pragma once

#include <torch/extension.h>

#include "common.h"

namespace f32blk {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// NBLK: H-wide input blocks ahead of the scalar tail (edge and virtual 2,
// the node block's [h | agg_e | agg_v] 3, its vel-only form 1). H is a
// multiple of 32, so K_STRIDE = 20 (mod 32) for every NBLK.
template <int H, int NBLK = 2>
struct Dims {
  static_assert(H == 32 || H == 64 || H == 128, "unsupported hidden width");
  static_assert(NBLK >= 1 && NBLK <= 3, "unsupported input block count");
  static constexpr int K_PAD = NBLK * H + 16;  // roundup16 of NBLK*H+1 .. +16
  static constexpr int K_STRIDE = K_PAD + 4;
  static_assert(K_STRIDE % 32 == 20, "float4 fragment reads would conflict");
  static constexpr int NT = H / 16;          // 16-column MFMA tiles per row
  static constexpr int HP = H / 4;           // float4 pieces per H row
  // 64-row tile of four wave sub-tiles; the tile is the only large region:
  // H=32 22 KB, H=64 38 KB, H=128 71 KB of the 160 KiB
  static constexpr int TILE = 64;
  static constexpr int THREADS = 256;
};

__device__ __forceinline__ float silu(float x) {
  return x / (1.f + __expf(-x));
}

// keeps LICM from hoisting every phase's weight fragments into registers
__device__ __forceinline__ const float* opaque(const float* p) {
  asm volatile("" : "+v"(p));
  return p;
}

// acc[NT] += A[16 x 16*KSTEPS] (LDS, this wave's rows at `a`, row stride
// a_stride floats) @ W^T. The weights W [16*NT][16*KSTEPS] come from global
// memory (L2-resident, shared by every block) in FRAGMENT ORDER
// wf[kk][nt][lane] = float4 W[nt*16 + (lane&15)][kk*16 + (lane>>4)*4 ..+3]
// (host side: frag_weight / ops.prep "frag16_f32"), so one wave load is 1 KiB
// contiguous, eight whole cache lines; row-major weights cost sixteen
// half-used lines per load, and with every wave streaming all the weights
// the vector L1 was the limit. Two accumulators alternate, so no MFMA waits
// on the one before it (40-cycle dependent latency against 32-cycle issue).
template <int KSTEPS, int NT>
__device__ __forceinline__ void mm(const float* a, int a_stride,
                                   const float* __restrict__ w, int lane,
                                   f32x4 (&acc)[NT]) {
  static_assert(NT % 2 == 0, "accumulators are taken in pairs");
  const float* arow = a + (lane & 15) * a_stride + (lane >> 4) * 4;
  const f32x4* wf = reinterpret_cast<const f32x4*>(w) + lane;
  __builtin_amdgcn_s_setprio(1);
#pragma unroll 2
  for (int kk = 0; kk < KSTEPS; ++kk) {
    f32x4 av = *reinterpret_cast<const f32x4*>(arow + kk * 16);
#pragma unroll
    for (int nt = 0; nt < NT; nt += 2) {
      f32x4 b0 = wf[(kk * NT + nt) * 64];
      f32x4 b1 = wf[(kk * NT + nt + 1) * 64];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b0[j], acc[nt],
                                                       0, 0, 0);
        acc[nt + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av[j], b1[j], acc[nt + 1], 0, 0, 0);
      }
    }
  }
  __builtin_amdgcn_s_setprio(0);
}

// dst[row][c] = silu(acc + bias[c]) for this wave's 16 rows (C/D layout)
template <int NT>
__device__ __forceinline__ void epi_silu(float* dst, int stride,
                                         const float* bias, int lane,
                                         const f32x4 (&acc)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int c = nt * 16 + (lane & 15);
    float bb = bias[c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dst[((lane >> 4) * 4 + r) * stride + c] = silu(acc[nt][r] + bb);
  }
}

// p[row] = sum_c silu(acc + bias[c]) * wv[c]; lanes with (lane & 15) == 0
// hold the four rows (lane >> 4) * 4 + r in part[r]. Fixed shuffle tree:
// the sum order does not depend on the launch.
template <int NT>
__device__ __forceinline__ void epi_head(const float* bias, const float* wv,
                                         int lane, const f32x4 (&acc)[NT],
                                         float (&part)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) part[r] = 0.f;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    int c = nt * 16 + (lane & 15);
    float bb = bias[c], ww = wv[c];
#pragma unroll
    for (int r = 0; r < 4; ++r) part[r] += silu(acc[nt][r] + bb) * ww;
  }
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[r] += __shfl_xor(part[r], off, 64);
}

// ---- host side ------------------------------------------------------------
inline bool f32_cuda(const torch::Tensor& t) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat;
}

// [H, k] (k <= k_pad, k_pad % 16 == 0) -> fragment order [k_pad/16][H/16]
// [64][4] of mm(), columns zero padded to k_pad. ops/prep.py "frag16_f32"
// is the cached python twin.
inline torch::Tensor frag_weight(const torch::Tensor& w, long k_pad) {
  long hdim = w.size(0);
  auto p = torch::constant_pad_nd(w.contiguous(), {0, k_pad - w.size(1)});
  return p.view({hdim / 16, 16, k_pad / 16, 4, 4})
      .permute({2, 0, 3, 1, 4})
      .contiguous();
}

// a weight of mm() as the kernel reads it: fp32, contiguous, hdim * k_pad
inline bool frag_ok(const torch::Tensor& w, long hdim, long k_pad) {
  return f32_cuda(w) && w.is_contiguous() && w.numel() == hdim * k_pad;
}

}  // namespace f32blk
