// Fused FastEGNN node block, forward only, all fp32 (gfx950).
//
// The forward of fused_node.hip without its bf16 rounding points, one row
// per node:
//   z1    = [h | agg_e | agg_v | attr] W1^T + b1     t1 = SiLU(z1)
//   h_out = h + (t1 W2^T + b2)
//   zv    = h Wv1^T + bv1      phiv = SiLU(zv) . wv2 + bv2
// with fp32 inputs, fp32 LDS tiles, the exact f32-in / f32-accumulate MFMA
// and fp32 outputs h_out [N,H], phiv [N,1]. The vel-only form (a layer whose
// feature update is skipped) computes phiv alone and never reads agg_e,
// agg_v, attr or the node_mlp weights. This is the no-grad (evaluation)
// path: nothing is saved for a backward. No atomics and a fixed reduction
// order: bitwise reproducible. MFMA operand order: mfma_f32.h.
//
// Row layout of the tile (Dims<H, 3>, K_STRIDE = 3H + 20 floats, for every
// node_attr_nf; the vel-only form holds h alone at K_STRIDE = H + 20):
//   [0, H)        h      GEMM1 input, vel-chain input, residual
//   [H, 2H)       agg_e  GEMM1 input
//   [2H, 3H)      agg_v  GEMM1 input
//   [3H, 3H+16)   attr, zero padded: the extra k-step of GEMM1, present and
//                 read only when node_attr_nf > 0
// h is needed three times, so nothing is ever written over [0, H). Order of
// the phases of one wave on its 16 rows:
//   1. vel chain: reads [0, H), phiv goes to global
//   2. GEMM1:     reads [0, 3H) or [0, 3H+16); then t1 -> [H, 2H) (agg_e is
//                 consumed)
//   3. GEMM2:     reads t1 at [H, 2H); then h_out = [0, H) + acc + b2
//                 -> [2H, 3H) (agg_v is consumed)
//   4. store:     [2H, 3H) -> h_out, float4 rows
// No phase reads input columns that an earlier phase has written over.
//
// LDS: a 64-row tile (four wave sub-tiles) is 29,696 B at H=32, 54,272 B at
// H=64 and 103,424 B at H=128, plus 4H floats of biases. At H=128 that is
// one block, four waves, per CU, so the full H=128 form runs 32-row tiles of
// two waves instead (51,712 B, three blocks and six waves per CU), which
// measured faster; every other form keeps 64 rows. docs/KERNELS.md has the
// figures.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "mfma_f32.h"

namespace {

using namespace f32blk;

constexpr int AMAX = 8;
constexpr int GRID_CAP = 4096;  // blocks; further tiles by grid stride

template <int H, bool VEL_ONLY>
struct NodeSmem {
  using D = Dims<H, VEL_ONLY ? 1 : 3>;
  // rows per block, one wave per 16: the full H=128 form takes two waves
  // (three blocks per CU) instead of four (one block per CU)
  static constexpr int TILE = (H == 128 && !VEL_ONLY) ? 32 : D::TILE;
  static constexpr int THREADS = TILE * 4;
  static constexpr int tile = 0;                            // [TILE][K_STRIDE]
  static constexpr int bias = tile + TILE * D::K_STRIDE * 4;     // [4*H]
  static constexpr int total = bias + 4 * H * 4;
  static_assert(total <= 160 * 1024, "tile does not fit the 160 KiB LDS");
};

// ATTR: node_attr_nf > 0, i.e. GEMM1 runs the extra k-step over the tail
template <int H, bool ATTR, bool VEL_ONLY>
__global__ __launch_bounds__(256) void fused_node_fwd_f32(
    const float* __restrict__ h,        // [N,H]
    const float* __restrict__ agg_e,    // [N,H]   (not read when VEL_ONLY)
    const float* __restrict__ agg_v,    // [N,H]   (not read when VEL_ONLY)
    const float* __restrict__ attr,     // [N,adim] (read when ATTR)
    const float* __restrict__ w1p,      // w1p [H][3H (+16)], w2, wv1 in mm()'s
                                        // fragment order
    const float* __restrict__ w2, const float* __restrict__ wv1,
    const float* __restrict__ b1, const float* __restrict__ b2,
    const float* __restrict__ bv1, const float* __restrict__ wv2,
    const float* __restrict__ bv2,      // [1]
    float* __restrict__ h_out,          // [N,H]   (not written when VEL_ONLY)
    float* __restrict__ phiv_out,       // [N]
    long n_rows, int adim) {
  using D = Dims<H, VEL_ONLY ? 1 : 3>;
  using L = NodeSmem<H, VEL_ONLY>;
  constexpr int K_STRIDE = D::K_STRIDE, NT = D::NT, HP = D::HP,
                TILE = L::TILE;
  constexpr int NBLK = VEL_ONLY ? 1 : 3;
  constexpr int K1STEPS = 3 * H / 16 + (ATTR ? 1 : 0);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  float* biases = reinterpret_cast<float*>(smem + L::bias);
  for (int i = tid; i < H; i += L::THREADS) {
    if constexpr (!VEL_ONLY) {
      biases[i] = b1[i];
      biases[H + i] = b2[i];
    }
    biases[2 * H + i] = bv1[i];
    biases[3 * H + i] = wv2[i];
  }
  __syncthreads();
  const float bv2v = bv2[0];

  // this wave's 16 rows of the tile
  float* wt = reinterpret_cast<float*>(smem + L::tile) + wave * 16 * K_STRIDE;

  for (long tile = blockIdx.x; tile * TILE < n_rows; tile += gridDim.x) {
    const long r0 = tile * TILE + wave * 16;   // this wave's first row
    const long left = n_rows - r0;
    const int nrow = left >= 16 ? 16 : (left > 0 ? (int)left : 0);

    // load [h | agg_e | agg_v] (rows past the end are zero)
    for (int idx = lane; idx < 16 * NBLK * HP; idx += 64) {
      int e = idx / (NBLK * HP), piece = idx % (NBLK * HP);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < nrow) {
        const float* src = piece < HP ? h : (piece < 2 * HP ? agg_e : agg_v);
        v = *reinterpret_cast<const f32x4*>(src + (r0 + e) * H +
                                            (piece % HP) * 4);
      }
      *reinterpret_cast<f32x4*>(wt + e * K_STRIDE + piece * 4) = v;
    }
    if constexpr (ATTR && !VEL_ONLY) {
      if (lane < 16) {
        // tail: attr row, zeros up to 3H+16 (adim <= AMAX < 16)
        float* trow = wt + lane * K_STRIDE + 3 * H;
#pragma unroll
        for (int k = 0; k < 16; ++k) trow[k] = 0.f;
        if (lane < nrow) {
          const float* ar = attr + (r0 + lane) * adim;
          for (int j = 0; j < adim; ++j) trow[j] = ar[j];
        }
      }
    }

    {  // vel chain on [0, H) -> phiv
      f32x4 acc[NT] = {};
      mm<H / 16, NT>(wt, K_STRIDE, opaque(wv1), lane, acc);
      float part[4];
      epi_head<NT>(biases + 2 * H, biases + 3 * H, lane, acc, part);
      if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int e = (lane >> 4) * 4 + r;
          if (e < nrow) phiv_out[r0 + e] = part[r] + bv2v;
        }
      }
    }
    if constexpr (!VEL_ONLY) {
      {  // GEMM1 over the whole row -> t1 over the agg_e columns [H, 2H)
        f32x4 acc[NT] = {};
        mm<K1STEPS, NT>(wt, K_STRIDE, opaque(w1p), lane, acc);
        epi_silu<NT>(wt + H, K_STRIDE, biases, lane, acc);
      }
      {  // GEMM2 on t1 -> h + out over the agg_v columns [2H, 3H)
        f32x4 acc[NT] = {};
        mm<H / 16, NT>(wt + H, K_STRIDE, opaque(w2), lane, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          int c = nt * 16 + (lane & 15);
          float bb = biases[H + c];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* row = wt + ((lane >> 4) * 4 + r) * K_STRIDE;
            row[2 * H + c] = row[c] + (acc[nt][r] + bb);
          }
        }
      }
      for (int idx = lane; idx < 16 * HP; idx += 64) {
        int e = idx / HP;
        if (e >= nrow) continue;
        int c4 = (idx % HP) * 4;
        *reinterpret_cast<f32x4*>(h_out + (r0 + e) * H + c4) =
            *reinterpret_cast<const f32x4*>(wt + e * K_STRIDE + 2 * H + c4);
      }
    }
  }
}

bool f32_contig(const torch::Tensor& t) {
  return f32_cuda(t) && t.is_contiguous();
}

// contiguous CUDA fp32 of exactly this shape
void check_f32(const torch::Tensor& t, std::initializer_list<long> shape,
               const char* name, const char* what) {
  bool ok = f32_cuda(t) && t.is_contiguous() &&
            t.dim() == (long)shape.size();
  if (ok) {
    long i = 0;
    for (long s : shape) ok = ok && t.size(i++) == s;
  }
  TORCH_CHECK(ok, name, " must be a contiguous CUDA fp32 ", what, " tensor");
}

}  // namespace

// prepped: w1, w2, wv1 in fragment order (frag_weight / ops.prep
// "frag16_f32"), then b1, b2, bv1, wv2, bv2 as contiguous fp32. vel_only
// reads h, wv1, bv1, wv2, bv2 alone; every other operand may be None.
std::vector<torch::Tensor> fused_node_forward_f32(
    torch::Tensor h, c10::optional<torch::Tensor> agg_e,
    c10::optional<torch::Tensor> agg_v, c10::optional<torch::Tensor> attr,
    c10::optional<torch::Tensor> w1, c10::optional<torch::Tensor> b1,
    c10::optional<torch::Tensor> w2, c10::optional<torch::Tensor> b2,
    torch::Tensor wv1, torch::Tensor bv1, torch::Tensor wv2,
    torch::Tensor bv2, bool vel_only, std::vector<torch::Tensor> prepped) {
  TORCH_CHECK(f32_cuda(h) && h.dim() == 2 && h.is_contiguous(),
              "h must be a contiguous CUDA fp32 [N, hidden_nf] tensor");
  const long n = h.size(0);
  const long hdim = h.size(1);
  TORCH_CHECK(hdim == 32 || hdim == 64 || hdim == 128,
              "fused fp32 node kernel is compiled for hidden_nf in "
              "{32, 64, 128}, got ", hdim);
  long adim = 0;
  if (!vel_only && attr.has_value()) {
    TORCH_CHECK(attr->dim() == 2, "attr must be [N, node_attr_nf]");
    adim = attr->size(1);
  }
  TORCH_CHECK(adim <= AMAX, "fused fp32 node kernel covers node_attr_nf <= 8, "
              "got ", adim);
  const long k_in = 3 * hdim + adim;
  const long k_pad = (k_in + 15) / 16 * 16;
  torch::Tensor w1p, w2c, b1c, b2c;
  if (!vel_only) {
    TORCH_CHECK(agg_e.has_value() && agg_v.has_value() && w1.has_value() &&
                    b1.has_value() && w2.has_value() && b2.has_value(),
                "agg_e, agg_v and the node_mlp weights may be None only "
                "with vel_only");
    check_f32(*agg_e, {n, hdim}, "agg_e", "[N, hidden_nf]");
    check_f32(*agg_v, {n, hdim}, "agg_v", "[N, hidden_nf]");
    if (adim > 0) check_f32(*attr, {n, adim}, "attr", "[N, node_attr_nf]");
    TORCH_CHECK(f32_contig(*w1) && f32_contig(*b1) && f32_contig(*w2) &&
                    f32_contig(*b2),
                "w1, b1, w2 and b2 must be contiguous CUDA fp32");
    TORCH_CHECK(w1->dim() == 2 && w1->size(0) == hdim && w1->size(1) == k_in,
                "w1 must be [hidden_nf, 3*hidden_nf+node_attr_nf] = [", hdim,
                ", ", k_in, "]");
    TORCH_CHECK(w2->dim() == 2 && w2->size(0) == hdim && w2->size(1) == hdim,
                "w2 must be [hidden_nf, hidden_nf]");
  }
  TORCH_CHECK(f32_contig(wv1) && f32_contig(bv1) && f32_contig(wv2) &&
                  f32_contig(bv2),
              "wv1, bv1, wv2 and bv2 must be contiguous CUDA fp32");
  TORCH_CHECK(wv1.dim() == 2 && wv1.size(0) == hdim && wv1.size(1) == hdim,
              "wv1 must be [hidden_nf, hidden_nf]");
  auto hout = torch::empty({vel_only ? 0 : n, hdim}, h.options());
  auto phiv = torch::empty({n, 1}, h.options());
  if (n == 0) return {hout, phiv};
  torch::Tensor wv1c, bv1c, wv2c, bv2c;
  if (!prepped.empty()) {
    TORCH_CHECK(prepped.size() == 8, "node fwd prepped wants 8 tensors");
    w1p = prepped[0]; w2c = prepped[1]; wv1c = prepped[2];
    b1c = prepped[3]; b2c = prepped[4]; bv1c = prepped[5];
    wv2c = prepped[6]; bv2c = prepped[7];
  } else {
    if (!vel_only) {
      w1p = frag_weight(*w1, k_pad);
      w2c = frag_weight(*w2, hdim);
      b1c = b1->contiguous(); b2c = b2->contiguous();
    }
    wv1c = frag_weight(wv1, hdim);
    bv1c = bv1.contiguous(); wv2c = wv2.contiguous();
    bv2c = bv2.contiguous();
  }
  // the kernel reads all of these as fp32 of exactly these sizes
  if (!vel_only) {
    TORCH_CHECK(frag_ok(w1p, hdim, k_pad),
                "w1 (fragment order) must be contiguous CUDA fp32 of "
                "hidden_nf * roundup16(3*hidden_nf+node_attr_nf) elements");
    TORCH_CHECK(frag_ok(w2c, hdim, hdim),
                "w2 (fragment order) must be contiguous CUDA fp32 of "
                "hidden_nf * hidden_nf elements");
    for (const auto& v : {b1c, b2c})
      TORCH_CHECK(f32_cuda(v) && v.is_contiguous() && v.numel() == hdim,
                  "b1/b2 must be contiguous CUDA fp32 [hidden_nf]");
  }
  TORCH_CHECK(frag_ok(wv1c, hdim, hdim),
              "wv1 (fragment order) must be contiguous CUDA fp32 of "
              "hidden_nf * hidden_nf elements");
  for (const auto& v : {bv1c, wv2c})
    TORCH_CHECK(f32_cuda(v) && v.is_contiguous() && v.numel() == hdim,
                "bv1/wv2 must be contiguous CUDA fp32 of hidden_nf elements");
  TORCH_CHECK(f32_cuda(bv2c) && bv2c.is_contiguous() && bv2c.numel() == 1,
              "bv2 must be a contiguous CUDA fp32 scalar");
  auto stream = at::hip::getCurrentHIPStream();
  // operands the vel-only form never reads stay null
  auto ptr = [](const torch::Tensor& t) -> const float* {
    return t.defined() ? t.data_ptr<float>() : nullptr;
  };
  const bool full = !vel_only;
  const float* agg_e_p = full ? ptr(*agg_e) : nullptr;
  const float* agg_v_p = full ? ptr(*agg_v) : nullptr;
  const float* attr_p = adim > 0 ? ptr(*attr) : nullptr;
  float* hout_p = full ? hout.data_ptr<float>() : nullptr;
#define LAUNCH_FWD(HH, AT, VO)                                               \
  do {                                                                       \
    auto kern = fused_node_fwd_f32<HH, AT, VO>;                              \
    using L = NodeSmem<HH, VO>;                                              \
    const int blocks =                                                       \
        (int)std::min<long>((n + L::TILE - 1) / L::TILE, GRID_CAP);          \
    kern<<<blocks, L::THREADS, L::total, stream>>>(                          \
        h.data_ptr<float>(), agg_e_p, agg_v_p, attr_p, ptr(w1p), ptr(w2c),   \
        ptr(wv1c), ptr(b1c), ptr(b2c), ptr(bv1c), ptr(wv2c), ptr(bv2c),      \
        hout_p, phiv.data_ptr<float>(), n, (int)adim);                       \
  } while (0)
#define LAUNCH_H(HH)                                                         \
  do {                                                                       \
    if (vel_only) LAUNCH_FWD(HH, false, true);                               \
    else if (adim > 0) LAUNCH_FWD(HH, true, false);                          \
    else LAUNCH_FWD(HH, false, false);                                       \
  } while (0)
  if (hdim == 32) LAUNCH_H(32);
  else if (hdim == 64) LAUNCH_H(64);
  else LAUNCH_H(128);
#undef LAUNCH_H
#undef LAUNCH_FWD
  HIP_CHECK(hipGetLastError());
  return {hout, phiv};
}
