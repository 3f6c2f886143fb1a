// Fused FastEGNN edge block, forward only, all fp32 (gfx950).
//
// The chain of fused_edge.hip, per edge e = (i = row[e], j = col[e]):
//   d = x_i - x_j, r2 = |d|^2, inv = 1/(sqrt(r2)+eps) or 1
//   ein = [h_i | h_j | r2 | a_e]                       (K_IN = 2H+3)
//   t1  = SiLU(ein W1^T + b1)     msg = SiLU(t1 W2^T + b2)
//   p   = SiLU(msg W3^T + b3) . w3v     trans = d inv p
// with fp32 inputs, fp32 LDS tiles, the exact f32-in / f32-accumulate MFMA
// and fp32 outputs msg [M,H], trans [M,3]. r2 and edge_attr enter GEMM1
// unrounded. This is the no-grad (evaluation) path: nothing is saved for a
// backward. No atomics and a fixed reduction order: bitwise reproducible.
// Tile layout, MFMA operand order and the LDS budget: mfma_f32.h.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "mfma_f32.h"

namespace {

using namespace f32blk;

constexpr int EA = 2;
constexpr int GRID_CAP = 4096;  // blocks; further tiles by grid stride

template <int H>
struct EdgeSmem {
  using D = Dims<H>;
  static constexpr int tile = 0;                            // [TILE][K_STRIDE]
  static constexpr int diff = tile + D::TILE * D::K_STRIDE * 4;  // [TILE][4]
  static constexpr int pvec = diff + D::TILE * 16;          // [TILE]
  static constexpr int bias = pvec + D::TILE * 4;           // [4*H]
  static constexpr int rows = bias + 4 * H * 4;             // [TILE] i32
  static constexpr int cols = rows + D::TILE * 4;           // [TILE] i32
  static constexpr int total = cols + D::TILE * 4;
};

template <int H>
__global__ __launch_bounds__(256) void fused_edge_fwd_f32(
    const float* __restrict__ h, const float* __restrict__ coord,
    const float* __restrict__ eattr, const long* __restrict__ row,
    const long* __restrict__ col,
    const float* __restrict__ w1p,  // [H][K_PAD] zero padded; w1p, w2 and
                                    // w3 in the fragment order of mm()
    const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, const float* __restrict__ w3v,
    float* __restrict__ msg_out, float* __restrict__ trans_out, long m,
    int normalize, float eps) {
  using D = Dims<H>;
  using L = EdgeSmem<H>;
  constexpr int K_IN = 2 * H + 1 + EA;
  constexpr int K_PAD = D::K_PAD, K_STRIDE = D::K_STRIDE, NT = D::NT,
                HP = D::HP, TILE = D::TILE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  float* biases = reinterpret_cast<float*>(smem + L::bias);
  for (int i = tid; i < H; i += D::THREADS) {
    biases[i] = b1[i];
    biases[H + i] = b2[i];
    biases[2 * H + i] = b3[i];
    biases[3 * H + i] = w3v[i];
  }
  __syncthreads();

  // this wave's 16 rows of every region
  float* wt = reinterpret_cast<float*>(smem + L::tile) + wave * 16 * K_STRIDE;
  float* dptr = reinterpret_cast<float*>(smem + L::diff) + wave * 16 * 4;
  float* pv = reinterpret_cast<float*>(smem + L::pvec) + wave * 16;
  int* rws = reinterpret_cast<int*>(smem + L::rows) + wave * 16;
  int* cls = reinterpret_cast<int*>(smem + L::cols) + wave * 16;

  // XCD-aware tile order as in fused_edge.hip: workgroup b runs on XCD
  // b % 8, and the bijective remap gives each XCD one contiguous range of
  // tiles, so its L2 holds about an eighth of the gathered rows.
  const long ntile = (m + TILE - 1) / TILE;
  const long tq = ntile >> 3, tr = ntile & 7;
  for (long vt = blockIdx.x; vt < ntile; vt += gridDim.x) {
    const long xcd = vt & 7, ti = vt >> 3;
    const long tile =
        (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + ti;
    const long e0 = tile * TILE + wave * 16;   // this wave's first edge
    const long left = m - e0;
    const int nedge = left >= 16 ? 16 : (left > 0 ? (int)left : 0);

    if (lane < 16) {
      rws[lane] = lane < nedge ? (int)row[e0 + lane] : 0;
      cls[lane] = lane < nedge ? (int)col[e0 + lane] : 0;
    }
    // gather [h_i | h_j] (rows past the end are zero)
    for (int idx = lane; idx < 16 * 2 * HP; idx += 64) {
      int e = idx / (2 * HP), piece = idx % (2 * HP);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < nedge) {
        long src = piece < HP ? rws[e] : cls[e];
        v = *reinterpret_cast<const f32x4*>(h + src * H + (piece % HP) * 4);
      }
      *reinterpret_cast<f32x4*>(wt + e * K_STRIDE + piece * 4) = v;
    }
    if (lane < 16) {
      int e = lane;
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
        if (normalize) {
          float inv = 1.f / (sqrtf(r2) + eps);
          dx *= inv; dy *= inv; dz *= inv;
        }
      }
      dptr[e * 4] = dx; dptr[e * 4 + 1] = dy; dptr[e * 4 + 2] = dz;
      float* trow = wt + e * K_STRIDE;
      trow[2 * H] = r2;
      trow[2 * H + 1] = a0;
      trow[2 * H + 2] = a1;
#pragma unroll
      for (int k = K_IN; k < K_PAD; ++k) trow[k] = 0.f;
    }

    {  // GEMM1 -> t1 over columns [0, H) of the rows just consumed
      f32x4 acc[NT] = {};
      mm<K_PAD / 16, NT>(wt, K_STRIDE, opaque(w1p), lane, acc);
      epi_silu<NT>(wt, K_STRIDE, biases, lane, acc);
    }
    {  // GEMM2 -> msg over columns [H, 2H)
      f32x4 acc[NT] = {};
      mm<H / 16, NT>(wt, K_STRIDE, opaque(w2), lane, acc);
      epi_silu<NT>(wt + H, K_STRIDE, biases + H, lane, acc);
    }
    {  // GEMM3 + head -> p
      f32x4 acc[NT] = {};
      mm<H / 16, NT>(wt + H, K_STRIDE, opaque(w3), lane, acc);
      float part[4];
      epi_head<NT>(biases + 2 * H, biases + 3 * H, lane, acc, part);
      if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[(lane >> 4) * 4 + r] = part[r];
      }
    }

    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = idx / HP;
      if (e >= nedge) continue;
      int c4 = (idx % HP) * 4;
      *reinterpret_cast<f32x4*>(msg_out + (e0 + e) * H + c4) =
          *reinterpret_cast<const f32x4*>(wt + e * K_STRIDE + H + c4);
    }
    if (lane < nedge) {
      float p = pv[lane];
      float* out = trans_out + (e0 + lane) * 3;
      out[0] = dptr[lane * 4] * p;
      out[1] = dptr[lane * 4 + 1] * p;
      out[2] = dptr[lane * 4 + 2] * p;
    }
  }
}

// ---- f32 MFMA layout probe: D = A[16x4] @ B[4x16], bt = B^T [16x4] -------
__global__ void mfma_probe_f32_kernel(const float* __restrict__ a,
                                      const float* __restrict__ bt,
                                      float* __restrict__ d) {
  int lane = threadIdx.x & 63;
  float av = a[(lane & 15) * 4 + (lane >> 4)];
  float bv = bt[(lane & 15) * 4 + (lane >> 4)];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    d[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor> fused_edge_forward_f32(
    torch::Tensor h, torch::Tensor coord, torch::Tensor eattr,
    torch::Tensor row, torch::Tensor col, torch::Tensor w1, torch::Tensor b1,
    torch::Tensor w2, torch::Tensor b2, torch::Tensor w3, torch::Tensor b3,
    torch::Tensor w3v, bool normalize, double eps,
    std::vector<torch::Tensor> prepped) {
  TORCH_CHECK(f32_cuda(h) && h.dim() == 2, "h must be CUDA fp32 [N,H]");
  TORCH_CHECK(f32_cuda(coord) && f32_cuda(eattr),
              "coord and edge_attr must be CUDA fp32");
  long hdim = h.size(1);
  TORCH_CHECK(hdim == 32 || hdim == 64 || hdim == 128,
              "fused fp32 edge kernel supports hidden_nf in {32, 64, 128}");
  TORCH_CHECK(eattr.dim() == 2 && eattr.size(1) == EA,
              "fused fp32 edge kernel requires edge_attr_nf=2");
  TORCH_CHECK(row.is_cuda() && col.is_cuda() &&
                  row.scalar_type() == torch::kLong &&
                  col.scalar_type() == torch::kLong &&
                  row.numel() == col.numel() && eattr.size(0) == row.numel(),
              "row/col must be CUDA int64 of one length, edge_attr [M,2]");
  long m = row.numel();
  auto msg = torch::empty({m, hdim}, h.options());
  auto trans = torch::empty({m, 3}, h.options());
  if (m == 0) return {msg, trans};
  long k_in = 2 * hdim + 1 + EA;
  long k_pad = 2 * hdim + 16;
  torch::Tensor w1p, w2c, w3c, b1c, b2c, b3c, w3vc;
  if (!prepped.empty()) {
    TORCH_CHECK(prepped.size() == 7, "edge fwd prepped wants 7 tensors");
    w1p = prepped[0]; w2c = prepped[1]; w3c = prepped[2];
    b1c = prepped[3]; b2c = prepped[4]; b3c = prepped[5]; w3vc = prepped[6];
  } else {
    TORCH_CHECK(w1.dim() == 2 && w1.size(0) == hdim && w1.size(1) == k_in,
                "w1 must be [hidden_nf, 2*hidden_nf+3]");
    TORCH_CHECK(w2.dim() == 2 && w2.size(0) == hdim && w2.size(1) == hdim &&
                    w3.dim() == 2 && w3.size(0) == hdim && w3.size(1) == hdim,
                "w2/w3 must be [hidden_nf, hidden_nf]");
    w1p = frag_weight(w1, k_pad);
    w2c = frag_weight(w2, hdim);
    w3c = frag_weight(w3, hdim);
    b1c = b1.contiguous(); b2c = b2.contiguous(); b3c = b3.contiguous();
    w3vc = w3v.contiguous();
  }
  // the kernel reads all of these as fp32 of exactly these sizes
  TORCH_CHECK(frag_ok(w1p, hdim, k_pad),
              "w1 (fragment order) must be contiguous CUDA fp32 of "
              "hidden_nf * (2*hidden_nf+16) elements");
  TORCH_CHECK(frag_ok(w2c, hdim, hdim) && frag_ok(w3c, hdim, hdim),
              "w2/w3 (fragment order) must be contiguous CUDA fp32 of "
              "hidden_nf * hidden_nf elements");
  for (const auto& v : {b1c, b2c, b3c, w3vc})
    TORCH_CHECK(f32_cuda(v) && v.is_contiguous() && v.numel() == hdim,
                "b1/b2/b3/w3v must be contiguous CUDA fp32 [hidden_nf]");
  auto hc = h.contiguous();
  auto cc = coord.contiguous();
  auto ec = eattr.contiguous();
  auto rc = row.contiguous();
  auto clc = col.contiguous();
  auto stream = at::hip::getCurrentHIPStream();
  long tiles = (m + 63) / 64;
  int blocks = (int)std::min<long>(tiles, GRID_CAP);
#define LAUNCH_FWD(HH)                                                       \
  fused_edge_fwd_f32<HH><<<blocks, Dims<HH>::THREADS, EdgeSmem<HH>::total,   \
                           stream>>>(                                        \
      hc.data_ptr<float>(), cc.data_ptr<float>(), ec.data_ptr<float>(),      \
      rc.data_ptr<long>(), clc.data_ptr<long>(), w1p.data_ptr<float>(),      \
      b1c.data_ptr<float>(), w2c.data_ptr<float>(), b2c.data_ptr<float>(),   \
      w3c.data_ptr<float>(), b3c.data_ptr<float>(), w3vc.data_ptr<float>(),  \
      msg.data_ptr<float>(), trans.data_ptr<float>(), m, normalize ? 1 : 0,  \
      (float)eps)
  if (hdim == 32) LAUNCH_FWD(32);
  else if (hdim == 64) LAUNCH_FWD(64);
  else LAUNCH_FWD(128);
#undef LAUNCH_FWD
  return {msg, trans};
}

torch::Tensor mfma_probe_f32(torch::Tensor a, torch::Tensor bt) {
  TORCH_CHECK(f32_cuda(a) && f32_cuda(bt) && a.dim() == 2 && bt.dim() == 2 &&
                  a.size(0) == 16 && a.size(1) == 4 && bt.size(0) == 16 &&
                  bt.size(1) == 4,
              "mfma_probe_f32: a and bt must be CUDA fp32 [16,4]");
  auto ac = a.contiguous();
  auto btc = bt.contiguous();
  auto d = torch::empty({16, 16}, a.options());
  auto stream = at::hip::getCurrentHIPStream();
  mfma_probe_f32_kernel<<<1, 64, 0, stream>>>(
      ac.data_ptr<float>(), btc.data_ptr<float>(), d.data_ptr<float>());
  return d;
}
