// Fused FastEGNN virtual-edge block, forward only, all fp32 (gfx950).
//
// The inference branch of fused_virtual.hip over rows r = (node n, channel
// c), R = N*C, b = batch[n]:
//   vdiff = X[b,c] - x_n, vrad = |vdiff|
//   vin   = [h_n | Z[b,c] | vrad | gram[b,c,:]]            (K_IN = 2H+1+C)
//   t1    = SiLU(vin W1^T + b1)     vmsg = SiLU(t1 W2^T + b2)
//   pxv   = SiLU(vmsg Wxv^T + bxv) . wxvv    pX = SiLU(vmsg WX^T + bX) . wXv
//   tv    = -vdiff pxv              tx = vdiff pX
// with fp32 inputs, fp32 LDS tiles, the exact f32-in / f32-accumulate MFMA
// and fp32 outputs vmsg [R,H], tv [R,3], tx [R,3]. No pre-activations are
// saved. No atomics and a fixed reduction order: bitwise reproducible.
// Tile layout, MFMA operand order and the LDS budget: mfma_f32.h.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "mfma_f32.h"

namespace {

using namespace f32blk;

constexpr int CMAX = 8;
constexpr int GRID_CAP = 4096;  // blocks; further tiles by grid stride

template <int H>
struct VirtSmem {
  using D = Dims<H>;
  static constexpr int tile = 0;                            // [TILE][K_STRIDE]
  static constexpr int diff = tile + D::TILE * D::K_STRIDE * 4;  // [TILE][4]
  static constexpr int scal = diff + D::TILE * 16;          // [TILE][2]
  static constexpr int bias = scal + D::TILE * 8;           // [6*H]
  static constexpr int total = bias + 6 * H * 4;
};

template <int H>
__global__ __launch_bounds__(256) void fused_virtual_fwd_f32(
    const float* __restrict__ h,        // [N,H]
    const float* __restrict__ coord,    // [N,3]
    const float* __restrict__ vcoord,   // [B,C,3]
    const float* __restrict__ vfeat,    // [B,C,H]
    const float* __restrict__ gram,     // [B,C,C]
    const long* __restrict__ batch,     // [N]
    const float* __restrict__ w1p,      // [H][K_PAD] zero padded; w1p, w2,
                                        // wxv, wX in mm()'s fragment order
    const float* __restrict__ w2, const float* __restrict__ wxv,
    const float* __restrict__ wX, const float* __restrict__ b1,
    const float* __restrict__ b2, const float* __restrict__ bxv,
    const float* __restrict__ bX, const float* __restrict__ wxvv,
    const float* __restrict__ wXv,
    float* __restrict__ vmsg_out,       // [R,H]
    float* __restrict__ tv_out,         // [R,3]
    float* __restrict__ tx_out,         // [R,3]
    long n_rows, int cdim) {
  using D = Dims<H>;
  using L = VirtSmem<H>;
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
    biases[2 * H + i] = bxv[i];
    biases[3 * H + i] = bX[i];
    biases[4 * H + i] = wxvv[i];
    biases[5 * H + i] = wXv[i];
  }
  __syncthreads();

  // this wave's 16 rows of every region
  float* wt = reinterpret_cast<float*>(smem + L::tile) + wave * 16 * K_STRIDE;
  float* dptr = reinterpret_cast<float*>(smem + L::diff) + wave * 16 * 4;
  float* sc = reinterpret_cast<float*>(smem + L::scal) + wave * 16 * 2;

  for (long tile = blockIdx.x; tile * TILE < n_rows; tile += gridDim.x) {
    const long r0 = tile * TILE + wave * 16;   // this wave's first row
    const long left = n_rows - r0;
    const int nrow = left >= 16 ? 16 : (left > 0 ? (int)left : 0);

    // gather [h_n | Z[b,c]] (rows past the end are zero)
    for (int idx = lane; idx < 16 * 2 * HP; idx += 64) {
      int e = idx / (2 * HP), piece = idx % (2 * HP);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (e < nrow) {
        long r = r0 + e;
        long n = r / cdim, c = r - n * cdim;
        const float* src = piece < HP
                               ? h + n * H
                               : vfeat + (batch[n] * cdim + c) * H;
        v = *reinterpret_cast<const f32x4*>(src + (piece % HP) * 4);
      }
      *reinterpret_cast<f32x4*>(wt + e * K_STRIDE + piece * 4) = v;
    }
    if (lane < 16) {
      int e = lane;
      float* trow = wt + e * K_STRIDE;
      float dx = 0, dy = 0, dz = 0, vr = 0;
      // tail: vrad, gram row, zeros up to K_PAD (cdim <= CMAX < 16)
#pragma unroll
      for (int k = 2 * H; k < K_PAD; ++k) trow[k] = 0.f;
      if (e < nrow) {
        long r = r0 + e;
        long n = r / cdim, c = r - n * cdim;
        long b = batch[n];
        const float* X = vcoord + (b * cdim + c) * 3;
        dx = X[0] - coord[n * 3];
        dy = X[1] - coord[n * 3 + 1];
        dz = X[2] - coord[n * 3 + 2];
        vr = sqrtf(dx * dx + dy * dy + dz * dz);
        trow[2 * H] = vr;
        const float* gr = gram + (b * cdim + c) * cdim;
        for (int j = 0; j < cdim; ++j) trow[2 * H + 1 + j] = gr[j];
      }
      dptr[e * 4] = dx; dptr[e * 4 + 1] = dy; dptr[e * 4 + 2] = dz;
    }

    {  // GEMM1 -> t1 over columns [0, H) of the rows just consumed
      f32x4 acc[NT] = {};
      mm<K_PAD / 16, NT>(wt, K_STRIDE, opaque(w1p), lane, acc);
      epi_silu<NT>(wt, K_STRIDE, biases, lane, acc);
    }
    {  // GEMM2 -> vmsg over columns [H, 2H)
      f32x4 acc[NT] = {};
      mm<H / 16, NT>(wt, K_STRIDE, opaque(w2), lane, acc);
      epi_silu<NT>(wt + H, K_STRIDE, biases + H, lane, acc);
    }
#pragma unroll
    for (int head = 0; head < 2; ++head) {  // phi_xv, then phi_X
      f32x4 acc[NT] = {};
      mm<H / 16, NT>(wt + H, K_STRIDE, opaque(head == 0 ? wxv : wX), lane,
                     acc);
      float part[4];
      epi_head<NT>(biases + (2 + head) * H, biases + (4 + head) * H, lane,
                   acc, part);
      if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sc[((lane >> 4) * 4 + r) * 2 + head] = part[r];
      }
    }

    for (int idx = lane; idx < 16 * HP; idx += 64) {
      int e = idx / HP;
      if (e >= nrow) continue;
      int c4 = (idx % HP) * 4;
      *reinterpret_cast<f32x4*>(vmsg_out + (r0 + e) * H + c4) =
          *reinterpret_cast<const f32x4*>(wt + e * K_STRIDE + H + c4);
    }
    if (lane < nrow) {
      long r = r0 + lane;
      float pxv = sc[lane * 2], pX = sc[lane * 2 + 1];
      float dx = dptr[lane * 4], dy = dptr[lane * 4 + 1],
            dz = dptr[lane * 4 + 2];
      tv_out[r * 3] = -dx * pxv;
      tv_out[r * 3 + 1] = -dy * pxv;
      tv_out[r * 3 + 2] = -dz * pxv;
      tx_out[r * 3] = dx * pX;
      tx_out[r * 3 + 1] = dy * pX;
      tx_out[r * 3 + 2] = dz * pX;
    }
  }
}

}  // namespace

std::vector<torch::Tensor> fused_virtual_forward_f32(
    torch::Tensor h, torch::Tensor coord, torch::Tensor vcoord,
    torch::Tensor vfeat, torch::Tensor gram, torch::Tensor batch,
    torch::Tensor w1, torch::Tensor b1, torch::Tensor w2, torch::Tensor b2,
    torch::Tensor wxv, torch::Tensor bxv, torch::Tensor wxvv,
    torch::Tensor wX, torch::Tensor bX, torch::Tensor wXv,
    std::vector<torch::Tensor> prepped) {
  TORCH_CHECK(f32_cuda(h) && h.dim() == 2, "h must be CUDA fp32 [N,H]");
  TORCH_CHECK(f32_cuda(coord) && f32_cuda(vcoord) && f32_cuda(vfeat) &&
                  f32_cuda(gram),
              "coord, vcoord, vfeat and gram must be CUDA fp32");
  TORCH_CHECK(vcoord.dim() == 3 && vfeat.dim() == 3 && gram.dim() == 3,
              "vcoord [B,C,3], vfeat [B,C,H], gram [B,C,C]");
  long hdim = h.size(1);
  TORCH_CHECK(hdim == 32 || hdim == 64 || hdim == 128,
              "fused fp32 virtual kernel is compiled for hidden_nf in "
              "{32, 64, 128}, got ", hdim);
  long n = h.size(0);
  long cdim = vcoord.size(1);
  long nb = vcoord.size(0);
  TORCH_CHECK(cdim >= 1 && cdim <= CMAX, "virtual_channels <= 8");
  TORCH_CHECK(coord.size(0) == n && coord.size(1) == 3 &&
                  vcoord.size(2) == 3 && vfeat.size(0) == nb &&
                  vfeat.size(1) == cdim && vfeat.size(2) == hdim &&
                  gram.size(0) == nb && gram.size(1) == cdim &&
                  gram.size(2) == cdim,
              "coord [N,3], vcoord [B,C,3], vfeat [B,C,hidden_nf], "
              "gram [B,C,C]");
  TORCH_CHECK(batch.is_cuda() && batch.scalar_type() == torch::kLong &&
                  batch.numel() == n,
              "batch must be CUDA int64 [N]");
  long k_in = 2 * hdim + 1 + cdim;
  long k_pad = 2 * hdim + 16;
  long rows = n * cdim;
  auto vmsg = torch::empty({rows, hdim}, h.options());
  auto tv = torch::empty({rows, 3}, h.options());
  auto tx = torch::empty({rows, 3}, h.options());
  if (rows == 0) return {vmsg, tv, tx};
  torch::Tensor w1p, w2c, wxvc, wXc, b1c, b2c, bxvc, bXc, wxvvc, wXvc;
  if (!prepped.empty()) {
    TORCH_CHECK(prepped.size() == 10, "virtual fwd prepped wants 10");
    w1p = prepped[0]; w2c = prepped[1]; wxvc = prepped[2]; wXc = prepped[3];
    b1c = prepped[4]; b2c = prepped[5]; bxvc = prepped[6]; bXc = prepped[7];
    wxvvc = prepped[8]; wXvc = prepped[9];
  } else {
    TORCH_CHECK(w1.dim() == 2 && w1.size(0) == hdim && w1.size(1) == k_in,
                "w1 must be [hidden_nf, 2*hidden_nf+1+virtual_channels]");
    for (const auto& w : {w2, wxv, wX})
      TORCH_CHECK(w.dim() == 2 && w.size(0) == hdim && w.size(1) == hdim,
                  "w2/wxv/wX must be [hidden_nf, hidden_nf]");
    w1p = frag_weight(w1, k_pad);
    w2c = frag_weight(w2, hdim);
    wxvc = frag_weight(wxv, hdim);
    wXc = frag_weight(wX, hdim);
    b1c = b1.contiguous(); b2c = b2.contiguous();
    bxvc = bxv.contiguous(); bXc = bX.contiguous();
    wxvvc = wxvv.contiguous(); wXvc = wXv.contiguous();
  }
  // the kernel reads all of these as fp32 of exactly these sizes
  TORCH_CHECK(w1.size(1) == k_in,
              "w1 must be [hidden_nf, 2*hidden_nf+1+virtual_channels]");
  TORCH_CHECK(frag_ok(w1p, hdim, k_pad),
              "w1 (fragment order) must be contiguous CUDA fp32 of "
              "hidden_nf * (2*hidden_nf+16) elements");
  for (const auto& w : {w2c, wxvc, wXc})
    TORCH_CHECK(frag_ok(w, hdim, hdim),
                "w2/wxv/wX (fragment order) must be contiguous CUDA fp32 of "
                "hidden_nf * hidden_nf elements");
  for (const auto& v : {b1c, b2c, bxvc, bXc, wxvvc, wXvc})
    TORCH_CHECK(f32_cuda(v) && v.is_contiguous() && v.numel() == hdim,
                "biases and head vectors must be contiguous CUDA fp32 "
                "[hidden_nf]");
  auto hc = h.contiguous();
  auto cc = coord.contiguous();
  auto vc = vcoord.contiguous();
  auto vf = vfeat.contiguous();
  auto gr = gram.contiguous();
  auto bp = batch.contiguous();
  auto stream = at::hip::getCurrentHIPStream();
  long tiles = (rows + 63) / 64;
  int blocks = (int)std::min<long>(tiles, GRID_CAP);
#define LAUNCH_FWD(HH)                                                       \
  fused_virtual_fwd_f32<HH><<<blocks, Dims<HH>::THREADS,                     \
                              VirtSmem<HH>::total, stream>>>(                \
      hc.data_ptr<float>(), cc.data_ptr<float>(), vc.data_ptr<float>(),      \
      vf.data_ptr<float>(), gr.data_ptr<float>(), bp.data_ptr<long>(),       \
      w1p.data_ptr<float>(), w2c.data_ptr<float>(), wxvc.data_ptr<float>(),  \
      wXc.data_ptr<float>(), b1c.data_ptr<float>(), b2c.data_ptr<float>(),   \
      bxvc.data_ptr<float>(), bXc.data_ptr<float>(),                         \
      wxvvc.data_ptr<float>(), wXvc.data_ptr<float>(),                       \
      vmsg.data_ptr<float>(), tv.data_ptr<float>(), tx.data_ptr<float>(),    \
      rows, (int)cdim)
  if (hdim == 32) LAUNCH_FWD(32);
  else if (hdim == 64) LAUNCH_FWD(64);
  else LAUNCH_FWD(128);
#undef LAUNCH_FWD
  return {vmsg, tv, tx};
}
