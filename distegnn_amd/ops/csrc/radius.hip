// GPU radius graph via uniform-grid cell list (gfx950).
//
// Replaces PyG/torch_cluster radius_graph (reference
// datasets/distribute_graphs.py:43,65,79; models/SchNet.py:264) with
// unbounded max_num_neighbors semantics. Output is the directed edge list
// (i, j), i != j, ||p_i - p_j|| <= r, SORTED BY ROW with a CSR rowptr —
// the layout every downstream segment reduction expects.
//
// Pipeline (host orchestration in ext.cpp, device tensors throughout):
//  1. bounding box (torch ops); cell id per point (cell_ids kernel)
//  2. sort points by cell id (torch.sort), cell_start via searchsorted
//  3. count_kernel: per point, scan the cells within r of it (27 as a
//     rule; the range comes from cell_axis, see radius_scan), count hits
//  4. rowptr = cumsum(counts); allocate M (one host sync, unavoidable —
//     output size is data-dependent; this op runs at data build time, and
//     once per forward only for SchNet's interaction graph)
//  5. fill_kernel: write col indices at rowptr[i]

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

struct GridSpec {
  float ox, oy, oz;   // origin
  float inv_r;        // 1 / cell size
  int nx, ny, nz;     // cells per dim
};

// THE cell coordinate of a point along one axis: binning (cell_ids) and the
// scan range (radius_scan) both go through this one expression, so they
// cannot disagree. Each step (fp32 subtract, fp32 multiply by inv_r > 0,
// truncation, clamp) is monotone non-decreasing in x, hence so is the whole.
__device__ __forceinline__ int cell_axis(float x, float o, float inv_r,
                                         int nd) {
  float t = (x - o) * inv_r;
  // compare in float: t may exceed the int range (or be NaN) when the grid
  // was capped far below extent / r
  if (!(t > 0.f)) return 0;
  if (t >= (float)(nd - 1)) return nd - 1;
  return (int)t;
}

__global__ void cell_ids(const float* __restrict__ pos, long* __restrict__ cid,
                         GridSpec g, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    int ix = cell_axis(pos[i * 3], g.ox, g.inv_r, g.nx);
    int iy = cell_axis(pos[i * 3 + 1], g.oy, g.inv_r, g.ny);
    int iz = cell_axis(pos[i * 3 + 2], g.oz, g.inv_r, g.nz);
    cid[i] = ((long)ix * g.ny + iy) * g.nz + iz;
  }
}

// For point i (in SORTED order so neighbors share cache lines), scan every
// cell that can hold a neighbor; count or fill. Templated to share the loop.
//
// Scanned range, per axis: cell_axis(xi - rs) .. cell_axis(xi + rs), with
// rs = fp32(r (1 + 2^-20)). The distance test below accepts j only if
// |xi - xj| <= r (1 + 2^-22) (fp32 rounding of the difference, of the three
// squares and their sum, and of r2), which is below rs; so
// xi - rs <= xj <= xi + rs in exact arithmetic, fp32 rounding of xi -+ rs
// is monotone and leaves the representable xj on the same side, and
// cell_axis is monotone: cell(xj) lies in the range. "ix - 1 .. ix + 1"
// does NOT have this property: the rounding error of (x - o) * inv_r grows
// with the cell index, and a pair closer than r can land two cells apart.
template <bool FILL>
__global__ void radius_scan(const float* __restrict__ pos,      // [n,3] orig
                            const int* __restrict__ sorted_idx,  // [n]
                            const int* __restrict__ cell_start,  // [ncell+1]
                            const long* __restrict__ rowptr,     // [n+1]
                            long* __restrict__ out_col,          // [m]
                            int* __restrict__ count,             // [n]
                            GridSpec g, float r2, float rs, int n) {
  for (int si = blockIdx.x * blockDim.x + threadIdx.x; si < n;
       si += gridDim.x * blockDim.x) {
    int i = sorted_idx[si];
    float xi = pos[i * 3], yi = pos[i * 3 + 1], zi = pos[i * 3 + 2];
    const int x0 = cell_axis(xi - rs, g.ox, g.inv_r, g.nx);
    const int x1 = cell_axis(xi + rs, g.ox, g.inv_r, g.nx);
    const int y0 = cell_axis(yi - rs, g.oy, g.inv_r, g.ny);
    const int y1 = cell_axis(yi + rs, g.oy, g.inv_r, g.ny);
    const int z0 = cell_axis(zi - rs, g.oz, g.inv_r, g.nz);
    const int z1 = cell_axis(zi + rs, g.oz, g.inv_r, g.nz);
    int c = 0;
    long base = FILL ? rowptr[i] : 0;
    for (int jx = x0; jx <= x1; ++jx) {
      for (int jy = y0; jy <= y1; ++jy) {
        // cells jz = z0..z1 are adjacent in the table: one run of points
        long cell = ((long)jx * g.ny + jy) * g.nz;
        for (int sj = cell_start[cell + z0]; sj < cell_start[cell + z1 + 1];
             ++sj) {
          int j = sorted_idx[sj];
          if (j == i) continue;
          float ddx = xi - pos[j * 3];
          float ddy = yi - pos[j * 3 + 1];
          float ddz = zi - pos[j * 3 + 2];
          if (ddx * ddx + ddy * ddy + ddz * ddz <= r2) {
            if (FILL) out_col[base + c] = j;
            ++c;
          }
        }
      }
    }
    if (!FILL) count[i] = c;
  }
}

}  // namespace

// returns (edge_index [2, M] row-sorted, rowptr [N+1])
std::tuple<torch::Tensor, torch::Tensor> radius_graph_gpu(torch::Tensor pos,
                                                          double r) {
  TORCH_CHECK(pos.is_cuda() && pos.dim() == 2 && pos.size(1) == 3,
              "pos must be [N,3] CUDA");
  TORCH_CHECK(r >= 0 && std::isfinite(r),
              "radius must be finite and >= 0, got ", r);
  TORCH_CHECK(pos.size(0) < (1L << 29), "radius_graph indexes with int32");
  auto p = pos.contiguous().to(torch::kFloat);
  long n = p.size(0);
  auto lopt = p.options().dtype(torch::kLong);
  auto iopt = p.options().dtype(torch::kInt);
  if (n == 0) {
    return {torch::zeros({2, 0}, lopt), torch::zeros({1}, lopt)};
  }
  auto stream = at::hip::getCurrentHIPStream();

  auto pmin = std::get<0>(p.min(0));
  auto pmax = std::get<0>(p.max(0));
  // grid geometry needs host scalars once per call (build-time op)
  auto pmin_h = pmin.cpu();
  auto pmax_h = pmax.cpu();
  const float* mn = pmin_h.data_ptr<float>();
  const float* mx = pmax_h.data_ptr<float>();
  GridSpec g;
  g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
  // Cell edge: r, but never below 2^-20 of the longest extent, so that a
  // tiny or zero r (r == 0 pairs up exact duplicates) forms neither 1/0
  // nor a cell count beyond int. Any cell edge is correct: the scan range
  // follows from r, not from the cell size.
  double ext = std::max({(double)mx[0] - mn[0], (double)mx[1] - mn[1],
                         (double)mx[2] - mn[2]});
  double edge = std::max(r, ext * (1.0 / (1 << 20)));
  if (!(edge > 0.0) || !std::isfinite((float)(1.0 / edge))) edge = 1.0;
  g.inv_r = (float)(1.0 / edge);
  auto dim = [&](float lo, float hi) {
    double d = std::floor(((double)hi - lo) / edge) + 1.0;
    return (d >= 1.0) ? (int)std::min(d, (double)(1 << 21)) : 1;
  };
  g.nx = dim(mn[0], mx[0]); g.ny = dim(mn[1], mx[1]); g.nz = dim(mn[2], mx[2]);
  // cap the cell table at ~64M entries (degenerate r): fall back by
  // coarsening the grid (correctness unaffected, only more candidates/cell)
  while ((long)g.nx * g.ny * g.nz > (1L << 26)) {
    g.inv_r *= 0.5f;
    g.nx = (g.nx + 1) / 2; g.ny = (g.ny + 1) / 2; g.nz = (g.nz + 1) / 2;
  }
  long ncell = (long)g.nx * g.ny * g.nz;

  // cell id per point (the kernels' own cell_axis) + sort
  int threads = 256;
  auto cid = torch::empty({n}, lopt);
  cell_ids<<<num_blocks(n, threads), threads, 0, stream>>>(
      p.data_ptr<float>(), cid.data_ptr<long>(), g, (int)n);
  auto sorted = cid.sort();
  auto sorted_cid = std::get<0>(sorted);
  auto sorted_idx = std::get<1>(sorted).to(torch::kInt);
  auto cell_start = torch::searchsorted(
      sorted_cid, torch::arange(ncell + 1, lopt)).to(torch::kInt);

  auto counts = torch::zeros({n}, iopt);
  float r2 = (float)(r * r);
  float rs = (float)(r * (1.0 + 1.0 / (1 << 20)));
  radius_scan<false><<<num_blocks(n, threads), threads, 0, stream>>>(
      p.data_ptr<float>(), sorted_idx.data_ptr<int>(),
      cell_start.data_ptr<int>(), nullptr, nullptr,
      counts.data_ptr<int>(), g, r2, rs, (int)n);

  auto rowptr = torch::zeros({n + 1}, lopt);
  rowptr.slice(0, 1, n + 1).copy_(counts.to(torch::kLong).cumsum(0));
  long m = rowptr[n].item<long>();  // one sync: output size

  auto col = torch::empty({m}, lopt);
  radius_scan<true><<<num_blocks(n, threads), threads, 0, stream>>>(
      p.data_ptr<float>(), sorted_idx.data_ptr<int>(),
      cell_start.data_ptr<int>(), rowptr.data_ptr<long>(),
      col.data_ptr<long>(), nullptr, g, r2, rs, (int)n);

  auto row = torch::repeat_interleave(
      torch::arange(n, lopt), rowptr.slice(0, 1, n + 1) - rowptr.slice(0, 0, n));
  return {torch::stack({row, col}), rowptr};
}
