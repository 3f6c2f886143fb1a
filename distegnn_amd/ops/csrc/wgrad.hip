// Split-K weight-gradient kernels: dW = g^T @ x for tall-skinny activations.
//
// Shapes: g [M, 64] bf16 (layer-output grad), x [M, I<=208] bf16
// (activation), M ~ 10^5..10^6. hipBLASLt's heuristic picks a non-split-K
// kernel here (6 workgroups on 256 CUs, 2.9 ms measured); torch's bmm
// split-K workaround costs 2.6 ms of HOST time per call re-running the
// batched-GEMM heuristic. These kernels own the shape:
//
// * wgrad_splitk: each block reduces one row chunk ("slab") with
//   mfma_f32_16x16x32_bf16. g and x are staged ROW-MAJOR into LDS with
//   16-byte stores and the MFMA operands are gathered with the transposed
//   LDS read ds_read_b64_tr_b16, so there is no hand transpose. LDS is
//   double-buffered (one barrier per staging round) and two rounds of
//   global loads are in flight per block (two register sets).
// * wgrad_combine: ONE launch folds the [n_slabs, 64, IP] fp32 slabs in a
//   fixed order (16 waves each own a contiguous slab range, then a fixed
//   16-term fold through LDS) -> run-to-run bit-identical.
//
// Both take up to MAX_GROUP problems per launch, described by value in the
// kernel arguments (safe under hipGraph capture). The split plan
// (chunk rows, slab count, staging round) is make_plan() below, exported
// as ext.wgrad_plan so tests and docs read it instead of repeating it.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <tuple>
#include <vector>

#include "common.h"

namespace {

constexpr int O_DIM = 64;       // rows of dW (layer width) — fixed
constexpr int THREADS = 256;    // 4 waves
constexpr int MAX_GROUP = 4;    // problems per launch
// Split plan: at most MAX_SLABS slabs (2 blocks per CU), at least
// MIN_CHUNK rows per slab so the fp32 slab traffic follows M.
constexpr int MAX_SLABS = 512;
constexpr int MIN_CHUNK = 448;
// LDS row strides in bf16 elements. A transposed read takes, per 32-lane
// half, eight consecutive image rows x 16 B; with a row stride of 8*odd
// dwords those eight rows start on the eight distinct multiples of 8
// banks -> conflict-free (degree 1). g: 64 + 16 = 80 elements = 40 dwords;
// x: IP elements when IP/16 is odd, IP + 16 otherwise (x_stride()).
constexpr int G_STRIDE = 80;
constexpr int COMBINE_WAVES = 16;

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__host__ __device__ inline int x_stride(int ip) {
  return ((ip >> 4) & 1) ? ip : ip + 16;
}

struct Problem {
  const bf16* g;   // [m, 64]
  const bf16* x;   // [m, i_dim]
  float* part;     // [n_slabs, 64, ip]
  long m;
  long chunk;      // rows per slab, a multiple of the staging round
  int i_dim;
  int ip;          // 16 * ceil(i_dim / 16)
  int block0;      // first block of this problem in the launch
};

struct Group {
  Problem p[MAX_GROUP];
  int n;
};

struct CombineProblem {
  const float* part;  // [n_slabs, cols]
  float* dst;         // [cols]
  int n_slabs;
  int block0;
};

struct CombineGroup {
  CombineProblem p[MAX_GROUP];
  int n;
};

// One transposed read: the 16 lanes of group l>>4 fetch a 4-row x 16-column
// block; lane 4q+p supplies the address of row q, columns 4p..4p+3, and
// lane i receives column i with row q in element q.
__device__ __forceinline__ s16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(p));
}

// The eight k-values of a lane's MFMA fragment for the 32-row k-step at
// `p` (the lane's own row/column offset already applied): image rows
// 4*(l>>4) + {0..3} and 16 + 4*(l>>4) + {0..3}. A and B use the same
// assignment, so the k order inside the step is permuted identically on
// both operands. Taking rows 4g.. (not 8g..) makes the two groups of a
// half read eight CONSECUTIVE rows, which the 8*odd-dword stride spreads
// over all 64 banks.
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p, int stride) {
  s16x4 lo = tr_read(p);
  s16x4 hi = tr_read(p + 16 * stride);
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// NTW = n-tiles (of 16 cols of x) per wave; wave w covers n-tiles
// [w*NTW, w*NTW+NTW). E_STEP = rows per staging round.
template <int NTW, int E_STEP>
__global__ __launch_bounds__(THREADS, NTW <= 2 ? 4 : (NTW == 3 ? 3 : 2)) void
wgrad_splitk(
    Group grp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave index as a scalar: the n-tile early-outs below must be
  // wave-uniform branches, the transposed reads need EXEC all ones
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // pick this block's problem with scalar selects (no indexed copy of the
  // argument struct -> no scratch)
  const bf16* g = grp.p[0].g;
  const bf16* x = grp.p[0].x;
  float* part = grp.p[0].part;
  long m = grp.p[0].m;
  long chunk = grp.p[0].chunk;
  int i_dim = grp.p[0].i_dim;
  int ip = grp.p[0].ip;
  int block0 = 0;
#pragma unroll
  for (int k = 1; k < MAX_GROUP; ++k) {
    if (k < grp.n && (int)blockIdx.x >= grp.p[k].block0) {
      g = grp.p[k].g;
      x = grp.p[k].x;
      part = grp.p[k].part;
      m = grp.p[k].m;
      chunk = grp.p[k].chunk;
      i_dim = grp.p[k].i_dim;
      ip = grp.p[k].ip;
      block0 = grp.p[k].block0;
    }
  }
  const int slab = (int)blockIdx.x - block0;
  const int itiles = ip >> 4;
  const int xs = x_stride(ip);
  const int cpw = ip >> 3;  // 16-byte chunks per x row

  // LDS: two buffers of { G [E_STEP][G_STRIDE], X [E_STEP][xs] } bf16
  __bf16* lds = reinterpret_cast<__bf16*>(smem);
  const int buf_elems = E_STEP * (G_STRIDE + xs);

  const long c0 = (long)slab * chunk;
  const long c1 = c0 + chunk < m ? c0 + chunk : m;

  constexpr int GITER = E_STEP * (O_DIM / 8) / THREADS;
  constexpr int XITER = (E_STEP * NTW * 8 + THREADS - 1) / THREADS;
  static_assert(E_STEP * (O_DIM / 8) % THREADS == 0, "g staging is exact");

  // per-thread staging coordinates are the same every round
  int xe[XITER], xi8[XITER];
#pragma unroll
  for (int it = 0; it < XITER; ++it) {
    int idx = tid + it * THREADS;
    int e = idx / cpw;
    xe[it] = e < E_STEP ? e : E_STEP;  // E_STEP = "no chunk for me"
    xi8[it] = (idx - e * cpw) * 8;
  }

  struct Regs {
    bf16x8 g[GITER];
    bf16x8 x[XITER];
  };

  // global -> registers; rows at or past c1 (and whole rounds past it)
  // load nothing and stage zeros
  auto load = [&](Regs& r, long e0) {
    long left = c1 - e0;
    int ne = left < 0 ? 0 : (left < E_STEP ? (int)left : E_STEP);
#pragma unroll
    for (int it = 0; it < GITER; ++it) {
      int idx = tid + it * THREADS;
      int e = idx >> 3;
      int o8 = (idx & 7) * 8;
      bf16x8 v = {};
      if (e < ne)
        v = *reinterpret_cast<const bf16x8*>(g + (e0 + e) * O_DIM + o8);
      r.g[it] = v;
    }
#pragma unroll
    for (int it = 0; it < XITER; ++it) {
      int e = xe[it];
      int i8 = xi8[it];
      bf16x8 v = {};
      if (e < ne) {
        if (i8 + 8 <= i_dim) {
          // 16-byte load, only 2-byte aligned when i_dim is odd
          v = *reinterpret_cast<const bf16x8*>(x + (e0 + e) * i_dim + i8);
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            int i = i8 + u;
            v[u] = i < i_dim ? ((const __bf16*)x)[(e0 + e) * i_dim + i]
                             : (__bf16)0.f;
          }
        }
      }
      r.x[it] = v;
    }
  };

  // registers -> LDS, row-major, one 16-byte store per chunk
  auto store = [&](const Regs& r, int b) {
    __bf16* gi = lds + b * buf_elems;
    __bf16* xi = gi + E_STEP * G_STRIDE;
#pragma unroll
    for (int it = 0; it < GITER; ++it) {
      int idx = tid + it * THREADS;
      *reinterpret_cast<bf16x8*>(gi + (idx >> 3) * G_STRIDE + (idx & 7) * 8) =
          r.g[it];
    }
#pragma unroll
    for (int it = 0; it < XITER; ++it) {
      if (xe[it] < E_STEP)
        *reinterpret_cast<bf16x8*>(xi + xe[it] * xs + xi8[it]) = r.x[it];
    }
  };

  f32x4 acc[4][NTW] = {};

  // D[o][i] += G[e][o] * X[e][i] — A rows = o, B cols = i, K = e
  const int frag_row = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int frag_col = 4 * (lane & 3);
  auto mfma = [&](int b) {
    const __bf16* gi = lds + b * buf_elems;
    const __bf16* xi = gi + E_STEP * G_STRIDE;
#pragma unroll
    for (int kk = 0; kk < E_STEP / 32; ++kk) {
      int row = kk * 32 + frag_row;
      bf16x8 a[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        a[mt] = tr_frag(gi + row * G_STRIDE + mt * 16 + frag_col, G_STRIDE);
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        if (wave * NTW + nt >= itiles) break;  // wave-uniform
        bf16x8 bfr =
            tr_frag(xi + row * xs + (wave * NTW + nt) * 16 + frag_col, xs);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[mt], bfr, acc[mt][nt], 0, 0, 0);
      }
    }
  };

  // Round r is staged into buffer r&1. While round r is in its MFMA phase,
  // the loads of rounds r+1 and r+2 are in flight (register sets rb, ra);
  // one barrier per round separates a buffer's readers from its next
  // writers. Plain global loads survive __syncthreads().
  Regs ra, rb;
  load(ra, c0);
  load(rb, c0 + E_STEP);
  store(ra, 0);
  load(ra, c0 + 2 * E_STEP);
  __syncthreads();
  for (long e0 = c0; e0 < c1; e0 += 2 * E_STEP) {
    mfma(0);
    store(rb, 1);
    load(rb, e0 + 3 * E_STEP);
    __syncthreads();
    if (e0 + E_STEP < c1) mfma(1);  // block-uniform
    store(ra, 0);
    load(ra, e0 + 4 * E_STEP);
    __syncthreads();
  }

  // write slab [64][ip]: C layout col=l&15(+16*(w*NTW+nt)), row=(l>>4)*4+r
  float* out = part + (long)slab * O_DIM * ip;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    if (wave * NTW + nt >= itiles) break;
    int i = (wave * NTW + nt) * 16 + (lane & 15);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int o = mt * 16 + (lane >> 4) * 4 + r;
        out[o * ip + i] = acc[mt][nt][r];
      }
    }
  }
}

// Slab combine, one launch per call or group. A block owns 128 adjacent
// columns (one float2 per lane); wave w adds slabs [w*per, (w+1)*per) in
// ascending order, eight independent loads at a time, and wave 0 folds the
// 16 wave sums in ascending order. The order depends only on n_slabs.
__global__ __launch_bounds__(COMBINE_WAVES * 64) void wgrad_combine(
    CombineGroup grp) {
  __shared__ float2 fold[COMBINE_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const float* part = grp.p[0].part;
  float* dst = grp.p[0].dst;
  int n_slabs = grp.p[0].n_slabs;
  int block0 = 0;
  int next0 = grp.n > 1 ? grp.p[1].block0 : (int)gridDim.x;
#pragma unroll
  for (int k = 1; k < MAX_GROUP; ++k) {
    if (k < grp.n && (int)blockIdx.x >= grp.p[k].block0) {
      part = grp.p[k].part;
      dst = grp.p[k].dst;
      n_slabs = grp.p[k].n_slabs;
      block0 = grp.p[k].block0;
      next0 = k + 1 < grp.n ? grp.p[k + 1].block0 : (int)gridDim.x;
    }
  }
  // the problem's blocks tile its columns exactly: cols = 128 * nblocks
  const long cols = 128L * (next0 - block0);
  const long col = 128L * ((int)blockIdx.x - block0) + 2 * lane;
  const int per = (n_slabs + COMBINE_WAVES - 1) / COMBINE_WAVES;
  int s = wave * per;
  const int s1 = s + per < n_slabs ? s + per : n_slabs;
  const float* src = part + col;
  float2 acc = make_float2(0.f, 0.f);
  for (; s + 8 <= s1; s += 8) {
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v[u] = *reinterpret_cast<const float2*>(src + (long)(s + u) * cols);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x += v[u].x;
      acc.y += v[u].y;
    }
  }
  for (; s < s1; ++s) {
    float2 v = *reinterpret_cast<const float2*>(src + (long)s * cols);
    acc.x += v.x;
    acc.y += v.y;
  }
  fold[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) {
    float2 t = fold[0][lane];
#pragma unroll
    for (int w = 1; w < COMBINE_WAVES; ++w) {
      t.x += fold[w][lane].x;
      t.y += fold[w][lane].y;
    }
    *reinterpret_cast<float2*>(dst + col) = t;
  }
}

struct Plan {
  long chunk;    // rows per slab
  long n_slabs;
  int round;     // rows per staging round
  int ntw;       // kernel template: n-tiles per wave
  int ip;
};

// The one place the split is decided. tests/test_wgrad_family_gpu.py reads
// it through ext.wgrad_plan; the `_chunk_len` of
// tests/test_linear_path_gpu.py is an older formula that now only supplies
// probe positions and need not follow this one.
Plan make_plan(long m, int i_dim) {
  Plan p;
  p.ip = ((i_dim + 15) / 16) * 16;
  p.ntw = (p.ip / 16 + 3) / 4;
  // the narrow template spends few registers per round: a 64-row round
  // keeps 2 x 16 KB of loads in flight per block
  p.round = p.ntw == 1 ? 64 : 32;
  long chunk = (m + MAX_SLABS - 1) / MAX_SLABS;
  if (chunk < MIN_CHUNK) chunk = MIN_CHUNK;
  p.chunk = (chunk + p.round - 1) / p.round * p.round;
  p.n_slabs = (m + p.chunk - 1) / p.chunk;
  return p;
}

template <int NTW, int E_STEP>
void launch_splitk(const Group& grp, int blocks, int max_ip,
                   hipStream_t stream) {
  int smem = 2 * E_STEP * (G_STRIDE + x_stride(max_ip)) * 2;
  wgrad_splitk<NTW, E_STEP><<<blocks, THREADS, smem, stream>>>(grp);
}

}  // namespace

std::tuple<int64_t, int64_t, int64_t> wgrad_plan(int64_t m, int64_t i_dim) {
  TORCH_CHECK(m >= 0 && i_dim >= 1 && i_dim <= 208,
              "wgrad kernel supports 1<=I<=208");
  Plan p = make_plan(m, (int)i_dim);
  return {p.chunk, p.n_slabs, p.round};
}

std::vector<torch::Tensor> wgrad_splitk_group_launch(
    std::vector<torch::Tensor> gs, std::vector<torch::Tensor> xs) {
  const int n = (int)gs.size();
  TORCH_CHECK(n >= 1 && n <= MAX_GROUP && xs.size() == gs.size(),
              "wgrad group takes 1..4 (g, x) pairs");
  std::vector<torch::Tensor> gc(n), xc(n), dw(n);
  std::vector<Plan> plan(n);
  long part_elems = 0;
  for (int k = 0; k < n; ++k) {
    TORCH_CHECK(gs[k].is_cuda() && gs[k].scalar_type() == torch::kBFloat16,
                "g must be CUDA bf16");
    TORCH_CHECK(xs[k].is_cuda() && xs[k].scalar_type() == torch::kBFloat16,
                "x must be CUDA bf16");
    TORCH_CHECK(gs[k].dim() == 2 && xs[k].dim() == 2 &&
                    gs[k].size(0) == xs[k].size(0),
                "g and x must be [M, 64] and [M, I]");
    TORCH_CHECK(gs[k].size(1) == O_DIM, "wgrad kernel requires out width 64");
    TORCH_CHECK(xs[k].size(1) >= 1 && xs[k].size(1) <= 208,
                "wgrad kernel supports 1<=I<=208");
    gc[k] = gs[k].contiguous();
    xc[k] = xs[k].contiguous();
    plan[k] = make_plan(gc[k].size(0), (int)xc[k].size(1));
    if (plan[k].n_slabs > 1)
      part_elems += plan[k].n_slabs * O_DIM * plan[k].ip;
  }
  auto f32 = gs[0].options().dtype(torch::kFloat);
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor part;
  if (part_elems) part = torch::empty({part_elems}, f32);

  Group sk[4];  // one split-K launch per kernel template (ntw 1..4)
  int sk_blocks[4] = {0, 0, 0, 0};
  int sk_ip[4] = {0, 0, 0, 0};
  for (auto& s : sk) s.n = 0;
  CombineGroup cg;
  cg.n = 0;
  int cg_blocks = 0;
  long part_off = 0;
  for (int k = 0; k < n; ++k) {
    const Plan& pl = plan[k];
    int i_dim = (int)xc[k].size(1);
    // no rows: a 0-block problem has nothing to launch — the gradient of
    // nothing is zero
    if (pl.n_slabs == 0) {
      dw[k] = torch::zeros({(long)O_DIM, (long)i_dim}, f32);
      continue;
    }
    dw[k] = torch::empty({(long)O_DIM, (long)pl.ip}, f32);
    float* dst = dw[k].data_ptr<float>();
    float* slabs = dst;  // a single slab IS the result
    if (pl.n_slabs > 1) {
      slabs = part.data_ptr<float>() + part_off;
      part_off += pl.n_slabs * O_DIM * pl.ip;
      CombineProblem& c = cg.p[cg.n++];
      c.part = slabs;
      c.dst = dst;
      c.n_slabs = (int)pl.n_slabs;
      c.block0 = cg_blocks;
      cg_blocks += O_DIM * pl.ip / 128;
    }
    int t = pl.ntw - 1;
    Problem& p = sk[t].p[sk[t].n++];
    p.g = reinterpret_cast<const bf16*>(gc[k].data_ptr());
    p.x = reinterpret_cast<const bf16*>(xc[k].data_ptr());
    p.part = slabs;
    p.m = gc[k].size(0);
    p.chunk = pl.chunk;
    p.i_dim = i_dim;
    p.ip = pl.ip;
    p.block0 = sk_blocks[t];
    sk_blocks[t] += (int)pl.n_slabs;
    if (pl.ip > sk_ip[t]) sk_ip[t] = pl.ip;
    dw[k] = dw[k].narrow(1, 0, i_dim);
  }
  if (sk[0].n) launch_splitk<1, 64>(sk[0], sk_blocks[0], sk_ip[0], stream);
  if (sk[1].n) launch_splitk<2, 32>(sk[1], sk_blocks[1], sk_ip[1], stream);
  if (sk[2].n) launch_splitk<3, 32>(sk[2], sk_blocks[2], sk_ip[2], stream);
  if (sk[3].n) launch_splitk<4, 32>(sk[3], sk_blocks[3], sk_ip[3], stream);
  if (cg.n)
    wgrad_combine<<<cg_blocks, COMBINE_WAVES * 64, 0, stream>>>(cg);
  return dw;
}

torch::Tensor wgrad_splitk_launch(torch::Tensor g, torch::Tensor x) {
  return wgrad_splitk_group_launch({g}, {x})[0];
}
