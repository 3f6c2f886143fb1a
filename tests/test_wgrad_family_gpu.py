"""GPU tests of the split-K weight-gradient family (csrc/wgrad.hip):
wgrad_splitk, wgrad_splitk_group, wgrad_plan and the grouped call sites of
the two fused blocks.

The split plan is read from ``ext.wgrad_plan(m, i) -> (chunk_rows, n_slabs,
round_rows)``; nothing here repeats its formula. References are float64 on
the device from the bf16 operands the kernels receive. Bounds (u23 = 2^-23,
``mag`` = the same product over absolute values):

* probe rows: every output element is one bf16 x bf16 product, exact in
  fp32, plus exact zeros -> bit-equal (bound 0)
* dense: fp32 dot product of M terms, any order -> M * u23 * mag
* group member vs single call, call vs call, replay vs eager: same plan and
  same summation order -> bit-equal
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import collate
from distegnn_amd.data.synthetic import make_cutoff_dataset
from distegnn_amd.ops import linear as L

U23 = 2.0 ** -23
DEV = "cuda:0"
WIDTHS = [1, 3, 16, 64, 67, 131, 144, 194, 208]
SMALL_M = [1, 63, 64, 65, 2085]


def _ext():
    return ops.hip_ext()


def _plan(m, i_dim):
    chunk, n_slabs, rnd = _ext().wgrad_plan(m, i_dim)
    return int(chunk), int(n_slabs), int(rnd)


def _cap_m(i_dim):
    """(smallest M at which n_slabs reaches its cap, the cap, the first M
    whose slabs are longer than the minimum). While the chunk stays at its
    minimum n_slabs grows with M; from the first longer chunk on it stays
    at or below the value reached just before."""
    c_min = _plan(1, i_dim)[0]
    lo, hi = 1, 10 ** 8           # chunk(lo) == c_min < chunk(hi)
    assert _plan(hi, i_dim)[0] > c_min
    while hi - lo > 1:            # the chunk length never shrinks with M
        mid = (lo + hi) // 2
        if _plan(mid, i_dim)[0] > c_min:
            hi = mid
        else:
            lo = mid
    cap = _plan(lo, i_dim)[1]
    cap_m = (cap - 1) * c_min + 1
    return cap_m, cap, hi


def _plan_ms(i_dim):
    """M values placed by the plan: a last slab shorter than one round, a
    slab count whose per-wave share in the combine is neither 1 nor a
    multiple of 8, the smallest M at the slab cap, one above it, and the
    first M whose slabs are longer than the minimum."""
    chunk, _, rnd = _plan(2085, i_dim)
    short_last = 5 * chunk + 7
    assert _plan(short_last, i_dim) == (chunk, 6, rnd) and 7 < rnd
    mid = 200 * chunk + 1
    assert _plan(mid, i_dim)[1] == 201
    cap_m, cap, grow_m = _cap_m(i_dim)
    assert _plan(cap_m, i_dim)[1] == cap and _plan(cap_m - 1, i_dim)[1] < cap
    return [short_last, mid, cap_m, cap_m + 1, grow_m]


def _cases():
    out = []
    for i_dim in WIDTHS:
        for m in SMALL_M + _plan_ms(i_dim):
            out.append((m, i_dim))
    return out


CASES = _cases()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16().to(DEV)


def _probe_rows(m, i_dim):
    """Up to 64 distinct rows: the ends, both sides of the first, a middle
    and the last slab boundary, both sides of a staging-round boundary
    inside a later slab, the last slab's rows, filled up at random."""
    chunk, n_slabs, rnd = _plan(m, i_dim)
    assert n_slabs == (m + chunk - 1) // chunk and chunk % rnd == 0
    want = [0, m - 1, 63, 64, 65]
    for s in {1, n_slabs // 2, n_slabs - 1}:
        if s >= 1:
            want += [s * chunk - 1, s * chunk]
    later = (n_slabs // 3) * chunk
    want += [later + rnd - 1, later + rnd, later + 2 * rnd - 1,
             later + 2 * rnd, later + 3 * rnd, later + chunk - 1]
    want += [(n_slabs - 1) * chunk + 1, m - 2]
    rows = []
    for r in want:
        if 0 <= r < m and r not in rows:
            rows.append(r)
    g = torch.Generator().manual_seed(m)
    fill = torch.randint(0, m, (256,), generator=g).tolist()
    for r in fill:
        if len(rows) >= min(64, m):
            break
        if r not in rows:
            rows.append(r)
    for r in range(m):            # tiny m: take what is left in order
        if len(rows) >= min(64, m):
            break
        if r not in rows:
            rows.append(r)
    return rows[:64]


def test_plan_follows_m():
    """chunk is a whole number of rounds, the slabs cover M exactly, and
    the slab count grows with M up to its cap instead of being fixed."""
    for i_dim in (64, 144, 208):
        seen = []
        for m in (1, 448, 2085, 113_140, 566_000, 1_650_000):
            chunk, n_slabs, rnd = _plan(m, i_dim)
            assert chunk % rnd == 0 and rnd in (32, 64)
            assert (n_slabs - 1) * chunk < m <= n_slabs * chunk
            seen.append(n_slabs)
        assert seen[0] == 1 and seen[3] < seen[5]
        cap = _cap_m(i_dim)[1]
        assert max(seen) <= cap
        for m in (10 ** 6, 10 ** 7, 10 ** 8):
            assert _plan(m, i_dim)[1] <= cap
    assert _plan(0, 64)[1] == 0


@pytest.mark.parametrize("m,i_dim", CASES)
def test_probe_rows_exact(m, i_dim):
    """g and x are zero except for the probe rows; probe k has one nonzero
    g[r_k, k] and a full random x[r_k, :], so each output element is one
    exact product: bit-equal to float64, rows without a probe exactly 0."""
    rows = _probe_rows(m, i_dim)
    k = len(rows)
    assert k == min(64, m) and 0 in rows and m - 1 in rows
    ridx = torch.tensor(rows, device=DEV)
    gen = torch.Generator().manual_seed(7 * m + i_dim)
    gval = (torch.rand(k, generator=gen) + 0.5) \
        * (torch.randint(0, 2, (k,), generator=gen) * 2 - 1)
    g = torch.zeros(m, 64, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(m, i_dim, device=DEV, dtype=torch.bfloat16)
    g[ridx, torch.arange(k, device=DEV)] = gval.bfloat16().to(DEV)
    x[ridx] = _rand((k, i_dim), 11 * m + i_dim)
    got = _ext().wgrad_splitk(g, x)
    want = (g[ridx].double().t() @ x[ridx].double()).float()
    assert got.dtype == torch.float32 and got.shape == (64, i_dim)
    assert torch.equal(got, want), \
        f"{int((got != want).sum())} elements differ"
    assert bool((got[k:] == 0).all())
    assert bool((want[:k] != 0).any())


@pytest.mark.parametrize("m,i_dim", CASES)
def test_dense(m, i_dim):
    g = _rand((m, 64), 3 * m + i_dim)
    x = _rand((m, i_dim), 5 * m + i_dim)
    got = _ext().wgrad_splitk(g, x)
    assert got.dtype == torch.float32 and got.shape == (64, i_dim)
    assert bool(torch.isfinite(got).all())
    want = g.double().t() @ x.double()
    mag = g.double().abs().t() @ x.double().abs()
    bound = m * U23 * mag
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"RATIO wgrad dense M={m} I={i_dim} slabs={_plan(m, i_dim)[1]} "
          f"err/bound={ratio:.5f}")
    assert bool((err <= bound).all()), ratio
    # run-to-run bit-identical
    assert torch.equal(got, _ext().wgrad_splitk(g, x))


GROUPS = [
    [(2085, 64)],
    [(65, 144), (2085, 64)],
    [(5000, 64), (5000, 64), (700, 131)],
    [(65, 144), (2085, 64), (0, 64), (1025, 208)],
    [(3000, 64), (1500, 16), (2500, 3), (900, 64)],
    [(0, 64), (0, 144)],
    [(40_000, 67), (1, 1), (90_001, 64), (30_000, 194)],
]


def _group_inputs(shapes, seed):
    gs = [_rand((m, 64), seed + 2 * k) for k, (m, _) in enumerate(shapes)]
    xs = [_rand((m, i), seed + 2 * k + 1) for k, (m, i) in enumerate(shapes)]
    return gs, xs


@pytest.mark.parametrize("shapes", GROUPS, ids=lambda s: "-".join(
    f"{m}x{i}" for m, i in s))
def test_group_members_equal_single_calls(shapes):
    gs, xs = _group_inputs(shapes, 100)
    got = _ext().wgrad_splitk_group(gs, xs)
    again = _ext().wgrad_splitk_group(gs, xs)
    assert len(got) == len(shapes)
    for (m, i_dim), g, x, a, b in zip(shapes, gs, xs, got, again):
        single = _ext().wgrad_splitk(g, x)
        assert a.dtype == torch.float32 and a.shape == (64, i_dim)
        assert torch.equal(a, single), (m, i_dim)
        assert torch.equal(a, b), (m, i_dim)
        if m == 0:
            assert bool((a == 0).all())
        else:
            assert bool((a != 0).any())


def test_group_rejects_bad_groups():
    gs, xs = _group_inputs([(10, 64)] * 5, 7)
    with pytest.raises(RuntimeError):
        _ext().wgrad_splitk_group(gs, xs)
    with pytest.raises(RuntimeError):
        _ext().wgrad_splitk_group([], [])
    with pytest.raises(RuntimeError):
        _ext().wgrad_splitk_group(gs[:2], xs[:1])


def test_group_capture_and_replay():
    """One grouped call captured in a graph; the inputs are rewritten in
    place before each of three replays, and every replay must be bit-equal
    to the eager result for those inputs. The descriptors travel in the
    kernel arguments, so nothing but the tensors' own memory is read."""
    shapes = [(65, 144), (2085, 64), (1025, 208), (5000, 64)]
    sets = [_group_inputs(shapes, 1000 * (r + 1)) for r in range(4)]
    eager = [[t.clone() for t in _ext().wgrad_splitk_group(gs, xs)]
             for gs, xs in sets]
    sg = [t.clone() for t in sets[0][0]]
    sx = [t.clone() for t in sets[0][1]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _ext().wgrad_splitk_group(sg, sx)
    kept = []
    for r in (1, 2, 3):
        for dst, src in zip(sg + sx, sets[r][0] + sets[r][1]):
            dst.copy_(src)
        graph.replay()
        kept.append([t.clone() for t in outs])
    torch.cuda.synchronize()
    for r, res in zip((1, 2, 3), kept):
        for k, (a, b) in enumerate(zip(res, eager[r])):
            assert torch.equal(a, b), (r, k)
    assert not torch.equal(kept[0][1], kept[1][1])


# ------------------------------------------------- grouped call sites
def _singles(pairs):
    return [L.chunked_wgrad(g, x) for g, x in pairs]


def _spy_grouped(monkeypatch, replace):
    sizes = []
    orig = L.grouped_wgrad

    def wrapper(pairs):
        sizes.append(len(pairs))
        return _singles(pairs) if replace else orig(pairs)

    monkeypatch.setattr(L, "grouped_wgrad", wrapper)
    return sizes


def _edge_run():
    bt = collate(make_cutoff_dataset("Water-3D", 1, seed=3,
                                     n_override=999)).to(DEV)
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 131), (64,), (64, 64), (64,), (64, 64), (64,), (64,)]
    scales = [0.08, 0.05, 0.1, 0.05, 0.1, 0.05, 0.05]
    ps = [(torch.randn(*s, generator=g) * c).to(DEV).requires_grad_(True)
          for s, c in zip(shapes, scales)]
    h = _rand((bt.num_nodes, 64), 21, 0.5).requires_grad_(True)
    coord = bt.pos.detach().clone().requires_grad_(True)
    am, at = ops.fused_edge_block(
        h, coord, bt.edge_attr, bt.edge_index[0], bt.edge_index[1],
        bt.rowptr, bt.colptr, bt.col_perm, *ps, False, 1e-8)
    (am.float().pow(2).sum() + at.pow(2).sum()).backward()
    assert bt.edge_index.size(1) > 999
    return [ps[0].grad, ps[2].grad, ps[4].grad]


def _virtual_run():
    c = 3
    bt = collate(make_cutoff_dataset("Water-3D", 1, seed=4,
                                     n_override=333)).to(DEV)
    assert bt.num_nodes * c == 999
    g = torch.Generator().manual_seed(6)

    def t(*shape, s=0.1):
        return (torch.randn(*shape, generator=g) * s).to(DEV)

    p = dict(w1=t(64, 129 + c), b1=t(64), w2=t(64, 64), b2=t(64),
             wxv=t(64, 64), bxv=t(64), wxvv=t(64),
             wX=t(64, 64), bX=t(64), wXv=t(64))
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    h = t(bt.num_nodes, 64, s=0.5).bfloat16().requires_grad_(True)
    coord = bt.pos.detach().clone().requires_grad_(True)
    vcoord = (bt.loc_mean.unsqueeze(1).expand(-1, c, 3).contiguous()
              + t(bt.num_graphs, c, 3, s=0.05)).requires_grad_(True)
    vfeat = t(bt.num_graphs, c, 64, s=0.5).requires_grad_(True)
    gram = t(bt.num_graphs, c, c, s=0.3).requires_grad_(True)
    chunks = None
    if bt.pool_chunk_begin is not None:
        chunks = (bt.pool_chunk_begin, bt.pool_chunk_end,
                  bt.pool_seg_chunk_ptr)
    vmsg, tv, tx = ops.fused_virtual_block(
        h, coord, vcoord, vfeat, gram, bt.batch, bt.ptr, chunks,
        p["w1"], p["b1"], p["w2"], p["b2"], p["wxv"], p["bxv"], p["wxvv"],
        p["wX"], p["bX"], p["wXv"])
    (vmsg.float().pow(2).sum() + tv.pow(2).sum() + tx.pow(2).sum()).backward()
    return [p["w1"].grad, p["w2"].grad, p["wxv"].grad, p["wX"].grad]


@pytest.mark.parametrize("run,members", [(_edge_run, 3), (_virtual_run, 4)],
                         ids=["edge", "virtual"])
def test_block_weight_grads_equal_single_calls(run, members, monkeypatch):
    """The fused blocks' weight gradients through the grouped call are
    bit-equal to the same backward with the group replaced by single
    chunked_wgrad calls."""
    sizes = _spy_grouped(monkeypatch, replace=False)
    grouped = [t.clone() for t in run()]
    assert sizes == [members]
    monkeypatch.undo()
    sizes = _spy_grouped(monkeypatch, replace=True)
    single = [t.clone() for t in run()]
    assert sizes == [members]
    for k, (a, b) in enumerate(zip(grouped, single)):
        assert a.dtype == torch.float32 and bool((a != 0).any()), k
        assert torch.equal(a, b), k
