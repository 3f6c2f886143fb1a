"""GPU tests of the node-sum edge backward: ``fused_edge_backward_lin``
(csrc/fused_edge_bwd.hip, EB_LIN), ``segment_reduce_csr_split``
(csrc/segment_reduce.hip) and the default path of ``ops.fused_edge_block``
that joins them.

The per-edge chain of the new kernel mode is the plain mode's, so its
per-edge tensors must be bit-equal to it; its atomically summed outputs are
held against float64 under the bounds of tests/test_edge_block_gpu.py (that
module's cases, stages and bounds are imported, not repeated). ``gw1_tail``
is new: an fp32 sum, in any order, of exact products of bf16 factors, so
its bound is the project's column-sum form n*u23*sum|terms| with n the
number of nonzero terms; it is summed without atomics, so it is also
bit-identical from call to call."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

import test_edge_block_gpu as EB  # noqa: E402

from distegnn_amd import ops  # noqa: E402
from distegnn_amd.ops import edge_reference as ER  # noqa: E402
from distegnn_amd.ops import prep  # noqa: E402

U23, DEV, EPS, TILE = EB.U23, EB.DEV, EB.EPS, EB.TILE
PER_EDGE = "DISTEGNN_EDGE_BWD_PER_EDGE"


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


# ------------------------------------------------------------- stage level
def _backward_lin(c):
    return ops.hip_ext().fused_edge_backward_lin(
        c.h, c.bt.pos, c.bt.edge_attr, c.row, c.col, c.dmsg_n, c.dtrans_n,
        *c._weights(), c.normalize, EPS)


def _check_lin(c, title):
    """Plain and node-sum kernels on the same inputs."""
    H = c.hdim
    plain = c.backward()
    ein, t1, msg, dz1, dz2, dz3, _dhr, _dhc, dcd, _dw3v, _gb = plain
    lin = _backward_lin(c)
    assert len(lin) == 9
    (l_t1, l_msg, l_dz1, l_dz2, l_dz3, l_dcd, l_dw3v, l_gb, l_tail) = lin
    R = EB._Ratios()
    for tag, got, want in (("t1", l_t1, t1), ("msg", l_msg, msg),
                           ("dz1", l_dz1, dz1), ("dz2", l_dz2, dz2),
                           ("dz3", l_dz3, dz3), ("dcd", l_dcd, dcd)):
        R.equal(tag, got, want)
    st = EB._Stages(c, plain).build()
    R.check("gb", l_gb, *st.refs["gb"])
    R.check("dw3v", l_dw3v, *st.refs["dw3v"])
    # gw1_tail[c, j] = sum_e dz1[e, c] * x[e, j], x = the bf16 r2 | attr
    # columns the first layer read (the plain mode's ein carries them;
    # test_edge_block_gpu judges those). Each product of two bf16 values is
    # exact in fp32; the sum is a fixed fold (16 rows per wave in order, then
    # a deterministic sum over the per-(tile, wave) partial rows), but the
    # bound does not rely on its order.
    assert l_tail.shape == (H, 3) and l_tail.dtype == torch.float32
    a = l_dz1.double()
    x = ein[:, 2 * H:2 * H + 3].double()
    want = a.t() @ x
    cnt = (a != 0).double().t() @ (x != 0).double()
    assert int(cnt.max()) <= c.m
    R.check("gw1_tail", l_tail, want, cnt * U23 * (a.abs().t() @ x.abs()))
    # no atomics on a weight gradient: a second call gives the same bits
    R.equal("gw1_tail.again", _backward_lin(c)[8], l_tail)
    R.report(title)
    return st, lin


LIN_GRAPHS = {
    "M1": lambda: EB.graph_random(1, 24),
    "M17": lambda: EB.graph_random(17, 24),
    "M65": lambda: EB.graph_random(65, 24),
    "M563": lambda: EB.graph_random(563, 97),
    "iso_hub": EB.graph_iso_hub,
}


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
@pytest.mark.parametrize("gname", list(LIN_GRAPHS))
def test_lin_stages(gname, hdim, normalize):
    c = EB._Case(LIN_GRAPHS[gname](), hdim, normalize)
    if gname.startswith("M"):
        assert c.m == int(gname[1:])
    st, lin = _check_lin(c, f"lin case={gname} H={hdim} "
                            f"norm={int(normalize)}")
    if c.m > 1:
        assert float(lin[8].abs().max()) > 0


def test_lin_second_tile_trip():
    """M = 16384*64 + 645 at H = 32: blocks 0..10 walk a second tile. Only
    the nodes whose rows own the second-trip tiles carry a cotangent, so a
    tile dropped from gw1_tail (or gb, dw3v) is several percent of the sum
    against a bound of about 1e-3 of it."""
    m, n = EB.GRID_CAP * TILE + 645, 2048
    assert m == EB.SECOND_TRIP_M
    c = EB._Case(EB.graph_random(m, n), 32, True)
    tiles = EB._second_trip_tiles(m)
    assert len(tiles) == 11 and max(tiles) == (m - 1) // TILE
    in_trip = torch.zeros(m, dtype=torch.bool, device=DEV)
    for t in tiles:
        in_trip[t * TILE:(t + 1) * TILE] = True
    nodes = torch.unique(c.row[in_trip])
    c.keep_cotangents(nodes)
    live = torch.isin(c.row, nodes)
    n_live = int(live.sum())
    share = int((live & in_trip).sum()) / n_live
    assert share >= 0.03 and n_live * U23 <= share / 10
    st, lin = _check_lin(c, "lin case=second_trip_acc H=32 norm=1")
    # the second trip alone is a visible part of every tail entry's terms
    a = lin[2].double().abs()
    x = st.ein[:, 64:67].double().abs()
    part = (a[in_trip].t() @ x[in_trip]) / (a.t() @ x)
    print(f"second-trip share of sum|terms| per tail entry: "
          f"min={float(part.min()):.3f}")
    assert float(part.min()) > 10 * n_live * U23


# ------------------------------------------------- segment_reduce_csr_split
def _split_lengths():
    g = torch.Generator().manual_seed(21)
    fixed = [0] + list(range(0, 41)) + [63, 64, 65, 127, 128, 129, 1000]
    rnd = torch.randint(0, 41, (8300 - len(fixed),), generator=g).tolist()
    return torch.tensor(fixed + rnd + [0])


_SPLIT_CACHE = {}


def _split_case(f):
    """Integer-valued bf16 rows whose segment sums stay below 2^16 (at most
    1000 rows of |v| <= 8), so the fp32 sum is exact in any order and
    hi + lo holds all 16 bits of it. Built once per f."""
    if f not in _SPLIT_CACHE:
        lens = _split_lengths()
        assert lens.numel() > 8192 and lens[0] == 0 and lens[-1] == 0
        rowptr = torch.cat([torch.zeros(1, dtype=torch.long),
                            lens.cumsum(0)])
        m = int(rowptr[-1])
        g = torch.Generator().manual_seed(22 + f)
        vals = torch.randint(-8, 9, (m, f), generator=g)
        perm = torch.randperm(m, generator=g)
        seg = torch.repeat_interleave(torch.arange(lens.numel()), lens)

        def ref(v):
            out = torch.zeros(lens.numel(), f, dtype=torch.long)
            return out.index_add_(0, seg, v)

        assert int(ref(vals).abs().max()) < 2 ** 16
        _SPLIT_CACHE[f] = dict(
            data=vals.to(torch.bfloat16).to(DEV), rowptr=rowptr.to(DEV),
            perm=perm.to(DEV), ref=ref(vals).to(DEV),
            ref_perm=ref(vals[perm]).to(DEV))
    return _SPLIT_CACHE[f]


@pytest.mark.parametrize("use_perm", [False, True])
@pytest.mark.parametrize("f", [32, 64, 128])
def test_segment_reduce_split(f, use_perm):
    ext = ops.hip_ext()
    cs = _split_case(f)
    data, rowptr = cs["data"], cs["rowptr"]
    n = rowptr.numel() - 1
    if use_perm:
        hi, lo = ext.segment_reduce_csr_split(data, rowptr, cs["perm"])
        plain = ext.segment_reduce_csr_perm(data, rowptr, cs["perm"], False)
        want = cs["ref_perm"]
    else:
        hi, lo = ext.segment_reduce_csr_split(data, rowptr)
        plain = ext.segment_reduce_csr(data, rowptr, False)
        want = cs["ref"]
    assert hi.shape == (n, f) and lo.shape == (n, f)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16
    assert torch.equal(hi, plain)
    assert torch.equal((hi.float() + lo.float()).long(), want)
    assert torch.equal(hi.float() + lo.float(), want.float())
    assert bool((lo != 0).any())          # some sum does need its low half
    assert bool((hi[0] == 0).all()) and bool((hi[-1] == 0).all())
    # halves written into column slices of wider buffers, as the edge
    # backward does: same values, the other columns untouched
    wide_hi = torch.full((n, 2 * f), 3.0, dtype=torch.bfloat16, device=DEV)
    wide_lo = torch.full((n, 2 * f), 5.0, dtype=torch.bfloat16, device=DEV)
    perm = cs["perm"] if use_perm else None
    ext.segment_reduce_csr_split(data, rowptr, perm, wide_hi[:, f:],
                                 wide_lo[:, :f])
    assert torch.equal(wide_hi[:, f:], hi) and torch.equal(wide_lo[:, :f], lo)
    assert bool((wide_hi[:, :f] == 3).all())
    assert bool((wide_lo[:, f:] == 5).all())


# ------------------------------------------- through ops.fused_edge_block
@pytest.mark.parametrize("hdim", [32, 64, 128])
@pytest.mark.parametrize("gname", ["iso_hub", "cutoff"])
def test_edge_block_lin_vs_per_edge(gname, hdim):
    """New default path and the per-edge path (environment switch) of
    ops.fused_edge_block, both against the float64 autograd reference.

    The two paths run the same dz chain, so every output but h.grad and
    w1.grad is equal between them; the bias and w3v gradients are fp32
    atomic sums of identical terms in a run-dependent order, each within
    M*u23*sum|terms| of the exact sum, so they may differ by twice that
    (sum|terms| from the float64 chain, with 10 % for its distance from the
    bf16 chain's terms). h.grad and w1.grad: the relative L2 error of the
    new path may be at most 1.25 times the per-edge path's (the number
    formats put the ratio at 0.96 and 1.00; the quarter is slack for
    different rounding draws on small graphs)."""
    bt, normalize = EB._e2e_graph(gname)
    bt = bt.to(DEV)
    row, col = bt.edge_index[0], bt.edge_index[1]
    n, m = bt.num_nodes, bt.num_edges
    params = EB.make_params(hdim, 300, round_all=True)
    g = torch.Generator().manual_seed(301)
    h0 = (torch.randn(n, hdim, generator=g) * 0.7).bfloat16().to(DEV)
    gm = (torch.randn(n, hdim, generator=g) * 0.5).bfloat16().to(DEV)
    gt = torch.randn(n, 3, generator=g).to(DEV)

    def run(per_edge):
        assert PER_EDGE not in os.environ
        if per_edge:
            os.environ[PER_EDGE] = "1"
        try:
            leaves = [h0.clone().requires_grad_(True),
                      bt.pos.clone().requires_grad_(True)] \
                + [p.clone().requires_grad_(True) for p in params]
            am, at = ops.fused_edge_block(
                leaves[0], leaves[1], bt.edge_attr, row, col, bt.rowptr,
                bt.colptr, bt.col_perm, *leaves[2:], normalize, EPS)
            grads = torch.autograd.grad((am, at), leaves,
                                        (gm.to(am.dtype), gt.to(at.dtype)))
        finally:
            os.environ.pop(PER_EDGE, None)
        return [am.detach(), at.detach()] + list(grads)

    leaves = [h0.double().requires_grad_(True),
              bt.pos.double().requires_grad_(True)] \
        + [p.double().requires_grad_(True) for p in params]
    am, at = ER.edge_block_mean(leaves[0], leaves[1], bt.edge_attr.double(),
                                row, col, *leaves[2:], normalize, EPS)
    ref = [am.detach(), at.detach()] + list(torch.autograd.grad(
        (am, at), leaves, (gm.double(), gt.double())))

    # sum|terms| of the atomically summed gradients, from the float64 chain
    p64 = [p.double() for p in params]
    deg = torch.bincount(row, minlength=n).clamp(min=1).double().unsqueeze(1)
    fwd = ER.edge_forward(h0.double(), bt.pos.double(),
                          bt.edge_attr.double(), row, col, *p64, normalize,
                          EPS)
    bwd = ER.edge_backward(fwd, row, col, gm.double() / deg,
                           gt.double() / deg, p64[0], p64[2], p64[4], p64[6],
                           n)
    mag = {"b1.grad": bwd["dz1"].abs().sum(0),
           "b2.grad": bwd["dz2"].abs().sum(0),
           "b3.grad": bwd["dz3"].abs().sum(0),
           "w3v.grad": (bwd["dp"].abs().unsqueeze(1)
                        * ER.silu(fwd["z3"]).abs()).sum(0)}

    new, old = run(False), run(True)
    bad = []
    for nm, r, a, b in zip(EB.E2E_NAMES, ref, new, old):
        assert a.shape == r.shape and b.shape == r.shape, nm
        assert a.dtype == b.dtype, nm
        if nm in ("h.grad", "w1.grad"):
            en = float((a.double() - r).norm() / r.norm())
            eo = float((b.double() - r).norm() / r.norm())
            print(f"LIN graph={gname} H={hdim} {nm} err_new={en:.3e} "
                  f"err_per_edge={eo:.3e} ratio={en / eo:.3f}")
            if not en <= 1.25 * eo:
                bad.append((nm, en, eo))
        elif nm in mag:
            diff = (a.double() - b.double()).abs()
            bound = 2 * 1.1 * m * U23 * mag[nm]
            print(f"LIN graph={gname} H={hdim} {nm} "
                  f"max diff/bound={float((diff / bound).max()):.4f}")
            if not bool((diff <= bound).all()):
                bad.append((nm, float(diff.max())))
        elif not torch.equal(a, b):
            bad.append((nm, "differs between the paths"))
    assert not bad, bad
