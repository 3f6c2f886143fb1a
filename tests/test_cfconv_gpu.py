"""GPU tests of the fused CFConv message kernel (csrc/cfconv.hip) against
the float64 reference distegnn_amd/ops/cfconv_reference.py.

The kernel emits only ``msg``, so the bound is propagated through the
stages (``_bound``), each term formed from the reference's own values
(u23 = 2^-23, u8 = 2^-8 = the bf16 unit roundoff, ``mag`` = the same
product over absolute values). Building blocks as in
tests/test_edge_block_gpu.py:

* bf16 storage of v costs u8*|v|;
* an fp32 MFMA accumulation of K products plus a bias costs
  2(K+1)*u23*mag (K = 64 for both GEMMs at F = 64: the gaussian dimension
  is zero-padded to 64; K = F for the second);
* the fast exponential costs (1 + |x|/2)*u23, relatively;
* softplus has slope <= 1;
* ``__logf`` and ``__cosf`` have no bound in this project: each gets the
  explicit absolute term 2^-18, a thousand times below the bf16 roundoff of
  the O(1) quantities next to it.

Stage by stage (x = coeff*(d - offset_k)^2 <= 0, g = exp(x)):

  gauss  x carries 5 fp32 roundings (the difference twice, two products,
         coeff itself): 2.5*u23*|x|, which exp turns into a relative
         error; with the fast exp and the bf16 store
           e_g = g*(u8 + (1 + 3|x|)*u23) + 2^-126     (flush to zero)
  pre1   e_p = e_g @ |W1|^T + 2*65*u23*mag1
  z1     ssp(p) = m + log(exp(p-m) + exp(-m)) - log 2, m = max(p, 0): one
         exponential is exp(0), the other is <= 1 with absolute error
         <= u23; their sum rounds by <= u23; log has slope <= 1 on [1, 2]
         and its own 2^-18; the two additions round by <= u23*(1+|p|)/2
         each:
           e_s = 2^-18 + (4 + |p|)*u23,  e_z = e_p + e_s, then the bf16
           store: e_z1 = e_z + u8*(|z1| + e_z)
  w      e_w = e_z1 @ |W2|^T + 2(F+1)*u23*mag2, then the bf16 store
  cf     the argument pi*d/cutoff carries 4 roundings of u23/2 (the
         product, pi/cutoff, and the fast cosine's own scaling by 1/2pi):
           e_c = (2*u23*|arg| + 2^-18)/2 + u23
  msg    e_m = |xj|*(e_w*(|cf| + e_c) + |w|*e_c) + 2*u23*|msg|, then the
         bf16 store.

At d = cutoff the reference message is ~1e-16 and the bound about
|xj|*|w|*2e-6: "within bound of 0". The backward is the bf16 eager chain
under autograd, which has no format-derived bound: it is MEASURED against
float64 autograd next to the eager bf16 composition (d_f <= max(0.02,
1.5*d_e), the in-model rule of tests/test_fused_virtual_h_gpu.py).
docs/KERNELS.md ("CFConv test bounds") records the measured ratios.
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.ops import cfconv_reference as CR
from distegnn_amd.ops import prep

U23 = 2.0 ** -23
U8 = 2.0 ** -8
FAST = 2.0 ** -18               # __logf / __cosf absolute term
DEV = "cuda:0"
TILE = 64
GRID_CAP = 16384
CUTOFF = 5.0
N = 300


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


class _Case:
    """Inputs of one kernel call. Weights are fp32 and NOT on bf16 values:
    the call rounds them as ``prep`` does, the reference rounds them
    itself."""

    def __init__(self, f, g, m, seed=0, n=N):
        gen = torch.Generator().manual_seed(1000 * f + 10 * g + seed)
        self.f, self.g, self.m, self.n = f, g, m, n
        self.xw1 = (torch.randn(n, f, generator=gen) * 0.7).bfloat16().to(DEV)
        self.row = torch.sort(torch.randint(0, n, (m,), generator=gen)) \
            .values.to(DEV)
        col = torch.randint(0, n, (m,), generator=gen)
        if m >= 2:
            col[0], col[-1] = 0, n - 1
        elif m == 1:
            col[0] = n - 1
        self.col = col.to(DEV)
        self.dist = (torch.rand(m, generator=gen) * CUTOFF).to(DEV)
        self.w1 = (torch.randn(f, g, generator=gen) * 0.3).to(DEV)
        self.b1 = (torch.randn(f, generator=gen) * 0.3).to(DEV)
        self.w2 = (torch.randn(f, f, generator=gen) * 1.5 / f ** 0.5).to(DEV)
        self.b2 = (torch.randn(f, generator=gen) * 0.3).to(DEV)
        self.offsets = torch.linspace(0.0, CUTOFF, g).to(DEV)
        self.coeff = -0.5 / float(self.offsets[1] - self.offsets[0]) ** 2

    def run(self, xw1=None, dist=None, rows=None):
        xw1 = self.xw1 if xw1 is None else xw1
        dist = self.dist if dist is None else dist
        row, col = self.row, self.col
        if rows is not None:
            dist, row, col = dist[rows], row[rows], col[rows]
        return ops.hip_ext().cfconv_forward(
            xw1, dist, row, col, prep.pad_gpad(self.w1), self.b1,
            prep.bf16c(self.w2), self.b2, self.offsets, self.coeff, CUTOFF)

    def stages(self, rows=None):
        dist, col = self.dist, self.col
        if rows is not None:
            dist, col = dist[rows], col[rows]
        return CR.cfconv_stages(
            self.xw1.double(), dist, col, self.w1.double(), self.b1,
            self.w2.double(), self.b2, self.offsets, self.coeff, CUTOFF), dist


def _bound(c, st, dist):
    """Elementwise bound on |msg_kernel - msg_reference| (module docstring)."""
    w1 = c.w1.bfloat16().double().abs()
    w2 = c.w2.bfloat16().double().abs()
    b1, b2 = c.b1.double().abs(), c.b2.double().abs()
    d = dist.double()
    dk = d.view(-1, 1) - c.offsets.double().view(1, -1)
    x = (c.coeff * dk * dk).abs()
    g = st["gauss"]
    e_g = g * (U8 + (1 + 3 * x) * U23) + 2.0 ** -126
    mag1 = (g + e_g) @ w1.t() + b1
    e_p = e_g @ w1.t() + 2 * (64 + 1) * U23 * mag1
    e_s = FAST + (4 + st["pre1"].abs()) * U23
    e_z = e_p + e_s
    e_z1 = e_z + U8 * (st["z1"].abs() + e_z)
    mag2 = (st["z1"].abs() + e_z1) @ w2.t() + b2
    e_w = e_z1 @ w2.t() + 2 * (c.f + 1) * U23 * mag2
    e_w = e_w + U8 * (st["w"].abs() + e_w)
    arg = (math.pi / CUTOFF) * d
    e_c = (0.5 * (2 * U23 * arg.abs() + FAST) + U23).view(-1, 1)
    cf = st["cf"].abs().view(-1, 1)
    e_m = st["xj"].abs() * (e_w * (cf + e_c) + st["w"].abs() * e_c) \
        + 2 * U23 * st["msg"].abs()
    return e_m + U8 * (st["msg"].abs() + e_m)


def _judge(tag, c, got, rows=None):
    st, dist = c.stages(rows)
    want = st["msg"]
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, tag
    assert bool(torch.isfinite(got.float()).all()), tag
    bound = _bound(c, st, dist)
    err = (got.double() - want).abs()
    r = float((err / bound).max()) if err.numel() else 0.0
    print(f"RATIO cfconv {tag} err/bound={r:.4f}")
    assert r <= 1.0, (tag, r)
    return err, bound


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 200])
def test_tile_tails(f, m):
    c = _Case(f, 50, m)
    got = c.run()
    assert got.shape == (m, f) and got.dtype == torch.bfloat16
    if m:
        assert int(c.col[0]) in (0, N - 1) and int(c.col[-1]) == N - 1
    _judge(f"F{f} m={m}", c, got)


@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("g", [2, 32, 33, 50, 64])
def test_gaussian_counts(f, g):
    c = _Case(f, g, 200, seed=1)
    _judge(f"F{f} G={g}", c, c.run())


@pytest.mark.parametrize("f", [64, 128])
def test_distance_edges(f):
    """d = 0, d = cutoff, 1.5 and 100 cutoffs, and d on the offsets."""
    c = _Case(f, 50, 200, seed=2)
    d = c.dist.clone()
    special = [0.0, CUTOFF, 1.5 * CUTOFF, 100 * CUTOFF]
    d[:4] = torch.tensor(special, device=DEV)
    d[60:68] = torch.tensor([0.0, CUTOFF, 1.5 * CUTOFF, 100 * CUTOFF] * 2,
                            device=DEV)       # across the tile boundary
    d[100:150] = c.offsets
    c.dist = d
    got = c.run()
    err, bound = _judge(f"F{f} distances", c, got)
    st, _ = c.stages()
    # d = cutoff: the message is 0 within the bound (which is tiny there)
    for e in (1, 61, 65):
        assert float(st["msg"][e].abs().max()) < 1e-14
        assert float(bound[e].max()) < 1e-4
        assert bool((got[e].double().abs() <= bound[e]).all())
    # 100 cutoffs: every gaussian is 0, z1 = ssp(b1) for that edge
    assert float(st["gauss"][3].max()) == 0.0
    ssp = F.softplus(c.b1.double()) - math.log(2.0)
    assert float((st["z1"][3] - ssp).abs().max()) < 1e-14


@pytest.mark.parametrize("f", [64, 128])
def test_softplus_tails(f):
    c = _Case(f, 50, 200, seed=3)
    c.b1[:8] = torch.tensor([30.0, -30.0, 90.0, -90.0] * 2, device=DEV)
    got = c.run()
    assert bool(torch.isfinite(got.float()).all())
    _judge(f"F{f} ssp-tails", c, got)


@pytest.mark.parametrize("f", [64, 128])
def test_non_contiguous_inputs_bit_equal(f):
    c = _Case(f, 50, 200, seed=4)
    wide_x = torch.zeros(N, 2 * f, dtype=torch.bfloat16, device=DEV)
    wide_x[:, :f] = c.xw1
    wide_d = torch.full((200, 2), 7.0, device=DEV)
    wide_d[:, 0] = c.dist
    xs, ds = wide_x[:, :f], wide_d[:, 0]
    assert not xs.is_contiguous() and not ds.is_contiguous()
    base = c.run()
    assert torch.equal(c.run(xw1=xs), base)
    assert torch.equal(c.run(dist=ds), base)
    print(f"RATIO cfconv F{f} strided err/bound=0.0000 (bit-equal)")


def test_second_trip_of_the_tile_loop():
    """m = 16384*64 + 65: blocks 0 and 1 run a second tile (a full one and
    a tail of one edge). The kernel is per-edge deterministic, so those
    rows must be bit-equal to a call on them alone; 4096 sampled rows are
    judged against the float64 bound."""
    m = GRID_CAP * TILE + 65
    c = _Case(64, 50, m, seed=5)
    got = c.run()
    assert got.shape == (m, 64)
    tail = torch.arange(GRID_CAP * TILE, m, device=DEV)
    alone = c.run(rows=tail)
    assert torch.equal(got[tail], alone), \
        f"{int((got[tail] != alone).any(1).sum())} second-trip rows differ"
    # the first tiles of blocks 0 and 1 were not disturbed by the second
    first = torch.arange(0, 2 * TILE, device=DEV)
    assert torch.equal(got[first], c.run(rows=first))
    gen = torch.Generator().manual_seed(6)
    sample = torch.cat([torch.randint(0, m, (4096 - 65,), generator=gen)
                        .to(DEV), tail])
    _judge("F64 second-trip", c, got[sample], rows=sample)


@pytest.mark.parametrize("f", [64, 128])
def test_direct_call_rejects_wrong_weights(f):
    """fp32 weights would be reinterpreted as bf16 bytes, an unpadded W1
    read past its rows."""
    c = _Case(f, 50, 10)
    ext = ops.hip_ext()
    w1p, w2b = prep.pad_gpad(c.w1), prep.bf16c(c.w2)
    tail = (c.offsets, c.coeff, CUTOFF)
    head = (c.xw1, c.dist, c.row, c.col)
    assert ext.cfconv_forward(*head, w1p, c.b1, w2b, c.b2, *tail).shape \
        == (10, f)
    with pytest.raises(RuntimeError, match="w1f"):
        ext.cfconv_forward(*head, w1p.float(), c.b1, w2b, c.b2, *tail)
    with pytest.raises(RuntimeError, match="w2f"):
        ext.cfconv_forward(*head, w1p, c.b1, w2b.float(), c.b2, *tail)
    with pytest.raises(RuntimeError, match="w1f"):
        ext.cfconv_forward(*head, c.w1.bfloat16(), c.b1, w2b, c.b2, *tail)


# ----------------------------------------------------- backward, dispatch
def _csr_of(col, n):
    perm = torch.argsort(col, stable=True)
    ptr = torch.zeros(n + 1, dtype=torch.long, device=col.device)
    ptr.scatter_add_(0, col[perm] + 1, torch.ones_like(col))
    return ptr.cumsum(0), perm


def _eager_bf16(lx, lw1, lb1, lw2, lb2, dist, col, offsets, coeff, cutoff):
    """The bf16 eager composition the fused op replaces (the chain that
    DISTEGNN_DISABLE_FUSED=1 selects in models/schnet.py), written out."""
    dk = dist.view(-1, 1) - offsets.view(1, -1)
    gauss = torch.exp(coeff * dk.pow(2)).bfloat16()
    cf = 0.5 * (torch.cos(dist * math.pi / cutoff) + 1.0)
    z1 = F.softplus(F.linear(gauss, lw1.bfloat16(), lb1.bfloat16())) \
        - math.log(2.0)
    w = F.linear(z1.bfloat16(), lw2.bfloat16(), lb2.bfloat16())
    return lx.index_select(0, col) * w * cf.view(-1, 1).bfloat16()


@pytest.mark.parametrize("f", [64, 128])
def test_backward_against_float64_autograd(f):
    """Gradients of ops.cfconv_msg w.r.t. xw1, w1, b1, w2, b2 (d_f) and of
    the eager bf16 composition (d_e): relative L2 distances to float64
    autograd of the reference; d_f <= max(0.02, 1.5*d_e) per tensor."""
    c = _Case(f, 50, 4000, seed=7)
    colptr, col_perm = _csr_of(c.col, N)
    gout = (torch.randn(4000, f, generator=torch.Generator().manual_seed(8))
            ).bfloat16().to(DEV)
    src = (c.xw1, c.w1, c.b1, c.w2, c.b2)

    ref_leaves = [t.double().requires_grad_(True) for t in src]
    msg_r = CR.cfconv_msg(ref_leaves[0], c.dist, c.col, *ref_leaves[1:],
                          c.offsets, c.coeff, CUTOFF)
    g_ref = torch.autograd.grad(msg_r, ref_leaves, gout.double())

    lf = [t.clone().requires_grad_(True) for t in src]
    msg_f = ops.cfconv_msg(lf[0], c.dist, c.row, c.col, colptr, col_perm,
                           lf[1], lf[2], lf[3], lf[4], c.offsets, c.coeff,
                           CUTOFF)
    g_f = torch.autograd.grad(msg_f, lf, gout)

    le = [t.clone().requires_grad_(True) for t in src]
    msg_e = _eager_bf16(*le, c.dist, c.col, c.offsets, c.coeff, CUTOFF)
    g_e = torch.autograd.grad(msg_e, le, gout)

    worst = 0.0
    for name, r, a, b in zip(("xw1", "w1", "b1", "w2", "b2"), g_ref, g_f,
                             g_e):
        assert a.shape == r.shape and bool(torch.isfinite(a.float()).all())
        d_f = float((a.double() - r).norm() / r.norm())
        d_e = float((b.double() - r).norm() / r.norm())
        lim = max(0.02, 1.5 * d_e)
        worst = max(worst, d_f / lim)
        print(f"F={f} d{name}: d_f={d_f:.4g} d_e={d_e:.4g}")
        assert d_f <= lim, (name, d_f, d_e)
    print(f"RATIO cfconv F{f} backward err/bound={worst:.4f}")


def test_in_model_fused_and_eager_against_cpu(monkeypatch):
    """FastSchNet (hidden 64, 50 gaussians, two small graphs) under bf16
    autocast with the fused CFConv and with DISTEGNN_DISABLE_FUSED=1, each
    against the CPU fp32 forward. A spy counts the calls of
    ops.cfconv_msg: a silent fallback in the fused arm fails. A layer's
    SchNet block has one interaction, whose features the coordinate output
    does not read, so the spy also keeps every call's inputs and output:
    each message tensor is held to the same rule against the float64
    reference, next to the eager bf16 composition of the same inputs."""
    from distegnn_amd.data.graph import collate
    from distegnn_amd.data.synthetic import make_cutoff_dataset
    from distegnn_amd.models.fastschnet import FastSchNet
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt_cpu = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                         n_override=400))
    bt = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                     n_override=400)).to(DEV)
    m = FastSchNet(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2,
                   hidden_nf=64, virtual_channels=3, cutoff=0.035,
                   n_layers=2)
    assert m.gcl_0.schnet_layer.num_gaussians == 50

    def forward(model, b):
        return model(b.x, b.pos, b.vel, b.loc_mean, b.edge_index, b.batch,
                     edge_attr=b.edge_attr, rowptr=b.rowptr, ptr=b.ptr,
                     counts=b.counts, colptr=b.colptr, col_perm=b.col_perm)

    with torch.no_grad():
        ref = [t.float() for t in forward(m, bt_cpu)]
    mg = m.to(DEV)
    calls = []
    real = ops.cfconv_msg

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((a, out))
        return out

    monkeypatch.setattr(ops, "cfconv_msg", spy)

    def gpu_forward(disable):
        if disable:
            monkeypatch.setenv("DISTEGNN_DISABLE_FUSED", "1")
        else:
            monkeypatch.delenv("DISTEGNN_DISABLE_FUSED", raising=False)
        del calls[:]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = forward(mg, bt)
        return [t.float().cpu() for t in out], list(calls)

    fused, seen = gpu_forward(False)
    eager, seen_eager = gpu_forward(True)
    n_fused, n_eager = len(seen), len(seen_eager)
    assert n_fused > 0, f"fused arm made {n_fused} cfconv_msg calls"
    assert n_eager == 0, f"eager arm made {n_eager} cfconv_msg calls"
    worst = 0.0
    for name, r, a_f, a_e in zip(("loc", "virtual_loc"), ref, fused, eager):
        assert bool(torch.isfinite(a_f).all())
        d_f = float((a_f - r).norm() / r.norm())
        d_e = float((a_e - r).norm() / r.norm())
        lim = max(0.02, 1.5 * d_e)
        worst = max(worst, d_f / lim)
        print(f"FastSchNet {name}: d_f={d_f:.4g} d_e={d_e:.4g} "
              f"calls={n_fused}/{n_eager}")
        assert d_f <= lim, (name, d_f, d_e)
    with torch.no_grad():
        for i, (a, out) in enumerate(seen):
            (xw1, dist, _, col, _, _, w1, b1, w2, b2, offsets, coeff,
             cutoff) = a
            assert out.dtype == torch.bfloat16
            assert out.size(0) == col.numel() > 0
            want = CR.cfconv_msg(xw1.double(), dist, col, w1.double(), b1, w2,
                                 b2, offsets, coeff, cutoff)
            msg_e = _eager_bf16(xw1, w1, b1, w2, b2, dist, col, offsets, coeff,
                                cutoff)
            d_f = float((out.double() - want).norm() / want.norm())
            d_e = float((msg_e.double() - want).norm() / want.norm())
            lim = max(0.02, 1.5 * d_e)
            worst = max(worst, d_f / lim)
            print(f"FastSchNet layer {i} msg: d_f={d_f:.4g} d_e={d_e:.4g}")
            assert d_f <= lim, (i, d_f, d_e)
    print(f"RATIO cfconv in-model err/bound={worst:.4f}")
