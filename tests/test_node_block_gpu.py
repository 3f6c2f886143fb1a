"""GPU tests of the fused node block (csrc/fused_node.hip), one emitted
tensor at a time, against the float64 reference
distegnn_amd/ops/node_reference.py (itself checked on the CPU against the
composition and autograd).

Inputs, weights and cotangents hold bf16 values, so the kernels read exactly
what the reference reads. As in tests/test_edge_block_gpu.py (whose ``U23``,
``U8`` and ``_Ratios`` are imported), every bound comes from the number
formats: u23 = 2^-23, u8 = 2^-8, ``mag`` = the same product over absolute
values, and

* fp32 MFMA accumulation of K bf16 products plus a bias: 2(K+1)*u23*mag;
* a pre-activation z rounded to bf16 before the SiLU is off by
  zerr = u8*|z| + 2(K+1)*u23*mag; silu stretches an error by at most 1.1,
  silu' by at most 0.5; the fast exponential doubles the accumulation term
  against a bf16 result and costs silu' 6*u23*(1+|z|)^2;
* an fp32 sum of n nonzero terms in any order: n*u23*sum|terms|.

Backward stages are judged from the kernel's own output of the stage before
(dagg_e, dagg_v, dh from the emitted dz1 / dzv; the column sums from the
emitted dz1 / dzv), so each check covers one rounding step. Every test
prints its worst err/bound per stage.

The grid is capped at two blocks per CU (512 blocks of 64 rows at H = 32);
``test_node_second_tile_trip`` goes past the cap.
"""

import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from test_edge_block_gpu import DEV, U8, U23, _bf, _Ratios  # noqa: E402

from distegnn_amd import ops  # noqa: E402
from distegnn_amd.ops import node_reference as NR  # noqa: E402
from distegnn_amd.ops import prep  # noqa: E402
from distegnn_amd.ops.linear import SplitKLinear  # noqa: E402

TILE = 64
GRID_CAP_H32 = 512   # 256 CUs x 2 resident blocks


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


@pytest.fixture(autouse=True)
def _clean_env():
    keys = ("DISTEGNN_DISABLE_FUSED", "DISTEGNN_NODE_EAGER")
    old = {k: os.environ.pop(k, None) for k in keys}
    ops._FALLBACK_WARNED.clear()
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


# ------------------------------------------------------------------ inputs
class _Case:
    """bf16-valued fp32 tensors on the GPU; ``live`` limits both cotangents
    to a row mask."""

    def __init__(self, n, hd, a, seed=0, vel_only=False, live=None,
                 zero_dphiv=False, zero_dh_out=False):
        g = torch.Generator().manual_seed(seed * 1000 + n + hd + a)

        def r(*shape, s=1.0):
            return _bf(torch.randn(*shape, generator=g) * s).to(DEV)

        self.n, self.hd, self.a, self.vel_only = n, hd, a, vel_only
        k1 = 3 * hd + a
        self.P = dict(
            w1=r(hd, k1, s=1.5 * k1 ** -0.5), b1=r(hd, s=0.3),
            w2=r(hd, hd, s=1.5 * hd ** -0.5), b2=r(hd, s=0.3),
            wv1=r(hd, hd, s=1.5 * hd ** -0.5), bv1=r(hd, s=0.3),
            wv2=r(hd, s=hd ** -0.5), bv2=r(1, s=0.3))
        self.h, self.agg_e, self.agg_v = r(n, hd), r(n, hd, s=0.7), r(n, hd,
                                                                     s=0.7)
        self.attr = r(n, a) if a else None
        self.dh_out, self.dphiv = r(n, hd), r(n, 1)
        if live is not None:
            self.dh_out = self.dh_out * live.unsqueeze(1)
            self.dphiv = self.dphiv * live.unsqueeze(1)
        if zero_dphiv:
            self.dphiv = torch.zeros_like(self.dphiv)
        if zero_dh_out:
            self.dh_out = torch.zeros_like(self.dh_out)

    def run(self):
        """Both kernels, called directly. Returns (h_out, phiv), backward
        outputs with the partial rows already summed."""
        ext = ops.hip_ext()
        P, vo = self.P, self.vel_only

        def bf(t):
            return None if t is None else t.bfloat16().contiguous()

        w1 = P["wv1"] if vo else P["w1"]
        b1 = P["bv1"] if vo else P["b1"]
        w2 = P["wv1"] if vo else P["w2"]
        b2 = P["bv1"] if vo else P["b2"]
        fw = [prep.pad_kpad(w1), bf(b1), bf(w2), bf(b2), bf(P["wv1"]),
              bf(P["bv1"]), bf(P["wv2"].view(1, -1)), bf(P["bv2"])]
        bw = [prep.pad_kpad(w1), prep.t_bf16(w1), bf(b1), prep.t_bf16(w2),
              bf(P["wv1"]), prep.t_bf16(P["wv1"]), bf(P["bv1"]),
              bf(P["wv2"].view(1, -1))]
        h = bf(self.h)
        ae, av = (h, h) if vo else (bf(self.agg_e), bf(self.agg_v))
        attr = None if vo else bf(self.attr)
        fwd = ext.fused_node_forward(h, ae, av, attr, fw, vo)
        dho = h if vo else bf(self.dh_out)
        outs = ext.fused_node_backward(dho, self.dphiv.contiguous(), h, ae,
                                       av, attr, bw, vo)
        return fwd, outs[:6], outs[6]


def _check(c, title):
    """Every stage of one case. Returns the ratios (already asserted)."""
    R = _Ratios()
    H, A, vo = c.hd, c.a, c.vel_only
    K1 = 3 * H + A
    (h_out, phiv), (dh, dagg_e, dagg_v, dz1, t1, dzv), parts = c.run()
    sums = parts.sum(0)
    assert phiv.dtype == torch.float32 and phiv.shape == (c.n, 1)
    # a rounding point: phiv is bf16-valued
    assert torch.equal(phiv, _bf(phiv))

    def D(t):
        return t.double()

    W1, b1, W2, b2, Wv1, bv1, wv2, bv2 = (D(c.P[k]) for k in (
        "w1", "b1", "w2", "b2", "wv1", "bv1", "wv2", "bv2"))
    h = D(c.h)
    dp = D(c.dphiv)

    # ---- vel chain, forward: zv and tv are not emitted. tv carries
    # ev = 1.1*u8|zv| (zv stored as bf16, through silu) + u8|tv| + the
    # doubled accumulation term; phiv = bf16(tv . wv2 + bv2) adds the
    # (H+1)-term accumulation over |tv| + ev and its own rounding.
    zv = NR.preact(h, Wv1, bv1)
    magv = h.abs() @ Wv1.abs().t() + bv1.abs()
    zerrv = U8 * zv.abs() + 2 * (H + 1) * U23 * magv
    tvr = NR.silu(zv)
    ev = 1.1 * U8 * zv.abs() + U8 * tvr.abs() + 4 * (H + 1) * U23 * magv
    want = (tvr @ wv2).unsqueeze(1) + bv2
    magp = ((tvr.abs() + ev) @ wv2.abs()).unsqueeze(1) + bv2.abs()
    R.check("fwd.phiv", phiv, want,
            (1 + U8) * ((ev @ wv2.abs()).unsqueeze(1)
                        + 2 * (H + 2) * U23 * magp) + U8 * want.abs())

    # ---- vel chain, backward. dphiv holds bf16 values (its rounding in
    # the kernel is exact). dzv = bf16(bf16(dp wv2) silu'(zv stored)): two
    # roundings of the result, |upstream| times the error of silu'.
    up = dp * wv2
    want = up * NR.dsilu(zv)
    R.check("bwd.dzv", dzv, want,
            (2.02 * U8 + 4 * U23) * want.abs()
            + (1 + U8) * up.abs() * (0.5 * zerrv
                                     + 6 * U23 * (1 + zv.abs()) ** 2))
    dzve = D(dzv)
    dhv = dzve @ Wv1
    magdhv = dzve.abs() @ Wv1.abs()

    def colsum(tag, x, got):
        # fp32 column sums of emitted values in any order
        cnt = (x != 0).sum(0).double()
        R.check(tag, got, x.sum(0), cnt * U23 * x.abs().sum(0))

    colsum("gbv1", dzve, sums[2 * H:3 * H])
    colsum("gbv2", dp, sums[-1:])
    # gwv2 = sum dp tv with the kernel's own (unemitted) tv: per term the
    # product rounding and tv's error ev
    n_dp = int((dp != 0).sum())
    terms = dp.abs() * (tvr.abs() + ev)
    R.check("gwv2", sums[3 * H:4 * H], (dp * tvr).sum(0),
            (n_dp + 1) * U23 * terms.sum(0) + (dp.abs() * ev).sum(0))

    if vo:
        assert h_out.numel() == 0 and dz1.numel() == 0
        R.check("bwd.dh", dh, dhv,
                U8 * dhv.abs() + 2 * (H + 1) * U23 * magdhv)
        R.report(title)
        return R

    # ---- node chain, forward: z1 and t1 not emitted. e1 as ev; out =
    # bf16(t1 W2^T + b2) carries e1 through |W2|, its accumulation and its
    # rounding; h_out = bf16(h + out).
    xin = NR.node_input(h, D(c.agg_e), D(c.agg_v),
                        None if c.attr is None else D(c.attr))
    z1 = NR.preact(xin, W1, b1)
    mag1 = xin.abs() @ W1.abs().t() + b1.abs()
    zerr1 = U8 * z1.abs() + 2 * (K1 + 1) * U23 * mag1
    t1r = NR.silu(z1)
    e1 = 1.1 * U8 * z1.abs() + U8 * t1r.abs() + 4 * (K1 + 1) * U23 * mag1
    outr = NR.preact(t1r, W2, b2)
    mag2 = (t1r.abs() + e1) @ W2.abs().t() + b2.abs()
    eo = ((1 + U8) * (e1 @ W2.abs().t() + 2 * (H + 1) * U23 * mag2)
          + U8 * outr.abs())
    want = h + outr
    R.check("fwd.h_out", h_out, want,
            (1 + U8) * eo + U8 * want.abs()
            + 2 * U23 * (h.abs() + outr.abs() + eo))

    # ---- node chain, backward
    R.check("bwd.t1", t1, t1r, e1)
    dho = D(c.dh_out)
    up1 = dho @ W2
    mag_up = dho.abs() @ W2.abs()
    want = up1 * NR.dsilu(z1)
    # dz1 = bf16(bf16(dh_out W2) silu'(z1 stored)): two roundings, the
    # H-term accumulation of the upstream times |silu'| <= 1.1, |upstream|
    # times the error of silu'
    R.check("bwd.dz1", dz1, want,
            (2.02 * U8 + 4 * U23) * want.abs()
            + 1.11 * 2 * (H + 1) * U23 * mag_up
            + ((1 + U8) * up1.abs() + 2 * (H + 1) * U23 * mag_up)
            * (0.5 * zerr1 + 6 * U23 * (1 + z1.abs()) ** 2))
    # din = dz1 W1 from the emitted dz1, bf16 out, K = H
    dz1e = D(dz1)
    W1h = W1[:, :3 * H]
    dein = dz1e @ W1h
    magd = dz1e.abs() @ W1h.abs()
    bnd = U8 * dein.abs() + 2 * (H + 1) * U23 * magd
    R.check("bwd.dagg_e", dagg_e, dein[:, H:2 * H], bnd[:, H:2 * H])
    R.check("bwd.dagg_v", dagg_v, dein[:, 2 * H:], bnd[:, 2 * H:])
    # dh = bf16(dh_out + dz1 W1[:, :H] + dzv Wv1): one 2H-term
    # accumulation and the add, one rounding
    want = dho + dein[:, :H] + dhv
    R.check("bwd.dh", dh, want,
            U8 * want.abs() + 2 * (2 * H + 2) * U23
            * (dho.abs() + magd[:, :H] + magdhv))
    colsum("gb1", dz1e, sums[:H])
    colsum("gb2", dho, sums[H:2 * H])
    if A:
        at = D(c.attr)
        R.check("gw1_tail", sums[4 * H:-1].view(H, A), dz1e.t() @ at,
                (c.n + 1) * U23 * (dz1e.abs().t() @ at.abs()))
    R.report(title)
    return R


# ------------------------------------------------------------------ stages
MODES = {"a0": (0, False), "a2": (2, False), "vel": (0, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("n", [1, 17, 63, 64, 65, 563])
def test_node_stages(n, hd, mode):
    a, vo = MODES[mode]
    _check(_Case(n, hd, a, vel_only=vo), f"node n={n} H={hd} {mode}")


@pytest.mark.parametrize("hd", [32, 64])
def test_node_zero_dphiv(hd):
    """dphiv = 0: the vel chain contributes exact zeros (bound 0)."""
    R = _check(_Case(563, hd, 2, seed=1, zero_dphiv=True),
               f"node dphiv=0 H={hd}")
    assert R["bwd.dzv"] == 0.0 and R["gwv2"] == 0.0 and R["gbv1"] == 0.0


@pytest.mark.parametrize("hd", [32, 64])
def test_node_zero_dh_out(hd):
    """dh_out = 0: dz1, dagg_e, dagg_v and the node-chain sums are exact
    zeros, dh is the vel chain's alone."""
    R = _check(_Case(563, hd, 2, seed=2, zero_dh_out=True),
               f"node dh_out=0 H={hd}")
    for k in ("bwd.dz1", "bwd.dagg_e", "bwd.dagg_v", "gb1", "gb2",
              "gw1_tail"):
        assert R[k] == 0.0, k


def test_node_second_tile_trip():
    """N = 512*64 + 645 at H = 32: blocks 0..10 walk a second tile. The
    cotangents live only on second-trip rows, so a dropped tile would take
    every term of the sums and every nonzero row of the data gradients."""
    n = GRID_CAP_H32 * TILE + 645
    live = torch.zeros(n, device=DEV)
    live[GRID_CAP_H32 * TILE:] = 1
    _check(_Case(n, 32, 2, seed=3, live=live), "node second_trip H=32 a2")
    _check(_Case(n, 32, 0, seed=3, live=live, vel_only=True),
           "node second_trip H=32 vel")


# ------------------------------------------------- weight gradients, repeat
def _mlps(hd, a, seed=0, dtype=torch.float32, linear=SplitKLinear):
    torch.manual_seed(seed)
    node_mlp = nn.Sequential(linear(3 * hd + a, hd), nn.SiLU(),
                             linear(hd, hd))
    vel_mlp = nn.Sequential(linear(hd, hd), nn.SiLU(), linear(hd, 1))
    return node_mlp.to(DEV, dtype), vel_mlp.to(DEV, dtype)


def _block_grads(c, node_mlp, vel_mlp, dtype=torch.bfloat16):
    """Through ops.fused_node_block and autograd. Returns outputs and the
    gradients of (h, agg_e, agg_v, every parameter)."""
    ins = [t.to(dtype).requires_grad_() for t in (c.h, c.agg_e, c.agg_v)]
    attr = None if c.attr is None else c.attr.to(dtype)
    params = list(node_mlp.parameters()) + list(vel_mlp.parameters())
    h_out, phiv = ops.fused_node_block(ins[0], ins[1], ins[2], attr,
                                       node_mlp, vel_mlp, True)
    grads = torch.autograd.grad(
        [h_out, phiv], ins + params,
        [c.dh_out.to(h_out.dtype), c.dphiv.to(phiv.dtype)])
    return (h_out.detach(), phiv.detach()), grads


@pytest.mark.parametrize("n", [65, 563])
def test_node_wgrads_grouped_equal_single_and_repeatable(n):
    """H = 64: the matrix gradients of the autograd path are bit-equal to
    single ``wgrad_splitk`` calls on the kernel's emitted operands, and
    every gradient (the attribute columns of dW1 included) is bit-identical
    over two calls."""
    hd, a = 64, 2
    c = _Case(n, hd, a, seed=4)
    node_mlp, vel_mlp = _mlps(hd, a)
    with torch.no_grad():
        for k, p in zip(("w1", "b1", "w2", "b2"), node_mlp.parameters()):
            p.copy_(c.P[k])
        for k, p in zip(("wv1", "bv1", "wv2", "bv2"), vel_mlp.parameters()):
            p.copy_(c.P[k].view(p.shape))
    _, g1 = _block_grads(c, node_mlp, vel_mlp)
    _, g2 = _block_grads(c, node_mlp, vel_mlp)
    for i, (x, y) in enumerate(zip(g1, g2)):
        assert torch.equal(x, y), f"gradient {i} differs between two calls"

    ext = ops.hip_ext()
    _, (dh, dagg_e, dagg_v, dz1, t1, dzv), parts = c.run()
    bf = torch.bfloat16
    h, ae, av = (t.to(bf) for t in (c.h, c.agg_e, c.agg_v))
    single = [ext.wgrad_splitk(dz1, h), ext.wgrad_splitk(dz1, ae),
              ext.wgrad_splitk(dz1, av),
              ext.wgrad_splitk(c.dh_out.to(bf).contiguous(), t1),
              ext.wgrad_splitk(dzv, h)]
    gw1, gw2, gwv1 = g1[3], g1[5], g1[7]
    R = _Ratios()
    for j in range(3):
        R.equal(f"gw1[{j}]", gw1[:, j * hd:(j + 1) * hd].contiguous(),
                single[j].float())
    R.equal("gw2", gw2, single[3].float())
    R.equal("gwv1", gwv1, single[4].float())
    # and against float64: N*u23*mag, one rounding of the result
    for tag, got, gg, xx in (("gw2.f64", gw2, c.dh_out, t1),
                             ("gwv1.f64", gwv1, dzv, c.h)):
        want = gg.double().t() @ xx.double()
        mag = gg.double().abs().t() @ xx.double().abs()
        R.check(tag, got, want, U8 * want.abs() + (n + 1) * U23 * mag)
    R.report(f"node wgrads n={n}")


# ---------------------------------------------------------------- dispatch
@pytest.fixture
def eager_calls(monkeypatch):
    calls = []
    real = ops.eager_node_block

    def spy(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(ops, "eager_node_block", spy)
    return calls


def test_dispatch_standard_configuration_is_fused(eager_calls, capsys):
    c = _Case(200, 64, 2, seed=5)
    node_mlp, vel_mlp = _mlps(64, 2)
    (h_out, phiv), _ = _block_grads(c, node_mlp, vel_mlp)
    assert not eager_calls
    assert phiv.dtype == torch.float32 and h_out.dtype == torch.bfloat16
    assert "fused_node_block" not in capsys.readouterr().out
    # vel-only returns h itself
    h = c.h.bfloat16()
    h2, pv = ops.fused_node_block(h, None, None, None, node_mlp, vel_mlp,
                                  True, vel_only=True)
    assert h2 is h and not eager_calls
    assert torch.equal(pv, phiv)
    # N = 0
    e_out, e_phiv = ops.fused_node_block(h[:0], h[:0], h[:0], None,
                                         *_mlps(64, 0), True)
    assert e_out.shape == (0, 64) and e_phiv.shape == (0, 1)
    assert not eager_calls


def test_dispatch_fp32_with_grad_falls_back_and_warns(eager_calls, capsys):
    c = _Case(100, 64, 0, seed=6)
    node_mlp, vel_mlp = _mlps(64, 0)
    (h_out, phiv), grads = _block_grads(c, node_mlp, vel_mlp,
                                        dtype=torch.float32)
    assert len(eager_calls) == 1 and h_out.dtype == torch.float32
    out = capsys.readouterr().out
    assert "fused_node_block" in out and "torch.float32" in out
    assert all(torch.isfinite(g).all() for g in grads)


def test_dispatch_unsupported_width_falls_back_and_warns(eager_calls,
                                                         capsys):
    c = _Case(100, 48, 0, seed=7)
    node_mlp, vel_mlp = _mlps(48, 0, dtype=torch.bfloat16)
    _block_grads(c, node_mlp, vel_mlp)
    assert len(eager_calls) == 1
    assert "hidden_nf=48" in capsys.readouterr().out


@pytest.mark.parametrize("var", ["DISTEGNN_DISABLE_FUSED",
                                 "DISTEGNN_NODE_EAGER"])
def test_dispatch_switches_reach_the_composition(var, eager_calls, capsys):
    c = _Case(100, 64, 2, seed=8)
    node_mlp, vel_mlp = _mlps(64, 2, dtype=torch.bfloat16)
    os.environ[var] = "1"
    (h_out, phiv), _ = _block_grads(c, node_mlp, vel_mlp)
    assert len(eager_calls) == 1 and phiv.dtype == torch.bfloat16
    assert "fused_node_block" not in capsys.readouterr().out


# ---------------------------------------------------------------- in model
def _rel(a, b):
    return float((a.double() - b.double()).norm()
                 / b.double().norm().clamp(min=1e-30))


def test_in_model_fused_matches_node_eager():
    """FastEGNN (two graphs, 200 nodes, H = 64, C = 3, node_attr_nf = 2)
    under bf16 autocast: the fused node block against DISTEGNN_NODE_EAGER=1,
    forward outputs and every parameter gradient, within the relative L2 of
    0.02 that tests/test_fused_virtual_gpu.py uses in-model."""
    from distegnn_amd.data.graph import collate
    from distegnn_amd.data.synthetic import make_cutoff_dataset
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                     n_override=100)).to(DEV)
    assert bt.num_nodes == 200
    m = FastEGNN(node_feat_nf=2, node_attr_nf=2, edge_attr_nf=2,
                 hidden_nf=64, virtual_channels=3, world_size=1,
                 n_layers=4).to(DEV)
    g = torch.Generator().manual_seed(1)
    node_attr = torch.randn(bt.num_nodes, 2, generator=g).to(DEV)
    target = bt.pos + 0.01 * torch.randn(bt.pos.shape, generator=g).to(DEV)

    def run(eager):
        if eager:
            os.environ["DISTEGNN_NODE_EAGER"] = "1"
        else:
            os.environ.pop("DISTEGNN_NODE_EAGER", None)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loc, vloc = m(bt.x, bt.pos, bt.vel, bt.loc_mean, bt.edge_index,
                          bt.batch, edge_attr=bt.edge_attr,
                          node_attr=node_attr, rowptr=bt.rowptr, ptr=bt.ptr,
                          counts=bt.counts, colptr=bt.colptr,
                          col_perm=bt.col_perm)
        loss = (loc - target).pow(2).mean() + vloc.pow(2).mean() * 1e-3
        loss.backward()
        os.environ.pop("DISTEGNN_NODE_EAGER", None)
        return (loc.detach(), vloc.detach(),
                {k: p.grad.clone() for k, p in m.named_parameters()
                 if p.grad is not None})

    loc_f, vloc_f, g_f = run(False)
    loc_e, vloc_e, g_e = run(True)
    assert set(g_f) == set(g_e)
    rels = {"loc": _rel(loc_f, loc_e), "vloc": _rel(vloc_f, vloc_e)}
    for k in g_e:
        if float(g_e[k].abs().max()) == 0.0:
            assert float(g_f[k].abs().max()) == 0.0, k
            continue
        rels[k] = _rel(g_f[k], g_e[k])
    worst = sorted(rels.items(), key=lambda kv: -kv[1])[:5]
    print("MODEL node fused vs eager, worst rel L2:",
          " ".join(f"{k}={v:.3e}" for k, v in worst))
    bad = {k: v for k, v in rels.items() if not v < 0.02}
    assert not bad, bad


# ----------------------------------------------------------------- capture
def test_capture_replay_reads_refreshed_weights():
    """Forward + backward captured with torch.cuda.graph; the weights then
    change in place and ``ops.refresh_weight_prep()`` runs. The replay must
    equal an eager call on the new weights, bit for bit (the kernels are
    deterministic): a prep kind left out of ``refresh`` would replay the
    old weights."""
    hd, a = 64, 2
    c = _Case(300, hd, a, seed=9)
    node_mlp, vel_mlp = _mlps(hd, a, seed=2)
    params = list(node_mlp.parameters()) + list(vel_mlp.parameters())
    bf = torch.bfloat16
    ins = [t.to(bf).requires_grad_() for t in (c.h, c.agg_e, c.agg_v)]
    attr = c.attr.to(bf)
    dh_out, dphiv = c.dh_out.to(bf), c.dphiv.clone()

    def step():
        h_out, phiv = ops.fused_node_block(ins[0], ins[1], ins[2], attr,
                                           node_mlp, vel_mlp, True)
        return [h_out, phiv] + list(torch.autograd.grad(
            [h_out, phiv], ins + params, [dh_out, dphiv]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    old = [t.clone() for t in static]
    with torch.no_grad():
        for i, p in enumerate(params):
            p.mul_(1.25 + 0.125 * i)
    assert ops.refresh_weight_prep() > 0
    graph.replay()
    torch.cuda.synchronize()
    new = step()
    assert not torch.equal(old[0], static[0])
    for i, (x, y) in enumerate(zip(static, new)):
        assert torch.equal(x, y), f"output {i}: replay differs from eager"
