"""GPU tests of the split-K linear path at its edges: wgrad_splitk,
tall_linear, SplitKLinear/_SplitKLinearFn and the version-keyed weight
cache (ops/prep.py), plus an edge-less graph through the fused edge block.

References are float64 on the device, computed from the bf16-rounded
operands the kernels receive. Bounds are derived, not tuned (u23 = 2^-23,
u8 = 2^-8, ``mag`` = the same product taken over absolute values):

* fp32 dot product of M terms, any order:         M * u23 * mag
* bf16 output of a K-term fp32 accumulation:      u8*|want| + 2(K+1)*u23*mag
  (half-ulp of the bf16 result + accumulation; the second term is doubled
  behind the fast-exp SiLU)
* bf16 result of chunked_wgrad's torch branches:  2 * u8 * mag
* bias gradient (bf16 column sum):                u8*|want| + M*u23*sum|g|

Each test prints its worst err/bound ratio; docs/KERNELS.md ("Linear-path
test bounds") records the measured values.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import collate
from distegnn_amd.data.synthetic import make_cutoff_dataset
from distegnn_amd.ops import linear as L
from distegnn_amd.ops import prep

U23 = 2.0 ** -23
U8 = 2.0 ** -8
DEV = "cuda:0"

SMALL_M = [1, 63, 64, 65, 1024, 1025, 2085]
WIDTHS = [1, 3, 16, 64, 67, 131, 144, 194, 208]
BIG_M = 66_000          # chunk length 96: every chunk ends in a half round
WGRAD_CASES = ([(m, i) for m in SMALL_M for i in WIDTHS]
               + [(BIG_M, i) for i in (64, 144, 208)])


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


def _rand(shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _ratio(err, bound):
    """max err/bound over the tensor; where the bound is 0 the error must
    be 0 as well."""
    zero = bound == 0
    assert bool((err[zero] == 0).all())
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


def _check(tag, got, want, bound):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert bool(torch.isfinite(got.float()).all()), tag
    r = _ratio((got.double() - want).abs(), bound)
    print(f"RATIO {tag} err/bound={r:.4f}")
    assert r <= 1.0, (tag, r)
    return r


def _chunk_len(m):
    """Split-K chunk length of wgrad_splitk_launch (csrc/wgrad.hip)."""
    return max(64, ((m + 1023) // 1024 + 31) // 32 * 32)


def _probe_rows(m):
    """Up to 64 distinct rows: row 0, the last row, both sides of every
    64-row boundary in the first 130 rows, both sides of the first, a
    middle and the last split-K chunk boundary, and both sides of a
    64-row staging round inside a later chunk; filled up at random."""
    chunk = _chunk_len(m)
    nchunk = (m + chunk - 1) // chunk
    want = [0, m - 1, 63, 64, 127, 128, 129]
    for c in {1, nchunk // 2, nchunk - 1}:
        if c >= 1:
            want += [c * chunk - 1, c * chunk]
    mid = (nchunk // 3) * chunk
    want += [mid + 31, mid + 32, mid + 63, mid + 64, mid + chunk - 1]
    rows = []
    for r in want:
        if 0 <= r < m and r not in rows:
            rows.append(r)
    g = torch.Generator().manual_seed(m)
    for r in torch.randperm(m, generator=g).tolist():
        if len(rows) >= min(64, m):
            break
        if r not in rows:
            rows.append(r)
    return rows[:64]


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("m,i_dim", WGRAD_CASES)
def test_wgrad_splitk_probe_rows_exact(m, i_dim):
    """g and x are zero except for the probe rows; probe k has one nonzero
    g[r_k, k] and a full random x[r_k, :]. Every output element is then one
    bf16 x bf16 product — exact in fp32 — so the result must be bit-equal
    to the float64 product, and rows of dW without a probe exactly 0."""
    rows = _probe_rows(m)
    chunk = _chunk_len(m)
    assert 0 in rows and m - 1 in rows
    for r in (63, 64, 127, 128, chunk - 1, chunk):
        assert r >= m or r in rows
    k = len(rows)
    ridx = torch.tensor(rows, device=DEV)
    gen = torch.Generator().manual_seed(7 * m + i_dim)
    gval = (torch.rand(k, generator=gen) + 0.5) \
        * (torch.randint(0, 2, (k,), generator=gen) * 2 - 1)
    g = torch.zeros(m, 64, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(m, i_dim, device=DEV, dtype=torch.bfloat16)
    g[ridx, torch.arange(k, device=DEV)] = gval.bfloat16().to(DEV)
    x[ridx] = _rand((k, i_dim), 11 * m + i_dim)
    got = ops.hip_ext().wgrad_splitk(g, x)
    want = (g.double().t() @ x.double()).float()
    assert got.dtype == torch.float32 and got.shape == (64, i_dim)
    assert torch.equal(got, want), \
        f"{int((got != want).sum())} elements differ"
    assert bool((got[k:] == 0).all())
    assert bool((want[:k] != 0).any())


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("m", SMALL_M)
@pytest.mark.parametrize("i_dim", WIDTHS)
def test_wgrad_splitk_dense(m, i_dim):
    g = _rand((m, 64), 3 * m + i_dim)
    x = _rand((m, i_dim), 5 * m + i_dim)
    got = ops.hip_ext().wgrad_splitk(g, x)
    assert got.dtype == torch.float32
    want = g.double().t() @ x.double()
    mag = g.double().abs().t() @ x.double().abs()
    _check(f"b wgrad M={m} I={i_dim}", got, want, m * U23 * mag)


@pytest.mark.parametrize("i_dim", [64, 144])
def test_wgrad_splitk_no_rows(i_dim):
    g = torch.zeros(0, 64, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(0, i_dim, device=DEV, dtype=torch.bfloat16)
    for got in (ops.hip_ext().wgrad_splitk(g, x), L.chunked_wgrad(g, x)):
        assert got.dtype == torch.float32 and got.shape == (64, i_dim)
        assert torch.equal(got, torch.zeros(64, i_dim, device=DEV))


# ---------------------------------------------------------------- (c)
def _tall_case(tag, m, k, o, bias, act, bias_dtype=torch.float32):
    x = _rand((m, k), 13 * m + k, 0.5)
    w = _rand((o, k), 17 * o + k, 0.3)
    b = _rand((o,), 19 * o, 0.3, bias_dtype) if bias else None
    got = ops.hip_ext().tall_linear(x, w, b, act)
    assert got.dtype == torch.bfloat16 and got.shape == (m, o)
    want = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    if bias:
        want = want + b.double()
        mag = mag + b.double().abs()
    acc = 2 * (k + 1) * U23 * mag
    if act == 1:
        want = F.silu(want)
        acc = 2 * acc
    return _check(tag, got, want, U8 * want.abs() + acc)


@pytest.mark.parametrize("k,o", [(1, 64), (3, 64), (50, 64), (64, 1),
                                 (64, 64), (131, 64), (64, 131), (64, 144),
                                 (192, 64), (208, 208)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_tall_linear_small(k, o, bias, act):
    for m in (1, 63, 64, 65, 129):
        _tall_case(f"c tall M={m} K={k} O={o} bias={bias} act={act}",
                   m, k, o, bias, act)


def test_tall_linear_bf16_bias():
    _tall_case("c tall bf16-bias", 65, 131, 64, True, 1, torch.bfloat16)


def test_tall_linear_second_grid_trip():
    """8192 blocks x 64 rows + 65: a second trip of the grid-stride loop
    and a ragged last tile; all rows compared on the device."""
    _tall_case("c tall multi-trip", 8192 * 64 + 65, 64, 64, True, 1)


# ---------------------------------------------------------------- (d)
def _spy(monkeypatch, obj, name, calls=None):
    calls = [] if calls is None else calls
    orig = getattr(obj, name)

    def wrapper(*a, **k):
        calls.append(name)
        return orig(*a, **k)

    monkeypatch.setattr(obj, name, staticmethod(wrapper)
                        if isinstance(obj, type) else wrapper)
    return calls


def test_splitk_linear_row_gate(monkeypatch):
    calls = _spy(monkeypatch, L._SplitKLinearFn, "apply")
    lin = L.SplitKLinear(64, 64).to(DEV)
    x = _rand((L._MIN_ROWS, 64), 1, 1.0, torch.float32)
    with torch.autocast("cuda", torch.bfloat16):
        y = lin(x[:-1])
        assert calls == []
        assert torch.equal(y, F.linear(x[:-1], lin.weight, lin.bias))
        lin(x)
        assert calls == ["apply"]


LIN_SHAPES = [((65536, 131), 64, True), ((65536, 64), 64, True),
              ((65536, 64), 1, False), ((65536, 1), 64, True),
              ((65536, 50), 64, True), ((2, 32768, 64), 64, True)]


@pytest.mark.parametrize("mode", ["autocast", "bf16", "fp32"])
@pytest.mark.parametrize("xshape,o,bias", LIN_SHAPES)
def test_splitk_linear_end_to_end(xshape, o, bias, mode, monkeypatch):
    k = xshape[-1]
    m = 65536
    torch.manual_seed(k + o)
    lin = L.SplitKLinear(k, o, bias=bias).to(DEV)
    in_dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x = _rand(xshape, 23 * k + o, 0.5, in_dt).requires_grad_(True)
    fn_calls = _spy(monkeypatch, L._SplitKLinearFn, "apply")
    ext_calls = []
    for name in ("tall_linear", "wgrad_splitk"):
        _spy(monkeypatch, ops.hip_ext(), name, ext_calls)
    if mode == "autocast":
        with torch.autocast("cuda", torch.bfloat16):
            y = lin(x)
    else:
        y = lin(x)
    cd = torch.float32 if mode == "fp32" else torch.bfloat16
    gout = _rand(y.shape, 29 * k + o, 1.0, cd)
    y.backward(gout)
    assert fn_calls == ["apply"]
    if mode == "fp32":
        assert ext_calls == []          # fp32 never reaches the extension
    else:
        assert ext_calls.count("tall_linear") == 2
        assert ext_calls.count("wgrad_splitk") == (1 if o == 64 else 0)

    # float64 autograd on the operands as the compute dtype sees them
    x64 = x.detach().to(cd).double().reshape(m, k).requires_grad_(True)
    w64 = lin.weight.detach().to(cd).double().requires_grad_(True)
    b64 = (lin.bias.detach().to(cd).double().requires_grad_(True)
           if bias else None)
    g64 = gout.double().reshape(m, o)
    y64 = F.linear(x64, w64, b64)
    y64.backward(g64)
    ax, aw, ag = x64.detach().abs(), w64.detach().abs(), g64.abs()
    mag_y = ax @ aw.t() + (b64.detach().abs() if bias else 0.0)
    mag_gx, mag_gw, sum_g = ag @ aw, ag.t() @ ax, ag.sum(0)
    yw, gxw = y64.detach(), x64.grad

    assert y.dtype == cd and y.shape == (*xshape[:-1], o)
    assert x.grad.dtype == in_dt and x.grad.shape == x.shape
    assert lin.weight.grad.dtype == torch.float32
    tag = f"d lin {tuple(xshape)}->{o} {mode}"
    if mode == "fp32":
        by = (k + 1) * U23 * mag_y
        bgx = (o + 1) * U23 * mag_gx
        bgw = m * U23 * mag_gw
        bgb = m * U23 * sum_g
    else:
        by = U8 * yw.abs() + 2 * (k + 1) * U23 * mag_y
        bgx = U8 * gxw.abs() + 2 * (o + 1) * U23 * mag_gx
        bgw = m * U23 * mag_gw if o == 64 else 2 * U8 * mag_gw
        bgb = U8 * (b64.grad.abs() if bias else 0.0) + m * U23 * sum_g
    _check(tag + " y", y.detach().reshape(m, o), yw, by)
    _check(tag + " gx", x.grad.reshape(m, k), gxw, bgx)
    _check(tag + " gw", lin.weight.grad, w64.grad, bgw)
    if bias:
        assert lin.bias.grad.dtype == torch.float32
        _check(tag + " gb", lin.bias.grad, b64.grad, bgb)


# ---------------------------------------------------------------- (e)
def _lin_reference(lin, x, gout):
    x64 = x.detach().double().requires_grad_(True)
    w64 = lin.weight.detach().bfloat16().double()
    b64 = lin.bias.detach().bfloat16().double()
    y64 = F.linear(x64, w64, b64)
    y64.backward(gout.double())
    ax, aw = x64.detach().abs(), w64.abs()
    by = U8 * y64.detach().abs() \
        + 2 * (x.size(1) + 1) * U23 * (ax @ aw.t() + b64.abs())
    bgx = U8 * x64.grad.abs() \
        + 2 * (w64.size(0) + 1) * U23 * (gout.double().abs() @ aw)
    return y64.detach(), x64.grad, by, bgx


def test_weight_cache_follows_inplace_update():
    """forward+backward, in-place parameter update, forward+backward again
    WITHOUT refresh(): y must come from the new bf16 copy and x.grad from
    the new transposed bf16 copy."""
    prep.clear()
    torch.manual_seed(0)
    m = L._MIN_ROWS
    lin = L.SplitKLinear(131, 64).to(DEV)
    g = torch.Generator().manual_seed(5)
    # positive operands: the 0.25 shift moves every y by >= 0.25*(13+1)
    # and every x.grad by >= 0.25*6.4, hundreds of bf16 ulps
    x = (torch.rand(m, 131, generator=g) + 0.1).bfloat16().to(DEV)
    gout = (torch.rand(m, 64, generator=g) + 0.1).bfloat16().to(DEV)

    def run():
        xi = x.clone().requires_grad_(True)
        y = lin(xi)
        y.backward(gout)
        return y.detach(), xi.grad

    y_old, gx_old = run()
    assert len(prep._CACHE) == 3        # weight bf16 + t_bf16, bias bf16
    ptrs = {k: e[1].data_ptr() for k, e in prep._CACHE.items()}
    with torch.no_grad():
        lin.weight.add_(0.25)
        lin.bias.add_(0.25)
    assert prep.any_stale()
    y_new, gx_new = run()
    assert not prep.any_stale()
    assert ptrs == {k: e[1].data_ptr() for k, e in prep._CACHE.items()}
    yw, gxw, by, bgx = _lin_reference(lin, x, gout)
    _check("e cache y", y_new, yw, by)
    _check("e cache gx", gx_new, gxw, bgx)
    # the stale results are far outside the same bounds
    assert float(((y_old.double() - yw).abs() / by).min()) > 10
    assert float(((gx_old.double() - gxw).abs() / bgx).min()) > 10


def test_weight_cache_buffers_and_refresh():
    prep.clear()
    w = torch.nn.Parameter(_rand((64, 131), 3, 1.0, torch.float32))
    kinds = ("bf16", "t_bf16", "pad_kpad", "tpad_kout")
    ptrs = [prep.get(w, kd).data_ptr() for kd in kinds]
    assert len(prep._CACHE) == 4 and not prep.any_stale()
    assert prep.refresh() == 0
    with torch.no_grad():
        w.add_(0.5)
    assert prep.any_stale()
    assert prep.refresh() == 4
    assert not prep.any_stale()
    assert prep.refresh() == 0
    with torch.no_grad():
        w.add_(0.5)
    assert prep.any_stale()
    for kd, p in zip(kinds, ptrs):      # eager path: get() itself refreshes
        buf = prep.get(w, kd)
        assert buf.data_ptr() == p, kd
        assert torch.equal(buf, prep._TRANSFORMS[kd](w)), kd
    assert not prep.any_stale()
    # a no-op transform is passed through and not cached
    b = torch.nn.Parameter(_rand((64,), 4, 1.0, torch.float32))
    n = len(prep._CACHE)
    assert prep.get(b, "f32").data_ptr() == b.data_ptr()
    assert len(prep._CACHE) == n
    prep.clear()


def _edge_params(hdim, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(hdim, 2 * hdim + 3), (hdim,), (hdim, hdim), (hdim,),
              (hdim, hdim), (hdim,), (hdim,)]
    scales = [0.08, 0.05, 0.1, 0.05, 0.1, 0.05, 0.05]
    return [(torch.randn(*s, generator=g) * c).to(DEV)
            for s, c in zip(shapes, scales)]


def test_fused_edge_block_tracks_inplace_update(monkeypatch):
    prep.clear()
    bt = collate(make_cutoff_dataset("Water-3D", 1, seed=7,
                                     n_override=300)).to(DEV)
    params = _edge_params(64, 0)
    h0 = _rand((bt.num_nodes, 64), 21, 0.5)

    def run(ps):
        h = h0.clone().requires_grad_(True)
        coord = bt.pos.detach().clone().requires_grad_(True)
        am, at = ops.fused_edge_block(
            h, coord, bt.edge_attr, bt.edge_index[0], bt.edge_index[1],
            bt.rowptr, bt.colptr, bt.col_perm, *ps, False, 1e-8)
        (am.float().pow(2).sum() + at.pow(2).sum()).backward()
        return am.detach().float(), at.detach(), h.grad.float(), coord.grad

    old = run(params)
    assert len(prep._CACHE) > 0
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in params:
            # as large as the weights themselves (scales 0.05..0.1):
            # most elements of the message and of h.grad move by more
            # than their gates
            p.add_((torch.randn(p.shape, generator=g) * 0.15).to(DEV))
    new = run(params)                   # no refresh() in between
    monkeypatch.setenv("DISTEGNN_DISABLE_FUSED", "1")
    ref = run([p.detach().clone() for p in params])
    monkeypatch.delenv("DISTEGNN_DISABLE_FUSED")
    assert torch.allclose(new[0], ref[0], atol=0.03, rtol=0.05), \
        (new[0] - ref[0]).abs().max()
    assert torch.allclose(new[1], ref[1], atol=0.03, rtol=0.05)
    assert torch.allclose(new[2], ref[2], atol=0.2, rtol=0.1)
    assert torch.allclose(new[3], ref[3], atol=0.2, rtol=0.1)
    # the update is visible at these gates: most elements of the message
    # and of h.grad of the old weights miss them (0.90 and 0.86 on an
    # MI355X, while the new results use under 0.15 of every gate).
    # coord.grad is too small here for its 0.2 gate to tell old from
    # new, so it says nothing about a stale backward copy; the
    # content of the tpad_kout/t_bf16 buffers after an update is checked
    # in test_weight_cache_buffers_and_refresh.
    for name, o, r, atol, rtol, sees in (
            ("msg", old[0], ref[0], 0.03, 0.05, True),
            ("h.grad", old[2], ref[2], 0.2, 0.1, True),
            ("coord.grad", old[3], ref[3], 0.2, 0.1, False)):
        over = ((o - r).abs() > atol + rtol * r.abs()).float().mean()
        print(f"STALE e edge-block {name}: {float(over):.3f} of the "
              f"elements of the old result miss the gate")
        if sees:
            assert float(over) > 0.5, name
    prep.clear()


# ---------------------------------------------------------------- (f)
@pytest.mark.parametrize("hdim", [64, 32])
def test_fused_edge_block_without_edges(hdim):
    n = 70
    empty = torch.zeros(0, dtype=torch.long, device=DEV)
    ptr = torch.zeros(n + 1, dtype=torch.long, device=DEV)
    eattr = torch.zeros(0, 2, device=DEV)
    ps = [p.requires_grad_(True) for p in _edge_params(hdim, 2)]
    h = _rand((n, hdim), 1, 0.5).requires_grad_(True)
    coord = _rand((n, 3), 2, 1.0, torch.float32).requires_grad_(True)
    am, at = ops.fused_edge_block(h, coord, eattr, empty, empty, ptr, ptr,
                                  empty, *ps, True, 1e-8)
    assert am.shape == (n, hdim) and at.shape == (n, 3)
    assert bool((am == 0).all()) and bool((at == 0).all())
    c1 = _rand((n, hdim), 3, 1.0, torch.float32)
    c2 = _rand((n, 3), 4, 1.0, torch.float32)
    ((am.float() * c1).sum() + (at * c2).sum()).backward()
    for t in [h, coord] + ps:
        assert t.grad is not None and t.grad.shape == t.shape
        assert bool(torch.isfinite(t.grad.float()).all())
        assert bool((t.grad == 0).all())
