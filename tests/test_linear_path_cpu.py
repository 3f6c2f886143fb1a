"""CPU tests of the split-K linear path (ops/linear.py, ops/prep.py and
the parameter broadcast that feeds the weight cache).

Every reference is float64, computed from the same already-rounded inputs
the code under test receives, and every bound is derived from the number
formats:

* fp32 result of an M-term dot product, any summation order:
  ``M * 2^-23 * mag`` with ``mag = |g|^T |x|`` (first-order bound
  ``(M-1) * u * mag`` with u = 2^-24, doubled for a non-round-to-nearest
  accumulate).
* bf16 result of the torch branches: ``2 * 2^-8 * mag``. One rounding to
  bf16 costs at most ``2^-8`` of the value it rounds (half an ulp). Every
  chunk partial is bounded by its share of ``mag``, so rounding all of them
  costs at most ``2^-8 * mag`` together; rounding their sum costs another
  ``2^-8 * mag`` at most.
"""

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from distegnn_amd.ops import linear as L
from distegnn_amd.ops import prep
from distegnn_amd.parallel import comm

U23 = 2.0 ** -23
U8 = 2.0 ** -8

WGRAD_SHAPES = [(0, 64, 144), (1, 64, 131), (63, 64, 64), (64, 64, 64),
                (65, 32, 67), (4097, 64, 131), (200, 1, 64), (200, 8, 64),
                (130, 16, 3), (4160, 128, 259)]


def _rand(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _ratio(err, bound):
    """max err/bound; an element with bound 0 must have err 0."""
    assert bool((err[bound == 0] == 0).all())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,o,i", WGRAD_SHAPES)
def test_chunked_wgrad_torch_branches(m, o, i, dtype):
    g = _rand((m, o), 1000 + m + o, dtype)
    x = _rand((m, i), 2000 + m + i, dtype)
    got = L.chunked_wgrad(g, x)
    # the torch branches return the INPUT dtype (the HIP kernel returns
    # fp32) — pinned here so the difference stays visible
    assert got.dtype == dtype
    assert got.shape == (o, i)
    want = g.double().t() @ x.double()
    mag = g.double().abs().t() @ x.double().abs()
    bound = (m * U23 if dtype == torch.float32 else 2 * U8) * mag
    err = (got.double() - want).abs()
    r = _ratio(err, bound)
    print(f"chunked_wgrad {dtype} M={m} O={o} I={i}: err/bound={r:.4f}")
    assert r <= 1.0
    if m == 0:
        assert torch.equal(got, torch.zeros(o, i, dtype=dtype))


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,k,o,bias", [(300, 67, 64, True),
                                        (130, 64, 1, False),
                                        (257, 1, 64, True)])
def test_splitk_fn_cpu_matches_float64(m, k, o, bias, dt):
    """_SplitKLinearFn on CPU tensors: output and all three gradients
    against float64 F.linear autograd on the rounded operands."""
    cd = torch.float32 if dt is None else dt
    x = _rand((m, k), 1, cd).requires_grad_(True)
    w = _rand((o, k), 2, torch.float32, 0.3).requires_grad_(True)
    b = _rand((o,), 3, torch.float32, 0.3).requires_grad_(True) \
        if bias else None
    gout = _rand((m, o), 4, cd)
    y = L._SplitKLinearFn.apply(x, w, b, dt)
    y.backward(gout)

    x64 = x.detach().double().requires_grad_(True)
    w64 = w.detach().to(cd).double().requires_grad_(True)
    b64 = b.detach().to(cd).double().requires_grad_(True) if bias else None
    y64 = F.linear(x64, w64, b64)
    y64.backward(gout.double())
    ax, aw, ag = (x64.detach().abs(), w64.detach().abs(),
                  gout.double().abs())
    mag_y = ax @ aw.t() + (b64.detach().abs() if bias else 0.0)
    mag_gx = ag @ aw
    mag_gw = ag.t() @ ax
    mag_gb = ag.sum(0)

    assert y.dtype == cd
    assert x.grad.dtype == cd                 # gx in compute dtype
    assert w.grad.dtype == torch.float32      # parameter grads in
    if bias:                                  # parameter dtype
        assert b.grad.dtype == torch.float32
    if dt is None:
        bounds = [(k + 1) * U23 * mag_y, o * U23 * mag_gx,
                  m * U23 * mag_gw, m * U23 * mag_gb]
    else:
        # bf16 results (unit roundoff u8): the final rounding costs
        # u8*|v| of the value v it rounds, |v| <= |want| + e for the
        # error e made before it, hence u8*|want| + (1 + u8)*e.
        # y: e = the fp32 accumulation, plus u8*mag for the bf16
        #    product that the bias is then added to.
        # gx, gb: one rounding of an fp32 accumulation.
        # gw: the torch branches of chunked_wgrad round every chunk
        #    partial and two full-size sums (main, main + remainder);
        #    neither sum is bounded by |want|, so 2*u8*mag as above.
        acc_y = 2 * (k + 1) * U23 * mag_y
        acc_gx = 2 * (o + 1) * U23 * mag_gx
        acc_gb = m * U23 * mag_gb
        mid_y = U8 * mag_y if bias else 0.0
        bounds = [U8 * y64.detach().abs() + (1 + U8) * (mid_y + acc_y),
                  U8 * x64.grad.abs() + (1 + U8) * acc_gx,
                  2 * U8 * mag_gw,
                  U8 * (b64.grad.abs() if bias else 0.0)
                  + (1 + U8) * acc_gb]
    pairs = [("y", y.detach(), y64.detach(), bounds[0]),
             ("gx", x.grad, x64.grad, bounds[1]),
             ("gw", w.grad, w64.grad, bounds[2])]
    if bias:
        pairs.append(("gb", b.grad, b64.grad, bounds[3]))
    for name, got, want, bound in pairs:
        assert got.shape == want.shape, name
        r = _ratio((got.double() - want).abs(), bound)
        print(f"_SplitKLinearFn {cd} {m}x{k}->{o} {name}: "
              f"err/bound={r:.4f}")
        assert r <= 1.0, name


@pytest.mark.parametrize("k,o,bias", [(131, 64, True), (64, 1, False),
                                      (1, 64, True)])
def test_splitk_linear_small_input_is_nn_linear(k, o, bias):
    """Below _MIN_ROWS (and on CPU at any size) the module IS nn.Linear:
    bit-equal output, identical state-dict keys."""
    torch.manual_seed(0)
    ref = nn.Linear(k, o, bias=bias)
    lin = L.SplitKLinear(k, o, bias=bias)
    assert list(lin.state_dict().keys()) == list(ref.state_dict().keys())
    lin.load_state_dict(ref.state_dict())
    for shape in [(L._MIN_ROWS - 1, k), (7, k), (2, 5, k), (k,)]:
        x = torch.randn(*shape)
        assert torch.equal(lin(x), ref(x))


@pytest.mark.parametrize("k_in", [67, 131, 259, 137])
def test_prep_transforms_match_definitions(k_in):
    o = 64
    w = _rand((o, k_in), k_in, torch.float32)
    wb = w.bfloat16()

    kp = prep.pad_kpad(w)
    k_pad = -(-k_in // 32) * 32
    assert kp.shape == (o, k_pad) and kp.dtype == torch.bfloat16
    assert kp.is_contiguous()
    assert torch.equal(kp[:, :k_in], wb)
    assert bool((kp[:, k_in:] == 0).all())

    tk = prep.tpad_kout(w)
    k_out = -(-k_in // 16) * 16
    assert tk.shape == (k_out, o) and tk.dtype == torch.bfloat16
    assert tk.is_contiguous()
    assert torch.equal(tk[:k_in], wb.t())
    assert bool((tk[k_in:] == 0).all())

    tb = prep.t_bf16(w)
    assert tb.shape == (k_in, o) and tb.dtype == torch.bfloat16
    assert tb.is_contiguous()
    assert torch.equal(tb, wb.t())

    # pad_gpad pads the gaussian (column) dimension G <= 64 of a
    # [F, G] filter weight to 64; F takes the K_IN values here
    for g_dim in (1, 50, 64):
        f = _rand((k_in, g_dim), k_in + g_dim, torch.float32)
        gp = prep.pad_gpad(f)
        assert gp.shape == (k_in, 64) and gp.dtype == torch.bfloat16
        assert gp.is_contiguous()
        assert torch.equal(gp[:, :g_dim], f.bfloat16())
        assert bool((gp[:, g_dim:] == 0).all())


def test_prep_get_cpu_does_not_cache():
    prep.clear()
    w = torch.randn(64, 131)
    for kind in ("bf16", "t_bf16", "pad_kpad", "tpad_kout"):
        a = prep.get(w, kind)
        b = prep.get(w, kind)
        assert a.data_ptr() != b.data_ptr(), kind
        assert torch.equal(a, b)
        assert torch.equal(a, prep._TRANSFORMS[kind](w))
    assert prep._CACHE == {}
    assert not prep.any_stale()
    assert prep.refresh() == 0


def test_broadcast_parameters_bumps_version(monkeypatch):
    """The broadcast write-back must move every parameter's version
    counter: prep.get keys its bf16 weight copies on it."""
    monkeypatch.setattr(comm, "is_distributed", lambda: True)
    monkeypatch.setattr(comm.dist, "broadcast", lambda *a, **k: None)
    torch.manual_seed(0)
    model = nn.Sequential(L.SplitKLinear(5, 7), nn.SiLU(),
                          L.SplitKLinear(7, 1, bias=False))
    params = list(model.parameters())
    before_v = [p._version for p in params]
    before = [p.detach().clone() for p in params]
    comm.GradBucket(model).broadcast_parameters()
    for p, v, val in zip(params, before_v, before):
        assert p._version > v
        assert torch.equal(p.detach(), val)
        assert p.requires_grad and p.is_leaf
