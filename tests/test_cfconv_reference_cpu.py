"""The float64 CFConv reference (distegnn_amd/ops/cfconv_reference.py)
against the plain composition of the modules in models/schnet.py —
GaussianSmearing -> Linear -> ShiftedSoftplus -> Linear -> cosine cutoff ->
gather -> multiply — and its autograd, all in float64 on the CPU."""

import math

import pytest
import torch
from torch import nn

from distegnn_amd.models.schnet import GaussianSmearing, ShiftedSoftplus
from distegnn_amd.ops import cfconv_reference as CR


def _inputs(f, g, m, n, seed):
    gen = torch.Generator().manual_seed(seed)
    cutoff = 5.0
    sm = GaussianSmearing(0.0, cutoff, g).double()
    # weights on bf16 values: the reference's rounding is then the identity
    bf = lambda t: t.bfloat16().double()
    w1 = bf(torch.randn(f, g, generator=gen) * 0.3)
    w2 = bf(torch.randn(f, f, generator=gen) * 0.2)
    b1 = torch.randn(f, generator=gen).double() * 0.3
    b2 = torch.randn(f, generator=gen).double() * 0.3
    xw1 = bf(torch.randn(n, f, generator=gen))
    dist = (torch.rand(m, generator=gen) * 1.5 * cutoff).double()
    col = torch.randint(0, n, (m,), generator=gen)
    return sm, cutoff, [xw1, w1, b1, w2, b2], dist, col


def _composition(sm, cutoff, leaves, dist, col):
    xw1, w1, b1, w2, b2 = leaves
    lin1, lin2 = nn.Linear(w1.size(1), w1.size(0)), nn.Linear(*w2.shape)
    lin1, lin2 = lin1.double(), lin2.double()
    # the modules' own forward, with the leaves as their parameters
    filt = torch.func.functional_call(
        nn.Sequential(lin1, ShiftedSoftplus(), lin2),
        {"0.weight": w1, "0.bias": b1, "2.weight": w2, "2.bias": b2},
        (sm(dist),))
    c = 0.5 * (torch.cos(dist * math.pi / cutoff) + 1.0)
    return xw1.index_select(0, col) * (filt * c.view(-1, 1))


@pytest.mark.parametrize("f,g", [(64, 50), (128, 33), (64, 2)])
def test_reference_matches_composition_and_autograd(f, g):
    m, n = 300, 40
    sm, cutoff, leaves, dist, col = _inputs(f, g, m, n, seed=f + g)
    la = [t.clone().requires_grad_(True) for t in leaves]
    lb = [t.clone().requires_grad_(True) for t in leaves]
    st = CR.cfconv_stages(la[0], dist, col, la[1], la[2], la[3], la[4],
                          sm.offset, sm.coeff, cutoff)
    want = _composition(sm, cutoff, lb, dist, col)
    assert st["msg"].dtype == torch.float64
    scale = float(want.detach().abs().max())
    assert float((st["msg"] - want).detach().abs().max()) <= 1e-13 * scale
    assert torch.allclose(st["gauss"], sm(dist), rtol=1e-12, atol=1e-300)
    assert st["cf"].shape == (m,) and st["z1"].shape == (m, f)
    gout = torch.randn(m, f, generator=torch.Generator().manual_seed(1),
                       dtype=torch.float64)
    ga = torch.autograd.grad(st["msg"], la, gout)
    gb = torch.autograd.grad(want, lb, gout)
    for a, b in zip(ga, gb):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_reference_rounds_weights_like_prep():
    """Unrounded weights give the result of their bf16 roundings, and the
    gradient passes the rounding unchanged."""
    sm, cutoff, leaves, dist, col = _inputs(64, 50, 100, 20, seed=3)
    xw1, w1, b1, w2, b2 = leaves
    gen = torch.Generator().manual_seed(4)
    w1r = (w1 + torch.randn(w1.shape, generator=gen).double() * 1e-4)
    w2r = (w2 + torch.randn(w2.shape, generator=gen).double() * 1e-4)
    args = (sm.offset, sm.coeff, cutoff)
    a = CR.cfconv_msg(xw1, dist, col, w1r, b1, w2r, b2, *args)
    b = CR.cfconv_msg(xw1, dist, col, w1r.bfloat16().double(), b1,
                      w2r.bfloat16().double(), b2, *args)
    assert torch.equal(a, b)
    w = w2r.clone().requires_grad_(True)
    wq = w2r.bfloat16().double().requires_grad_(True)
    ga, = torch.autograd.grad(
        CR.cfconv_msg(xw1, dist, col, w1r, b1, w, b2, *args).sum(), w)
    gb, = torch.autograd.grad(
        CR.cfconv_msg(xw1, dist, col, w1r, b1, wq, b2, *args).sum(), wq)
    assert torch.equal(ga, gb)


def test_reference_edges_of_the_domain():
    """d = 0, d = cutoff (message exactly ~0), beyond the cutoff (no mask),
    far beyond (every gaussian 0: z1 = ssp(b1)), softplus tails."""
    sm, cutoff, leaves, _, _ = _inputs(64, 50, 1, 8, seed=5)
    xw1, w1, b1, w2, b2 = leaves
    b1 = b1.clone()
    b1[:4] = torch.tensor([30.0, -30.0, 90.0, -90.0], dtype=torch.float64)
    dist = torch.tensor([0.0, cutoff, 1.5 * cutoff, 100 * cutoff],
                        dtype=torch.float64)
    col = torch.tensor([0, 7, 3, 3])
    st = CR.cfconv_stages(xw1, dist, col, w1, b1, w2, b2, sm.offset,
                          sm.coeff, cutoff)
    assert all(bool(torch.isfinite(v).all()) for v in st.values())
    assert float(st["cf"][0]) == 1.0
    assert abs(float(st["cf"][1])) < 1e-30
    assert abs(float(st["cf"][2]) - 0.5) < 1e-15       # cos(1.5 pi) = 0
    assert float(st["msg"][1].abs().max()) < 1e-28
    assert float(st["gauss"][3].max()) == 0.0
    ssp = torch.log1p(torch.exp(-b1.abs())) + b1.clamp(min=0) - math.log(2)
    assert float((st["z1"][3] - ssp).abs().max()) < 1e-14
    assert abs(float(st["z1"][3, 2]) - (90 - math.log(2))) < 1e-13
    assert abs(float(st["z1"][3, 3]) + math.log(2)) < 1e-13
