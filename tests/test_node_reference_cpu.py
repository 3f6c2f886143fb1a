"""CPU check of distegnn_amd/ops/node_reference.py, the float64 reference
of the fused node block (csrc/fused_node.hip): the exact chain (no
rounding) against the ``nn.Sequential`` composition the model ran before
the block was fused, outputs and every gradient via ``torch.autograd``, in
float64. Both agree to rounding of the float64 sums; 1e-12 relative to the
largest entry leaves three orders of magnitude over the observed 1e-15."""

import pytest
import torch
from torch import nn

from distegnn_amd import ops
from distegnn_amd.ops import node_reference as NR

TOL = 1e-12


def _mlps(hd, a, seed):
    g = torch.Generator().manual_seed(seed)
    node_mlp = nn.Sequential(nn.Linear(3 * hd + a, hd), nn.SiLU(),
                             nn.Linear(hd, hd)).double()
    vel_mlp = nn.Sequential(nn.Linear(hd, hd), nn.SiLU(),
                            nn.Linear(hd, 1)).double()
    with torch.no_grad():
        for p in list(node_mlp.parameters()) + list(vel_mlp.parameters()):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64)
                    * 0.3)
    return node_mlp, vel_mlp


def _close(tag, got, want):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max()) / scale
    assert err <= TOL, (tag, err)


@pytest.mark.parametrize("a,vel_only", [(0, False), (2, False), (0, True)])
def test_reference_matches_composition_and_autograd(a, vel_only):
    hd, n = 16, 37
    g = torch.Generator().manual_seed(3)
    node_mlp, vel_mlp = _mlps(hd, a, 5)
    h, agg_e, agg_v = (torch.randn(n, hd, generator=g, dtype=torch.float64,
                                   ).requires_grad_() for _ in range(3))
    attr = (torch.randn(n, a, generator=g, dtype=torch.float64)
            if a else None)
    dh_out = torch.randn(n, hd, generator=g, dtype=torch.float64)
    dphiv = torch.randn(n, 1, generator=g, dtype=torch.float64)

    # the composition, through the dispatcher's CPU path
    h_out, phiv = ops.fused_node_block(h, agg_e, agg_v, attr, node_mlp,
                                       vel_mlp, True, vel_only=vel_only)
    params = [node_mlp[0].weight, node_mlp[0].bias, node_mlp[2].weight,
              node_mlp[2].bias, vel_mlp[0].weight, vel_mlp[0].bias,
              vel_mlp[2].weight, vel_mlp[2].bias]
    w1, b1, w2, b2, wv1, bv1, wv2m, bv2 = [p.detach() for p in params]
    wv2 = wv2m.reshape(-1)

    r_h_out, r_phiv = NR.node_block(h.detach(), agg_e.detach(),
                                    agg_v.detach(), attr, w1, b1, w2, b2,
                                    wv1, bv1, wv2, bv2, vel_only=vel_only)
    _close("phiv", r_phiv, phiv.detach())
    _close("h_out", r_h_out, h_out.detach())

    f = NR.node_forward(h.detach(), agg_e.detach(), agg_v.detach(), attr,
                        w1, b1, w2, b2, wv1, bv1, wv2, bv2,
                        vel_only=vel_only)
    gr = NR.node_backward(f, dh_out, dphiv, h.detach(), w1, w2, wv1, wv2,
                          vel_only=vel_only)
    if vel_only:
        ins, names = [h] + params[4:], ["dh", "gwv1", "gbv1", "gwv2", "gbv2"]
        grads = torch.autograd.grad(phiv, ins, dphiv)
    else:
        ins = [h, agg_e, agg_v] + params
        names = ["dh", "dagg_e", "dagg_v", "gw1", "gb1", "gw2", "gb2",
                 "gwv1", "gbv1", "gwv2", "gbv2"]
        grads = torch.autograd.grad([h_out, phiv], ins, [dh_out, dphiv])
    for name, want in zip(names, grads):
        _close(name, gr[name].reshape(want.shape), want)


def test_bf16_round_is_idempotent_and_nearest():
    t = torch.tensor([1.0, 1.00390625, 1.001953125, -3.14159], dtype=torch.float64)
    r = NR.bf16_round(t)
    assert r.dtype == torch.float64
    assert torch.equal(NR.bf16_round(r), r)
    assert torch.equal(r, t.bfloat16().double())
