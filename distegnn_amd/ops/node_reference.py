"""Stage-by-stage reference of the fused node block and its backward.

Plain torch in whatever dtype the inputs carry (the tests pass float64), the
companion of ``edge_reference`` / ``virtual_reference`` for
csrc/fused_node.hip. Every function takes a ``rnd`` callable that is applied
at the rounding points of the kernels (and of the composition they
replace): the identity gives the exact chain, ``bf16_round`` the chain as
the bf16 kernels round it. tests/test_node_reference_cpu.py holds the exact
chain against the ``nn.Sequential`` composition and ``torch.autograd``.

Chain (one row per node; ``attr`` may be None):

  xin = [h | agg_e | agg_v | attr]
  z1 = xin W1^T + b1     t1  = silu(z1)
  out = t1 W2^T + b2     h_out = h + out
  zv = h Wv1^T + bv1     tv  = silu(zv)     phiv = tv . wv2 + bv2

  dtv = dphiv wv2        dzv = dtv silu'(zv)
  dt1 = dh_out W2        dz1 = dt1 silu'(z1)
  din = dz1 W1 = [din_h | dagg_e | dagg_v | .]
  dh  = dh_out + din_h + dzv Wv1
  gW1 = dz1^T xin   gW2 = dh_out^T t1   gWv1 = dzv^T h   gwv2 = dphiv^T tv
  gb1 = sum dz1     gb2 = sum dh_out    gbv1 = sum dzv   gbv2 = sum dphiv

Rounding points: z1, t1, out, h + out, zv, tv, phiv; dt1, dz1, dtv, dzv.
The vel-only mode (a layer whose feature update is skipped) is the vel
chain alone, with dh = dzv Wv1.
"""

from __future__ import annotations

import torch

from .edge_reference import dsilu, preact, silu


def identity(t):
    return t


def bf16_round(t):
    """Round to the nearest bf16 value, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def node_input(h, agg_e, agg_v, attr=None):
    parts = [h, agg_e, agg_v]
    if attr is not None and attr.size(1) > 0:
        parts.append(attr.to(h.dtype))
    return torch.cat(parts, dim=1)


def vel_forward(h, wv1, bv1, wv2, bv2, rnd=identity):
    """wv2 [H], bv2 [1]. Returns dict(zv, tv, phiv [N,1])."""
    zv = rnd(preact(h, wv1, bv1))
    tv = rnd(silu(zv))
    phiv = rnd((tv @ wv2).unsqueeze(1) + bv2)
    return dict(zv=zv, tv=tv, phiv=phiv)


def node_forward(h, agg_e, agg_v, attr, w1, b1, w2, b2, wv1, bv1, wv2, bv2,
                 rnd=identity, vel_only=False):
    """Every forward stage as a dict; ``vel_only`` leaves the node chain
    out."""
    f = vel_forward(h, wv1, bv1, wv2, bv2, rnd)
    if vel_only:
        return f
    xin = node_input(h, agg_e, agg_v, attr)
    z1 = rnd(preact(xin, w1, b1))
    t1 = rnd(silu(z1))
    out = rnd(preact(t1, w2, b2))
    f.update(xin=xin, z1=z1, t1=t1, out=out, h_out=rnd(h + out))
    return f


def node_backward(f, dh_out, dphiv, h, w1, w2, wv1, wv2, rnd=identity,
                  vel_only=False):
    """Backward of ``node_forward`` from its stage dict ``f``. dphiv [N,1].
    Returns a dict of every data and parameter gradient."""
    hd = h.size(1)
    dtv = rnd(dphiv * wv2.unsqueeze(0))
    dzv = rnd(dtv * dsilu(f["zv"]))
    g = dict(dzv=dzv, gwv1=dzv.t() @ h, gbv1=dzv.sum(0),
             gwv2=(dphiv * f["tv"]).sum(0), gbv2=dphiv.sum(0))
    dh_v = dzv @ wv1
    if vel_only:
        g["dh"] = dh_v
        return g
    dt1 = rnd(dh_out @ w2)
    dz1 = rnd(dt1 * dsilu(f["z1"]))
    din = dz1 @ w1
    g.update(dt1=dt1, dz1=dz1,
             dh=dh_out + din[:, :hd] + dh_v,
             dagg_e=din[:, hd:2 * hd], dagg_v=din[:, 2 * hd:3 * hd],
             gw1=dz1.t() @ f["xin"], gb1=dz1.sum(0),
             gw2=dh_out.t() @ f["t1"], gb2=dh_out.sum(0))
    return g


def node_block(h, agg_e, agg_v, attr, w1, b1, w2, b2, wv1, bv1, wv2, bv2,
               rnd=identity, vel_only=False):
    """(h_out [N,H], phiv [N,1]): the return of ``ops.fused_node_block``;
    ``h_out`` is ``h`` itself in vel-only mode."""
    f = node_forward(h, agg_e, agg_v, attr, w1, b1, w2, b2, wv1, bv1, wv2,
                     bv2, rnd, vel_only)
    return (h if vel_only else f["h_out"]), f["phiv"]
