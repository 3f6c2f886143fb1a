"""Stage-by-stage reference of the fused virtual-edge block (forward).

Plain torch in whatever dtype the inputs carry (the tests pass float64), the
companion of ``edge_reference`` for csrc/fused_virtual.hip and
csrc/fused_virtual_f32.hip. ``ops.eager_virtual_block`` narrows the two
heads with ``.float()`` and so cannot serve as a float64 reference; nothing
here changes a dtype. tests/test_virtual_reference_cpu.py holds it against
``ops.eager_virtual_block`` in fp32.

Chain (row r = (node n, channel c), b = batch[n]):

  vdiff = X[b,c] - x_n       vrad = |vdiff|
  vin = [h_n | Z[b,c] | vrad | gram[b,c,:]]
  z1  = vin  W1^T + b1       t1   = silu(z1)
  z2  = t1   W2^T + b2       vmsg = silu(z2)
  zxv = vmsg Wxv^T + bxv     pxv  = silu(zxv) . wxvv
  zX  = vmsg WX^T  + bX      pX   = silu(zX)  . wXv
  tv = -vdiff pxv            tx = vdiff pX
"""

from __future__ import annotations

import torch

from .edge_reference import preact, silu


def geometry(coord, vcoord, batch):
    """vdiff [N,C,3], vrad [N,C]."""
    vdiff = vcoord.index_select(0, batch) - coord.unsqueeze(1)
    return vdiff, (vdiff * vdiff).sum(-1).sqrt()


def virtual_input(h, vfeat, vrad, gram, batch):
    """vin [N,C,2H+1+C]."""
    n, c = vrad.shape
    return torch.cat([h.unsqueeze(1).expand(n, c, h.size(1)),
                      vfeat.index_select(0, batch),
                      vrad.unsqueeze(-1),
                      gram.index_select(0, batch)], dim=-1)


def virtual_forward(h, coord, vcoord, vfeat, gram, batch,
                    w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv):
    """Every forward stage, unrounded, [N,C,.] each. Returns a dict."""
    vdiff, vrad = geometry(coord, vcoord, batch)
    vin = virtual_input(h, vfeat, vrad, gram, batch)
    z1 = preact(vin, w1, b1)
    t1 = silu(z1)
    z2 = preact(t1, w2, b2)
    vmsg = silu(z2)
    zxv = preact(vmsg, wxv, bxv)
    zX = preact(vmsg, wX, bX)
    pxv = silu(zxv) @ wxvv
    pX = silu(zX) @ wXv
    return dict(vdiff=vdiff, vrad=vrad, vin=vin, z1=z1, t1=t1, z2=z2,
                vmsg=vmsg, zxv=zxv, zX=zX, pxv=pxv, pX=pX,
                tv=-vdiff * pxv.unsqueeze(-1), tx=vdiff * pX.unsqueeze(-1))


def virtual_block(h, coord, vcoord, vfeat, gram, batch,
                  w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv):
    """(v_msg [N,C,H], tv [N,C,3], tx [N,C,3]): the return of
    ``ops.eager_virtual_block``, in the dtype of the inputs."""
    f = virtual_forward(h, coord, vcoord, vfeat, gram, batch,
                        w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv)
    return f["vmsg"], f["tv"], f["tx"]
