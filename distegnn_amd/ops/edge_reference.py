"""Stage-by-stage reference of the fused edge block and its backward.

Plain torch in whatever dtype the inputs carry (the tests pass float64), one
function per stage of csrc/fused_edge.hip and csrc/fused_edge_bwd.hip, so a
test can feed each stage the kernel's own output of the stage before and
judge exactly one rounding step. ``edge_forward`` / ``edge_backward`` chain
the stages without any rounding; tests/test_edge_reference_cpu.py holds them
against ``ops.eager_edge_block`` and ``torch.autograd.grad``.

Chain (row i, col j of edge e; the radial norm is detached in the
normalisation, as in ``ops.eager_edge_block``):

  d = x_i - x_j      r2 = |d|^2      inv = 1/(sqrt(r2)+eps) or 1
  ein = [h_i | h_j | r2 | a_e]
  z1 = ein W1^T + b1     t1  = silu(z1)
  z2 = t1  W2^T + b2     msg = silu(z2)
  z3 = msg W3^T + b3     p   = silu(z3) . w3v
  trans = d inv p

  dp   = (dtrans_i . d) inv
  dz3  = dp w3v silu'(z3)              dw3v = sum_e dp silu(z3)
  dz2  = (dmsg_i + dz3 W3) silu'(z2)
  dz1  = (dz2 W2) silu'(z1)
  dein = dz1 W1 = [dh_i | dh_j | dr2 | .]
  dcd  = p dtrans_i inv + 2 d dr2
  gb   = column sums of dz1 | dz2 | dz3
"""

from __future__ import annotations

import torch


def silu(z):
    return z * torch.sigmoid(z)


def dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def geometry(coord, row, col, normalize, eps):
    """d [M,3], r2 [M], inv [M] (ones without ``normalize``)."""
    d = coord.index_select(0, row) - coord.index_select(0, col)
    r2 = (d * d).sum(1)
    inv = 1 / (r2.sqrt() + eps) if normalize else torch.ones_like(r2)
    return d, r2, inv


def edge_input(h, r2, eattr, row, col):
    return torch.cat([h.index_select(0, row), h.index_select(0, col),
                      r2.unsqueeze(1).to(h.dtype), eattr.to(h.dtype)], dim=1)


def preact(x, w, b):
    return x @ w.t() + b


def head(z3, w3v):
    return silu(z3) @ w3v


def translation(d, inv, p):
    return d * (inv * p).unsqueeze(1)


def head_cotangent(dtrans_e, d, inv):
    """dp [M] from the per-edge cotangent of trans."""
    return (dtrans_e * d).sum(1) * inv


def dz_head(dp, w3v, z3):
    return dp.unsqueeze(1) * w3v * dsilu(z3)


def dw3v(dp, z3):
    return (dp.unsqueeze(1) * silu(z3)).sum(0)


def dz_hidden(upstream, z):
    return upstream * dsilu(z)


def dcoord_diff(p, dtrans_e, inv, d, dr2):
    return (p * inv).unsqueeze(1) * dtrans_e + 2 * d * dr2.unsqueeze(1)


def edge_forward(h, coord, eattr, row, col, w1, b1, w2, b2, w3, b3, w3v,
                 normalize, eps):
    """Every forward stage, unrounded. Returns a dict."""
    d, r2, inv = geometry(coord, row, col, normalize, eps)
    ein = edge_input(h, r2, eattr, row, col)
    z1 = preact(ein, w1, b1)
    t1 = silu(z1)
    z2 = preact(t1, w2, b2)
    msg = silu(z2)
    z3 = preact(msg, w3, b3)
    p = head(z3, w3v)
    return dict(d=d, r2=r2, inv=inv, ein=ein, z1=z1, t1=t1, z2=z2, msg=msg,
                z3=z3, p=p, trans=translation(d, inv, p))


def edge_backward(fwd, row, col, dmsg_n, dtrans_n, w1, w2, w3, w3v,
                  num_nodes):
    """Every backward stage from ``edge_forward``'s dict and the per-NODE
    cotangents dmsg_n [N,H], dtrans_n [N,3] (edge e receives row i's).
    Returns a dict with the per-edge stages, the parameter gradients and
    the node gradients gh [N,H], gc [N,3]."""
    hdim = w1.size(0)
    dtrans_e = dtrans_n.index_select(0, row)
    dp = head_cotangent(dtrans_e, fwd["d"], fwd["inv"])
    dz3 = dz_head(dp, w3v, fwd["z3"])
    dz2 = dz_hidden(dmsg_n.index_select(0, row) + dz3 @ w3, fwd["z2"])
    dz1 = dz_hidden(dz2 @ w2, fwd["z1"])
    dein = dz1 @ w1
    dhr, dhc, dr2 = dein[:, :hdim], dein[:, hdim:2 * hdim], dein[:, 2 * hdim]
    dcd = dcoord_diff(fwd["p"], dtrans_e, fwd["inv"], fwd["d"], dr2)
    gh = torch.zeros(num_nodes, hdim, dtype=dein.dtype, device=dein.device)
    gh.index_add_(0, row, dhr).index_add_(0, col, dhc)
    gc = torch.zeros(num_nodes, 3, dtype=dcd.dtype, device=dcd.device)
    gc.index_add_(0, row, dcd).index_add_(0, col, -dcd)
    return dict(dp=dp, dz3=dz3, dz2=dz2, dz1=dz1, dein=dein, dhr=dhr,
                dhc=dhc, dr2=dr2, dcd=dcd,
                dw3v=dw3v(dp, fwd["z3"]),
                gb=torch.cat([dz1.sum(0), dz2.sum(0), dz3.sum(0)]),
                gw1=dz1.t() @ fwd["ein"], gw2=dz2.t() @ fwd["t1"],
                gw3=dz3.t() @ fwd["msg"], gh=gh, gc=gc)


def edge_backward_factored(fwd, h, eattr, row, col, dmsg_n, dtrans_n, w1, w2,
                           w3, w3v, num_nodes):
    """``edge_backward`` with dh and dW1 taken from per-NODE sums of dz1.

    z1 is linear in ein and ein = [h_i | h_j | r2 | a] gathers node rows, so
    with S_row[n] = sum of dz1 over the edges whose row is n and S_col
    likewise over col (both [N,H]):

      gh            = S_row W1[:, :H] + S_col W1[:, H:2H]
      gw1[:, :H]    = S_row^T h        gw1[:, H:2H] = S_col^T h
      gw1[:, 2H:]   = sum_e dz1_e (x) [r2_e, a_e]     (per edge, three columns)
      dr2_e         = dz1_e . W1[:, 2H]               (all of dein that dcd needs)

    No [M, 2H+3] dein or ein product is formed. Returns the dict of
    ``edge_backward`` without dein/dhr/dhc, plus s_row, s_col, gw1_tail."""
    hdim = w1.size(0)
    dtrans_e = dtrans_n.index_select(0, row)
    dp = head_cotangent(dtrans_e, fwd["d"], fwd["inv"])
    dz3 = dz_head(dp, w3v, fwd["z3"])
    dz2 = dz_hidden(dmsg_n.index_select(0, row) + dz3 @ w3, fwd["z2"])
    dz1 = dz_hidden(dz2 @ w2, fwd["z1"])
    s_row = torch.zeros(num_nodes, hdim, dtype=dz1.dtype, device=dz1.device)
    s_row.index_add_(0, row, dz1)
    s_col = torch.zeros_like(s_row).index_add_(0, col, dz1)
    gh = s_row @ w1[:, :hdim] + s_col @ w1[:, hdim:2 * hdim]
    tail_in = torch.cat([fwd["r2"].unsqueeze(1).to(dz1.dtype),
                         eattr.to(dz1.dtype)], dim=1)
    gw1_tail = dz1.t() @ tail_in
    gw1 = torch.cat([s_row.t() @ h, s_col.t() @ h, gw1_tail], dim=1)
    dr2 = dz1 @ w1[:, 2 * hdim]
    dcd = dcoord_diff(fwd["p"], dtrans_e, fwd["inv"], fwd["d"], dr2)
    gc = torch.zeros(num_nodes, 3, dtype=dcd.dtype, device=dcd.device)
    gc.index_add_(0, row, dcd).index_add_(0, col, -dcd)
    return dict(dp=dp, dz3=dz3, dz2=dz2, dz1=dz1, dr2=dr2, dcd=dcd,
                s_row=s_row, s_col=s_col, gw1_tail=gw1_tail,
                dw3v=dw3v(dp, fwd["z3"]),
                gb=torch.cat([dz1.sum(0), dz2.sum(0), dz3.sum(0)]),
                gw1=gw1, gw2=dz2.t() @ fwd["t1"],
                gw3=dz3.t() @ fwd["msg"], gh=gh, gc=gc)


def edge_block_mean(h, coord, eattr, row, col, w1, b1, w2, b2, w3, b3, w3v,
                    normalize, eps):
    """(agg_msg [N,H], agg_trans [N,3]): per-node means over the row
    segments, with plain index_add_ and a degree clamped to 1; differentiable
    by autograd (the norm in the normalisation is detached)."""
    n = coord.size(0)
    d = coord.index_select(0, row) - coord.index_select(0, col)
    r2 = (d * d).sum(1)
    if normalize:
        d = d / (r2.sqrt().detach() + eps).unsqueeze(1)
    ein = edge_input(h, r2, eattr, row, col)
    msg = silu(preact(silu(preact(ein, w1, b1)), w2, b2))
    trans = d * head(preact(msg, w3, b3), w3v).unsqueeze(1)
    deg = torch.bincount(row, minlength=n).clamp(min=1).to(msg.dtype)
    agg_msg = torch.zeros(n, msg.size(1), dtype=msg.dtype, device=msg.device)
    agg_msg = agg_msg.index_add(0, row, msg) / deg.unsqueeze(1)
    agg_trans = torch.zeros(n, 3, dtype=msg.dtype, device=msg.device)
    agg_trans = agg_trans.index_add(0, row, trans) / deg.unsqueeze(1)
    return agg_msg, agg_trans
