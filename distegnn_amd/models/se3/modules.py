"""SE(3)-equivariant layers (TFN / SE(3)-Transformer), DGL-free.

Re-owned from reference se3_dynamics/equivariant_attention/modules.py:
GConvSE3 (:82-189), RadialFunc (:192-227), PairwiseConv (:230-266),
G1x1SE3 (:269-299), GNormSE3 (:302-367), BN (:370-382), GConvSE3Partial
(:385-467), GMABSE3 (:471-553, with edge_softmax re-expressed as a
segmented max/exp/sum), GSE3Res (:556+), GSum/GCat and the pooling heads.
Message passing runs on plain edge lists (EdgeGraph) with our aggregation
helpers instead of DGL's update_all/apply_edges.
"""

from __future__ import annotations

from typing import Dict

import numpy as np
import torch
from torch import nn

from ...ops import reference as ref_ops
from .fibers import Fiber, fiber2head


def _segment_mean(data, index, n):
    shape = data.shape
    flat = data.reshape(shape[0], -1)
    out = ref_ops.segment_mean(flat, index, n)
    return out.reshape(n, *shape[1:])


def _segment_sum(data, index, n):
    shape = data.shape
    flat = data.reshape(shape[0], -1)
    out = ref_ops.segment_sum(flat, index, n)
    return out.reshape(n, *shape[1:])


class _EdgeSoftmaxFn(torch.autograd.Function):
    """Fused CSR edge softmax (csrc/segment_reduce.hip edge_softmax_csr):
    one wave per destination segment, max/sum-exp/write passes in
    registers. Backward uses the standard softmax identity with a CSR
    segment sum."""

    @staticmethod
    def forward(ctx, scores, dst, dstptr, perm, num_nodes):
        from ... import ops as _ops

        attn = _ops.hip_ext().edge_softmax_fwd(
            scores.float().contiguous(), dstptr, perm)
        ctx.save_for_backward(attn, dst)
        ctx.n = num_nodes
        return attn.to(scores.dtype)

    @staticmethod
    def backward(ctx, g):
        attn, dst = ctx.saved_tensors
        ag = attn * g.float()
        s = _segment_sum(ag, dst, ctx.n)
        dscores = ag - attn * s.index_select(0, dst)
        return dscores.to(g.dtype), None, None, None, None


def edge_softmax(scores: torch.Tensor, dst: torch.Tensor,
                 num_nodes: int, csr=None) -> torch.Tensor:
    """Softmax over each node's incoming edges (DGL edge_softmax).

    With ``csr=(dstptr, perm)`` on GPU (power-of-two head count), the
    fused CSR kernel runs; otherwise the scatter/exp/segment composition.
    """
    from ... import ops as _ops

    h = scores.shape[-1]
    if (csr is not None and scores.is_cuda and scores.dim() == 2
            and 1 <= h <= 64 and (h & (h - 1)) == 0
            and _ops.hip_ext() is not None):
        return _EdgeSoftmaxFn.apply(scores, dst, csr[0], csr[1], num_nodes)
    # segment max for stability
    mx = torch.full((num_nodes,) + scores.shape[1:], -torch.inf,
                    dtype=scores.dtype, device=scores.device)
    idx = dst.view(-1, *([1] * (scores.dim() - 1))).expand_as(scores)
    mx = mx.scatter_reduce(0, idx, scores, reduce="amax",
                           include_self=True)
    ex = torch.exp(scores - mx.index_select(0, dst))
    den = _segment_sum(ex, dst, num_nodes).clamp(min=1e-20)
    return ex / den.index_select(0, dst)


class BN(nn.Module):
    """SE(3)-equivariant normalization (LayerNorm on norms)."""

    def __init__(self, m):
        super().__init__()
        self.bn = nn.LayerNorm(m)

    def forward(self, x):
        return self.bn(x)


class RadialFunc(nn.Module):
    """NN-parameterized radial profile (reference :192-227)."""

    def __init__(self, num_freq, in_dim, out_dim, edge_dim: int = 0,
                 act_fn=None):
        super().__init__()
        act_fn = act_fn if act_fn is not None else nn.ReLU()
        self.num_freq = num_freq
        self.in_dim = in_dim
        self.mid_dim = 32
        self.out_dim = out_dim
        self.edge_dim = edge_dim
        self.net = nn.Sequential(
            nn.Linear(edge_dim + 1, self.mid_dim), BN(self.mid_dim), act_fn,
            nn.Linear(self.mid_dim, self.mid_dim), BN(self.mid_dim), act_fn,
            nn.Linear(self.mid_dim, num_freq * in_dim * out_dim))
        nn.init.kaiming_uniform_(self.net[0].weight)
        nn.init.kaiming_uniform_(self.net[3].weight)
        nn.init.kaiming_uniform_(self.net[6].weight)

    def forward(self, x):
        return self.net(x).view(-1, self.out_dim, 1, self.in_dim, 1,
                                self.num_freq)


class PairwiseConv(nn.Module):
    """Kernel between one input and one output degree (reference :230-266)."""

    def __init__(self, degree_in, nc_in, degree_out, nc_out, edge_dim=0,
                 act_fn=None):
        super().__init__()
        self.degree_in = degree_in
        self.degree_out = degree_out
        self.nc_in = nc_in
        self.nc_out = nc_out
        self.num_freq = 2 * min(degree_in, degree_out) + 1
        self.d_out = 2 * degree_out + 1
        self.edge_dim = edge_dim
        self.rp = RadialFunc(self.num_freq, nc_in, nc_out, edge_dim,
                             act_fn=act_fn)

    def forward(self, feat, basis):
        r = self.rp(feat)
        kernel = torch.sum(
            r * basis[f"{self.degree_in},{self.degree_out}"], -1)
        return kernel.view(kernel.shape[0], self.d_out * self.nc_out, -1)


class _ConvSE3Base(nn.Module):
    """Shared kernel plumbing for GConvSE3 / GConvSE3Partial."""

    def __init__(self, f_in: Fiber, f_out: Fiber, self_interaction=False,
                 edge_dim=0, act_fn=None):
        super().__init__()
        self.f_in = f_in
        self.f_out = f_out
        self.edge_dim = edge_dim
        self.self_interaction = self_interaction
        self.kernel_unary = nn.ModuleDict()
        for (mi, di) in f_in.structure:
            for (mo, do) in f_out.structure:
                self.kernel_unary[f"({di},{do})"] = PairwiseConv(
                    di, mi, do, mo, edge_dim=edge_dim, act_fn=act_fn)
        self.kernel_self = nn.ParameterDict()
        if self_interaction:
            for m_in, d_in in f_in.structure:
                if d_in in f_out.degrees:
                    m_out = f_out.structure_dict[d_in]
                    self.kernel_self[f"{d_in}"] = nn.Parameter(
                        torch.randn(1, m_out, m_in) / np.sqrt(m_in))

    def _edge_feat(self, G, r):
        if "w" in G.edata:
            return torch.cat([G.edata["w"], r], -1)
        return r

    def _edge_messages(self, h, G, r, basis, d_out):
        """Per-edge messages for one output degree: [M, mo, 2*d_out+1]."""
        src = G.src
        msg = 0
        for m_in, d_in in self.f_in.structure:
            kernel = self._kernels[f"({d_in},{d_out})"]
            src_feat = h[f"{d_in}"].index_select(0, src).reshape(
                -1, m_in * (2 * d_in + 1), 1)
            msg = msg + torch.matmul(kernel, src_feat)
        msg = msg.view(msg.shape[0], -1, 2 * d_out + 1)
        if self.self_interaction and f"{d_out}" in self.kernel_self.keys():
            dst_feat = h[f"{d_out}"].index_select(0, G.dst)
            msg = msg + torch.matmul(self.kernel_self[f"{d_out}"], dst_feat)
        return msg

    def _compute_kernels(self, G, r, basis):
        feat = self._edge_feat(G, r)
        self._kernels = {}
        for (mi, di) in self.f_in.structure:
            for (mo, do) in self.f_out.structure:
                etype = f"({di},{do})"
                self._kernels[etype] = self.kernel_unary[etype](feat, basis)


class GConvSE3(_ConvSE3Base):
    """TFN graph convolution: per-edge kernels + MEAN aggregation at dst
    (reference :82-189)."""

    def forward(self, h, G=None, r=None, basis=None, **kwargs):
        self._compute_kernels(G, r, basis)
        out = {}
        for d in self.f_out.degrees:
            msg = self._edge_messages(h, G, r, basis, d)
            out[f"{d}"] = _segment_mean(msg, G.dst, G.num_nodes)
        self._kernels = None
        return out


class GConvSE3Partial(_ConvSE3Base):
    """Per-EDGE convolution (no aggregation) — reference :385-467."""

    def forward(self, h, G=None, r=None, basis=None, **kwargs):
        self._compute_kernels(G, r, basis)
        out = {}
        for d in self.f_out.degrees:
            out[f"{d}"] = self._edge_messages(h, G, r, basis, d)
        self._kernels = None
        return out


class G1x1SE3(nn.Module):
    """Per-degree linear map (self-interaction) — reference :269-299."""

    def __init__(self, f_in: Fiber, f_out: Fiber, learnable=True):
        super().__init__()
        self.f_in = f_in
        self.f_out = f_out
        self.transform = nn.ParameterDict()
        for m_out, d_out in f_out.structure:
            m_in = f_in.structure_dict[d_out]
            self.transform[str(d_out)] = nn.Parameter(
                torch.randn(m_out, m_in) / np.sqrt(m_in),
                requires_grad=learnable)

    def forward(self, features, **kwargs):
        out = {}
        for k, v in features.items():
            if str(k) in self.transform.keys():
                out[k] = torch.matmul(self.transform[str(k)], v)
        return out


class GNormSE3(nn.Module):
    """Norm-gated nonlinearity (reference :302-367)."""

    def __init__(self, fiber: Fiber, act_fn=None, num_layers: int = 0):
        super().__init__()
        act_fn = act_fn if act_fn is not None else nn.ReLU(inplace=True)
        self.fiber = fiber
        self.act_fn = act_fn
        self.num_layers = num_layers
        self.eps = 1e-12
        self.transform = nn.ModuleDict()
        for m, d in fiber.structure:
            self.transform[str(d)] = self._build_net(int(m))

    def _build_net(self, m):
        net = []
        for i in range(self.num_layers):
            net.append(BN(m))
            net.append(self.act_fn)
            net.append(nn.Linear(m, m, bias=(i == self.num_layers - 1)))
            nn.init.kaiming_uniform_(net[-1].weight)
        if self.num_layers == 0:
            net.append(BN(m))
            net.append(self.act_fn)
        return nn.Sequential(*net)

    def forward(self, features, **kwargs):
        out = {}
        for k, v in features.items():
            norm = v.norm(2, -1, keepdim=True).clamp_min(self.eps) \
                .expand_as(v)
            phase = v / norm
            transformed = self.transform[str(k)](norm[..., 0]).unsqueeze(-1)
            out[k] = (transformed * phase).view(*v.shape)
        return out


class GMABSE3(nn.Module):
    """Multi-headed SE(3) attention block (reference :471-553)."""

    def __init__(self, f_value: Fiber, f_key: Fiber, n_heads: int):
        super().__init__()
        self.f_value = f_value
        self.f_key = f_key
        self.n_heads = n_heads

    def forward(self, v: Dict, k: Dict = None, q: Dict = None, G=None,
                **kwargs):
        h = self.n_heads
        values = {}
        for m, d in self.f_value.structure:
            values[d] = v[f"{d}"].view(-1, h, m // h, 2 * d + 1)
        keys = fiber2head(k, h, self.f_key, squeeze=True)       # [M, h, f]
        queries = fiber2head(q, h, self.f_key, squeeze=True)    # [N, h, f]
        scores = (keys * queries.index_select(0, G.dst)).sum(-1)  # [M, h]
        scores = scores / np.sqrt(self.f_key.n_features)
        attn = edge_softmax(scores, G.dst, G.num_nodes,
                            csr=G.dst_csr() if scores.is_cuda else None)
        out = {}
        for m, d in self.f_value.structure:
            weighted = attn.unsqueeze(-1).unsqueeze(-1) * values[d]
            agg = _segment_sum(weighted, G.dst, G.num_nodes)
            out[f"{d}"] = agg.reshape(-1, m, 2 * d + 1)
        return out


class GSE3Res(nn.Module):
    """Attention block: value/key edge-convs + query projection + GMAB
    (reference :556+; the residual projection is commented out there too)."""

    def __init__(self, f_in: Fiber, f_out: Fiber, edge_dim: int = 0,
                 div: float = 4, n_heads: int = 1, act_fn=None,
                 learnable_skip=True):
        super().__init__()
        act_fn = act_fn if act_fn is not None else nn.ReLU()
        self.f_in = f_in
        self.f_out = f_out
        f_mid_out = {k: int(v // div) for k, v in f_out.structure_dict.items()}
        self.f_mid_out = Fiber(dictionary=f_mid_out)
        f_mid_in = {d: m for d, m in f_mid_out.items() if d in f_in.degrees}
        self.f_mid_in = Fiber(dictionary=f_mid_in)
        self.GMAB = nn.ModuleDict()
        self.GMAB["v"] = GConvSE3Partial(f_in, self.f_mid_out,
                                         edge_dim=edge_dim, act_fn=act_fn)
        self.GMAB["k"] = GConvSE3Partial(f_in, self.f_mid_in,
                                         edge_dim=edge_dim, act_fn=act_fn)
        self.GMAB["q"] = G1x1SE3(f_in, self.f_mid_in)
        self.GMAB["attn"] = GMABSE3(self.f_mid_out, self.f_mid_in,
                                    n_heads=n_heads)

    def forward(self, features, G, **kwargs):
        v = self.GMAB["v"](features, G=G, **kwargs)
        k = self.GMAB["k"](features, G=G, **kwargs)
        q = self.GMAB["q"](features, G=G)
        return self.GMAB["attn"](v, k=k, q=q, G=G)


class GSum(nn.Module):
    """Degree-wise sum with zero-padding on channel mismatch."""

    def __init__(self, f_x: Fiber, f_y: Fiber):
        super().__init__()
        self.f_x = f_x
        self.f_y = f_y
        self.f_out = Fiber.combine_max(f_x, f_y)

    def forward(self, x, y):
        out = {}
        for k in self.f_out.degrees:
            k = str(k)
            if k in x and k in y:
                if x[k].shape[1] > y[k].shape[1]:
                    diff = x[k].shape[1] - y[k].shape[1]
                    zeros = y[k].new_zeros(y[k].shape[0], diff,
                                           y[k].shape[2])
                    y[k] = torch.cat([y[k], zeros], 1)
                elif x[k].shape[1] < y[k].shape[1]:
                    diff = y[k].shape[1] - x[k].shape[1]
                    zeros = x[k].new_zeros(x[k].shape[0], diff,
                                           x[k].shape[2])
                    x[k] = torch.cat([x[k], zeros], 1)
                out[k] = x[k] + y[k]
            elif k in x:
                out[k] = x[k]
            else:
                out[k] = y[k]
        return out


class GCat(nn.Module):
    """Degree-wise concat for degrees present in f_x."""

    def __init__(self, f_x: Fiber, f_y: Fiber):
        super().__init__()
        self.f_x = f_x
        self.f_y = f_y
        f_out = {}
        for k in f_x.degrees:
            f_out[k] = f_x.dict[k]
            if k in f_y.degrees:
                f_out[k] += f_y.dict[k]
        self.f_out = Fiber(dictionary=f_out)

    def forward(self, x, y):
        out = {}
        for k in self.f_out.degrees:
            k = str(k)
            if k in y:
                out[k] = torch.cat([x[k], y[k]], 1)
            else:
                out[k] = x[k]
        return out


class GAvgPooling(nn.Module):
    """Graph average pooling of degree-0 (or -1) features."""

    def __init__(self, type="0"):
        super().__init__()
        self.pool_type = type

    def forward(self, G, features, batch=None, **kwargs):
        f = features
        if batch is None:
            return f.mean(0, keepdim=True)
        b = int(batch.max()) + 1
        return ref_ops.graph_mean_pool(f, batch, b)


class GMaxPooling(nn.Module):
    """Graph max pooling of pre-pooled scalar features."""

    def forward(self, G, features, batch=None, **kwargs):
        if batch is None:
            return features.max(0, keepdim=True).values
        b = int(batch.max()) + 1
        out = features.new_full((b,) + features.shape[1:], -torch.inf)
        idx = batch.view(-1, *([1] * (features.dim() - 1))).expand_as(features)
        return out.scatter_reduce(0, idx, features, reduce="amax",
                                  include_self=True)
