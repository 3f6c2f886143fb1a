"""FastEGNN / DistEGNN — E(3)-equivariant GNN with multi-channel virtual
nodes, rebuilt MI355X-first.

Semantics parity with reference models/FastEGNN.py (E_GCL_vel :46-276,
FastEGNN :279-307): identical parameterization (module names and weight
shapes match, so checkpoints are format-compatible), identical math per
layer:

  edge msg      m_ij   = phi_e([h_i, h_j, |x_i-x_j|^2, a_ij])
  virtual msg   m_ic   = phi_ev([h_i, Z_c, |X_c - x_i|, gram(X)_c])
  coord update  x_i   += mean_j((x_i-x_j) phi_x(m_ij))
                       + mean_c(-(X_c-x_i) phi_xv(m_ic)) + phi_v(h_i) v_i
  virtual coord X_c   += pool_mean_i((X_c-x_i) phi_X(m_ic))   [+ all-reduce]
  node feat     h_i   += phi_h([h_i, mean_j m_ij, mean_c m_ic, u_i])
  virtual feat  Z_c   += phi_hv([Z_c, pool_mean_i m_ic])      [+ all-reduce]

MI355X-first redesign (what is intentionally different from the reference):

* **[B, C, H] virtual layout** — the reference stores virtual state as
  [B, H, C] and permutes around every virtual MLP (FastEGNN.py:158,192,230);
  we keep channels-major [B, C, H] natively so every Linear is a contiguous
  GEMM and no permute kernels run in the hot loop. The learnable parameter
  keeps the reference's [1, H, C] shape for checkpoint compatibility and is
  transposed once per forward.
* **No host syncs** — batch size comes from loc_mean.shape[0]; per-graph
  node counts are a device-side bincount (Batch.counts), replacing the
  reference's per-graph ``.item()`` loops (FastEGNN.py:196,226,260 — 12
  host syncs per forward).
* **Fused collectives** — the three weighted-average all-reduce sites per
  layer (FastEGNN.py:195-197,225-227,259-261 = 6 RCCL calls/layer) become
  2: coord_mean, then ONE fused flat-buffer reduce carrying both virtual
  aggregates. Weights (node counts) are step-constants reduced once per
  step, not per site. See parallel/comm.py.
* **CSR segment reductions** — edge aggregations use the row-sorted edge
  list + rowptr (deterministic HIP kernel), not scatter_add atomics.
* Aggregation and coordinate math stay fp32; MLP GEMMs may run bf16 under
  autocast (equivariance holds to bf16 tolerance; fp32 path is exact).
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops
from ..ops.linear import SplitKLinear
from ..parallel import comm

# nn.Linear drop-in with split-K weight gradients for the [N]/[N*C]-row
# activations (state-dict compatible; see ops/linear.py)
Linear = SplitKLinear


class EGCLVel(nn.Module):
    """One FastEGNN layer (reference E_GCL_vel, models/FastEGNN.py:46-276)."""

    def __init__(self, node_feat_nf, node_feat_out_nf, node_attr_nf,
                 edge_attr_nf, hidden_nf, virtual_channels, world_size,
                 act_fn=None, residual=True, attention=False, normalize=False,
                 coords_agg="mean", tanh=False, gravity=None,
                 skip_feature_update=False):
        super().__init__()
        act_fn = act_fn if act_fn is not None else nn.SiLU()
        # the layer's h / virtual_feat outputs are discarded by the caller
        # (FastEGNN's last layer): forward skips agg_v, agg_vf and both
        # node MLPs and returns the incoming features. Modules and state
        # dict are the same either way.
        self.skip_feature_update = skip_feature_update
        self.residual = residual
        self.attention = attention
        self.normalize = normalize
        self.coords_agg = coords_agg
        self.hidden_nf = hidden_nf
        self.tanh = tanh
        self.world_size = world_size
        self.virtual_channels = virtual_channels
        self.epsilon = 1e-8
        edge_coords_nf = 1

        self.edge_mlp = nn.Sequential(  # phi_e
            Linear(2 * node_feat_nf + edge_coords_nf + edge_attr_nf, hidden_nf),
            act_fn,
            Linear(hidden_nf, hidden_nf),
            act_fn,
        )
        self.edge_mlp_virtual = nn.Sequential(  # phi_ev (no edge feat)
            Linear(2 * node_feat_nf + edge_coords_nf + virtual_channels, hidden_nf),
            act_fn,
            Linear(hidden_nf, hidden_nf),
            act_fn,
        )
        if attention:
            self.att_mlp = nn.Sequential(Linear(hidden_nf, 1), nn.Sigmoid())
            self.att_mlp_virtual = nn.Sequential(Linear(hidden_nf, 1), nn.Sigmoid())

        def coord_head():
            last = Linear(hidden_nf, 1, bias=False)
            nn.init.xavier_uniform_(last.weight, gain=0.001)
            mods = [Linear(hidden_nf, hidden_nf), act_fn, last]
            if tanh:
                mods.append(nn.Tanh())
            return nn.Sequential(*mods)

        self.coord_mlp_r = coord_head()            # phi_x
        self.coord_mlp_r_virtual = coord_head()    # phi_xv
        self.coord_mlp_v_virtual = coord_head()    # phi_X
        self.coord_mlp_vel = nn.Sequential(        # phi_v
            Linear(node_feat_nf, hidden_nf), act_fn, Linear(hidden_nf, 1)
        )
        self.gravity = gravity
        if gravity is not None:
            self.gravity_mlp = nn.Sequential(
                Linear(node_feat_nf, hidden_nf), act_fn, Linear(hidden_nf, 1)
            )
        self.node_mlp = nn.Sequential(  # phi_h
            Linear(3 * hidden_nf + node_attr_nf, hidden_nf),
            act_fn,
            Linear(hidden_nf, node_feat_out_nf),
        )
        self.node_mlp_virtual = nn.Sequential(  # phi_hv
            Linear(2 * hidden_nf, hidden_nf),
            act_fn,
            Linear(hidden_nf, node_feat_out_nf),
        )

    # --- geometry -------------------------------------------------------
    def coord2radial(self, edge_index, coord, rowptr=None, colptr=None,
                     col_perm=None):
        row, col = edge_index[0], edge_index[1]
        coord_diff = (ops.gather_rows(coord, row, rowptr)
                      - ops.gather_rows(coord, col, colptr, col_perm))
        radial = coord_diff.pow(2).sum(dim=1, keepdim=True)
        if self.normalize:
            norm = radial.sqrt().detach() + self.epsilon
            coord_diff = coord_diff / norm
        return radial, coord_diff

    # --- forward --------------------------------------------------------
    def forward(self, h, edge_index, coord, vel, virtual_coord, virtual_feat,
                batch, edge_attr=None, node_attr=None, *,
                rowptr=None, ptr=None, counts=None, counts_global=None,
                num_graphs=None, pool_chunks=None, colptr=None,
                col_perm=None):
        """virtual_coord: [B, C, 3]; virtual_feat: [B, C, H] (channels-major).

        rowptr/ptr/counts/counts_global come from the Batch (device-side);
        num_graphs is a host int (loader-known, no sync)."""
        n = coord.size(0)
        b = num_graphs if num_graphs is not None else virtual_coord.size(0)
        c = self.virtual_channels
        row = edge_index[0]
        dist_active = self.world_size > 1 and comm.is_distributed()

        # --- edge block (real-real): phi_e messages + phi_x translations -
        # Fusable form (the standard FastEGNN configuration): one MFMA HIP
        # kernel computes gather + phi_e MLP + phi_x head + d_ij * phi_x and
        # returns the per-node segment MEANS directly (ops.fused_edge_block;
        # csrc/fused_edge.hip). Non-standard variants (attention, tanh,
        # sum aggregation, no edge_attr) take the composed eager path.
        fuse = (not self.attention and not self.tanh
                and self.coords_agg == "mean" and edge_attr is not None)
        if fuse:
            agg_e, agg = ops.fused_edge_block(
                h, coord, edge_attr, row, edge_index[1], rowptr, colptr,
                col_perm,
                self.edge_mlp[0].weight, self.edge_mlp[0].bias,
                self.edge_mlp[2].weight, self.edge_mlp[2].bias,
                self.coord_mlp_r[0].weight, self.coord_mlp_r[0].bias,
                self.coord_mlp_r[2].weight.reshape(-1),
                self.normalize, self.epsilon)
        else:
            radial, coord_diff = self.coord2radial(
                edge_index, coord, rowptr=rowptr, colptr=colptr,
                col_perm=col_perm)
            h_row = ops.gather_rows(h, row, rowptr)
            h_col = ops.gather_rows(h, edge_index[1], colptr, col_perm)
            edge_in = torch.cat(
                [h_row, h_col, radial, edge_attr] if edge_attr is not None
                else [h_row, h_col, radial], dim=1)
            edge_feat = self.edge_mlp(edge_in)
            if self.attention:
                edge_feat = edge_feat * self.att_mlp(edge_feat)

        # --- global coord mean (site A collective) ----------------------
        coord_mean = ops.graph_mean_pool(coord, batch, b, ptr=ptr, counts=counts,
                                         chunks=pool_chunks)
        if dist_active:
            coord_mean = comm.fused_weighted_average_reduce(
                [coord_mean], counts, counts_global)

        # gram(X): [B, C, C] O(3)-invariant channel mixing
        m_x = virtual_coord - coord_mean.unsqueeze(1)
        gram = torch.matmul(m_x, m_x.transpose(1, 2))

        # --- virtual edge block, phi_ev + phi_xv/phi_X heads ------------
        # Fusable form: one MFMA kernel over (node, channel) rows builds
        # the inputs (vdiff / vradial / concat) in LDS and returns per-row
        # messages + head translations (ops.fused_virtual_block;
        # csrc/fused_virtual.hip). attention/tanh variants compose eagerly.
        vfuse = not self.attention and not self.tanh
        if vfuse:
            v_msg, tv, trans_x = ops.fused_virtual_block(
                h, coord, virtual_coord, virtual_feat, gram, batch, ptr,
                pool_chunks,
                self.edge_mlp_virtual[0].weight,
                self.edge_mlp_virtual[0].bias,
                self.edge_mlp_virtual[2].weight,
                self.edge_mlp_virtual[2].bias,
                self.coord_mlp_r_virtual[0].weight,
                self.coord_mlp_r_virtual[0].bias,
                self.coord_mlp_r_virtual[2].weight.reshape(-1),
                self.coord_mlp_v_virtual[0].weight,
                self.coord_mlp_v_virtual[0].bias,
                self.coord_mlp_v_virtual[2].weight.reshape(-1))
            # channel means + graph-mean pools of the block's outputs in
            # one op (ops.virtual_aggregate)
            if self.skip_feature_update:
                trans_v = ops.mid_mean(tv)
            else:
                agg_v, trans_v, agg_vf, agg_vc = ops.virtual_aggregate(
                    v_msg, tv, trans_x, batch, ptr, counts, pool_chunks,
                    num_graphs=b)
        else:
            vdiff = (ops.gather_rows(virtual_coord, batch, ptr,
                                     chunks=pool_chunks)
                     - coord.unsqueeze(1))
            vradial = vdiff.norm(p=2, dim=-1, keepdim=True)
            v_in = torch.cat([
                h.unsqueeze(1).expand(n, c, h.size(1)),
                ops.gather_rows(virtual_feat, batch, ptr,
                                chunks=pool_chunks),
                vradial,
                ops.gather_rows(gram, batch, ptr, chunks=pool_chunks),
            ], dim=-1)
            v_msg = self.edge_mlp_virtual(v_in)
            if self.attention:
                v_msg = v_msg * self.att_mlp_virtual(v_msg)
            trans_v = (-vdiff * self.coord_mlp_r_virtual(v_msg)).mean(dim=1)
            trans_x = vdiff * self.coord_mlp_v_virtual(v_msg)  # [N, C, 3]

        # --- coord model (real), phi_x / phi_xv / phi_v ------------------
        if not fuse:
            trans = coord_diff * self.coord_mlp_r(edge_feat)
            if self.coords_agg == "mean":
                agg = ops.segment_mean(trans, row, n, rowptr=rowptr)
            elif self.coords_agg == "sum":
                agg = ops.segment_sum(trans, row, n, rowptr=rowptr)
            else:
                raise ValueError(f"coords_agg {self.coords_agg}")
        # --- node block, phi_h + phi_v ----------------------------------
        # One kernel pair for both per-node MLPs (ops.fused_node_block;
        # csrc/fused_node.hip): h, agg_e, agg_v and node_attr all exist
        # here. A layer whose feature update is skipped needs phi_v only.
        skip = self.skip_feature_update
        if skip:
            h_out, phiv = ops.fused_node_block(
                h, None, None, None, self.node_mlp, self.coord_mlp_vel,
                self.residual, vel_only=True)
        else:
            if not fuse:
                agg_e = ops.segment_mean(edge_feat, row, n, rowptr=rowptr)
            if not vfuse:
                agg_v = ops.mid_mean(v_msg)
            h_out, phiv = ops.fused_node_block(
                h, agg_e, agg_v, node_attr, self.node_mlp,
                self.coord_mlp_vel, self.residual)
        # fused tail: coord + agg + trans_v + phi_v(h) * vel in one
        # kernel pair (ops.coord_update; eager composition off-GPU)
        coord = ops.coord_update(coord, agg, trans_v, phiv, vel)
        if self.gravity is not None:
            coord = coord + self.gravity_mlp(h) * self.gravity.to(h.device)

        # --- virtual aggregates (fused site B+C collective) -------------
        if not vfuse or skip:
            agg_vc = ops.graph_mean_pool(
                trans_x.reshape(n, -1), batch, b, ptr=ptr, counts=counts,
                chunks=pool_chunks
            ).reshape(b, c, 3)
        if not vfuse and not skip:
            agg_vf = ops.graph_mean_pool(
                v_msg.reshape(n, -1), batch, b, ptr=ptr, counts=counts,
                chunks=pool_chunks
            ).reshape(b, c, self.hidden_nf)
        if dist_active and skip:
            agg_vc = comm.fused_weighted_average_reduce(
                [agg_vc], counts, counts_global)
        elif dist_active:
            agg_vc, agg_vf = comm.fused_weighted_average_reduce(
                [agg_vc, agg_vf], counts, counts_global)
        virtual_coord = virtual_coord + agg_vc
        if skip:
            return h, coord, virtual_feat, virtual_coord

        # --- virtual node model, phi_hv ---------------------------------
        vf_out = self.node_mlp_virtual(torch.cat([virtual_feat, agg_vf], dim=-1))
        if self.residual:
            vf_out = virtual_feat + vf_out

        return h_out, coord, vf_out, virtual_coord


class FastEGNN(nn.Module):
    """Stack of EGCLVel layers (reference FastEGNN, models/FastEGNN.py:279-307)."""

    def __init__(self, node_feat_nf, node_attr_nf, edge_attr_nf, hidden_nf,
                 virtual_channels, world_size, act_fn=None, n_layers=4,
                 residual=True, attention=False, normalize=False, tanh=False,
                 gravity=None, skip_dead_update=True):
        super().__init__()
        assert virtual_channels > 0, (
            f"Channels of virtual node must be greater than 0 "
            f"(got {virtual_channels})")
        act_fn = act_fn if act_fn is not None else nn.SiLU()
        self.hidden_nf = hidden_nf
        self.n_layers = n_layers
        self.node_attr_nf = node_attr_nf
        self.virtual_channels = virtual_channels
        # [1, H, C]: reference-compatible parameter shape (FastEGNN.py:288)
        self.virtual_node_feat = nn.Parameter(
            torch.randn(1, hidden_nf, virtual_channels))
        self.embedding_in = Linear(node_feat_nf, hidden_nf)
        if gravity is not None:
            gravity = torch.tensor(gravity)
        for i in range(n_layers):
            self.add_module(
                f"gcl_{i}",
                EGCLVel(hidden_nf, hidden_nf, node_attr_nf, edge_attr_nf,
                        hidden_nf, virtual_channels=virtual_channels,
                        world_size=world_size, act_fn=act_fn,
                        residual=residual, attention=attention,
                        normalize=normalize, tanh=tanh, gravity=gravity,
                        # forward() discards the last layer's h and
                        # virtual_feat
                        skip_feature_update=(skip_dead_update
                                             and i == n_layers - 1)))

    def forward(self, node_feat, node_loc, node_vel, loc_mean, edge_index,
                data_batch, edge_attr=None, node_attr=None, *,
                rowptr=None, ptr=None, counts=None, counts_global=None,
                pool_chunks=None, colptr=None, col_perm=None):
        """Returns (loc_pred [N, 3], virtual_node_loc [B, 3, C]).

        API parity with the reference forward (FastEGNN.py:296-307); the
        keyword-only CSR/count args are the MI355X fast path (supplied by
        the trainer from Batch; recomputed device-side if absent).
        """
        b = loc_mean.size(0)  # host-known batch size: no .item() sync
        n = node_loc.size(0)
        if counts is None:
            counts = torch.bincount(data_batch, minlength=b).to(node_loc.dtype)
        if counts_global is None:
            counts_global = comm.global_counts(counts)

        virtual_feat = self.virtual_node_feat.transpose(1, 2).expand(
            b, self.virtual_channels, self.hidden_nf).contiguous()  # [B,C,H]
        virtual_loc = loc_mean.unsqueeze(1).expand(
            b, self.virtual_channels, 3).contiguous()               # [B,C,3]

        h = self.embedding_in(node_feat)
        loc = node_loc
        for i in range(self.n_layers):
            h, loc, virtual_feat, virtual_loc = self._modules[f"gcl_{i}"](
                h, edge_index, loc, node_vel, virtual_loc, virtual_feat,
                data_batch, edge_attr=edge_attr, node_attr=node_attr,
                rowptr=rowptr, ptr=ptr, counts=counts,
                counts_global=counts_global, num_graphs=b,
                pool_chunks=pool_chunks, colptr=colptr, col_perm=col_perm)
        return loc, virtual_loc.transpose(1, 2)  # [B, 3, C] API parity
