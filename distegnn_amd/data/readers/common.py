"""Sample assembly shared by the single-device (cutoff) pipelines."""

from __future__ import annotations

import numpy as np
import torch

from ...ops import reference as ref_ops
from ...utils.rotate import random_rotate
from ..graph import Data


def _cutoff_edge(edge_index: torch.Tensor, pos: torch.Tensor,
                 cutoff_rate: float) -> torch.Tensor:
    # same rule as preprocess.cutoff_edge (kept local: preprocess imports us)
    if cutoff_rate <= 0:
        return edge_index
    d = (pos[edge_index[0]] - pos[edge_index[1]]).norm(p=2, dim=1)
    keep = torch.sort(d).indices[: int(edge_index.size(1) * (1 - cutoff_rate))]
    return edge_index[:, keep]


def build_cutoff_sample(loc_0: torch.Tensor, vel_0: torch.Tensor,
                        loc_t: torch.Tensor, attr: torch.Tensor,
                        radius: float, cutoff_rate: float) -> Data:
    """One full-graph sample (reference process_dataset.py:176-198 protein,
    :263-277 water): radius graph on ``loc_0`` without self loops, optional
    longest-edge cutoff, edge_attr = distance x2, x = [|v|, attr / max attr],
    loc_mean = centroid."""
    ei = ref_ops.radius_graph(loc_0, radius)
    ei = _cutoff_edge(ei, loc_0, cutoff_rate)
    ea = (loc_0[ei[0]] - loc_0[ei[1]]).norm(p=2, dim=1) \
        .unsqueeze(-1).repeat(1, 2)
    speed = vel_0.pow(2).sum(1, keepdim=True).sqrt()
    x = torch.cat([speed, attr / attr.max()], dim=1)
    return Data(
        x=x, pos=loc_0, vel=vel_0, attr=attr, target=loc_t,
        loc_mean=loc_0.mean(0, keepdim=True), edge_index=ei, edge_attr=ea,
        special_nodes=torch.ones(loc_0.size(0), dtype=torch.bool))


def apply_test_augmentation(loc_0: torch.Tensor, vel_0: torch.Tensor,
                            loc_t: torch.Tensor, test_rot: bool,
                            test_trans: bool, box=None):
    """Test-split rigid motion (reference process_dataset.py:162-174): one
    random rotation applied to positions, velocities and targets, then one
    random translation ~ N(0, (box/2)^2) applied to positions and targets."""
    if test_rot:
        rot = torch.from_numpy(random_rotate()).to(loc_0.dtype)
        loc_0, vel_0, loc_t = loc_0 @ rot, vel_0 @ rot, loc_t @ rot
    if test_trans:
        box = np.ones(3) if box is None else np.asarray(box, dtype=np.float64)
        trans = torch.from_numpy(np.random.randn(3) * box[:3] / 2) \
            .unsqueeze(0).to(loc_0.dtype)
        loc_0, loc_t = loc_0 + trans, loc_t + trans
    return loc_0, vel_0, loc_t
