"""Water-3D HDF5 reader: one group per trajectory holding ``particle_type``
[N] and ``position`` [T, N, 3] (dataset_generation/Water-3D/tfrecord_to_h5.py).

h5py is used when installed; otherwise the in-tree ``hdf5lite`` reader, which
covers the subset of the format those files use."""

from __future__ import annotations

import random
from typing import Iterator, List, Tuple

import numpy as np
import torch


def _open(path: str):
    try:
        import h5py
    except ImportError:
        from . import hdf5lite

        return hdf5lite.File(path)
    return h5py.File(path, "r")


def iter_water3d_trajectories(path: str
                              ) -> Iterator[Tuple[str, torch.Tensor,
                                                  torch.Tensor]]:
    """Yield ``(key, particle_type [N,1] float, position [T,N,3] float)`` per
    trajectory group, in the file's key order (reference
    process_dataset.py:240-243)."""
    with _open(path) as f:
        for key in list(f.keys()):
            grp = f[key]
            ptype = torch.tensor(np.array(grp["particle_type"])).float() \
                .unsqueeze(-1)
            pos = torch.tensor(np.array(grp["position"])).float()
            yield key, ptype, pos


def sample_frames(num_frames: int, budget: int, max_frame: int = 250
                  ) -> List[int]:
    """``min(num_frames, budget)`` start frames drawn uniformly from
    [0, max_frame] with the global ``random`` state (reference :245)."""
    max_frame = max(0, int(max_frame))
    return [random.randint(0, max_frame)
            for _ in range(max(0, min(num_frames, budget)))]
