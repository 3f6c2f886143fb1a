"""AdK equilibrium trajectory (the protein dataset) via MDAnalysis.

MDAnalysis/MDAnalysisData are optional: importing this module never needs
them, ``load_adk`` raises a clear ImportError when they are missing (the
synthetic protein path in data/preprocess.py does not call it)."""

from __future__ import annotations

import torch

# reference process_dataset.py:205-209
TRAIN_VALID_TEST_SPLIT = {
    "train": (0, 2481),
    "valid": (2481, 2481 + 827),
    "test": (2481 + 827, 2481 + 827 + 863),
}


def load_adk(data_dir: str, backbone: bool = True):
    """Returns ``(universe, atom_ix, charges [N,1], n_frames, dimensions)``
    for the AdK equilibrium dataset cached (or fetched) under ``data_dir``."""
    try:
        import MDAnalysis
        import MDAnalysisData
    except ImportError as e:
        raise ImportError(
            "the real protein dataset needs MDAnalysis and MDAnalysisData "
            f"({e}); install them or set data.synthetic") from e
    adk = MDAnalysisData.datasets.fetch_adk_equilibrium(data_home=data_dir)
    universe = MDAnalysis.Universe(adk.topology, adk.trajectory)
    ag = universe.select_atoms("backbone") if backbone else universe.atoms
    atom_ix = ag.ix
    charges = torch.tensor(universe.atoms[atom_ix].charges).float() \
        .unsqueeze(-1)
    return (universe, atom_ix, charges, len(universe.trajectory),
            universe.trajectory[0].dimensions.copy())


def read_frame_triplet(universe, atom_ix, t: int, delta_t: int):
    """``(loc_0, vel_0, loc_t, box)`` for start frame ``t`` (reference
    :149-159): velocity is the one-frame position difference."""
    # copy each timestep: the trajectory reader reuses its frame buffer
    ts_0 = universe.trajectory[t].copy()
    ts_1 = universe.trajectory[t + 1].copy()
    ts_t = universe.trajectory[t + delta_t].copy()
    loc_0 = torch.tensor(ts_0.positions[atom_ix])
    vel_0 = torch.tensor(ts_1.positions[atom_ix]) - loc_0
    loc_t = torch.tensor(ts_t.positions[atom_ix])
    return loc_0, vel_0, loc_t, ts_0.dimensions[:3]
