"""Real-data readers for the four reference workloads.

* ``water3d``   — per-trajectory HDF5 groups (h5py when installed, else the
  in-tree ``hdf5lite`` subset reader).
* ``fluid113k`` — 16-chunk msgpack(.zst) simulations with a built-in
  msgpack_numpy-compatible array codec.
* ``protein``   — AdK equilibrium trajectory via guarded MDAnalysis.
* ``common``    — sample assembly shared by the cutoff-mode pipelines.

nbody ``.npy`` files need no reader of their own (data/preprocess.py).
"""
