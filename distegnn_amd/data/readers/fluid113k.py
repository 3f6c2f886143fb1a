"""Fluid113K record reader/writer.

A simulation is 16 chunk files ``sim_NNNN_CC.msgpack.zst``; each chunk is a
msgpack list of frame dicts (``pos``/``vel`` [N,3], per-particle
``viscosity``/``m``, ``frame_id``) whose numpy values use the msgpack_numpy
wire format (reference process_dataset.py:480-497). The codec below is
compatible with that format without needing the msgpack_numpy package.
zstd (de)compression needs the optional ``zstandard`` package; uncompressed
``.msgpack`` chunks are accepted everywhere a ``.zst`` one is."""

from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np
import torch

NUM_CHUNKS = 16


def encode_numpy(obj):
    """msgpack ``default=`` hook: numpy arrays/scalars -> msgpack_numpy maps."""
    if isinstance(obj, np.ndarray):
        if obj.dtype.kind in "OV":
            raise TypeError(f"cannot pack arrays of dtype {obj.dtype}")
        return {b"nd": True, b"type": obj.dtype.str, b"kind": b"",
                b"shape": list(obj.shape),
                b"data": np.ascontiguousarray(obj).tobytes()}
    if isinstance(obj, (np.bool_, np.number)):
        return {b"nd": False, b"type": obj.dtype.str, b"data": obj.tobytes()}
    raise TypeError(f"cannot pack object of type {type(obj)}")


def _decode_numpy(obj):
    """msgpack ``object_hook=``: msgpack_numpy maps -> numpy arrays/scalars
    (keys arrive as bytes or str depending on how the file was packed)."""
    def get(k):
        return obj[k] if k in obj else obj[k.decode()]

    if b"nd" not in obj and "nd" not in obj:
        return obj
    descr = get(b"type")
    if isinstance(descr, bytes):
        descr = descr.decode()
    if get(b"nd"):
        arr = np.frombuffer(get(b"data"), dtype=np.dtype(descr))
        return arr.reshape(get(b"shape")).copy()
    return np.frombuffer(get(b"data"), dtype=np.dtype(descr))[0]


def _zstd():
    try:
        import zstandard
    except ImportError as e:
        raise ImportError(
            "reading or writing .zst chunks needs the zstandard package; "
            "use uncompressed .msgpack chunks without it") from e
    return zstandard


def write_chunk(path: str, frames) -> None:
    """Pack a list of frame dicts to ``path`` (zstd when it ends in .zst)."""
    import msgpack

    zstd = _zstd() if path.endswith(".zst") else None
    packed = msgpack.packb(list(frames), default=encode_numpy,
                           use_bin_type=True)
    if zstd is not None:
        packed = zstd.ZstdCompressor().compress(packed)
    with open(path, "wb") as f:
        f.write(packed)


def _read_chunk(path: str) -> list:
    """All frame dicts of one chunk file."""
    import msgpack

    zstd = _zstd() if path.endswith(".zst") else None
    with open(path, "rb") as f:
        raw = f.read()
    if zstd is not None:
        raw = zstd.ZstdDecompressor().decompress(raw)
    return msgpack.unpackb(raw, raw=False, object_hook=_decode_numpy,
                           strict_map_key=False)


def _chunk_path(base_dir: str, idx: int, chunk: int) -> str:
    stem = os.path.join(base_dir, f"sim_{idx:04d}_{chunk:02d}.msgpack")
    if os.path.exists(stem + ".zst") or not os.path.exists(stem):
        return stem + ".zst"
    return stem


def read_fluid_sim(base_dir: str, idx: int
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                              torch.Tensor]:
    """``(position [T,N,3], velocity [T,N,3], viscosity [N], mass [N])`` of
    simulation ``idx``, frames concatenated over its 16 chunks in order."""
    position: List[np.ndarray] = []
    vel: List[np.ndarray] = []
    viscosity = mass = None
    for c in range(NUM_CHUNKS):
        path = _chunk_path(base_dir, idx, c)
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} (or its uncompressed .msgpack) not found: place the "
                f"Fluid113K records under data_dir, or set data.synthetic")
        frames = _read_chunk(path)
        for frame in frames:
            position.append(np.asarray(frame["pos"]))
            vel.append(np.asarray(frame["vel"]))
        if frames:
            viscosity, mass = frames[0]["viscosity"], frames[0]["m"]
    return (torch.tensor(np.array(position)).float(),
            torch.tensor(np.array(vel)).float(),
            torch.tensor(np.array(viscosity)).float(),
            torch.tensor(np.array(mass)).float())
