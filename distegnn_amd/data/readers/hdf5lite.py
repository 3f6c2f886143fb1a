"""Pure-python reader/writer for the HDF5 subset the Water-3D files use.

h5py is not always installable next to a ROCm PyTorch stack; the Water-3D
trajectories (dataset_generation/Water-3D/tfrecord_to_h5.py) only need a small
corner of the format, which this module implements from the public HDF5 file
format specification (version 0 superblock era, what h5py writes by default):

* superblock version 0/1, also behind a user block (searched at 0, 512, ...),
* version 1 object headers incl. continuation blocks,
* old-style groups: symbol table message -> v1 B-tree -> symbol table nodes
  -> local heap names,
* datasets of little/big-endian integers and IEEE floats with contiguous or
  compact layout (data layout message versions 1-3).

Not covered (NotImplementedError): superblock >= 2 / new-style groups,
chunked or filtered datasets, compound/string/vlen types, shared messages.

``write(path, tree)`` emits files of the same subset from a nested dict
``{name: ndarray | {name: ...}}``; they open in h5py/libhdf5.
"""

from __future__ import annotations

import struct
from typing import Dict, List, Tuple

import numpy as np

SIGNATURE = b"\x89HDF\r\n\x1a\n"
UNDEF = 0xFFFFFFFFFFFFFFFF
_LEAF_K = 4        # symbol table node holds 2K entries
_INTERNAL_K = 16   # group B-tree node holds 2K children
_HEAP_FREE_NULL = 1

MSG_DATASPACE = 0x0001
MSG_DATATYPE = 0x0003
MSG_FILL = 0x0005
MSG_LAYOUT = 0x0008
MSG_CONTINUATION = 0x0010
MSG_SYMBOL_TABLE = 0x0011


# ---------------------------------------------------------------------------
# reader

class _Reader:
    def __init__(self, path: str):
        self.f = open(path, "rb")
        self.base = 0
        self.root_header = self._superblock()

    def read(self, addr: int, n: int) -> bytes:
        self.f.seek(self.base + addr)
        buf = self.f.read(n)
        if len(buf) != n:
            raise ValueError(f"truncated HDF5 file: wanted {n} bytes at "
                             f"{self.base + addr}, got {len(buf)}")
        return buf

    def _superblock(self) -> int:
        self.f.seek(0, 2)
        end = self.f.tell()
        at = 0
        while at < end:
            self.f.seek(at)
            if self.f.read(8) == SIGNATURE:
                break
            at = 512 if at == 0 else at * 2
        else:
            raise ValueError("not an HDF5 file (no superblock signature)")
        self.f.seek(at + 8)
        head = self.f.read(16)
        version = head[0]
        if version > 1:
            raise NotImplementedError(
                f"HDF5 superblock version {version} (hdf5lite reads 0/1)")
        if head[5] != 8 or head[6] != 8:
            raise NotImplementedError("only 8-byte offsets/lengths supported")
        # v1 adds indexed-storage K (2) + reserved (2) before the addresses
        off = at + 8 + 16 + (4 if version == 1 else 0)
        self.f.seek(off)
        base, _free, _eof, _drv = struct.unpack("<4Q", self.f.read(32))
        entry = self.f.read(40)
        # files behind a user block store base 0 but address relative to the
        # superblock
        self.base = base if base else at
        return struct.unpack_from("<Q", entry, 8)[0]

    # -- object headers ----------------------------------------------------
    def messages(self, addr: int) -> List[Tuple[int, int, bytes]]:
        """[(type, flags, data)] of a version 1 object header."""
        prefix = self.read(addr, 16)
        if prefix[:4] == b"OHDR":
            raise NotImplementedError("version 2 object headers")
        version, _, nmsg, _refs, size = struct.unpack_from("<BBHII", prefix)
        if version != 1:
            raise ValueError(f"bad object header version {version} at {addr}")
        out: List[Tuple[int, int, bytes]] = []
        blocks = [(addr + 16, size)]
        while blocks and len(out) < nmsg:
            baddr, bsize = blocks.pop(0)
            buf = self.read(baddr, bsize)
            p = 0
            while p + 8 <= bsize and len(out) < nmsg:
                mtype, msize, flags = struct.unpack_from("<HHB", buf, p)
                data = buf[p + 8:p + 8 + msize]
                p += 8 + msize
                if mtype == MSG_CONTINUATION:
                    blocks.append(struct.unpack_from("<QQ", data))
                out.append((mtype, flags, data))
        return out

    # -- groups --------------------------------------------------------------
    def group_entries(self, btree: int, heap: int) -> Dict[str, int]:
        """name -> object header address, in B-tree (name) order."""
        hp = self.read(heap, 32)
        if hp[:4] != b"HEAP":
            raise ValueError(f"bad local heap signature at {heap}")
        seg_size, _free, seg_addr = struct.unpack_from("<QQQ", hp, 8)
        names = self.read(seg_addr, seg_size)
        out: Dict[str, int] = {}
        self._walk_group_tree(btree, names, out)
        return out

    def _walk_group_tree(self, addr: int, names: bytes, out: Dict[str, int]):
        head = self.read(addr, 24)
        if head[:4] == b"SNOD":
            nsym = struct.unpack_from("<H", head, 6)[0]
            buf = self.read(addr + 8, nsym * 40)
            for i in range(nsym):
                name_off, obj = struct.unpack_from("<QQ", buf, i * 40)
                end = names.index(b"\0", name_off)
                out[names[name_off:end].decode()] = obj
            return
        if head[:4] != b"TREE" or head[4] != 0:
            raise ValueError(f"bad group B-tree node at {addr}")
        used = struct.unpack_from("<H", head, 6)[0]
        buf = self.read(addr + 24, (2 * used + 1) * 8)
        for i in range(used):
            child = struct.unpack_from("<Q", buf, (2 * i + 1) * 8)[0]
            self._walk_group_tree(child, names, out)


def _decode_dtype(data: bytes) -> np.dtype:
    cls = data[0] & 0x0F
    bits0 = data[1]
    size = struct.unpack_from("<I", data, 4)[0]
    order = ">" if bits0 & 1 else "<"
    if cls == 0:
        kind = "i" if bits0 & 0x08 else "u"
    elif cls == 1:
        kind = "f"
        if size not in (2, 4, 8):
            raise NotImplementedError(f"{size}-byte floating point")
    else:
        raise NotImplementedError(f"HDF5 datatype class {cls}")
    return np.dtype(f"{order}{kind}{size}")


def _decode_shape(data: bytes) -> Tuple[int, ...]:
    version, rank = data[0], data[1]
    if version == 1:
        off = 8
    elif version == 2:
        if data[3] == 2:       # null dataspace
            return (0,)
        off = 4
    else:
        raise NotImplementedError(f"dataspace message version {version}")
    return tuple(struct.unpack_from(f"<{rank}Q", data, off))


class Dataset:
    """Lazy dataset handle: ``np.array(ds)`` / ``ds[...]`` read the data."""

    def __init__(self, reader: _Reader, msgs):
        self._r = reader
        self.shape: Tuple[int, ...] = ()
        self.dtype = None
        self._addr = UNDEF
        self._inline = None
        for mtype, flags, data in msgs:
            if flags & 0x02 and mtype in (MSG_DATATYPE, MSG_DATASPACE):
                raise NotImplementedError("shared (committed) messages")
            if mtype == MSG_DATASPACE:
                self.shape = _decode_shape(data)
            elif mtype == MSG_DATATYPE:
                self.dtype = _decode_dtype(data)
            elif mtype == MSG_LAYOUT:
                self._decode_layout(data)
            elif mtype == 0x000B:
                raise NotImplementedError("filtered (compressed) datasets")
        if self.dtype is None:
            raise ValueError("dataset without a datatype message")

    def _decode_layout(self, data: bytes):
        version = data[0]
        if version == 3:
            cls = data[1]
            if cls == 1:
                self._addr = struct.unpack_from("<Q", data, 2)[0]
            elif cls == 0:
                n = struct.unpack_from("<H", data, 2)[0]
                self._inline = data[4:4 + n]
            else:
                raise NotImplementedError("chunked datasets")
        elif version in (1, 2):
            rank, cls = data[1], data[2]
            if cls == 1:
                self._addr = struct.unpack_from("<Q", data, 8)[0]
            elif cls == 0:
                p = 8 + 4 * rank
                n = struct.unpack_from("<I", data, p)[0]
                self._inline = data[p + 4:p + 4 + n]
            else:
                raise NotImplementedError("chunked datasets")
        else:
            raise NotImplementedError(f"data layout version {version}")

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64))

    def __len__(self) -> int:
        return self.shape[0]

    def _load(self) -> np.ndarray:
        nbytes = self.size * self.dtype.itemsize
        if self._inline is not None:
            raw = self._inline[:nbytes]
        elif self._addr == UNDEF or nbytes == 0:
            # never-written contiguous dataset: default fill value
            return np.zeros(self.shape, dtype=self.dtype.newbyteorder("="))
        else:
            raw = self._r.read(self._addr, nbytes)
        arr = np.frombuffer(raw, dtype=self.dtype).reshape(self.shape)
        return arr.astype(self.dtype.newbyteorder("="))

    def __array__(self, dtype=None, copy=None):
        arr = self._load()
        return arr if dtype is None else arr.astype(dtype, copy=False)

    def __getitem__(self, idx):
        return self._load()[idx]


class Group:
    def __init__(self, reader: _Reader, btree: int, heap: int):
        self._r = reader
        self._entries = reader.group_entries(btree, heap)

    def keys(self):
        return self._entries.keys()

    def __iter__(self):
        return iter(self._entries)

    def __len__(self) -> int:
        return len(self._entries)

    def __contains__(self, name) -> bool:
        return name in self._entries

    def __getitem__(self, name: str):
        node = self
        for part in name.strip("/").split("/"):
            node = node._child(part)
        return node

    def _child(self, name: str):
        if name not in self._entries:
            raise KeyError(name)
        msgs = self._r.messages(self._entries[name])
        for mtype, _flags, data in msgs:
            if mtype == MSG_SYMBOL_TABLE:
                return Group(self._r, *struct.unpack_from("<QQ", data))
        if any(m[0] == MSG_LAYOUT for m in msgs):
            return Dataset(self._r, msgs)
        raise NotImplementedError(
            f"object {name!r} is neither an old-style group nor a dataset")


class File(Group):
    """Read-only file handle; use as a context manager like ``h5py.File``."""

    def __init__(self, path: str, mode: str = "r"):
        if mode != "r":
            raise ValueError("hdf5lite.File is read-only; see hdf5lite.write")
        reader = _Reader(path)
        try:
            for mtype, _flags, data in reader.messages(reader.root_header):
                if mtype == MSG_SYMBOL_TABLE:
                    super().__init__(reader,
                                     *struct.unpack_from("<QQ", data))
                    break
            else:
                raise NotImplementedError("root group is not an old-style "
                                          "(symbol table) group")
        except Exception:
            reader.f.close()
            raise

    def close(self):
        self._r.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------
# writer

def _encode_dtype(dt: np.dtype) -> bytes:
    big = 1 if dt.byteorder == ">" else 0
    if dt.kind in "iu":
        bits0 = big | (0x08 if dt.kind == "i" else 0)
        return struct.pack("<BBBBIHH", 0x10, bits0, 0, 0, dt.itemsize,
                           0, 8 * dt.itemsize)
    if dt.kind == "f" and dt.itemsize in (2, 4, 8):
        exp_bits, man_bits, bias = {2: (5, 10, 15), 4: (8, 23, 127),
                                    8: (11, 52, 1023)}[dt.itemsize]
        # implied-msb mantissa normalization, sign in the top bit
        return struct.pack("<BBBBIHHBBBBI", 0x11, 0x20 | big,
                           8 * dt.itemsize - 1, 0, dt.itemsize,
                           0, 8 * dt.itemsize, man_bits, exp_bits, 0,
                           man_bits, bias)
    raise TypeError(f"hdf5lite.write: unsupported dtype {dt}")


def _message(mtype: int, data: bytes, flags: int = 0) -> bytes:
    data += b"\0" * (-len(data) % 8)
    return struct.pack("<HHB3x", mtype, len(data), flags) + data


def _object_header(msgs: List[bytes]) -> bytes:
    body = b"".join(msgs)
    return struct.pack("<BBHII4x", 1, 0, len(msgs), 1, len(body)) + body


class _Writer:
    def __init__(self):
        self.buf = bytearray(96)     # superblock is filled in last

    def put(self, data: bytes) -> int:
        self.buf += b"\0" * (-len(self.buf) % 8)
        addr = len(self.buf)
        self.buf += data
        return addr

    def dataset(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        if arr.dtype.byteorder == "=":
            arr = arr.astype(arr.dtype.newbyteorder("<"))
        data_addr = self.put(arr.tobytes()) if arr.size else UNDEF
        space = struct.pack("<BBB5x", 1, arr.ndim, 0) \
            + struct.pack(f"<{arr.ndim}Q", *arr.shape)
        msgs = [
            _message(MSG_DATASPACE, space),
            _message(MSG_DATATYPE, _encode_dtype(arr.dtype), flags=1),
            # v2 fill message: late allocation, write-if-set, default value
            _message(MSG_FILL, struct.pack("<BBBBI", 2, 2, 2, 1, 0), flags=1),
            _message(MSG_LAYOUT, struct.pack("<BBQQ", 3, 1, data_addr,
                                             arr.nbytes)),
        ]
        return self.put(_object_header(msgs))

    def group(self, tree: dict) -> Tuple[int, int, int]:
        """Write a group and everything below it; returns (object header,
        B-tree, local heap) addresses."""
        children = {}
        for name, node in tree.items():
            if isinstance(node, dict):
                children[name.encode()] = self.group(node)[0]
            else:
                children[name.encode()] = self.dataset(np.asarray(node))
        names = sorted(children)     # bytewise order == strcmp order

        # local heap: "" at offset 0, the names, then one free block
        seg = bytearray(8)
        name_off = {}
        for n in names:
            name_off[n] = len(seg)
            seg += n + b"\0"
            seg += b"\0" * (-len(seg) % 8)
        free_head = len(seg)
        seg += struct.pack("<QQ", _HEAP_FREE_NULL, 16)
        seg_addr = self.put(bytes(seg))
        heap = self.put(b"HEAP" + struct.pack("<B3xQQQ", 0, len(seg),
                                               free_head, seg_addr))

        # symbol table nodes, 2K entries each, all slots allocated
        per = 2 * _LEAF_K
        level = []                   # [(address, heap offset of last name)]
        for i in range(0, len(names), per):
            part = names[i:i + per]
            node = bytearray(b"SNOD" + struct.pack("<BBH", 1, 0, len(part)))
            for n in part:
                node += struct.pack("<QQII16x", name_off[n], children[n],
                                    0, 0)
            node += b"\0" * (8 + per * 40 - len(node))
            level.append((self.put(bytes(node)), name_off[part[-1]]))

        # B-tree levels above them, 2K children per node
        fan = 2 * _INTERNAL_K
        node_size = 24 + (2 * fan + 1) * 8
        depth = 0
        while True:
            groups = [level[i:i + fan] for i in range(0, len(level), fan)] \
                or [[]]
            addrs = [self.put(b"\0" * node_size) for _ in groups]
            left_key = 0
            for gi, grp in enumerate(groups):
                node = bytearray(b"TREE" + struct.pack(
                    "<BBHQQ", 0, depth, len(grp),
                    addrs[gi - 1] if gi > 0 else UNDEF,
                    addrs[gi + 1] if gi + 1 < len(groups) else UNDEF))
                node += struct.pack("<Q", left_key)
                for child, last in grp:
                    node += struct.pack("<QQ", child, last)
                    left_key = last
                self.buf[addrs[gi]:addrs[gi] + len(node)] = node
            level = [(a, g[-1][1] if g else 0)
                     for a, g in zip(addrs, groups)]
            depth += 1
            if len(level) == 1:
                break
        btree = level[0][0]
        header = self.put(_object_header(
            [_message(MSG_SYMBOL_TABLE, struct.pack("<QQ", btree, heap))]))
        return header, btree, heap

    def finish(self, root: Tuple[int, int, int]) -> bytes:
        header, btree, heap = root
        self.buf += b"\0" * (-len(self.buf) % 8)
        sb = SIGNATURE + struct.pack(
            "<BBBBBBBBHHI", 0, 0, 0, 0, 0, 8, 8, 0, _LEAF_K, _INTERNAL_K, 0)
        sb += struct.pack("<QQQQ", 0, UNDEF, len(self.buf), UNDEF)
        # root symbol table entry caches its B-tree/heap (cache type 1)
        sb += struct.pack("<QQIIQQ", 0, header, 1, 0, btree, heap)
        assert len(sb) == 96
        self.buf[:96] = sb
        return bytes(self.buf)


def write(path: str, tree: dict) -> None:
    """Write ``{name: ndarray | nested dict}`` as an HDF5 file."""
    w = _Writer()
    data = w.finish(w.group(tree))
    with open(path, "wb") as f:
        f.write(data)
