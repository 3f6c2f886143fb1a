"""Version-cached weight transforms for the fused HIP kernels.

The fused edge/virtual kernels read weights from padded/transposed/casted
global copies (bf16 K-contiguous fragments, fp32 biases — docs/KERNELS.md).
Round 1 recomputed those per call: ~150 tiny cast/pad/transpose kernels per
training step, replayed inside the captured hipGraph (~0.7-1.2 ms/step of
pure launch-sized kernels; profiles/README.md roadmap #3).

This cache keys each transform on the source tensor's ``_version`` counter:

* eager path: ``get`` checks the version per call and recomputes in place
  (``copy_`` into the existing buffer — stable addresses) only after the
  optimizer actually stepped.
* captured path: at capture time the cache is warm, so the graph records
  only READS of the cached buffers. Replays never run host code, therefore
  the runtime must call :func:`refresh` after every optimizer step (the
  trainer/bench optimizer regions do; see runtime/trainer.py) — it
  recomputes stale entries into the SAME buffers the graph references.

No-op transforms (e.g. ``.float()`` of an fp32 bias) are detected by
storage identity and passed through uncached.
"""

from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch
import torch.nn.functional as F

# Pad targets derive from the weight's input width (K_IN = w.size(1)):
# K_PAD = next multiple of the 32-wide MFMA k-step (aligned 16-B
# B-fragments), K_OUT = next multiple of 16 (dgrad n-tiles). H=64's
# K_IN=131 reproduces the tuned constants 160/144; the same formulas
# serve the H in {32, 128} edge-kernel instantiations and the virtual
# block's K_IN = 129+C.


def bf16c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().bfloat16().contiguous()


def f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def pad_kpad(t: torch.Tensor) -> torch.Tensor:
    """[O, k] -> [O, roundup32(k)] bf16 (column zero-pad)."""
    k_pad = (t.size(1) + 31) // 32 * 32
    return F.pad(t.detach().bfloat16(), (0, k_pad - t.size(1))).contiguous()


def frag16_f32(t: torch.Tensor) -> torch.Tensor:
    """[H, k] -> fp32 [roundup16(k)/16, H/16, 64, 4]: a weight of the fp32
    forward kernels in the order their MFMA loop reads it (csrc/mfma_f32.h).
    Columns are zero padded to a multiple of the 16-wide k-step; entry
    [kk, nt, lane] is the float4 W[nt*16 + (lane & 15)][kk*16 + (lane >> 4)*4
    .. +3], so one wave load is 1 KiB contiguous. Both blocks' W1 land on
    2H+16 columns (edge k = 2H+3, virtual k = 2H+1+C <= 2H+9)."""
    h, k = t.shape
    k_pad = (k + 15) // 16 * 16
    w = F.pad(t.detach().float(), (0, k_pad - k))
    return (w.view(h // 16, 16, k_pad // 16, 4, 4).permute(2, 0, 3, 1, 4)
            .reshape(k_pad // 16, h // 16, 64, 4).contiguous())


def tpad_kout(t: torch.Tensor) -> torch.Tensor:
    """[O, k] -> [roundup16(k), O] bf16 (transpose, row zero-pad)."""
    tt = t.detach().bfloat16().t().contiguous()
    k_out = (tt.size(0) + 15) // 16 * 16
    return F.pad(tt, (0, 0, 0, k_out - tt.size(0))).contiguous()


def t_bf16(t: torch.Tensor) -> torch.Tensor:
    return t.detach().bfloat16().t().contiguous()


def pad_gpad(t: torch.Tensor) -> torch.Tensor:
    """[F, G] -> [F, 64] bf16 (CFConv filter L1, gaussian dim padded)."""
    return F.pad(t.detach().bfloat16(), (0, 64 - t.size(1))).contiguous()


def hh_t(t: torch.Tensor) -> torch.Tensor:
    """Edge W1 [H, 2H+k] -> [H, 2H] bf16 holding [W1[:, :H]^T | W1[:, H:2H]^T]:
    the B matrix of ``gh = [S_row | S_col] @ B^T`` in the edge backward."""
    h = t.size(0)
    w = t.detach().bfloat16()
    return torch.cat([w[:, :h].t(), w[:, h:2 * h].t()], dim=1).contiguous()


_TRANSFORMS: Dict[str, Callable[[torch.Tensor], torch.Tensor]] = {
    "bf16": bf16c, "f32": f32c, "pad_kpad": pad_kpad,
    "tpad_kout": tpad_kout, "t_bf16": t_bf16, "pad_gpad": pad_gpad,
    "hh_t": hh_t, "frag16_f32": frag16_f32,
}

# Kinds read only by eager no-grad code (the fp32 evaluation kernels), never
# by a captured graph: ``get`` brings them up to date at their next use, so
# ``refresh`` / ``any_stale`` leave them alone and a training step pays
# nothing for the copies an evaluation epoch left behind.
_LAZY_KINDS = frozenset({"frag16_f32"})

# (id(tensor), kind) -> [version, buffer, source-tensor-ref]
_CACHE: Dict[Tuple[int, str], list] = {}


def get(t: torch.Tensor, kind: str) -> torch.Tensor:
    fn = _TRANSFORMS[kind]
    if not t.is_cuda:
        return fn(t)                      # CPU path: no caching needed
    key = (id(t), kind)
    ent = _CACHE.get(key)
    v = t._version
    if ent is None:
        buf = fn(t)
        if buf.data_ptr() == t.data_ptr() and buf.dtype == t.dtype:
            return buf                    # no-op transform: don't cache
        _CACHE[key] = [v, buf, t]         # keep t alive (id stability)
        return buf
    if ent[0] != v:
        ent[1].copy_(fn(t))
        ent[0] = v
    return ent[1]


def refresh() -> int:
    """Recompute every stale cached transform in place. MUST be called
    after optimizer steps when training under captured hipGraphs (replays
    read the cached buffers without running this module). Returns the
    number of refreshed entries."""
    n = 0
    for (tid, kind), ent in _CACHE.items():
        t = ent[2]
        if kind not in _LAZY_KINDS and ent[0] != t._version:
            ent[1].copy_(_TRANSFORMS[kind](t))
            ent[0] = t._version
            n += 1
    return n


def any_stale() -> bool:
    """Host-only version scan (no kernels) — lets GraphedStep decide
    whether a side-stream refresh is needed before replaying."""
    return any(ent[0] != ent[2]._version
               for (_, kind), ent in _CACHE.items()
               if kind not in _LAZY_KINDS)


def clear():
    _CACHE.clear()
