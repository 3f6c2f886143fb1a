"""Stage-by-stage reference of the fused CFConv message (csrc/cfconv.hip).

Plain torch in the dtype of ``xw1`` (the tests pass float64), mirroring the
kernel's contract and nothing of its arithmetic:

* ``xw1`` [N, F] holds bf16 values (the kernel reads bf16 rows);
* ``w1`` [F, G] and ``w2`` [F, F] are rounded to bf16 here, as
  ``prep.get(w, "pad_gpad" / "bf16")`` delivers them to the kernel (straight
  through for autograd: the gradient is that of the rounded weight);
* ``b1``, ``b2``, ``offsets``, ``dist`` keep their fp32 values;
* there is no mask beyond the cutoff: the cosine simply continues, as in
  models/schnet.py.

Chain, per edge e with source node j = col[e]:

  gauss_k = exp(coeff (d_e - offset_k)^2)                  [M, G]
  z1      = softplus(gauss W1^T + b1) - log 2              [M, F]
  w       = z1 W2^T + b2                                   [M, F]
  cf      = (cos(pi d_e / cutoff) + 1) / 2                 [M]
  msg     = xw1[j] * w * cf                                [M, F]

No stage is rounded. tests/test_cfconv_reference_cpu.py holds the chain
against the modules of models/schnet.py and against autograd.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """bf16 values in t's dtype; identity for autograd."""
    d = t.detach()
    return t + (d.bfloat16().to(t.dtype) - d)


def cfconv_stages(xw1, dist, col, w1, b1, w2, b2, offsets, coeff, cutoff):
    """All stages of the chain above: dict with ``gauss`` [M, G],
    ``pre1`` [M, F] (the argument of the softplus), ``z1`` [M, F],
    ``w`` [M, F], ``cf`` [M], ``xj`` [M, F] and ``msg`` [M, F]."""
    dt = xw1.dtype
    dist, b1, b2, offsets = (t.to(dt) for t in (dist, b1, b2, offsets))
    w1, w2 = round_bf16(w1.to(dt)), round_bf16(w2.to(dt))
    dk = dist.view(-1, 1) - offsets.view(1, -1)
    gauss = torch.exp(coeff * dk * dk)
    pre1 = gauss @ w1.t() + b1
    # beyond x = 40, softplus(x) - x = e^-40 is below float64 resolution
    z1 = F.softplus(pre1, beta=1.0, threshold=40.0) - math.log(2.0)
    w = z1 @ w2.t() + b2
    cf = 0.5 * (torch.cos(dist * (math.pi / cutoff)) + 1.0)
    xj = xw1.index_select(0, col)
    msg = xj * w * cf.view(-1, 1)
    return dict(gauss=gauss, pre1=pre1, z1=z1, w=w, cf=cf, xj=xj, msg=msg)


def cfconv_msg(xw1, dist, col, w1, b1, w2, b2, offsets, coeff, cutoff):
    return cfconv_stages(xw1, dist, col, w1, b1, w2, b2, offsets, coeff,
                         cutoff)["msg"]
