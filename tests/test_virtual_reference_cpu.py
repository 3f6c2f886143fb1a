"""CPU tests of ops/virtual_reference.py (the dtype-generic reference of the
fused virtual-edge block) against ``ops.eager_virtual_block``, and of the
fp32 weight order the fp32 forward kernels read."""

import pytest
import torch

from distegnn_amd import ops
from distegnn_amd.ops import prep
from distegnn_amd.ops import virtual_reference as VR

PARAMS = ("w1", "b1", "w2", "b2", "wxv", "bxv", "wxvv", "wX", "bX", "wXv")


def make_inputs(hd, n, c, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)

    def t(*shape, s):
        return (torch.randn(*shape, generator=g, dtype=torch.float64)
                * s).to(dtype)

    k_in = 2 * hd + 1 + c
    params = [t(hd, k_in, s=1.5 / k_in ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2), t(hd, s=0.3),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2), t(hd, s=0.3)]
    data = [t(n, hd, s=0.7), t(n, 3, s=1.0), t(2, c, 3, s=1.0),
            t(2, c, hd, s=0.7), t(2, c, c, s=0.5)]
    batch = torch.cat([torch.zeros(n // 2, dtype=torch.long),
                       torch.ones(n - n // 2, dtype=torch.long)])
    return data, batch, params


@pytest.mark.parametrize("hd,n,c", [(32, 21, 3), (64, 7, 8), (16, 5, 1)])
def test_matches_eager_fp32(hd, n, c):
    data, batch, params = make_inputs(hd, n, c)
    got = VR.virtual_block(*data, batch, *params)
    want = ops.eager_virtual_block(*data, batch, *params)
    for name, a, b in zip(("vmsg", "tv", "tx"), got, want):
        assert a.shape == b.shape and a.dtype == torch.float32, name
        assert float(b.norm()) > 0, name
        # same fp32 math; the reference takes the norm as sqrt(sum of
        # squares) and the dot of the heads in another order
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name


def test_float64_stays_float64_and_refines_fp32():
    data, batch, params = make_inputs(32, 33, 3, seed=1, dtype=torch.float64)
    f = VR.virtual_forward(*data, batch, *params)
    for k, v in f.items():
        assert v.dtype == torch.float64, k
    assert f["vin"].shape == (33, 3, 2 * 32 + 1 + 3)
    assert f["vmsg"].shape == (33, 3, 32)
    assert f["tv"].shape == f["tx"].shape == (33, 3, 3)
    lo = VR.virtual_block(*(t.float() for t in data), batch,
                          *(t.float() for t in params))
    for name, a, b in zip(("vmsg", "tv", "tx"), lo,
                          (f["vmsg"], f["tv"], f["tx"])):
        rel = float((a.double() - b).norm() / b.norm())
        assert rel < 1e-6, (name, rel)


def test_stage_identities():
    data, batch, params = make_inputs(32, 10, 2, seed=2, dtype=torch.float64)
    h, coord, vcoord, vfeat, gram = data
    f = VR.virtual_forward(*data, batch, *params)
    n = h.size(0)
    for i in (0, n // 2, n - 1):
        b = int(batch[i])
        for c in range(2):
            d = vcoord[b, c] - coord[i]
            assert torch.equal(f["vdiff"][i, c], d)
            want = torch.cat([h[i], vfeat[b, c], d.norm().view(1),
                              gram[b, c]])
            assert torch.allclose(f["vin"][i, c], want, rtol=0, atol=1e-15)
    assert torch.equal(f["tv"], -f["vdiff"] * f["pxv"].unsqueeze(-1))
    assert torch.equal(f["tx"], f["vdiff"] * f["pX"].unsqueeze(-1))


@pytest.mark.parametrize("hd,k", [(32, 67), (64, 131), (128, 259), (32, 66),
                                  (64, 137), (128, 262), (64, 64), (32, 32)])
def test_frag16_f32(hd, k):
    """The weight order of the fp32 kernels' MFMA loop: entry [kk, nt, lane]
    is the float4 W[nt*16 + (lane & 15)][kk*16 + (lane >> 4)*4 .. +3] of the
    weight zero padded to a multiple of 16 columns. Edge W1 (k = 2H+3) and
    virtual W1 (k = 2H+1+C, C <= 8) both pad to 2H+16."""
    w = torch.randn(hd, k, dtype=torch.float64)
    p = prep.get(w, "frag16_f32")
    k_pad = (k + 15) // 16 * 16
    if k > hd:
        assert k_pad == 2 * hd + 16
    assert p.dtype == torch.float32 and p.is_contiguous()
    assert p.shape == (k_pad // 16, hd // 16, 64, 4)
    wp = torch.zeros(hd, k_pad)
    wp[:, :k] = w.float()
    for kk in range(k_pad // 16):
        for nt in range(hd // 16):
            for lane in (0, 1, 15, 16, 37, 63):
                r, c = nt * 16 + (lane & 15), kk * 16 + (lane >> 4) * 4
                assert torch.equal(p[kk, nt, lane], wp[r, c:c + 4])
    # a permutation of the padded weight: nothing lost, nothing doubled
    assert torch.equal(p.flatten().sort().values, wp.flatten().sort().values)
