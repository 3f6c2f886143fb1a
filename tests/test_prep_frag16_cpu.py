"""``prep.frag16_f32`` on the node block's W1 [H, 3H+A]: the fragment order
the fp32 kernels' MFMA loop reads (csrc/mfma_f32.h), against a direct index
formula. A = 0 gives 3H/16 k-steps and no padding, A in 1..8 one more k-step
whose columns past 3H+A are zero."""

import pytest
import torch

from distegnn_amd.ops import prep


@pytest.mark.parametrize("a", [0, 2, 8])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_frag16_f32_node_w1(hd, a):
    k = 3 * hd + a
    ksteps = 3 * hd // 16 + (1 if a else 0)
    # distinct values: every misplaced element shows
    w = torch.arange(1, hd * k + 1, dtype=torch.float32).view(hd, k)
    got = prep.frag16_f32(w)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert got.shape == (ksteps, hd // 16, 64, 4)
    kk = torch.arange(ksteps).view(-1, 1, 1, 1)
    nt = torch.arange(hd // 16).view(1, -1, 1, 1)
    lane = torch.arange(64).view(1, 1, -1, 1)
    j = torch.arange(4).view(1, 1, 1, -1)
    row = (nt * 16 + (lane & 15)).expand(got.shape)
    col = (kk * 16 + (lane >> 4) * 4 + j).expand(got.shape)
    want = torch.where(col < k, w[row, col.clamp(max=k - 1)],
                       torch.zeros(()))
    assert torch.equal(got, want)
    # every weight appears exactly once, the rest is padding
    assert int((got != 0).sum()) == hd * k
    assert got.numel() == hd * ksteps * 16


def test_frag16_f32_is_detached_and_leaves_its_source_alone():
    w = torch.randn(32, 98, requires_grad=True)
    before = w.detach().clone()
    got = prep.frag16_f32(w)
    assert not got.requires_grad
    assert torch.equal(w.detach(), before)
