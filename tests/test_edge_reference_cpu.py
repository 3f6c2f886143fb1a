"""CPU check of the stage reference the GPU edge-block tests trust
(distegnn_amd/ops/edge_reference.py): in float64 its forward is
``ops.eager_edge_block`` and its hand-derived backward chain is
``torch.autograd.grad`` of that composition."""

import pytest
import torch

from distegnn_amd import ops
from distegnn_amd.data.graph import Data, collate
from distegnn_amd.ops import edge_reference as ER

H = 8
N = 12
M = 64 + 7          # one full 64-edge tile and a tail
ISOLATED = 5        # neither a row nor a col of any edge


def _graph():
    g = torch.Generator().manual_seed(0)
    nodes = torch.tensor([i for i in range(N) if i != ISOLATED])
    row = nodes[torch.randint(0, N - 1, (M,), generator=g)]
    col = nodes[torch.randint(0, N - 1, (M,), generator=g)]
    col = torch.where(col == row, nodes[(row + 1) % (N - 1)], col)
    col = torch.where(col == row, nodes[(row + 2) % (N - 1)], col)
    bt = collate([Data(
        pos=torch.randn(N, 3, generator=g, dtype=torch.float64),
        edge_index=torch.stack([row, col]),
        edge_attr=torch.randn(M, 2, generator=g, dtype=torch.float64))])
    assert bt.num_edges == M and M % 64 != 0
    assert not bool((bt.edge_index == ISOLATED).any())
    assert bool((bt.edge_index[0] != bt.edge_index[1]).all())
    return bt


def _params():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return [r(H, 2 * H + 3) * 0.3, r(H) * 0.2, r(H, H) * 0.4, r(H) * 0.2,
            r(H, H) * 0.4, r(H) * 0.2, r(H) * 0.5]


def _rel(got, want):
    return float((got - want).norm() / want.norm())


@pytest.mark.parametrize("normalize", [False, True])
def test_stage_reference_is_the_eager_composition(normalize):
    bt = _graph()
    row, col = bt.edge_index[0], bt.edge_index[1]
    g = torch.Generator().manual_seed(2)
    h = torch.randn(N, H, generator=g, dtype=torch.float64)
    params = _params()
    dmsg_n = torch.randn(N, H, generator=g, dtype=torch.float64)
    dtrans_n = torch.randn(N, 3, generator=g, dtype=torch.float64)
    eps = 1e-8

    leaves = [t.clone().requires_grad_(True)
              for t in [h, bt.pos] + params]
    msg_e, trans_e = ops.eager_edge_block(
        leaves[0], leaves[1], bt.edge_attr, row, col, bt.rowptr, bt.colptr,
        bt.col_perm, *leaves[2:], normalize, eps)
    assert msg_e.dtype == torch.float64 and trans_e.dtype == torch.float64

    fwd = ER.edge_forward(h, bt.pos, bt.edge_attr, row, col, *params,
                          normalize, eps)
    assert _rel(fwd["msg"], msg_e.detach()) <= 1e-12
    assert _rel(fwd["trans"], trans_e.detach()) <= 1e-12

    grads = torch.autograd.grad(
        (msg_e, trans_e), leaves,
        grad_outputs=(dmsg_n.index_select(0, row),
                      dtrans_n.index_select(0, row)))
    w1, _, w2, _, w3, _, w3v = params
    bwd = ER.edge_backward(fwd, row, col, dmsg_n, dtrans_n, w1, w2, w3, w3v,
                           N)
    gb1, gb2, gb3 = bwd["gb"].split(H)
    got = [bwd["gh"], bwd["gc"], bwd["gw1"], gb1, bwd["gw2"], gb2,
           bwd["gw3"], gb3, bwd["dw3v"]]
    names = ["h", "coord", "w1", "b1", "w2", "b2", "w3", "b3", "w3v"]
    for nm, a, b in zip(names, got, grads):
        assert a.shape == b.shape, nm
        assert float(b.norm()) > 0, nm
        assert _rel(a, b) <= 1e-10, (nm, _rel(a, b))
    # the isolated node receives nothing
    assert bool((bwd["gh"][ISOLATED] == 0).all())
    assert bool((bwd["gc"][ISOLATED] == 0).all())

    # the aggregated form used by the end-to-end GPU test: same function
    leaves2 = [t.clone().requires_grad_(True)
               for t in [h, bt.pos] + params]
    am, at = ER.edge_block_mean(leaves2[0], leaves2[1], bt.edge_attr, row,
                                col, *leaves2[2:], normalize, eps)
    deg = torch.bincount(row, minlength=N).clamp(min=1).double()
    want_m = torch.zeros(N, H, dtype=torch.float64).index_add_(
        0, row, msg_e.detach()) / deg.unsqueeze(1)
    want_t = torch.zeros(N, 3, dtype=torch.float64).index_add_(
        0, row, trans_e.detach()) / deg.unsqueeze(1)
    assert _rel(am.detach(), want_m) <= 1e-12
    assert _rel(at.detach(), want_t) <= 1e-12
    # cotangent dagg = deg * dX_n gives the per-edge cotangents used above
    g2 = torch.autograd.grad(
        (am, at), leaves2,
        grad_outputs=(dmsg_n * deg.unsqueeze(1), dtrans_n * deg.unsqueeze(1)))
    for nm, a, b in zip(names, g2, grads):
        assert _rel(a, b) <= 1e-10, (nm, _rel(a, b))


def test_chunk_tables_match_batch():
    """Batch builds its pooling tables with build_chunk_tables: 256-row
    chunks, only above 4096 nodes."""
    from distegnn_amd.data.graph import build_chunk_tables

    cb, ce, scp = build_chunk_tables(torch.tensor([0, 0, 1, 257, 769, 769]))
    assert cb.tolist() == [0, 1, 257, 513]
    assert ce.tolist() == [1, 257, 513, 769]
    assert scp.tolist() == [0, 0, 1, 2, 4, 4]
    small = collate([Data(pos=torch.zeros(4096, 3))])
    assert small.pool_chunk_begin is None
    big = collate([Data(pos=torch.zeros(4097, 3)),
                   Data(pos=torch.zeros(10, 3))])
    assert big.pool_chunk_begin.tolist() == list(range(0, 4097, 256)) + [4097]
    assert big.pool_chunk_end.tolist() == (
        list(range(256, 4097, 256)) + [4097, 4107])
    assert big.pool_seg_chunk_ptr.tolist() == [0, 17, 18]
