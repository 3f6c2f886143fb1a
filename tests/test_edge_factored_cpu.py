"""``edge_reference.edge_backward_factored`` (dh and dW1 from per-node sums
of dz1) against ``edge_reference.edge_backward`` (per-edge dein and ein), in
float64 on the CPU. The two are the same algebra, so gh, gw1 and gc must
agree to rounding: 1e-12 of the largest entry."""

import pytest
import torch

from distegnn_amd.ops import edge_reference as ER

EPS = 1e-8
TOL = 1e-12


def _edges(nodes, m, g):
    k = nodes.numel()
    a = torch.randint(0, k, (m,), generator=g)
    b = (a + torch.randint(1, k, (m,), generator=g)) % k
    return nodes[a], nodes[b]


def graph_random():
    g = torch.Generator().manual_seed(1)
    row, col = _edges(torch.arange(40), 500, g)
    return 40, row, col


def graph_iso_hub():
    """Nodes 0, 20 and 59 touch no edge; node 7 is the row of 200 edges."""
    g = torch.Generator().manual_seed(2)
    nodes = torch.tensor([i for i in range(60) if i not in (0, 20, 59)])
    others = nodes[nodes != 7]
    hub_col = others[torch.randint(0, others.numel(), (200,), generator=g)]
    row, col = _edges(others, 150, g)
    return 60, torch.cat([torch.full((200,), 7), row]), torch.cat(
        [hub_col, col])


def graph_never_col():
    """Node 5 is a row of several edges but nobody's column: S_col[5] = 0
    while S_row[5] is not."""
    g = torch.Generator().manual_seed(3)
    others = torch.tensor([i for i in range(30) if i != 5])
    row, col = _edges(others, 200, g)
    extra_col = others[torch.randint(0, others.numel(), (9,), generator=g)]
    row = torch.cat([row, torch.full((9,), 5)])
    col = torch.cat([col, extra_col])
    assert not bool((col == 5).any()) and bool((row == 5).any())
    return 30, row, col


GRAPHS = {"random": graph_random, "iso_hub": graph_iso_hub,
          "never_col": graph_never_col}


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [8, 32])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_factored_matches_per_edge(gname, hdim, normalize):
    n, row, col = GRAPHS[gname]()
    # row-sorted, as the collated batches are (the algebra does not need it)
    order = torch.argsort(row, stable=True)
    row, col = row[order], col[order]
    m = row.numel()
    g = torch.Generator().manual_seed(10 + hdim)
    dd = torch.float64
    k_in = 2 * hdim + 3
    h = torch.randn(n, hdim, generator=g, dtype=dd) * 0.7
    pos = torch.randn(n, 3, generator=g, dtype=dd)
    eattr = torch.randn(m, 2, generator=g, dtype=dd)
    w1 = torch.randn(hdim, k_in, generator=g, dtype=dd) * 1.5 / k_in ** 0.5
    w2 = torch.randn(hdim, hdim, generator=g, dtype=dd) * 1.5 / hdim ** 0.5
    w3 = torch.randn(hdim, hdim, generator=g, dtype=dd) * 1.5 / hdim ** 0.5
    b1, b2, b3 = (torch.randn(hdim, generator=g, dtype=dd) * 0.2
                  for _ in range(3))
    w3v = torch.randn(hdim, generator=g, dtype=dd) * 0.3
    dmsg_n = torch.randn(n, hdim, generator=g, dtype=dd) * 0.5
    dtrans_n = torch.randn(n, 3, generator=g, dtype=dd)

    fwd = ER.edge_forward(h, pos, eattr, row, col, w1, b1, w2, b2, w3, b3,
                          w3v, normalize, EPS)
    ref = ER.edge_backward(fwd, row, col, dmsg_n, dtrans_n, w1, w2, w3, w3v,
                           n)
    fac = ER.edge_backward_factored(fwd, h, eattr, row, col, dmsg_n,
                                    dtrans_n, w1, w2, w3, w3v, n)
    for name in ("gh", "gw1", "gc"):
        r, f = ref[name], fac[name]
        assert f.shape == r.shape, name
        scale = float(r.abs().max())
        assert scale > 0, name
        err = float((f - r).abs().max()) / scale
        print(f"factored {gname} H={hdim} norm={int(normalize)} {name} "
              f"rel={err:.2e}")
        assert err <= TOL, (name, err)
    # the pieces: dr2 is the one dein column kept, the tail the per-edge
    # columns of gw1
    assert torch.allclose(fac["dr2"], ref["dr2"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(fac["gw1_tail"], ref["gw1"][:, 2 * hdim:],
                          rtol=1e-12, atol=1e-13)
    if gname == "never_col":
        assert bool((fac["s_col"][5] == 0).all())
        assert bool((fac["s_row"][5] != 0).any())
    if gname == "iso_hub":
        for i in (0, 20, 59):
            assert bool((fac["gh"][i] == 0).all())
