"""GPU tests of the cell-list radius graph (csrc/radius.hip) against a
brute-force float64 reference, at the edges of the cell list.

Reference: float64 distances from explicit blocked differences of the fp32
positions (no cdist, no tree), or a closed form where the point set is
planted (tests/radius_cases.py).

Band. The kernel decides ``fl32(dx^2 + dy^2 + dz^2) <= fl32(r^2)``: with
u = 2^-24, the differences are rounded once (u each, 2u on a square), the
sum carries at most 3 more roundings and r^2 one, so the decision can
differ from the exact one only for |d/r - 1| of a few u. tau = 2^-20 is
well above that:

* every pair with d <= r (1 - tau) must be present,
* no pair with d > r (1 + tau) may be present,
* pairs in between may go either way.

So that the band cannot hide a defect, a case may hold at most
max(2, 1e-4 M) pairs in it (M = edges of the reference); this is asserted
before the judgement. A uniform cloud expects about 6 tau M; planted cases
have none. docs/KERNELS.md ("Radius graph test band") records the observed
band populations.

Every case also checks the output contract: int64 [2, M] on pos's device,
row-sorted, rowptr consistent, no self loop, no duplicate, symmetric, and
``ext.radius_graph`` equal to ``radius_graph_gpu``'s edge_index.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

import radius_cases as RC
from distegnn_amd import ops
from distegnn_amd.ops import reference as R

DEV = "cuda:0"
TAU = 2.0 ** -20


def _run(pos, r):
    """Call both entry points; check the contract; return (ei, rowptr)."""
    ext = ops.hip_ext()
    ei, rowptr = ext.radius_graph_gpu(pos, r)
    n = pos.size(0)
    assert ei.dtype == torch.int64 and rowptr.dtype == torch.int64
    assert ei.dim() == 2 and ei.size(0) == 2 and ei.device == pos.device
    m = ei.size(1)
    assert rowptr.shape == (n + 1,) and int(rowptr[-1]) == m
    row, col = ei[0], ei[1]
    if m:
        assert int(ei.min()) >= 0 and int(ei.max()) < n
        assert bool((row[1:] >= row[:-1]).all()), "not row-sorted"
        assert not bool((row == col).any()), "self loop"
    assert torch.equal(rowptr[1:] - rowptr[:-1],
                       torch.bincount(row, minlength=n)[:n])
    key = row * max(n, 1) + col
    assert torch.unique(key).numel() == m, "duplicate edge"
    rkey = torch.sort(col * max(n, 1) + row).values
    assert torch.equal(torch.sort(key).values, rkey), "not symmetric"
    assert torch.equal(ext.radius_graph(pos, r), ei)
    return ei, rowptr


def _judge_brute(tag, pos, r, ei):
    """Band judgement against blocked float64 differences (n^2 work)."""
    n = pos.size(0)
    p = pos.double()
    got = torch.zeros(n, n, dtype=torch.bool, device=pos.device)
    got[ei[0], ei[1]] = True
    ref_m = band = missing = extra = 0
    for s in range(0, n, 1024):
        d = p[s:s + 1024, None, :] - p[None, :, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
                + d[..., 2] * d[..., 2]).sqrt()
        rows = torch.arange(s, min(s + 1024, n), device=pos.device)
        dist[rows - s, rows] = float("inf")          # no self pairs
        must = dist <= r * (1 - TAU)
        may = dist <= r * (1 + TAU)
        g = got[s:s + 1024]
        ref_m += int((dist <= r).sum())
        band += int((may & ~must).sum())
        missing += int((must & ~g).sum())
        extra += int((g & ~may).sum())
    cap = max(2, 1e-4 * ref_m)
    print(f"RATIO radius {tag} n={n} M_ref={ref_m} M_got={ei.size(1)} "
          f"band={band} cap={cap:.1f} missing={missing} extra={extra} "
          f"err/bound={band / cap:.4f}")
    assert band <= cap, (tag, band, cap)
    assert missing == 0 and extra == 0, (tag, missing, extra)
    return ref_m


def _judge_pairs(tag, ei, pairs, n):
    """Closed form: exactly the planted pairs, both directions."""
    pairs = torch.from_numpy(pairs).to(ei.device)
    want = torch.cat([pairs, pairs.flip(1)]).t()
    want = want[:, torch.argsort(want[0] * n + want[1])]
    wkey = want[0] * n + want[1]
    gkey = torch.sort(ei[0] * n + ei[1]).values
    missing = int((~torch.isin(wkey, gkey)).sum())
    extra = int((~torch.isin(gkey, wkey)).sum())
    print(f"RATIO radius {tag} n={n} M_ref={want.size(1)} "
          f"M_got={ei.size(1)} band=0 missing={missing} extra={extra} "
          f"err/bound=0.0000")
    assert missing == 0, f"{tag}: {missing} planted edges missing"
    assert extra == 0, f"{tag}: {extra} edges that were not planted"
    # one edge per row: row-sorted output has exactly one order
    assert torch.equal(ei, want)


def _cloud(n, seed, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g) * torch.tensor(scale) \
        + torch.tensor(shift)
    return pos.to(DEV)


# ------------------------------------------------------------ tiny inputs
def test_zero_one_two_points():
    for n in (0, 1):
        ei, rowptr = _run(torch.zeros(n, 3, device=DEV) + 0.3, 0.5)
        assert ei.shape == (2, 0) and rowptr.tolist() == [0] * (n + 1)
    two = torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.8]], device=DEV)
    ei, _ = _run(two, 0.75)                      # d = 0.5 <= r
    assert ei.tolist() == [[0, 1], [1, 0]]
    ei, rowptr = _run(two, 0.25)                 # d = 0.5 > r
    assert ei.shape == (2, 0) and rowptr.tolist() == [0, 0, 0]
    print("RATIO radius tiny err/bound=0.0000")


def test_copies_of_one_point():
    """300 coincident points: a 1 x 1 x 1 grid, the complete graph."""
    pos = torch.tensor([[0.3, -1.7, 2.9]], device=DEV).repeat(300, 1)
    ei, _ = _run(pos, 0.1)
    assert ei.size(1) == 300 * 299
    _judge_brute("copies", pos, 0.1, ei)


def test_radius_beyond_domain():
    """r = 10 x the domain diameter: one cell, the complete graph."""
    pos = _cloud(200, 3)
    r = 10 * 3 ** 0.5
    ei, _ = _run(pos, r)
    assert ei.size(1) == 200 * 199
    _judge_brute("r>domain", pos, r, ei)


@pytest.mark.parametrize("tag,scale,r", [
    ("planar", (1.0, 1.0, 0.0), 0.05),
    ("collinear", (1.0, 0.0, 0.0), 0.004),
])
def test_flat_domains(tag, scale, r):
    """nz = 1, and ny = nz = 1."""
    pos = _cloud(1000, 5, scale=scale, shift=(0.0, 0.25, -0.75))
    ei, _ = _run(pos, r)
    assert _judge_brute(tag, pos, r, ei) > 1000


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (1000.0, -1000.0, 512.0)],
                         ids=["origin", "translated"])
def test_lattice_on_cell_boundaries(shift):
    """12^3 lattice of spacing r/2 (1 - 2^-10): after the origin shift every
    point sits on (or a rounding away from) a cell boundary. Neighbours at
    lattice distance^2 <= 4 are inside by 2^-10 r, the next shell
    (sqrt(5)/2 r) is far outside: the band is empty."""
    r = 0.3
    s = 0.5 * r * (1 - 2.0 ** -10)
    i = torch.arange(12, dtype=torch.float64)
    g = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    pos = (g * s + torch.tensor(shift, dtype=torch.float64)).float().to(DEV)
    ei, _ = _run(pos, r)
    ref_m = _judge_brute(f"lattice{shift[0]:.0f}", pos, r, ei)
    # shells 1, 2, 3, 4 of the cubic lattice, clipped by the 12^3 box
    q = ((g[:, None, :] - g[None, :, :]) ** 2).sum(-1)
    assert ref_m == int(((q > 0) & (q <= 4)).sum())


# -------------------------------------------------------- planted cases
def test_elongated_domain_planted_pairs():
    """~4100 x 2 x 2 cells; 4000 pairs inside the radius by 2^-15 r, about
    2% of which the fp32 cell expression bins TWO cells apart (asserted on
    the CPU in test_radius_cases_cpu.py). A scan of ix-1 .. ix+1 drops
    those edges silently."""
    pos, r, pairs, (ox, inv_r) = RC.elongated_case()
    ca, cb = RC.pair_cells(pos, pairs, ox, inv_r)
    two = int((cb - ca == 2).sum())
    assert two > 0
    print(f"elongated: {two} of {len(pairs)} pairs two cells apart")
    p = torch.from_numpy(pos).to(DEV)
    ei, _ = _run(p, r)
    _judge_pairs("elongated", ei, pairs, len(pos))
    _judge_brute("elongated-brute", p, r, ei)


def test_coarsened_grid_planted_pairs():
    """r = 1/600 in the unit cube: above 2^26 cells, the grid coarsens."""
    pos, r, pairs = RC.coarsened_case()
    ei, _ = _run(torch.from_numpy(pos).to(DEV), r)
    _judge_pairs("coarsened", ei, pairs, len(pos))


def test_second_grid_stride_trip():
    """532,480 points: more than 2048 blocks x 256 threads."""
    pos, r, pairs = RC.second_trip_case()
    assert len(pos) > 2048 * 256
    ei, _ = _run(torch.from_numpy(pos).to(DEV), r)
    _judge_pairs("second-trip", ei, pairs, len(pos))


# ------------------------------------------------------------- r == 0
def test_zero_radius_returns_duplicates():
    """r = 0 pairs up exact duplicates, as the CPU reference does."""
    g = torch.Generator().manual_seed(9)
    pos = torch.rand(500, 3, generator=g)
    pos[17] = pos[400]
    pos[18] = pos[400]
    pos[250] = pos[3]
    pos[499] = pos[0]
    want = R.radius_graph(pos, 0.0)
    assert want.size(1) == 6 + 2 + 2
    got = ops.radius_graph(pos.to(DEV), 0.0)
    assert got.is_cuda and got.dtype == torch.int64
    key = lambda e: torch.sort(e[0] * 500 + e[1]).values
    assert torch.equal(key(got.cpu()), key(want))
    assert bool((got[0][1:] >= got[0][:-1]).all())
    ei, _ = _run(pos.to(DEV), 0.0)
    assert torch.equal(key(ei.cpu()), key(want))
    print("RATIO radius r=0 err/bound=0.0000")


@pytest.mark.parametrize("r", [-1.0, float("nan"), float("inf")])
def test_direct_call_rejects_bad_radius(r):
    with pytest.raises(RuntimeError, match="radius"):
        ops.hip_ext().radius_graph_gpu(torch.rand(10, 3, device=DEV), r)
