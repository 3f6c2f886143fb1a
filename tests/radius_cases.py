"""Planted point sets for the radius-graph tests (no GPU needed here).

The cell list of csrc/radius.hip bins a point along an axis at

    cell(x) = trunc( fl32( fl32(x - o) * fl32(1 / edge) ) )

with o the smallest coordinate of the cloud and edge the cell edge (r, or
2r after one coarsening step). ``cell_index_f32`` is that expression in
numpy float32. Its rounding error grows with the index, so two points
closer than r can be binned two cells apart; ``plant_pairs`` builds exactly
such pairs: A is the LAST float32 of cell k-1, B the largest float32 with
B - A <= r (1 - 2^-15). B - A is exact (Sterbenz), so the pair is an edge
by 2^-15 r, far outside the judgement band of 2^-20 r.

tests/test_radius_cases_cpu.py asserts that the elongated case really
holds pairs whose cells differ by two, so the GPU test that runs it
(tests/test_radius_graph_gpu.py) cannot pass vacuously.
"""

import numpy as np

F32 = np.float32
INSIDE = 1.0 - 2.0 ** -15


def cell_index_f32(x, o, inv_edge):
    """The kernel's cell coordinate (before its clamp to the grid)."""
    x = np.asarray(x, dtype=F32)
    t = (x - F32(o)).astype(F32) * F32(inv_edge)
    return np.trunc(t.astype(F32)).astype(np.int64)


def scan_range_f32(x, r, o, inv_edge):
    """The kernel's scanned cells (before the clamp) around x along one
    axis: cell(x - rs) .. cell(x + rs), rs = fp32(r (1 + 2^-20))."""
    x = np.asarray(x, dtype=F32)
    rs = F32(r * (1.0 + 2.0 ** -20))
    return (cell_index_f32((x - rs).astype(F32), o, inv_edge),
            cell_index_f32((x + rs).astype(F32), o, inv_edge))


def _last_float_of_cell(k, o, edge, inv_edge):
    """Largest float32 x with cell(x) == k - 1 (k >= 1, vectorised)."""
    # cell() is monotone: bisect between a point of cell k-1 and one of
    # cell k until no float32 lies strictly between them
    mid = np.float64(o) + k.astype(np.float64) * edge
    lo, hi = (mid - 0.5 * edge).astype(F32), (mid + 0.5 * edge).astype(F32)
    assert (cell_index_f32(lo, o, inv_edge) == k - 1).all()
    assert (cell_index_f32(hi, o, inv_edge) == k).all()
    for _ in range(200):
        x = (0.5 * (lo.astype(np.float64) + hi)).astype(F32)
        if ((x == lo) | (x == hi)).all():
            break
        below = cell_index_f32(x, o, inv_edge) < k
        inner = (x != lo) & (x != hi)
        lo = np.where(inner & below, x, lo).astype(F32)
        hi = np.where(inner & ~below, x, hi).astype(F32)
    assert (np.nextafter(lo, F32(np.inf)) == hi).all()
    assert (cell_index_f32(lo, o, inv_edge) == k - 1).all()
    assert (cell_index_f32(hi, o, inv_edge) == k).all()
    return lo


def plant_pairs(k, o, r, edge):
    """x coordinates (xa, xb) of the pairs at cell boundaries ``k``."""
    inv_edge = F32(1.0 / edge)
    xa = _last_float_of_cell(k, o, edge, inv_edge)
    xb = (xa.astype(np.float64) + r * INSIDE).astype(F32)
    over = xb.astype(np.float64) - xa.astype(np.float64) > r * INSIDE
    xb = np.where(over, np.nextafter(xb, F32(-np.inf)), xb).astype(F32)
    d = xb.astype(np.float64) - xa.astype(np.float64)
    assert (d <= r * INSIDE).all() and (d > r * (1.0 - 2.0 ** -9)).all()
    return xa, xb


def _assemble(xa, xb, y, z, corners, seed):
    """Interleave the pairs, append the two corner points, shuffle.
    Returns (pos float32 [n, 3], pairs int64 [P, 2] into pos)."""
    p = xa.size
    pos = np.empty((2 * p + 2, 3), dtype=F32)
    pos[0:2 * p:2, 0], pos[1:2 * p:2, 0] = xa, xb
    pos[0:2 * p:2, 1] = pos[1:2 * p:2, 1] = y
    pos[0:2 * p:2, 2] = pos[1:2 * p:2, 2] = z
    pos[2 * p], pos[2 * p + 1] = corners
    order = np.random.default_rng(seed).permutation(2 * p + 2)
    where = np.empty_like(order)
    where[order] = np.arange(order.size)
    pairs = np.stack([where[0:2 * p:2], where[1:2 * p:2]], axis=1)
    return pos[order], pairs.astype(np.int64)


ELONGATED_R = 0.0123
ELONGATED_ORIGIN = (-3.7, 0.61, -1.13)     # no short binary fractions
ELONGATED_PAIRS = 4000


def elongated_case(seed=0):
    """About 4100 cells along x, 2 x 2 across; 4000 pairs, each at its own
    cell boundary k in [256, 4096), spaced so that every point has exactly
    one neighbour: four (y, z) lanes 1.5 r apart, and within a lane the
    boundaries are at least three cells apart. The corner points fix the
    bounding box (origin and cell counts) and are isolated.

    Returns (pos, r, pairs, (ox, inv_r))."""
    r = ELONGATED_R
    ox, oy, oz = (F32(v) for v in ELONGATED_ORIGIN)
    rng = np.random.default_rng(seed)
    per_lane = ELONGATED_PAIRS // 4
    ks, ys, zs = [], [], []
    for lane in range(4):
        slots = rng.choice(1280, size=per_lane, replace=False)
        ks.append(256 + 3 * slots)
        ys.append(np.full(per_lane, F32(oy + F32(1.5 * r * (lane & 1)))))
        zs.append(np.full(per_lane, F32(oz + F32(1.5 * r * (lane >> 1)))))
    k = np.concatenate(ks).astype(np.int64)
    y, z = np.concatenate(ys), np.concatenate(zs)
    xa, xb = plant_pairs(k, ox, r, r)
    far = F32(np.float64(ox) + 4100 * r)
    corners = np.array([[ox, oy, oz], [far, y.max(), z.max()]], dtype=F32)
    pos, pairs = _assemble(xa, xb, y, z, corners, seed + 1)
    assert pos[:, 0].min() == ox and pos[:, 1].min() == oy
    return pos, r, pairs, (ox, F32(1.0 / r))


def pair_cells(pos, pairs, ox, inv_edge):
    """Emulated x cell of both points of every pair."""
    return (cell_index_f32(pos[pairs[:, 0], 0], ox, inv_edge),
            cell_index_f32(pos[pairs[:, 1], 0], ox, inv_edge))


COARSE_R = 1.0 / 600.0
COARSE_PAIRS = 1000


def coarsened_case(seed=0):
    """Unit cube, r = 1/600: 600^3 or 601^3 cells of edge r, above the
    2^26-cell cap, so the grid is rebuilt once with edge 2r. 1000 pairs
    on distinct sites of a 10^3 lattice (pitch 0.09), each straddling a
    boundary of the COARSENED grid along x. Returns (pos, r, pairs)."""
    r = COARSE_R
    rng = np.random.default_rng(seed)
    site = rng.choice(1000, size=COARSE_PAIRS, replace=False)
    ix, iy, iz = site // 100, (site // 10) % 10, site % 10
    k = np.floor((0.05 + 0.09 * ix) / (2 * r)).astype(np.int64) + 1
    k += rng.integers(0, 10, size=k.size)
    xa, xb = plant_pairs(k, F32(0.0), r, 2 * r)
    y = (0.05 + 0.09 * iy).astype(F32)
    z = (0.05 + 0.09 * iz).astype(F32)
    corners = np.array([[0, 0, 0], [1, 1, 1]], dtype=F32)
    pos, pairs = _assemble(xa, xb, y, z, corners, seed + 1)
    return pos, r, pairs


TRIP_R = 1.0
TRIP_SHAPE = (65, 64, 64)       # pair centres; 2 * 65*64*64 = 532,480 points


def second_trip_case(seed=0):
    """Isolated pairs on a lattice of pitch 4r: more points than one pass
    of the capped grid (2048 blocks x 256 threads = 524,288). All values
    are small binary fractions, so every distance is exact: 0.875 r inside
    a pair, at least 3.125 r between pairs. Returns (pos, r, pairs)."""
    a, b, c = TRIP_SHAPE
    g = np.stack(np.meshgrid(np.arange(a), np.arange(b), np.arange(c),
                             indexing="ij"), axis=-1).reshape(-1, 3)
    centre = (4.0 * g).astype(F32)
    p = centre.shape[0]
    pos = np.empty((2 * p, 3), dtype=F32)
    pos[0::2] = centre
    pos[1::2] = centre
    pos[0::2, 0] -= F32(0.4375)
    pos[1::2, 0] += F32(0.4375)
    order = np.random.default_rng(seed).permutation(2 * p)
    where = np.empty_like(order)
    where[order] = np.arange(order.size)
    pairs = np.stack([where[0::2], where[1::2]], axis=1).astype(np.int64)
    return pos[order], TRIP_R, pairs
