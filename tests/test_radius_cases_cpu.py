"""CPU checks of the planted radius-graph cases (tests/radius_cases.py).

The elongated case exists to catch a cell list that scans only the cells
ix-1 .. ix+1: it must therefore CONTAIN pairs that are closer than r and
that the kernel's fp32 cell expression, emulated here in numpy float32,
bins two cells apart. Without this the GPU test could pass for the wrong
reason."""

import numpy as np

import radius_cases as RC


def _brute_pairs(pos, r):
    """All i < j with float64 distance <= r, blocked."""
    p = pos.astype(np.float64)
    out = []
    for s in range(0, len(p), 512):
        d = p[s:s + 512, None, :] - p[None, :, :]
        hit = np.argwhere((d * d).sum(-1) <= r * r)
        hit[:, 0] += s
        out.append(hit[hit[:, 0] < hit[:, 1]])
    return np.concatenate(out)


def _same_pairs(got, pairs):
    want = np.sort(pairs, axis=1)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    return got.shape == want.shape and bool((got == want).all())


def test_elongated_case_has_pairs_two_cells_apart():
    pos, r, pairs, (ox, inv_r) = RC.elongated_case()
    assert pos.dtype == np.float32 and len(pairs) == RC.ELONGATED_PAIRS
    ca, cb = RC.pair_cells(pos, pairs, ox, inv_r)
    assert ca.min() >= 255 and cb.max() < 4100
    gap = cb - ca
    two = int((gap == 2).sum())
    print(f"elongated: {two} of {len(pairs)} pairs two cells apart, "
          f"{int((gap == 1).sum())} one cell apart")
    assert set(np.unique(gap)) <= {1, 2}
    assert two > 0
    # every pair is inside the radius by 2^-15 r, in exact arithmetic
    d = (pos[pairs[:, 1], 0].astype(np.float64)
         - pos[pairs[:, 0], 0].astype(np.float64))
    assert (d > 0).all() and (d <= r * (1 - 2.0 ** -15)).all()
    # ... and the planted pairs are ALL the pairs
    assert _same_pairs(_brute_pairs(pos, r * (1 + 2.0 ** -10)), pairs)


def test_scan_range_covers_every_planted_partner():
    """The rule the kernel scans by, emulated: cell(x - rs) .. cell(x + rs)
    holds the partner's cell for every planted pair, from either end; the
    rule "own cell - 1 .. own cell + 1" does not."""
    pos, r, pairs, (ox, inv_r) = RC.elongated_case()
    ca, cb = RC.pair_cells(pos, pairs, ox, inv_r)
    xa, xb = pos[pairs[:, 0], 0], pos[pairs[:, 1], 0]
    lo_a, hi_a = RC.scan_range_f32(xa, r, ox, inv_r)
    lo_b, hi_b = RC.scan_range_f32(xb, r, ox, inv_r)
    assert ((lo_a <= cb) & (cb <= hi_a)).all()
    assert ((lo_b <= ca) & (ca <= hi_b)).all()
    assert (hi_a - lo_a <= 3).all() and (hi_b - lo_b <= 3).all()
    assert not ((ca - 1 <= cb) & (cb <= ca + 1)).all()


def test_coarsened_case_is_isolated_pairs():
    pos, r, pairs = RC.coarsened_case()
    assert pos.min() == 0.0 and pos.max() == 1.0
    assert np.floor(1.0 / r) + 1 >= 600 and 600 ** 3 > 2 ** 26
    assert 301 ** 3 <= 2 ** 26       # one coarsening step is enough
    ca, cb = RC.pair_cells(pos, pairs, 0.0, np.float32(1.0 / (2 * r)))
    assert ((cb - ca) >= 1).all()    # each pair straddles a coarse boundary
    assert _same_pairs(_brute_pairs(pos, r * (1 + 2.0 ** -10)), pairs)


def test_second_trip_case_shape():
    pos, r, pairs = RC.second_trip_case()
    assert len(pos) == 532480 > 2048 * 256
    d = pos[pairs[:, 1]].astype(np.float64) - pos[pairs[:, 0]]
    assert (np.abs(d[:, 0]) == 0.875).all() and (d[:, 1:] == 0).all()
