"""Exact GPU tests of the CSR reduction family (csrc/segment_reduce.hip)
and the grid-stride elementwise kernels next to it (csrc/elementwise.hip).

The data are small integers (values in [-2, 2], every |sum| < 2^24), so an
fp32 accumulation is exact in ANY order and sum mode must be BIT-EQUAL to
the int64 reference cast to the output dtype; rounding the exact integer
sum to bf16 is the only rounding a bf16 output may carry. Mean mode divides
(or multiplies by a rounded reciprocal) once: 1/len rounded, the product
rounded, both below u23/2 -> 3*u23*|want| covers it, plus u8*|want| for the
rounding of a bf16 output (u23 = 2^-23, u8 = 2^-8).

Sizes are chosen so that every kernel's dispatch branch, every segment
length mod 8 of ``seg_reduce_wave4`` and the second trip of every capped
grid-stride loop run (``num_blocks`` caps grids at 2048 blocks = 8192
waves, the coordinate update at 8192 blocks).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import build_chunk_tables

U23 = 2.0 ** -23
U8 = 2.0 ** -8
DEV = "cuda:0"
GRID_CAP = 2048                 # num_blocks() in csrc/common.h
WAVE_CAP = GRID_CAP * 4         # 256-thread blocks = 4 waves
DTYPES = [torch.float32, torch.bfloat16]


def _ints(shape, seed):
    """int64 values in [-2, 2], drawn on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g, device=DEV)


def _ptr(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.long),
                      torch.cumsum(torch.tensor(lengths), 0)])


def _segment_sums(data_i64, ptr):
    """int64 segment sums on the device (cumsum difference: exact)."""
    cs = torch.cat([torch.zeros(1, *data_i64.shape[1:], dtype=torch.long,
                                device=data_i64.device),
                    torch.cumsum(data_i64, 0)])
    return cs.index_select(0, ptr[1:]) - cs.index_select(0, ptr[:-1])


def _judge(tag, got, sums, lens, mean, dtype):
    """sum: bit-equal. mean: err <= 3*u23*|want| (+ u8*|want| for bf16);
    an empty segment is exactly 0 either way."""
    assert got.dtype == dtype and got.shape == sums.shape, tag
    assert int(sums.abs().max()) < 2 ** 24, tag
    if not mean:
        want = sums.double().to(dtype)
        assert torch.equal(got, want), \
            f"{tag}: {int((got != want).sum())} elements differ"
        print(f"RATIO seg {tag} err/bound=0.0000 (bit-equal)")
        return
    div = lens.clamp(min=1).double().view(-1, *([1] * (sums.dim() - 1)))
    want = sums.double() / div
    bound = (3 * U23 + (U8 if dtype == torch.bfloat16 else 0)) * want.abs()
    err = (got.double() - want).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), tag
    r = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0
    print(f"RATIO seg {tag} err/bound={r:.4f}")
    assert r <= 1.0, (tag, r)


def _csr_case(tag, lengths, f, dtype, mean, use_perm, seed):
    ptr = _ptr(lengths).to(DEV)
    m = int(ptr[-1])
    data = _ints((m, f), seed).to(DEV)          # CSR order
    lens = ptr[1:] - ptr[:-1]
    sums = _segment_sums(data, ptr)
    ext = ops.hip_ext()
    if use_perm:
        # store the rows permuted: stored[perm[k]] = data[k]
        g = torch.Generator().manual_seed(seed + 1)
        perm = torch.randperm(m, generator=g).to(DEV)
        stored = torch.empty_like(data)
        stored[perm] = data
        assert torch.equal(stored.index_select(0, perm), data)
        got = ext.segment_reduce_csr_perm(stored.to(dtype), ptr, perm, mean)
    else:
        got = ext.segment_reduce_csr(data.to(dtype), ptr, mean)
    _judge(tag, got, sums, lens, mean, dtype)


# ---------------------------------------------------------------- group 1
# every length 0..40 (every length mod 8 several times, below and above the
# 8-row unroll), the 64/128 neighbourhoods, one long segment; empty
# segments at the very start and the very end
LENGTHS = [0] + list(range(0, 41)) + [63, 64, 65, 127, 128, 129, 1000] + [0]
# f <= 4 | 5..15 | >= 16 and f % 4 == 0 | >= 16 otherwise select different
# kernels; 68, 128, 320 give wave4 more than one feature-quad round
WIDTHS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 18, 20, 63, 64, 65, 68, 128, 320]


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", WIDTHS)
def test_segment_reduce_csr_exact(f, dtype, mean):
    assert LENGTHS[0] == 0 and LENGTHS[-1] == 0
    assert {n % 8 for n in LENGTHS} == set(range(8))
    for use_perm in (False, True):
        _csr_case(f"csr f={f} {dtype} mean={mean} perm={use_perm}", LENGTHS,
                  f, dtype, mean, use_perm, seed=f)


# ---------------------------------------------------------------- group 2
@pytest.mark.parametrize("use_perm", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", [3, 15, 16, 18])
def test_segment_reduce_csr_second_trip(f, dtype, use_perm):
    """2*8192 + 77 segments: every wave takes a second segment, 77 a
    third."""
    n = 2 * WAVE_CAP + 77
    lengths = [i % 6 for i in range(n)]
    for mean in (False, True):
        _csr_case(f"csr-trip f={f} {dtype} mean={mean} perm={use_perm}",
                  lengths, f, dtype, mean, use_perm, seed=50 + f)


@pytest.mark.parametrize("dtype,f,n_idx,word", [
    (torch.bfloat16, 64, 140_000, 16),     # 8 x 16-byte words per row
    (torch.bfloat16, 4, 1_100_000, 8),     # one 8-byte word per row
    (torch.float32, 3, 360_000, 4),        # 3 x 4-byte words per row
])
def test_gather_rows_fast_second_trip(dtype, f, n_idx, word):
    row_bytes = f * (2 if dtype == torch.bfloat16 else 4)
    assert row_bytes % word == 0 and (word == 16 or row_bytes % (2 * word))
    assert n_idx * (row_bytes // word) > 2 * GRID_CAP * 256
    g = torch.Generator().manual_seed(f)
    x = torch.randn(1000, f, generator=g).to(dtype).to(DEV)
    idx = torch.randint(0, 1000, (n_idx,), generator=g).to(DEV)
    got = ops.hip_ext().gather_rows_fast(x, idx)
    assert torch.equal(got, x.index_select(0, idx))


@pytest.mark.parametrize("dtype", DTYPES)
def test_mid_reduce_expand_second_trip(dtype):
    n, c, f = 17000, 5, 64
    assert n * f > 2 * GRID_CAP * 256
    ext = ops.hip_ext()
    xi = _ints((n, c, f), 1).to(DEV)
    gi = _ints((n, f), 2).to(DEV)
    x, g = xi.to(dtype), gi.to(dtype)
    s = xi.sum(1)
    for scale in (1.0, -1.0):
        want = (scale * s.double()).to(dtype)
        assert torch.equal(ext.mid_reduce(x, scale), want)
        want = (scale * gi.double()).to(dtype).unsqueeze(1).expand(n, c, f)
        assert torch.equal(ext.mid_expand(g, c, scale), want)
    # scale 1/5: the fp32 value of 1/5 and one product, then the output
    # rounding -> the mean bound
    rel = 3 * U23 + (U8 if dtype == torch.bfloat16 else 0)
    for tag, got, want in (
            ("mid_reduce", ext.mid_reduce(x, 1.0 / c), s.double() / c),
            ("mid_expand", ext.mid_expand(g, c, 1.0 / c),
             (gi.double() / c).unsqueeze(1).expand(n, c, f))):
        assert got.dtype == dtype and got.shape == want.shape
        err, bound = (got.double() - want).abs(), rel * want.abs()
        assert bool((err[bound == 0] == 0).all())
        r = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"RATIO seg {tag} 1/5 {dtype} err/bound={r:.4f}")
        assert r <= 1.0, (tag, r)


def test_coord_update_second_trip():
    """More than 2*8192*256 nodes: both coordinate-update kernels take a
    third trip of their grid-stride loops. Integer data: exact."""
    n = 2 * 8192 * 256 + 1000
    ext = ops.hip_ext()
    coord, agg, tv, vel = (_ints((n, 3), 10 + i).to(DEV) for i in range(4))
    phiv = _ints((n, 1), 20).to(DEV)
    got = ext.coord_update_forward(coord.float(), agg.float(), tv.float(),
                                   phiv.float(), vel.float())
    assert torch.equal(got, (coord + agg + tv + phiv * vel).float())
    g = _ints((n, 3), 21).to(DEV)
    got = ext.coord_update_backward(g.float(), vel.float())
    assert got.shape == (n, 1)
    assert torch.equal(got, (g * vel).sum(1, keepdim=True).float())


# ---------------------------------------------------------------- group 3
def _chunked_case(tag, counts, f, dtype, mean, seed, chunk=256):
    ptr = _ptr(counts)
    cb, ce, scp = (t.to(DEV) for t in build_chunk_tables(ptr, chunk))
    ptr = ptr.to(DEV)
    m = int(ptr[-1])
    data = _ints((m, f), seed).to(DEV)
    got = ops.hip_ext().segment_reduce_chunked(data.to(dtype), ptr, cb, ce,
                                               scp, mean)
    _judge(tag, got, _segment_sums(data, ptr), ptr[1:] - ptr[:-1], mean,
           dtype)
    return cb.numel()


# f <= 4 | 5..16 | > 16 and f % 4 == 0 | > 16 otherwise select different
# stage-1 kernels; 1024 is the widest the virtual block's pool() produces
# (C = 8, H = 128); 1028 gives seg_reduce_chunk4 two feature tiles
CHUNK_WIDTHS = [3, 15, 16, 17, 24, 64, 1024, 1028]
# empty segments first and last, one row, and 255 / 256 / 257 rows around
# the chunk length, one 20-chunk segment
CHUNK_COUNTS = [0, 1, 255, 256, 257, 5000, 0]


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", CHUNK_WIDTHS)
def test_segment_reduce_chunked_exact(f, dtype, mean):
    _chunked_case(f"chunked f={f} {dtype} mean={mean}", CHUNK_COUNTS, f,
                  dtype, mean, seed=70 + f)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f,rows", [(3, 300_000), (17, 300_000),
                                    (64, 300_000), (3, 1_100_000)])
def test_segment_reduce_chunked_second_trip_chunks(f, rows, dtype):
    """Two segments of ``rows`` rows. 300,000 rows make 2344 chunks: a
    second trip of the one-block-per-chunk stage-1 kernels (f = 17, 64).
    The small-f kernel runs one WAVE per chunk, so f = 3 takes its second
    trip only above 8192 chunks: 1,100,000 rows make 8594."""
    for mean in (False, True):
        nchunks = _chunked_case(
            f"chunked-trip f={f} rows={rows} {dtype} mean={mean}",
            [rows, rows], f, dtype, mean, seed=80 + f)
    assert nchunks > (WAVE_CAP if rows > 300_000 else GRID_CAP)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_reduce_chunked_second_trip_combine(dtype):
    """2100 one-chunk segments at f = 3: more (segment, feature-tile)
    pairs than the combine's 2048 blocks."""
    counts = [1 + i % 7 for i in range(2100)]
    for mean in (False, True):
        _chunked_case(f"chunked-combine {dtype} mean={mean}", counts, 3,
                      dtype, mean, seed=90)


def test_segment_reduce_chunked_bf16_sum_deterministic():
    """Run-to-run bit equality in bf16 sum mode on random (non-integer)
    data, where the order of the fp32 additions shows."""
    n, f = 120_000, 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, f, generator=g).bfloat16().to(DEV)
    ptr = torch.tensor([0, 50_000, n])
    cb, ce, scp = (t.to(DEV) for t in build_chunk_tables(ptr))
    args = (x, ptr.to(DEV), cb, ce, scp, False)
    a = ops.hip_ext().segment_reduce_chunked(*args)
    b = ops.hip_ext().segment_reduce_chunked(*args)
    assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    want = torch.stack([x[:50_000].double().sum(0), x[50_000:].double().sum(0)])
    # 256-row chunk partials, then ~200-470 partials per segment, all fp32:
    # (rows)*u23*sum|x| bounds any order; u8*|want| the bf16 output
    mag = torch.stack([x[:50_000].double().abs().sum(0),
                       x[50_000:].double().abs().sum(0)])
    rows = torch.tensor([[50_000.0], [70_000.0]], device=DEV,
                        dtype=torch.float64)
    assert bool(((a.double() - want).abs()
                 <= U8 * want.abs() + rows * U23 * mag).all())
