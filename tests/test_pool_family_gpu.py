"""GPU tests of the chunked graph-pool family and of ops.virtual_aggregate
(csrc/segment_reduce.hip: pool_chunks, pool_combine, the channel-mean rider
and virtual_aggregate_bwd_kernel).

Integer data in [-2, 2] keep every fp32 sum exact in any order (|sum| <
2^24), so sum mode must be BIT-EQUAL to an int64 cumsum reference. Mean mode
divides once: 3*u23*|want| covers the rounded quotient, plus u8*|want| for
the rounding of a bf16 output (the bound test_segment_family_gpu.py
derives; u23 = 2^-23, u8 = 2^-8). The channel means must be bit-equal to
ext.mid_reduce and the fused backward torch.equal to the composition of
mid_expand, the pool backward's divide-and-gather and autograd's add, all
computed on the same device.
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
# empty segments first, in the middle and last; one row; 255 / 256 / 257
# rows around the chunk length; two and twenty chunks
LENGTHS = [0, 1, 255, 256, 257, 513, 0, 5000, 0]


def _ints(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g, device=DEV)


def _tables(lengths):
    ptr = torch.cat([torch.zeros(1, dtype=torch.long),
                     torch.cumsum(torch.tensor(lengths), 0)])
    cb, ce, scp = (t.to(DEV) for t in build_chunk_tables(ptr))
    return ptr.to(DEV), cb, ce, scp


def _segment_sums(data_i64, ptr):
    cs = torch.cat([torch.zeros(1, *data_i64.shape[1:], dtype=torch.long,
                                device=data_i64.device),
                    torch.cumsum(data_i64, 0)])
    return cs.index_select(0, ptr[1:]) - cs.index_select(0, ptr[:-1])


def _judge(tag, got, sums, ptr, mean, dtype):
    assert got.dtype == dtype and got.shape == sums.shape, tag
    assert int(sums.abs().max()) < 2 ** 24, tag
    if not mean:
        want = sums.double().to(dtype)
        assert torch.equal(got, want), \
            f"{tag}: {int((got != want).sum())} elements differ"
        return
    lens = (ptr[1:] - ptr[:-1]).clamp(min=1).double()
    want = sums.double() / lens.view(-1, *([1] * (sums.dim() - 1)))
    bound = (3 * U23 + (U8 if dtype == torch.bfloat16 else 0)) * want.abs()
    err = (got.double() - want).abs()
    r = float((err / bound.clamp(min=1e-300))[bound > 0].max())
    print(f"RATIO pool {tag} err/bound={r:.4f}")
    assert bool((err[bound == 0] == 0).all()), tag
    assert r <= 1.0, (tag, r)


def _operands(kind, n, seed):
    """(int64 logical data, tensor handed to the kernel) per operand."""
    if kind == "set":
        a = _ints((n, 320), seed)
        b = _ints((n * 5, 8), seed + 1)          # 5 of 8 columns are pooled
        c = _ints((n, 15), seed + 2)
        return [(a, a.bfloat16()),
                (b.view(n, 5, 8)[:, :, :5],
                 b.float().view(n, 5, 8)[:, :, :5]),
                (c, c.float())]
    a = _ints((n, kind), seed)
    return [(a, a.float()), (a, a.bfloat16())]


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("kind", ["set", 3, 25, 64])
def test_group_exact(kind, mean):
    ptr, cb, ce, scp = _tables(LENGTHS)
    ops_ = _operands(kind, int(ptr[-1]), 11)
    assert kind != "set" or not ops_[1][1].is_contiguous()
    ext = ops.hip_ext()
    tensors = [t for _, t in ops_]
    got = ext.segment_reduce_chunked_group(tensors, ptr, cb, ce, scp,
                                           [mean] * len(tensors))
    for i, ((ref, t), g) in enumerate(zip(ops_, got)):
        _judge(f"group {kind}[{i}] mean={mean}", g, _segment_sums(ref, ptr),
               ptr, mean, t.dtype)
        # each result is what the single entry gives for that operand
        single = ext.segment_reduce_chunked(t, ptr, cb, ce, scp, mean)
        assert torch.equal(g, single)


def test_group_second_trip():
    """300,000 rows in each of two segments make 2344 chunks, more than
    the 2048-block grid cap, so stage 1 takes a second trip of its
    grid-stride loop (f = 64, fp32 and bf16 in one launch). Then 2100
    segments at f = 3 with five operands: more (operand, segment, tile)
    items than combine blocks, and a second launch pair past four
    operands."""
    rows = 300_000
    ptr, cb, ce, scp = _tables([rows, rows])
    assert cb.numel() > GRID_CAP
    a = _ints((2 * rows, 64), 5)
    ext = ops.hip_ext()
    for mean in (False, True):
        got = ext.segment_reduce_chunked_group(
            [a.float(), a.bfloat16()], ptr, cb, ce, scp, [mean, mean])
        sums = _segment_sums(a, ptr)
        _judge(f"trip f32 mean={mean}", got[0], sums, ptr, mean,
               torch.float32)
        _judge(f"trip bf16 mean={mean}", got[1], sums, ptr, mean,
               torch.bfloat16)
    # more (segment, feature-tile) pairs than combine blocks
    lengths = [1 + i % 7 for i in range(2100)]
    ptr, cb, ce, scp = _tables(lengths)
    b = _ints((int(ptr[-1]), 3), 6)
    got = ext.segment_reduce_chunked_group(
        [b.float()] * 5, ptr, cb, ce, scp, [False] * 5)
    for g in got:
        _judge("trip combine", g, _segment_sums(b, ptr), ptr, False,
               torch.float32)


def _vagg_inputs(n, c, h, seed, ints=True):
    if ints:
        v = _ints((n, c, h), seed).bfloat16()
        tv = _ints((n, c, 3), seed + 1).float()
        tx = _ints((n, c, 3), seed + 2).float()
    else:
        g = torch.Generator(device=DEV).manual_seed(seed)
        v = torch.randn(n, c, h, generator=g, device=DEV).bfloat16()
        tv = torch.randn(n, c, 3, generator=g, device=DEV)
        tx = torch.randn(n, c, 3, generator=g, device=DEV)
    return v, tv, tx


# H = 256 and 512 put 32 and 64 feature-lanes in a row-lane; 512 is the
# widest the rider takes (a row-lane must fit in one wave)
@pytest.mark.parametrize("c,h", [(c, h) for h in (32, 64, 128)
                                 for c in (1, 3, 5, 8)]
                         + [(4, 256), (1, 512), (2, 512)])
def test_virtual_aggregate_forward(c, h):
    ptr, cb, ce, scp = _tables(LENGTHS)
    n = int(ptr[-1])
    v, tv, tx = _vagg_inputs(n, c, h, 20 + c)
    ext = ops.hip_ext()
    agg_v, trans_v, agg_vf, agg_vc = ext.virtual_aggregate_forward(
        v, tv, tx, ptr, cb, ce, scp)
    assert torch.equal(agg_v, ext.mid_reduce(v, 1.0 / c))
    assert torch.equal(trans_v, ext.mid_reduce(tv, 1.0 / c))
    _judge(f"vagg vf c={c} h={h}", agg_vf, _segment_sums(v.long(), ptr), ptr,
           True, torch.bfloat16)
    _judge(f"vagg vc c={c} h={h}", agg_vc, _segment_sums(tx.long(), ptr), ptr,
           True, torch.float32)


def test_virtual_aggregate_rows_outside_segments():
    """ptr = [3, 300, 700] over 750 rows: rows 0..2 and 700..749 are in no
    graph. Their channel means are still written; the pools ignore them."""
    n, c, h = 750, 5, 64
    ptr = torch.tensor([3, 300, 700])
    cb, ce, scp = (t.to(DEV) for t in build_chunk_tables(ptr))
    ptr = ptr.to(DEV)
    v, tv, tx = _vagg_inputs(n, c, h, 31)
    ext = ops.hip_ext()
    agg_v, trans_v, agg_vf, agg_vc = ext.virtual_aggregate_forward(
        v, tv, tx, ptr, cb, ce, scp)
    assert torch.equal(agg_v, ext.mid_reduce(v, 1.0 / c))
    assert torch.equal(trans_v, ext.mid_reduce(tv, 1.0 / c))
    _judge("vagg outside vf", agg_vf, _segment_sums(v.long(), ptr), ptr, True,
           torch.bfloat16)
    _judge("vagg outside vc", agg_vc, _segment_sums(tx.long(), ptr), ptr,
           True, torch.float32)


@pytest.mark.parametrize("c,h", [(1, 520), (1, 1024), (2, 516)])
def test_virtual_aggregate_above_limit_falls_back(c, h):
    """H above 512 (or not a multiple of 8): the extension refuses the
    shape and ops.virtual_aggregate is the composition of mid_mean and
    graph_mean_pool."""
    ptr, cb, ce, scp = _tables(LENGTHS)
    n, b = int(ptr[-1]), len(LENGTHS)
    batch = torch.repeat_interleave(
        torch.arange(b, device=DEV), ptr[1:] - ptr[:-1])
    v, tv, tx = _vagg_inputs(n, c, h, 33)
    with pytest.raises(RuntimeError):
        ops.hip_ext().virtual_aggregate_forward(v, tv, tx, ptr, cb, ce, scp)
    counts = (ptr[1:] - ptr[:-1]).float()
    kw = dict(ptr=ptr, counts=counts, chunks=(cb, ce, scp))
    got = ops.virtual_aggregate(v, tv, tx, batch, ptr, counts, (cb, ce, scp),
                                num_graphs=b)
    want = (ops.mid_mean(v), ops.mid_mean(tv),
            ops.graph_mean_pool(v.reshape(n, -1), batch, b,
                                **kw).reshape(b, c, h),
            ops.graph_mean_pool(tx.reshape(n, -1), batch, b,
                                **kw).reshape(b, c, 3))
    for a, w in zip(got, want):
        assert a.shape == w.shape and torch.equal(a, w)
    _judge(f"vagg fallback c={c} h={h}", got[2], _segment_sums(v.long(), ptr),
           ptr, True, torch.bfloat16)


def _old_backward(dagg_v, dtrans_v, dagg_vf, dagg_vc, batch, ptr, c):
    """mid_expand + (divide by count, gather by batch) + add: what autograd
    ran for mid_mean and graph_mean_pool of the same tensors."""
    ext = ops.hip_ext()
    cnt = (ptr[1:] - ptr[:-1]).clamp(min=1)
    g_mid = ext.mid_expand(dagg_v, c, 1.0 / c)
    g_pool = (dagg_vf / cnt.to(dagg_vf.dtype).view(-1, 1, 1)) \
        .index_select(0, batch)
    dtv = ext.mid_expand(dtrans_v, c, 1.0 / c)
    dtx = (dagg_vc / cnt.to(dagg_vc.dtype).view(-1, 1, 1)) \
        .index_select(0, batch)
    return g_mid + g_pool, dtv, dtx


@pytest.mark.parametrize("c", [1, 5, 8])
def test_virtual_aggregate_backward(c):
    lengths = [0, 300, 1, 7001, 0]      # an empty graph first and last
    ptr, _, _, _ = _tables(lengths)
    n, b, h = int(ptr[-1]), len(lengths), 64
    batch = torch.repeat_interleave(
        torch.arange(b, device=DEV), ptr[1:] - ptr[:-1])
    g = torch.Generator(device=DEV).manual_seed(40 + c)
    dagg_v = torch.randn(n, h, generator=g, device=DEV).bfloat16()
    dagg_vf = (100 * torch.randn(b, c, h, generator=g, device=DEV)).bfloat16()
    dtrans_v = torch.randn(n, 3, generator=g, device=DEV)
    dagg_vc = 100 * torch.randn(b, c, 3, generator=g, device=DEV)
    got = ops.hip_ext().virtual_aggregate_backward(
        dagg_v, dtrans_v, dagg_vf, dagg_vc, batch, ptr)
    want = _old_backward(dagg_v, dtrans_v, dagg_vf, dagg_vc, batch, ptr, c)
    for name, a, w in zip(("dv_msg", "dtv", "dtx"), got, want):
        assert a.dtype == w.dtype and a.shape == w.shape, name
        assert torch.equal(a, w), \
            f"{name}: {int((a != w).sum())} of {a.numel()} differ"


def test_deterministic():
    """Normal-distributed bf16 data, where the order of the fp32 additions
    shows: every new entry twice, bit-equal."""
    ptr, cb, ce, scp = _tables([50_000, 0, 70_001])
    n, c, h = int(ptr[-1]), 5, 64
    v, tv, tx = _vagg_inputs(n, c, h, 3, ints=False)
    wide = torch.randn(n * c, 8, device=DEV)
    ext = ops.hip_ext()
    batch = torch.repeat_interleave(
        torch.arange(3, device=DEV), ptr[1:] - ptr[:-1])

    def run():
        out = ext.segment_reduce_chunked_group(
            [v, wide.view(n, c, 8)[:, :, :c], tx], ptr, cb, ce, scp,
            [False, False, True])
        fwd = ext.virtual_aggregate_forward(v, tv, tx, ptr, cb, ce, scp)
        bwd = ext.virtual_aggregate_backward(
            fwd[0], fwd[1], fwd[2], fwd[3], batch, ptr)
        return list(out) + list(fwd) + list(bwd)

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_virtual_aggregate_autograd():
    """ops.virtual_aggregate against the composition it replaces, 3 graphs
    and 700 nodes in bf16: gradients torch.equal; pooled outputs within
    n*u23*sum|terms| (any order of n fp32 additions) + u8*|want| (the bf16
    output) of a float64 reference; channel means bit-equal."""
    lengths = [300, 1, 399]
    ptr, cb, ce, scp = _tables(lengths)
    n, b, c, h = int(ptr[-1]), len(lengths), 5, 64
    batch = torch.repeat_interleave(
        torch.arange(b, device=DEV), ptr[1:] - ptr[:-1])
    counts = (ptr[1:] - ptr[:-1]).float()
    v, tv, tx = _vagg_inputs(n, c, h, 9, ints=False)
    g = torch.Generator(device=DEV).manual_seed(10)
    cots = [torch.randn(n, h, generator=g, device=DEV).bfloat16(),
            torch.randn(n, 3, generator=g, device=DEV),
            torch.randn(b, c, h, generator=g, device=DEV).bfloat16(),
            torch.randn(b, c, 3, generator=g, device=DEV)]

    def run(fused):
        leaves = [t.clone().requires_grad_(True) for t in (v, tv, tx)]
        lv, ltv, ltx = leaves
        if fused:
            outs = ops.virtual_aggregate(lv, ltv, ltx, batch, ptr, counts,
                                         (cb, ce, scp), num_graphs=b)
        else:
            kw = dict(ptr=ptr, counts=counts, chunks=(cb, ce, scp))
            outs = (ops.mid_mean(lv), ops.mid_mean(ltv),
                    ops.graph_mean_pool(lv.reshape(n, -1), batch, b,
                                        **kw).reshape(b, c, h),
                    ops.graph_mean_pool(ltx.reshape(n, -1), batch, b,
                                        **kw).reshape(b, c, 3))
        grads = torch.autograd.grad(outs, leaves, grad_outputs=cots)
        return outs, grads

    (o_new, g_new), (o_old, g_old) = run(True), run(False)
    for a, w in zip(g_new, g_old):
        assert a.dtype == w.dtype and torch.equal(a, w)
    assert torch.equal(o_new[0], o_old[0]) and torch.equal(o_new[1], o_old[1])
    for name, got, x in (("agg_vf", o_new[2], v), ("agg_vc", o_new[3], tx)):
        for i, ln in enumerate(lengths):
            rows = x[int(ptr[i]):int(ptr[i + 1])].double()
            want = rows.sum(0) / ln
            # terms of the mean are x / ln; the bound's factor n over the
            # n - 1 additions at unit roundoff u23 / 2 also covers the one
            # rounding of the fp32 quotient
            bound = (ln * U23 * (rows.abs() / ln).sum(0)
                     + (U8 if got.dtype == torch.bfloat16 else 0.0)
                     * want.abs())
            err = (got[i].detach().double() - want).abs()
            r = float((err / bound).max())
            print(f"RATIO pool autograd {name}[{i}] err/bound={r:.4f}")
            assert r <= 1.0, (name, i, r)
