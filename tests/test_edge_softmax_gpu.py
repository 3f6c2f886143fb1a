"""GPU tests of the fused CSR edge softmax (``edge_softmax_csr`` in
csrc/segment_reduce.hip) against a float64 softmax per destination segment.

Reference: ``_Ref`` gathers every segment's scores through ``dstptr`` and
``perm`` into a padded [n, Lmax, h] float64 block and takes a plain softmax
over it; it uses no scatter_reduce / segment path of the project and is
differentiable, so the backward is judged against its float64 autograd.

Layout of the kernel: one wave per segment, lane = (edge sublane, head),
nrl = 64/h edge sublanes. Each lane walks ceil(L/nrl) edges, then log2(nrl)
xor-shuffle steps combine the sublanes (none at h = 64).

Bound on an output a_i = exp(x_i)/den, x_i = s_i - max <= 0 (u23 = 2^-23):

* x_i is one fp32 subtraction: u23/2*|x_i| absolute, which the exponential
  turns into a relative error; the fast exponential itself costs
  (1 + |x_i|/2)*u23: together eps_i = (1 + |x_i|)*u23, relatively;
* den sums terms e_j that each carry eps_j: relatively, sum_j a_j*eps_j
  (the weights are the softmax itself);
* den's additions: ceil(L/nrl) per lane plus log2(nrl) shuffle adds, each
  u23/2 relatively, all terms positive: (ceil(L/nrl) + log2(nrl))*u23/2;
* one division: u23/2.

  |err_i| <= a_i*u23*[(1 + |x_i|) + sum_j a_j (1 + |x_j|)
                      + (ceil(L/nrl) + log2(nrl) + 1)/2]

Bound-judged cases keep x >= -80, so no exponential reaches the denormal
range (exp(-80) = 1.8e-35). Every non-empty segment's outputs must also sum
to 1 within (L + 4)*u23.

Backward (``_EdgeSoftmaxFn``): ds = a*g - a*S, S = sum_j a_j g_j over the
segment, evaluated in fp32 from the forward's a (error <= B, the bound
above) with S an fp32 sum of L terms in any order:

  e_S  = sum_j |g_j| B_j + (L + 1)*u23/2 * sum_j |a_j g_j|
  e_ds = B*(|g| + |S| + e_S) + a*e_S + u23*(|a g| + a|S|)

docs/KERNELS.md ("Edge softmax test bounds") records the measured ratios.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.models.se3.modules import edge_softmax

U23 = 2.0 ** -23
U8 = 2.0 ** -8
DEV = "cuda:0"
HEADS = [1, 2, 4, 8, 16, 32, 64]
HUB = 5000
WAVE_CAP = 16384 * 4            # blocks are capped at 16384 x 4 waves


def seg_lengths(h):
    """Empty first and last, two adjacent empties, lengths around nrl, a
    hub. At h = 64 (nrl = 1) ``nrl - 1`` is one more empty segment."""
    nrl = 64 // h
    return [0, 1, nrl - 1, nrl, 0, 0, nrl + 1, 2 * nrl + 1, HUB, 0]


class _Graph:
    """Edges stored in shuffled order: ``perm`` is not the identity."""

    def __init__(self, lengths, seed):
        g = torch.Generator().manual_seed(seed)
        lens = torch.as_tensor(lengths, dtype=torch.long)
        self.n, self.m = lens.numel(), int(lens.sum())
        dst = torch.repeat_interleave(torch.arange(self.n), lens)
        dst = dst[torch.randperm(self.m, generator=g)]
        perm = torch.argsort(dst, stable=True)
        assert self.m < 2 or not torch.equal(perm, torch.arange(self.m))
        self.lens = lens.to(DEV)
        self.dst, self.perm = dst.to(DEV), perm.to(DEV)
        self.dstptr = torch.cat([torch.zeros(1, dtype=torch.long),
                                 lens.cumsum(0)]).to(DEV)
        lmax = max(int(lens.max()), 1)
        k = torch.arange(lmax, device=DEV).view(1, -1)
        self.valid = k < self.lens.view(-1, 1)                  # [n, Lmax]
        pos = (self.dstptr[:-1].view(-1, 1) + k).clamp(max=max(self.m - 1, 0))
        self.rows = self.perm[pos] if self.m else pos           # [n, Lmax]
        self.edge_len = self.lens[self.dst]                     # [M]


class _Ref:
    """float64 softmax per segment; ``a`` [M, h], ``x`` = s - max [M, h],
    ``t`` = sum_j a_j (1 + |x_j|) of the edge's segment [M, h]."""

    def __init__(self, G, scores):
        s = scores.double()[G.rows]                             # [n, L, h]
        s = s.masked_fill(~G.valid.unsqueeze(-1), -math.inf)
        mx = s.max(1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        x = s - mx.detach()
        e = torch.exp(x)
        a = e / e.sum(1, keepdim=True).clamp(min=1e-300)
        t = (a * (1 + x.abs().masked_fill(~G.valid.unsqueeze(-1), 0))) \
            .sum(1, keepdim=True).expand_as(a)
        idx = (G.rows[G.valid],)
        blank = torch.zeros(G.m, scores.size(1), dtype=torch.float64,
                            device=scores.device)
        self.a = blank.index_put(idx, a[G.valid])
        self.x = blank.index_put(idx, x[G.valid]).detach()
        self.t = blank.index_put(idx, t[G.valid]).detach()


def _fwd_bound(G, ref, h):
    nrl = 64 // h
    adds = torch.ceil(G.edge_len.double() / nrl) + math.log2(nrl) + 1
    return ref.a.detach() * U23 * ((1 + ref.x.abs()) + ref.t
                                   + 0.5 * adds.view(-1, 1))


def _segment_sums(G, v):
    """float64 per-segment sums of v [M, h] -> [n, h] (padded gather)."""
    return (v.double()[G.rows] * G.valid.unsqueeze(-1)).sum(1)


def _judge_forward(tag, G, scores, got, h):
    ref = _Ref(G, scores)
    want = ref.a.detach()
    assert got.shape == want.shape and got.dtype == torch.float32, tag
    # the whole tensor: every edge lies in a segment, every row is written
    assert bool(torch.isfinite(got).all()), tag
    assert float(ref.x.min()) >= -80.0, tag
    bound = _fwd_bound(G, ref, h)
    err = (got.double() - want).abs()
    r = float((err / bound).max()) if err.numel() else 0.0
    sums = _segment_sums(G, got)
    full = G.lens > 0
    dev1 = (sums[full] - 1).abs() / ((G.lens[full].double() + 4) * U23) \
        .view(-1, 1)
    r1 = float(dev1.max()) if dev1.numel() else 0.0
    print(f"RATIO softmax {tag} err/bound={r:.4f} sum-to-1/bound={r1:.4f}")
    assert r <= 1.0 and r1 <= 1.0, (tag, r, r1)
    return ref, bound


def _run(G, scores):
    return ops.hip_ext().edge_softmax_fwd(scores, G.dstptr, G.perm)


def _scores(G, h, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(G.m, h, generator=g) * scale).to(DEV)


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("h", HEADS)
def test_forward_segment_lengths(h):
    G = _Graph(seg_lengths(h), seed=h)
    assert G.lens[0] == 0 and G.lens[-1] == 0
    _judge_forward(f"h={h} lengths", G, _scores(G, h, 10 + h),
                   _run(G, _scores(G, h, 10 + h)), h)


@pytest.mark.parametrize("h", HEADS)
def test_equal_scores_give_one_over_length(h):
    G = _Graph(seg_lengths(h), seed=20 + h)
    scores = torch.full((G.m, h), 3.25, device=DEV)
    got = _run(G, scores)
    _judge_forward(f"h={h} equal", G, scores, got, h)
    inv = 1.0 / G.edge_len.double().view(-1, 1)
    nrl = 64 // h
    adds = torch.ceil(G.edge_len.double() / nrl) + math.log2(nrl) + 1
    bound = inv * U23 * (2 + 0.5 * adds.view(-1, 1))
    assert bool(((got.double() - inv).abs() <= bound).all())


@pytest.mark.parametrize("h", [1, 8, 64])
def test_shift_invariance(h):
    """Scores on multiples of 2^-6 in [-4, 4]: adding 1e4 is exact in fp32,
    and so is every s - max; the shifted call must be bit-equal to the
    unshifted one and within the bound of the float64 softmax of the
    UNSHIFTED scores. One segment is shifted, then all of them."""
    G = _Graph(seg_lengths(h), seed=30 + h)
    g = torch.Generator().manual_seed(31 + h)
    base = (torch.randint(-256, 257, (G.m, h), generator=g).float() / 64) \
        .to(DEV)
    plain = _run(G, base)
    _judge_forward(f"h={h} unshifted", G, base, plain, h)
    hub = int(torch.argmax(G.lens))
    in_hub = (G.dst == hub).double().view(-1, 1)
    for tag, shift in (("hub", 1e4 * in_hub),
                       ("all", 1e4 * torch.ones_like(in_hub))):
        shifted = (base.double() + shift).float()
        assert torch.equal(shifted.double(), base.double() + shift)  # exact
        got = _run(G, shifted)
        assert torch.equal(got, plain), f"h={h} shift {tag}"
        _judge_forward(f"h={h} shift-{tag}", G, base, got, h)


@pytest.mark.parametrize("h", [1, 8, 64])
def test_dominant_score(h):
    """One score per segment and head exceeds the others by 200: that edge
    gets 1 within the bound, the others at most 1e-37 and no NaN."""
    G = _Graph(seg_lengths(h), seed=40 + h)
    scores = _scores(G, h, 41 + h, scale=0.0)
    first = G.rows[:, 0][G.lens > 0]            # one edge of every segment
    scores[first] += 200.0
    got = _run(G, scores)
    assert bool(torch.isfinite(got).all())
    win = torch.zeros(G.m, dtype=torch.bool, device=DEV)
    win[first] = True
    nrl = 64 // h
    adds = torch.ceil(G.edge_len[win].double() / nrl) + math.log2(nrl) + 1
    bound = U23 * (2 + 0.5 * adds.view(-1, 1))
    err = (got[win].double() - 1).abs()
    print(f"RATIO softmax h={h} dominant "
          f"err/bound={float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    assert float(got[~win].max()) <= 1e-37 and float(got[~win].min()) >= 0


def test_second_grid_stride_trip():
    """n = 16384*4 + 3 segments of lengths 0..3 at h = 4: the last three
    segments are a wave's second trip."""
    n = WAVE_CAP + 3
    g = torch.Generator().manual_seed(50)
    lens = torch.randint(0, 4, (n,), generator=g)
    lens[-3:] = torch.tensor([3, 1, 2])
    G = _Graph(lens, seed=51)
    scores = _scores(G, 4, 52)
    _judge_forward("h=4 second-trip", G, scores, _run(G, scores), 4)


# ------------------------------------------------- the model's entry point
@pytest.mark.parametrize("h", [3, 5])
def test_non_power_of_two_heads_take_the_composition(h, monkeypatch):
    G = _Graph([0, 1, 7, 0, 300, 2], seed=60 + h)
    scores = _scores(G, h, 61 + h)
    with pytest.raises(RuntimeError, match="power of two"):
        _run(G, scores)
    calls = []
    monkeypatch.setattr(ops.hip_ext(), "edge_softmax_fwd",
                        lambda *a, **k: calls.append(1))
    got = edge_softmax(scores, G.dst, G.n, csr=(G.dstptr, G.perm))
    assert not calls, "the kernel was called with a head count it rejects"
    want = _Ref(G, scores).a
    assert got.dtype == torch.float32
    assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-30)
    print(f"RATIO softmax h={h} composition err/bound="
          f"{float(((got.double() - want).abs() / (1e-5 * want)).max()):.4f}")


@pytest.mark.parametrize("h", [1, 8, 64])
def test_bf16_scores_return_bf16(h):
    G = _Graph(seg_lengths(h), seed=70 + h)
    scores = _scores(G, h, 71 + h).bfloat16()
    got = edge_softmax(scores, G.dst, G.n, csr=(G.dstptr, G.perm))
    assert got.dtype == torch.bfloat16 and got.shape == scores.shape
    ref = _Ref(G, scores.float())
    fb = _fwd_bound(G, ref, h)
    bound = fb + U8 * (ref.a + fb)
    err = (got.double() - ref.a).abs()
    r = float((err / bound).max())
    print(f"RATIO softmax h={h} bf16 err/bound={r:.4f}")
    assert r <= 1.0


# --------------------------------------------------------------- backward
@pytest.mark.parametrize("h", [1, 8, 64])
def test_backward_against_float64_autograd(h):
    G = _Graph(seg_lengths(h), seed=80 + h)
    scores = _scores(G, h, 81 + h)
    g = torch.randn(G.m, h, generator=torch.Generator().manual_seed(82 + h)) \
        .to(DEV)
    s64 = scores.double().requires_grad_(True)
    ref = _Ref(G, s64)
    want, = torch.autograd.grad(ref.a, s64, g.double())
    sf = scores.clone().requires_grad_(True)
    attn = edge_softmax(sf, G.dst, G.n, csr=(G.dstptr, G.perm))
    got, = torch.autograd.grad(attn, sf, g)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())

    a = ref.a.detach()
    B = _fwd_bound(G, ref, h)
    gd = g.double()
    S = _segment_sums(G, a * gd)[G.dst]
    A1 = _segment_sums(G, (a * gd).abs())[G.dst]
    EB = _segment_sums(G, gd.abs() * B)[G.dst]
    L = G.edge_len.double().view(-1, 1)
    e_S = EB + (L + 1) * 0.5 * U23 * A1
    bound = B * (gd.abs() + S.abs() + e_S) + a * e_S \
        + U23 * ((a * gd).abs() + a * S.abs())
    err = (got.double() - want).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all())
    r = float((err[~zero] / bound[~zero]).max())
    print(f"RATIO softmax h={h} backward err/bound={r:.4f}")
    assert r <= 1.0
