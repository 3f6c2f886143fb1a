"""GPU tests of the forward-only fp32 node kernel (csrc/fused_node_f32.hip)
against the float64 ``node_reference`` (``rnd`` = identity). Inputs are
fp32 and not rounded to bf16.

Element bounds, after the model of test_edge_f32_gpu.py: u = 2^-23, ``mag``
= the same product over absolute values, K_IN = 3H + A.

  a1 = 2(K_IN+1) u mag1                fp32 accumulation of K_IN products and
                                       the bias (the inputs are exact: no
                                       term for roundings ahead of GEMM1)
  e1 = 1.1 a1 + 2u|z1||t1| + u|t1|     silu stretches by <= 1.1; the fast
                                       exponential; the final division
  a2 = e1 |W2|^T + 2(H+1) u mag2       mag2 = (|t1|+e1)|W2|^T + |b2|
  h_out: a2 + u |h_out|                out = t1 W2^T + b2 has no activation;
                                       one more rounding for h + out
  phiv:  u (4(H+2) mag_p + 2 fx) + u |phiv|
                                       the head bound of
                                       test_virtual_f32_gpu.py on the exact
                                       input h (mag_p = (|h||Wv1|^T + |bv1|)
                                       |wv2|, fx = (|zv| |silu(zv)|) |wv2|),
                                       one more rounding for + bv2

A bound of 0 requires an error of 0. The relative L2 error of h_out and phiv
against float64 is at most 2^-17, the project's gate between fp32 and any
bf16 rounding. phiv is a signed sum of H terms and can cancel when there
are few rows, so the L2 gate is applied to the first seed whose head
condition number |sum_c |silu(zv_c) wv2_c|| / |phiv - bv2| (L2 over rows,
from the float64 reference alone) is at most 2 sqrt(H); the seeds passed
over are still judged element by element. Two calls give bitwise equal
results.

Rows: one row, a partial and a full 16-row wave sub-tile, a partial, a full
and a second 64-row tile (the full H=128 form has 32-row tiles: 17 and 63
are its partial second tile, 64 and 65 its full second and a third), several
blocks; A in {0, 2, 8} are GEMM1's two
depths (3H/16 and 3H/16 + 1 k-steps) and the widest tail. The grid is capped
at 4096 blocks: ``test_node_f32_second_trip`` goes one tile past it.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.ops import edge_reference as ER
from distegnn_amd.ops import node_reference as NR

U = 2.0 ** -23
GATE = 2.0 ** -17
DEV = "cuda:0"
TILE = 64
GRID_CAP = 4096      # csrc/fused_node_f32.hip
ROWS = (1, 15, 16, 17, 63, 64, 65, 333)
PARAM_KEYS = ("w1", "b1", "w2", "b2", "wv1", "bv1", "wv2", "bv2")


def make_inputs(hd, n, a, seed=0, vel_only=False):
    """CPU fp32 (h, agg_e, agg_v, attr or None) and the eight parameters
    (wv2 [H], bv2 [1]), not rounded to bf16."""
    g = torch.Generator().manual_seed(
        1000 * seed + 7 * n + a + (500 if vel_only else 0))

    def t(*shape, s):
        return torch.randn(*shape, generator=g) * s

    k_in = 3 * hd + a
    params = [t(hd, k_in, s=1.5 / k_in ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2), t(hd, s=0.3),
              t(1, s=0.2)]
    data = [t(n, hd, s=0.7), t(n, hd, s=0.7), t(n, hd, s=0.7),
            t(n, a, s=1.0) if a else None]
    return data, params


def reference(data, params, vel_only):
    d = [None if t is None else t.double() for t in data]
    return NR.node_forward(*d, *[p.double() for p in params],
                           vel_only=vel_only)


def head_condition(ref, params):
    """|sum_c |silu(zv_c) wv2_c|| / |phiv - bv2| over all rows, from the
    float64 reference alone."""
    wv2, bv2 = params[6].double(), params[7].double()
    terms = ER.silu(ref["zv"]).abs() @ wv2.abs()
    return float(terms.norm() / (ref["phiv"].squeeze(1) - bv2).norm())


def conditioned_inputs(hd, n, a, vel_only=False):
    """``make_inputs`` at the first seed in range(64) whose float64
    reference has a head condition number of at most 2 sqrt(H) (see
    test_virtual_f32_gpu.py ``conditioned_inputs``). The choice looks at the
    float64 reference only, never at a kernel output."""
    for seed in range(64):
        data, params = make_inputs(hd, n, a, seed, vel_only)
        ref = reference(data, params, vel_only)
        k = head_condition(ref, params)
        if k <= 2 * hd ** 0.5:
            return data, params, ref, seed, k
    raise AssertionError("no well-conditioned draw in 64 seeds")


def worst_ratio(got, want, bound):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    err = (got.double().cpu() - want).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


def h_out_bound(hd, a, ref, params):
    k_in = 3 * hd + a
    W1, b1, W2, b2 = [p.double() for p in params[:4]]
    mag1 = ref["xin"].abs() @ W1.abs().t() + b1.abs()
    a1 = 2 * (k_in + 1) * U * mag1
    t1 = ref["t1"].abs()
    e1 = 1.1 * a1 + 2 * U * ref["z1"].abs() * t1 + U * t1
    mag2 = (t1 + e1) @ W2.abs().t() + b2.abs()
    a2 = e1 @ W2.abs().t() + 2 * (hd + 1) * U * mag2
    return a2 + U * ref["h_out"].abs()


def phiv_bound(hd, h, ref, params):
    Wv1, bv1, wv2 = [p.double() for p in params[4:7]]
    mag = h.double().abs() @ Wv1.abs().t() + bv1.abs()
    z = ref["zv"]
    mag_p = mag @ wv2.abs()
    fx = (z.abs() * ER.silu(z).abs()) @ wv2.abs()
    return (U * (4 * (hd + 2) * mag_p + 2 * fx).unsqueeze(1)
            + U * ref["phiv"].abs())


def rel_l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


def call(data, params, vel_only):
    ext = ops.hip_ext()
    p = [t.to(DEV) for t in params]
    h = data[0].to(DEV)
    if vel_only:
        # none of the node chain's operands is handed over, let alone read
        return ext.fused_node_forward_f32(h, None, None, None, None, None,
                                          None, None, *p[4:], True)
    d = [None if t is None else t.to(DEV) for t in data]
    return ext.fused_node_forward_f32(*d, *p, False)


def check(hd, n, a, vel_only, data, params, ref, l2_gate):
    h_out, phiv = call(data, params, vel_only)
    assert phiv.shape == (n, 1) and phiv.dtype == torch.float32
    r_p = worst_ratio(phiv, ref["phiv"], phiv_bound(hd, data[0], ref, params))
    e_p = rel_l2(phiv, ref["phiv"])
    # the fp32 composition on the GPU, for information only
    eager = NR.node_block(
        *[None if t is None else t.to(DEV) for t in data],
        *[p.to(DEV) for p in params], vel_only=vel_only)
    r_h = e_h = ee_h = 0.0
    if vel_only:
        assert h_out.shape == (0, hd)
    else:
        assert h_out.shape == (n, hd) and h_out.dtype == torch.float32
        r_h = worst_ratio(h_out, ref["h_out"],
                          h_out_bound(hd, a, ref, params))
        e_h = rel_l2(h_out, ref["h_out"])
        ee_h = rel_l2(eager[0], ref["h_out"])
    print(f"RATIO node_f32 N={n} H={hd} A={a} vel_only={int(vel_only)} "
          f"h_out={r_h:.4f} phiv={r_p:.4f}  L2 h_out={e_h:.3e} "
          f"phiv={e_p:.3e} (eager fp32: {ee_h:.3e} "
          f"{rel_l2(eager[1], ref['phiv']):.3e})"
          f"{'' if l2_gate else '  [ill-conditioned draw, no L2 gate]'}")
    assert max(r_h, r_p) <= 1.0, (r_h, r_p)
    if l2_gate:
        assert max(e_h, e_p) <= GATE, (e_h, e_p)
    again = call(data, params, vel_only)
    assert torch.equal(h_out, again[0]) and torch.equal(phiv, again[1])


def run_case(hd, n, a, vel_only):
    data, params, ref, seed, kappa = conditioned_inputs(hd, n, a, vel_only)
    print(f"node_f32 N={n} H={hd} A={a} vel_only={int(vel_only)}: "
          f"seed {seed}, kappa {kappa:.1f}")
    # the draws passed over are judged too, element by element
    for s in range(seed):
        d, p = make_inputs(hd, n, a, s, vel_only)
        check(hd, n, a, vel_only, d, p, reference(d, p, vel_only),
              l2_gate=False)
    check(hd, n, a, vel_only, data, params, ref, l2_gate=True)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("a", [0, 2, 8])
@pytest.mark.parametrize("n", ROWS)
def test_node_f32(n, a, hd):
    run_case(hd, n, a, False)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("n", ROWS)
def test_node_f32_vel_only(n, hd):
    run_case(hd, n, 0, True)


@pytest.mark.parametrize("vel_only", [False, True])
def test_node_f32_second_trip(vel_only):
    """One tile past GRID_CAP tiles: block 0 walks a second tile."""
    run_case(32, GRID_CAP * TILE + TILE, 0 if vel_only else 2, vel_only)


def test_node_f32_rejects_unsupported_inputs():
    ext = ops.hip_ext()

    def dev(hd, n, a):
        data, params = make_inputs(hd, n, a)
        return ([None if t is None else t.to(DEV) for t in data],
                [p.to(DEV) for p in params])

    data, params = dev(48, 20, 2)
    with pytest.raises(RuntimeError, match=r"32, 64, 128"):
        ext.fused_node_forward_f32(*data, *params, False)
    data, params = dev(64, 20, 9)
    with pytest.raises(RuntimeError, match="node_attr_nf <= 8"):
        ext.fused_node_forward_f32(*data, *params, False)
    data, params = dev(64, 20, 2)
    with pytest.raises(RuntimeError, match="fp32"):
        ext.fused_node_forward_f32(data[0].bfloat16(), *data[1:], *params,
                                   False)
    with pytest.raises(RuntimeError, match="fp32"):          # bf16 agg_v
        ext.fused_node_forward_f32(data[0], data[1], data[2].bfloat16(),
                                   data[3], *params, False)
    with pytest.raises(RuntimeError, match="fp32"):          # bf16 weight
        ext.fused_node_forward_f32(*data, params[0], params[1],
                                   params[2].bfloat16(), *params[3:], False)
    with pytest.raises(RuntimeError, match="fp32"):          # bf16 vel weight
        ext.fused_node_forward_f32(*data, *params[:4], params[4].bfloat16(),
                                   *params[5:], True)
    with pytest.raises(RuntimeError, match="fp32"):          # strided rows
        wide = torch.randn(20, 128, device=DEV)
        ext.fused_node_forward_f32(data[0], wide[:, :64], *data[2:], *params,
                                   False)
    with pytest.raises(RuntimeError, match="fp32"):          # strided h
        wide = torch.randn(20, 128, device=DEV)
        ext.fused_node_forward_f32(wide[:, :64], *data[1:], *params, False)
    with pytest.raises(RuntimeError, match="w1 must be"):
        ext.fused_node_forward_f32(*data, params[0][:, :-1].contiguous(),
                                   *params[1:], False)
    with pytest.raises(RuntimeError, match="w1 must be"):    # attr left out
        ext.fused_node_forward_f32(*data[:3], None, *params, False)


@pytest.mark.parametrize("vel_only", [False, True])
def test_node_f32_empty(vel_only):
    data, params = make_inputs(64, 4, 2)
    data = [t[:0].to(DEV) for t in data]
    params = [p.to(DEV) for p in params]
    h_out, phiv = ops.hip_ext().fused_node_forward_f32(*data, *params,
                                                       vel_only)
    assert h_out.shape == (0, 64) and phiv.shape == (0, 1)
    assert h_out.dtype == phiv.dtype == torch.float32
