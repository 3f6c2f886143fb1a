"""GPU tests of the fp32 no-grad branch of ``ops.fused_node_block``
(csrc/fused_node_f32.hip) and of FastEGNN evaluated in fp32 with all three
blocks of a layer on the fused fp32 kernels. The float64 truth is
``node_reference.node_block``; 2^-17 relative L2 is the project's gate
between fp32 and any bf16 rounding (tests/test_node_f32_gpu.py holds the
element-wise bounds)."""

import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import collate
from distegnn_amd.data.synthetic import make_cutoff_dataset
from distegnn_amd.ops import node_reference as NR
from distegnn_amd.ops import prep

GATE = 2.0 ** -17
DEV = "cuda:0"
ENTRIES = {"node": "fused_node_forward_f32",
           "edge": "fused_edge_forward_f32",
           "virtual": "fused_virtual_forward_f32"}
VEL_ONLY_ARG = 12     # position of vel_only in fused_node_forward_f32


@pytest.fixture(autouse=True)
def _fresh_state(monkeypatch):
    monkeypatch.delenv("DISTEGNN_DISABLE_FUSED", raising=False)
    monkeypatch.delenv("DISTEGNN_NODE_EAGER", raising=False)
    prep.clear()
    ops._FALLBACK_WARNED.clear()
    yield
    prep.clear()


@pytest.fixture
def calls(monkeypatch):
    """Counts calls of the three fp32 extension functions; ``vel_only``
    lists the flag of every node-block call. An entry the extension lacks
    counts nothing."""
    ext = ops.hip_ext()
    n = {"node": 0, "edge": 0, "virtual": 0, "vel_only": []}
    for key, name in ENTRIES.items():
        real = getattr(ext, name, None)
        if real is None:
            continue

        def counted(*a, _real=real, _key=key, **kw):
            n[_key] += 1
            if _key == "node":
                n["vel_only"].append(bool(kw.get("vel_only",
                                                 a[VEL_ONLY_ARG]
                                                 if len(a) > VEL_ONLY_ARG
                                                 else False)))
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, counted)
    return n


@pytest.fixture
def eager_calls(monkeypatch):
    seen = []
    real = ops.eager_node_block

    def spy(*args, **kw):
        seen.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(ops, "eager_node_block", spy)
    return seen


def rel_l2(got, want):
    return float((got.double().cpu() - want.cpu()).norm() / want.norm())


def mlps(hd, a, seed=0, act=nn.SiLU, requires_grad=True):
    torch.manual_seed(seed)
    node_mlp = nn.Sequential(nn.Linear(3 * hd + a, hd), act(),
                             nn.Linear(hd, hd)).to(DEV)
    vel_mlp = nn.Sequential(nn.Linear(hd, hd), nn.SiLU(),
                            nn.Linear(hd, 1)).to(DEV)
    for p in list(node_mlp.parameters()) + list(vel_mlp.parameters()):
        p.requires_grad_(requires_grad)
    return node_mlp, vel_mlp


def inputs(hd, a, n=333, seed=0):
    g = torch.Generator().manual_seed(500 + seed + hd + a)

    def t(*shape):
        return (torch.randn(*shape, generator=g) * 0.7).to(DEV)

    return t(n, hd), t(n, hd), t(n, hd), (t(n, a) if a else None)


def truth(data, node_mlp, vel_mlp, vel_only=False):
    """``node_reference.node_block`` in float64 on the modules' weights."""
    p = [node_mlp[0].weight, node_mlp[0].bias, node_mlp[2].weight,
         node_mlp[2].bias, vel_mlp[0].weight, vel_mlp[0].bias,
         vel_mlp[2].weight.view(-1), vel_mlp[2].bias]
    return NR.node_block(
        *[None if t is None else t.detach().double() for t in data],
        *[t.detach().double() for t in p], vel_only=vel_only)


# ------------------------------------------------------------------ block
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_no_grad_takes_fp32_kernel(hd, calls, eager_calls, capsys):
    a = 2
    data = inputs(hd, a)
    # parameters that require grad, as a model's do: no_grad decides
    node_mlp, vel_mlp = mlps(hd, a)
    with torch.no_grad():
        h_out, phiv = ops.fused_node_block(*data, node_mlp, vel_mlp, True)
    assert calls["node"] == 1 and calls["vel_only"] == [False]
    assert not eager_calls
    assert "fused_node_block" not in capsys.readouterr().out
    assert h_out.dtype == torch.float32 and h_out.shape == (333, hd)
    assert phiv.dtype == torch.float32 and phiv.shape == (333, 1)
    assert not h_out.requires_grad and not phiv.requires_grad
    want_h, want_p = truth(data, node_mlp, vel_mlp)
    e_h, e_p = rel_l2(h_out, want_h), rel_l2(phiv, want_p)
    print(f"DISPATCH node H={hd} h_out={e_h:.3e} phiv={e_p:.3e}")
    assert e_h <= GATE and e_p <= GATE
    # vel-only: h itself comes back, phiv is the same head on the same h
    with torch.no_grad():
        h2, pv = ops.fused_node_block(data[0], None, None, None, node_mlp,
                                      vel_mlp, True, vel_only=True)
    assert h2 is data[0] and torch.equal(pv, phiv)
    assert calls["node"] == 2 and calls["vel_only"] == [False, True]
    assert not eager_calls
    assert "fused_node_block" not in capsys.readouterr().out


def test_grad_free_inputs_take_fp32_kernel_with_grad_mode_on(calls,
                                                             eager_calls):
    """Grad mode on but nothing requires grad: no gradient is needed."""
    data = inputs(64, 0)
    node_mlp, vel_mlp = mlps(64, 0, requires_grad=False)
    assert torch.is_grad_enabled()
    h_out, phiv = ops.fused_node_block(*data, node_mlp, vel_mlp, True)
    assert calls["node"] == 1 and not eager_calls
    assert not h_out.requires_grad and not phiv.requires_grad


def test_with_grad_takes_composition_and_differentiates(calls, eager_calls,
                                                        capsys):
    data = inputs(64, 2, n=100)
    h = data[0].requires_grad_(True)
    node_mlp, vel_mlp = mlps(64, 2)
    params = list(node_mlp.parameters()) + list(vel_mlp.parameters())
    h_out, phiv = ops.fused_node_block(h, *data[1:], node_mlp, vel_mlp, True)
    grads = torch.autograd.grad(h_out.pow(2).sum() + phiv.pow(2).sum(),
                                [h] + params)
    assert calls["node"] == 0 and len(eager_calls) == 1
    out = capsys.readouterr().out
    assert "fused_node_block" in out and "torch.float32" in out
    assert "forward-only" in out
    for g, t in zip(grads, [h] + params):
        assert g.shape == t.shape and bool(torch.isfinite(g).all())
        assert float(g.abs().max()) > 0


@pytest.mark.parametrize("var", ["DISTEGNN_DISABLE_FUSED",
                                 "DISTEGNN_NODE_EAGER"])
def test_switches_reach_the_composition(var, calls, eager_calls, capsys,
                                        monkeypatch):
    data = inputs(64, 2)
    node_mlp, vel_mlp = mlps(64, 2)
    monkeypatch.setenv(var, "1")
    with torch.no_grad():
        got = ops.fused_node_block(*data, node_mlp, vel_mlp, True)
        want = ops.eager_node_block(*data, node_mlp, vel_mlp, True, False)
    assert calls["node"] == 0 and len(eager_calls) == 2
    assert "fused_node_block" not in capsys.readouterr().out
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_weight_copies_follow_updates_without_refresh(calls):
    """The fragment-order copies are cached per weight version and are
    outside ``prep.refresh``: the next fp32 call itself picks up an in-place
    weight update."""
    data = inputs(64, 2)
    node_mlp, vel_mlp = mlps(64, 2)
    with torch.no_grad():
        before = ops.fused_node_block(*data, node_mlp, vel_mlp, True)
        assert any(k[1] == "frag16_f32" for k in prep._CACHE)
        node_mlp[0].weight.mul_(0.5)
        node_mlp[2].weight.add_(0.01)
        vel_mlp[0].weight.mul_(1.25)
        assert not prep.any_stale() and prep.refresh() == 0
        after = ops.fused_node_block(*data, node_mlp, vel_mlp, True)
    assert calls["node"] == 2
    assert not torch.equal(before[0], after[0])
    assert not torch.equal(before[1], after[1])
    want = truth(data, node_mlp, vel_mlp)
    assert rel_l2(after[0], want[0]) <= GATE
    assert rel_l2(after[1], want[1]) <= GATE


@pytest.mark.parametrize("case,names", [
    ("width", "hidden_nf=48"),
    ("attr", "node_attr_nf=9"),
    ("residual", "residual=False"),
    ("activation", "not Linear-SiLU-Linear"),
])
def test_fallback_warns_and_names_its_cause(case, names, calls, eager_calls,
                                            capsys):
    hd = 48 if case == "width" else 64
    a = 9 if case == "attr" else 2
    data = inputs(hd, a, n=50)
    node_mlp, vel_mlp = mlps(hd, a,
                             act=nn.ReLU if case == "activation" else nn.SiLU)
    with torch.no_grad():
        h_out, phiv = ops.fused_node_block(*data, node_mlp, vel_mlp,
                                           case != "residual")
    assert calls["node"] == 0 and len(eager_calls) == 1
    out = capsys.readouterr().out
    assert "fused_node_block" in out and names in out
    assert h_out.shape == (50, hd) and phiv.shape == (50, 1)


# --------------------------------------------------------------- in model
_BATCH = {}


def model_batches():
    if not _BATCH:
        _BATCH["cpu"] = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                                    n_override=1200))
        _BATCH["gpu"] = collate(make_cutoff_dataset(
            "Water-3D", 2, seed=3, n_override=1200)).to(DEV)
        g = torch.Generator().manual_seed(1)
        _BATCH["attr"] = torch.randn(_BATCH["cpu"].num_nodes, 2, generator=g)
    return _BATCH["cpu"], _BATCH["gpu"], _BATCH["attr"]


def run_model(m, bt, node_attr, cast=None):
    f = (lambda t: t.to(cast)) if cast is not None else (lambda t: t)
    kw = dict(edge_attr=f(bt.edge_attr), rowptr=bt.rowptr, ptr=bt.ptr,
              counts=f(bt.counts), colptr=getattr(bt, "colptr", None),
              col_perm=getattr(bt, "col_perm", None))
    if node_attr is not None:
        kw["node_attr"] = f(node_attr)
    with torch.no_grad():
        return m(f(bt.x), f(bt.pos), f(bt.vel), f(bt.loc_mean),
                 bt.edge_index, bt.batch, **kw)


@pytest.mark.parametrize("attr_nf", [0, 2])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_in_model_fp32_eval_runs_three_fused_blocks(hd, attr_nf, calls,
                                                    eager_calls, capsys):
    """FastEGNN (L=4, C=3) under no_grad in fp32 on the 2,400-node Water-3D
    synthetic batch: every layer runs its edge, virtual and node block on
    the fp32 kernels (the last layer's node block in its vel-only form) and
    nothing is printed. Gates as in test_f32_dispatch_gpu.py
    ``test_in_model_fp32_eval``: the displacement loc_pred - pos within
    2^-12 of a CPU float64 copy, virtual_loc within 2^-17."""
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt_cpu, bt, attr = model_batches()
    assert bt.num_nodes == 2400
    attr = attr if attr_nf else None
    m = FastEGNN(node_feat_nf=2, node_attr_nf=attr_nf, edge_attr_nf=2,
                 hidden_nf=hd, virtual_channels=3, world_size=1, n_layers=4)
    loc64, vloc64 = run_model(copy.deepcopy(m).double(), bt_cpu, attr,
                              cast=torch.float64)
    assert loc64.dtype == torch.float64
    assert len(eager_calls) == 4      # the CPU model runs the composition
    eager_calls.clear()
    mg = copy.deepcopy(m).to(DEV)
    loc_f, vloc_f = run_model(mg, bt, None if attr is None else attr.to(DEV))
    assert calls["node"] == 4
    assert sorted(calls["vel_only"]) == [False, False, False, True]
    assert calls["edge"] == 4 and calls["virtual"] == 4
    assert not eager_calls
    assert "fused_" not in capsys.readouterr().out
    pos = bt_cpu.pos.double()
    d_f = rel_l2(loc_f.double().cpu() - pos, loc64 - pos)
    v_f = rel_l2(vloc_f, vloc64)
    print(f"MODEL fp32 eval H={hd} node_attr_nf={attr_nf} disp={d_f:.3e} "
          f"virtual_loc={v_f:.3e}")
    assert loc_f.dtype == torch.float32
    assert d_f <= 2.0 ** -12, d_f
    assert v_f <= GATE, v_f
