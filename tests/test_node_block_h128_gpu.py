"""GPU tests of the fused node block at hidden_nf = 128
(csrc/fused_node_h128.hip), with the cases, the float64 reference and the
format-derived bounds of tests/test_node_block_gpu.py (``_Case`` and
``_check`` are imported unchanged: the entry points and the prepped lists
are the same at every width, and the bounds do not depend on the order of a
sum, so the other mapping of this width changes nothing in them).

What is different at this width and is therefore aimed at here:

* the four waves of a block split the output COLUMNS and share one 64-row
  tile, so the sizes walk every 16-row subtile edge and the 64-row block
  edge (N = 31, 32, 33 cost nothing and cover a 32-row tile as well);
* the weights are read from global memory, K step by K step with two steps
  in flight: A = 0 walks 12 steps (K1 = 384), A = 2 and A = 8 walk 13 with
  a zero-padded tail (386 and 392 -> 416). W1 is not streamed through LDS
  slabs, so there is no slab boundary to hit;
* a block writes one partial row, each wave its own columns, and phiv is
  folded over the waves through LDS.
"""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from test_edge_block_gpu import DEV  # noqa: E402
from test_node_block_gpu import (  # noqa: E402
    _block_grads, _Case, _check, _mlps, _rel)

from distegnn_amd import ops  # noqa: E402
from distegnn_amd.ops import prep  # noqa: E402

H = 128
# from the launch code of csrc/fused_node_h128.hip: TILE rows per block and
# trip, grid capped at GRID_CAP blocks (256 CUs x 2 resident blocks)
TILE = 64
GRID_CAP = 512


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


@pytest.fixture(autouse=True)
def _clean_env():
    keys = ("DISTEGNN_DISABLE_FUSED", "DISTEGNN_NODE_EAGER")
    old = {k: os.environ.pop(k, None) for k in keys}
    ops._FALLBACK_WARNED.clear()
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


# ------------------------------------------------------------------ stages
MODES = {"a0": (0, False), "a2": (2, False), "vel": (0, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 17, 31, 32, 33, 63, 64, 65, 563])
def test_node_h128_stages(n, mode):
    a, vo = MODES[mode]
    _check(_Case(n, H, a, vel_only=vo), f"node n={n} H={H} {mode}")


def test_node_h128_stages_a8():
    """The widest attribute tail: K1 = 392, eight attribute-column sums per
    lane and column tile."""
    _check(_Case(65, H, 8), f"node n=65 H={H} a8")


def test_node_h128_zero_dphiv():
    """dphiv = 0: the vel chain contributes exact zeros (bound 0)."""
    R = _check(_Case(563, H, 2, seed=1, zero_dphiv=True),
               f"node dphiv=0 H={H}")
    assert R["bwd.dzv"] == 0.0 and R["gwv2"] == 0.0 and R["gbv1"] == 0.0


def test_node_h128_zero_dh_out():
    """dh_out = 0: dz1, dagg_e, dagg_v and the node-chain sums are exact
    zeros, dh is the vel chain's alone."""
    R = _check(_Case(563, H, 2, seed=2, zero_dh_out=True),
               f"node dh_out=0 H={H}")
    for k in ("bwd.dz1", "bwd.dagg_e", "bwd.dagg_v", "gb1", "gb2",
              "gw1_tail"):
        assert R[k] == 0.0, k


@pytest.mark.parametrize("mode", ["a2", "vel"])
def test_node_h128_second_tile_trip(mode):
    """N = 512*64 + 645: blocks 0..10 walk a second tile. The cotangents
    live only on second-trip rows, so a dropped tile would take every term
    of the sums and every nonzero row of the data gradients."""
    a, vo = MODES[mode]
    n = GRID_CAP * TILE + 645
    live = torch.zeros(n, device=DEV)
    live[GRID_CAP * TILE:] = 1
    _check(_Case(n, H, a, seed=3, live=live, vel_only=vo),
           f"node second_trip H={H} {mode}")


# ------------------------------------------------------------ repeatability
def _copy_params(c, node_mlp, vel_mlp):
    with torch.no_grad():
        for k, p in zip(("w1", "b1", "w2", "b2"), node_mlp.parameters()):
            p.copy_(c.P[k])
        for k, p in zip(("wv1", "bv1", "wv2", "bv2"), vel_mlp.parameters()):
            p.copy_(c.P[k].view(p.shape))


def test_node_h128_kernels_repeatable():
    """Two direct calls of each kernel: both forward and all seven backward
    outputs (the partial rows included, before their sum) are bit-equal."""
    c = _Case(563, H, 2, seed=4)
    (f1, b1, p1), (f2, b2, p2) = c.run(), c.run()
    for i, (x, y) in enumerate(zip(list(f1) + list(b1) + [p1],
                                   list(f2) + list(b2) + [p2])):
        assert torch.equal(x, y), f"output {i} differs between two calls"


def test_node_h128_autograd_repeatable():
    """Through ``ops.fused_node_block`` and autograd, twice: every gradient
    is bit-equal. The data gradients, the bias / head gradients and the
    attribute columns of dW1 come from the kernel; the 128-wide matrix
    gradients come from the library split-K path (``chunked_wgrad`` at
    O = 128), which was bit-repeatable on the MI355X when this test was
    written, so they are held to the same equality."""
    a = 2
    c = _Case(563, H, a, seed=4)
    node_mlp, vel_mlp = _mlps(H, a)
    _copy_params(c, node_mlp, vel_mlp)
    _, g1 = _block_grads(c, node_mlp, vel_mlp)
    _, g2 = _block_grads(c, node_mlp, vel_mlp)
    names = ["dh", "dagg_e", "dagg_v", "gw1", "gb1", "gw2", "gb2", "gwv1",
             "gbv1", "gwv2", "gbv2"]
    library = {"gw2", "gwv1"}
    for k, x, y in zip(names, g1, g2):
        if k == "gw1":
            assert torch.equal(x[:, 3 * H:], y[:, 3 * H:]), \
                "dW1 attribute columns differ between two calls"
            same = torch.equal(x[:, :3 * H], y[:, :3 * H])
            print(f"H128 repeat gw1[:, :3H] (library) equal={same}")
            assert same, "gw1[:, :3H] differs between two calls"
        else:
            same = torch.equal(x, y)
            if k in library:
                print(f"H128 repeat {k} (library) equal={same}")
            assert same, f"{k} differs between two calls"


# ---------------------------------------------------------------- dispatch
@pytest.fixture
def eager_calls(monkeypatch):
    calls = []
    real = ops.eager_node_block

    def spy(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(ops, "eager_node_block", spy)
    return calls


def test_dispatch_h128_is_fused(eager_calls, capsys):
    c = _Case(200, H, 2, seed=5)
    node_mlp, vel_mlp = _mlps(H, 2)
    (h_out, phiv), _ = _block_grads(c, node_mlp, vel_mlp)
    assert not eager_calls
    assert phiv.dtype == torch.float32 and h_out.dtype == torch.bfloat16
    assert "fused_node_block" not in capsys.readouterr().out
    # vel-only returns h itself
    h = c.h.bfloat16()
    h2, pv = ops.fused_node_block(h, None, None, None, node_mlp, vel_mlp,
                                  True, vel_only=True)
    assert h2 is h and not eager_calls
    assert torch.equal(pv, phiv)
    # N = 0
    e_out, e_phiv = ops.fused_node_block(h[:0], h[:0], h[:0], None,
                                         *_mlps(H, 0), True)
    assert e_out.shape == (0, H) and e_phiv.shape == (0, 1)
    assert not eager_calls
    assert "fused_node_block" not in capsys.readouterr().out


@pytest.mark.parametrize("var", ["DISTEGNN_DISABLE_FUSED",
                                 "DISTEGNN_NODE_EAGER"])
def test_dispatch_h128_switches_reach_the_composition(var, eager_calls,
                                                      capsys):
    c = _Case(100, H, 2, seed=8)
    node_mlp, vel_mlp = _mlps(H, 2, dtype=torch.bfloat16)
    os.environ[var] = "1"
    (h_out, phiv), _ = _block_grads(c, node_mlp, vel_mlp)
    assert len(eager_calls) == 1 and phiv.dtype == torch.bfloat16
    assert "fused_node_block" not in capsys.readouterr().out


# ---------------------------------------------------------------- in model
def test_in_model_h128_fused_matches_node_eager():
    """FastEGNN (two graphs, 200 nodes, H = 128, C = 3, node_attr_nf = 2,
    4 layers) under bf16 autocast: the fused node block against
    DISTEGNN_NODE_EAGER=1, forward outputs and every parameter gradient,
    within the project's in-model relative L2 of 0.02."""
    from distegnn_amd.data.graph import collate
    from distegnn_amd.data.synthetic import make_cutoff_dataset
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                     n_override=100)).to(DEV)
    assert bt.num_nodes == 200
    m = FastEGNN(node_feat_nf=2, node_attr_nf=2, edge_attr_nf=2,
                 hidden_nf=H, virtual_channels=3, world_size=1,
                 n_layers=4).to(DEV)
    g = torch.Generator().manual_seed(1)
    node_attr = torch.randn(bt.num_nodes, 2, generator=g).to(DEV)
    target = bt.pos + 0.01 * torch.randn(bt.pos.shape, generator=g).to(DEV)

    def run(eager):
        if eager:
            os.environ["DISTEGNN_NODE_EAGER"] = "1"
        else:
            os.environ.pop("DISTEGNN_NODE_EAGER", None)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loc, vloc = m(bt.x, bt.pos, bt.vel, bt.loc_mean, bt.edge_index,
                          bt.batch, edge_attr=bt.edge_attr,
                          node_attr=node_attr, rowptr=bt.rowptr, ptr=bt.ptr,
                          counts=bt.counts, colptr=bt.colptr,
                          col_perm=bt.col_perm)
        loss = (loc - target).pow(2).mean() + vloc.pow(2).mean() * 1e-3
        loss.backward()
        os.environ.pop("DISTEGNN_NODE_EAGER", None)
        return (loc.detach(), vloc.detach(),
                {k: p.grad.clone() for k, p in m.named_parameters()
                 if p.grad is not None})

    loc_f, vloc_f, g_f = run(False)
    loc_e, vloc_e, g_e = run(True)
    assert set(g_f) == set(g_e)
    rels = {"loc": _rel(loc_f, loc_e), "vloc": _rel(vloc_f, vloc_e)}
    for k in g_e:
        if float(g_e[k].abs().max()) == 0.0:
            assert float(g_f[k].abs().max()) == 0.0, k
            continue
        rels[k] = _rel(g_f[k], g_e[k])
    worst = sorted(rels.items(), key=lambda kv: -kv[1])[:5]
    print("MODEL node H=128 fused vs eager, worst rel L2:",
          " ".join(f"{k}={v:.3e}" for k, v in worst))
    bad = {k: v for k, v in rels.items() if not v < 0.02}
    assert not bad, bad


# ----------------------------------------------------------------- capture
def test_capture_replay_h128_reads_refreshed_weights():
    """Forward + backward captured with torch.cuda.graph; the weights then
    change in place and ``ops.refresh_weight_prep()`` runs. The replay must
    equal an eager call on the new weights, bit for bit: everything the
    kernels produce, and the library's matrix gradients as well (repeatable
    here, see ``test_node_h128_autograd_repeatable``). A prep kind left out
    of ``refresh`` would replay the old weights."""
    a = 2
    c = _Case(300, H, a, seed=9)
    node_mlp, vel_mlp = _mlps(H, a, seed=2)
    params = list(node_mlp.parameters()) + list(vel_mlp.parameters())
    bf = torch.bfloat16
    ins = [t.to(bf).requires_grad_() for t in (c.h, c.agg_e, c.agg_v)]
    attr = c.attr.to(bf)
    dh_out, dphiv = c.dh_out.to(bf), c.dphiv.clone()

    def step():
        h_out, phiv = ops.fused_node_block(ins[0], ins[1], ins[2], attr,
                                           node_mlp, vel_mlp, True)
        return [h_out, phiv] + list(torch.autograd.grad(
            [h_out, phiv], ins + params, [dh_out, dphiv]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    old = [t.clone() for t in static]
    with torch.no_grad():
        for i, p in enumerate(params):
            p.mul_(1.25 + 0.125 * i)
    assert ops.refresh_weight_prep() > 0
    graph.replay()
    torch.cuda.synchronize()
    new = step()
    assert not torch.equal(old[0], static[0])
    for i, (x, y) in enumerate(zip(static, new)):
        assert torch.equal(x, y), f"output {i}: replay differs from eager"
