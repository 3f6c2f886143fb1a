"""GPU tests of the fp32 no-grad dispatch in ``ops.fused_edge_block`` and
``ops.fused_virtual_block``, and of FastEGNN evaluated in fp32 on the fused
fp32 kernels (csrc/fused_edge_f32.hip, csrc/fused_virtual_f32.hip)."""

import contextlib
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import Data, collate
from distegnn_amd.data.synthetic import make_cutoff_dataset
from distegnn_amd.ops import edge_reference as ER
from distegnn_amd.ops import prep
from distegnn_amd.ops import virtual_reference as VR

GATE = 2.0 ** -17
DEV = "cuda:0"
EPS = 1e-8
ISO_N, HUB, HUB_DEG = 301, 7, 200
ISOLATED = (0, 150, 300)


@pytest.fixture(autouse=True)
def _fresh_state():
    prep.clear()
    ops._FALLBACK_WARNED.clear()
    yield
    prep.clear()


@contextlib.contextmanager
def fused_disabled(disable=True):
    saved = os.environ.get("DISTEGNN_DISABLE_FUSED")
    if disable:
        os.environ["DISTEGNN_DISABLE_FUSED"] = "1"
    else:
        os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
        else:
            os.environ["DISTEGNN_DISABLE_FUSED"] = saved


@pytest.fixture
def calls(monkeypatch):
    """Counts calls of the two fp32 extension functions."""
    ext = ops.hip_ext()
    n = {"edge": 0, "virtual": 0}
    for key, name in (("edge", "fused_edge_forward_f32"),
                      ("virtual", "fused_virtual_forward_f32")):
        real = getattr(ext, name)

        def counted(*a, _real=real, _key=key, **kw):
            n[_key] += 1
            return _real(*a, **kw)

        monkeypatch.setattr(ext, name, counted)
    return n


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


# ------------------------------------------------------------ edge block
def iso_hub_graph():
    """Isolated nodes at 0, the middle and N-1, a 200-edge row at node 7."""
    g = torch.Generator().manual_seed(11)
    nodes = torch.tensor([i for i in range(ISO_N) if i not in ISOLATED])
    others = nodes[nodes != HUB]
    k = others.numel()
    hub_col = others[torch.randint(0, k, (HUB_DEG,), generator=g)]
    a = torch.randint(0, k, (150,), generator=g)
    b = (a + torch.randint(1, k, (150,), generator=g)) % k
    row = torch.cat([torch.full((HUB_DEG,), HUB), others[a]])
    col = torch.cat([hub_col, others[b]])
    bt = collate([Data(pos=torch.randn(ISO_N, 3, generator=g),
                       edge_index=torch.stack([row, col]),
                       edge_attr=torch.randn(row.numel(), 2, generator=g))])
    for i in ISOLATED:
        assert not bool((bt.edge_index == i).any())
    return bt.to(DEV)


def edge_inputs(hdim, bt, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    k_in = 2 * hdim + 3

    def t(*shape, s):
        return (torch.randn(*shape, generator=g) * s).to(DEV)

    params = [t(hdim, k_in, s=1.5 / k_in ** 0.5), t(hdim, s=0.2),
              t(hdim, hdim, s=1.5 / hdim ** 0.5), t(hdim, s=0.2),
              t(hdim, hdim, s=1.5 / hdim ** 0.5), t(hdim, s=0.2),
              t(hdim, s=0.3)]
    return t(bt.num_nodes, hdim, s=0.7), params


def edge_block(bt, h, pos, params, normalize):
    return ops.fused_edge_block(
        h, pos, bt.edge_attr, bt.edge_index[0], bt.edge_index[1], bt.rowptr,
        bt.colptr, bt.col_perm, *params, normalize, EPS)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
def test_edge_block_no_grad_takes_fp32_kernel(hdim, normalize, calls,
                                              capsys):
    bt = iso_hub_graph()
    h, params = edge_inputs(hdim, bt)
    # parameters that require grad, as a model's do: no_grad decides
    params = [p.requires_grad_(True) for p in params]
    with fused_disabled(False), torch.no_grad():
        agg_msg, agg_trans = edge_block(bt, h, bt.pos, params, normalize)
    assert calls["edge"] == 1
    assert "fused_edge_block" not in capsys.readouterr().out
    assert agg_msg.dtype == torch.float32 and agg_msg.shape == (ISO_N, hdim)
    assert agg_trans.dtype == torch.float32 and agg_trans.shape == (ISO_N, 3)
    assert not agg_msg.requires_grad and not agg_trans.requires_grad
    want_msg, want_trans = ER.edge_block_mean(
        h.double(), bt.pos.double(), bt.edge_attr.double(),
        bt.edge_index[0], bt.edge_index[1],
        *[p.detach().double() for p in params], normalize,
        float(torch.tensor(EPS, dtype=torch.float32)))
    e_msg, e_trans = rel_l2(agg_msg, want_msg), rel_l2(agg_trans, want_trans)
    print(f"DISPATCH edge H={hdim} norm={int(normalize)} "
          f"agg_msg={e_msg:.3e} agg_trans={e_trans:.3e}")
    assert e_msg <= GATE and e_trans <= GATE
    for i in ISOLATED:
        assert bool((agg_msg[i] == 0).all()) and bool((agg_trans[i] == 0).all())


def test_edge_block_grad_free_inputs_take_fp32_kernel_with_grad_mode_on(
        calls):
    """Grad mode on but nothing requires grad: no gradient is needed."""
    bt = iso_hub_graph()
    h, params = edge_inputs(64, bt)
    with fused_disabled(False):
        edge_block(bt, h, bt.pos, params, True)
    assert calls["edge"] == 1


def test_edge_block_disable_env_takes_eager(calls, capsys):
    bt = iso_hub_graph()
    h, params = edge_inputs(64, bt)
    with fused_disabled(True), torch.no_grad():
        eager = edge_block(bt, h, bt.pos, params, True)
    assert calls["edge"] == 0
    assert "fused_edge_block" not in capsys.readouterr().out
    with fused_disabled(False), torch.no_grad():
        fused = edge_block(bt, h, bt.pos, params, True)
    assert calls["edge"] == 1
    for a, b in zip(fused, eager):
        assert rel_l2(a, b.double()) <= 2 * GATE


def test_weight_copies_follow_updates_without_refresh(calls):
    """The fragment-order weight copies are cached per weight version. They
    are outside ``prep.refresh`` (a training step must not pay for what an
    evaluation left behind), so the next fp32 call itself must pick up an
    in-place weight update."""
    bt = iso_hub_graph()
    h, params = edge_inputs(64, bt)
    with fused_disabled(False), torch.no_grad():
        before = edge_block(bt, h, bt.pos, params, True)
        assert any(k[1] == "frag16_f32" for k in prep._CACHE)
        params[0].mul_(0.5)
        params[2].add_(0.01)
        assert not prep.any_stale() and prep.refresh() == 0
        after = edge_block(bt, h, bt.pos, params, True)
    assert calls["edge"] == 2
    assert not torch.equal(before[0], after[0])
    want = ER.edge_block_mean(
        h.double(), bt.pos.double(), bt.edge_attr.double(),
        bt.edge_index[0], bt.edge_index[1], *[p.double() for p in params],
        True, float(torch.tensor(EPS, dtype=torch.float32)))
    assert rel_l2(after[0], want[0]) <= GATE
    assert rel_l2(after[1], want[1]) <= GATE


def test_edge_block_with_grad_takes_eager_and_differentiates(calls, capsys):
    bt = iso_hub_graph()
    h, params = edge_inputs(64, bt)
    h = h.requires_grad_(True)
    params = [p.requires_grad_(True) for p in params]
    with fused_disabled(False):
        agg_msg, agg_trans = edge_block(bt, h, bt.pos, params, True)
        grads = torch.autograd.grad(
            agg_msg.pow(2).sum() + agg_trans.pow(2).sum(), [h] + params)
    assert calls["edge"] == 0
    assert "forward-only" in capsys.readouterr().out
    for g, t in zip(grads, [h] + params):
        assert g.shape == t.shape and bool(torch.isfinite(g).all())
        assert float(g.abs().max()) > 0


def test_edge_block_unsupported_width_names_the_width(calls, capsys):
    bt = iso_hub_graph()
    h, params = edge_inputs(48, bt)
    with fused_disabled(False), torch.no_grad():
        edge_block(bt, h, bt.pos, params, False)
    assert calls["edge"] == 0
    assert "hidden_nf=48" in capsys.readouterr().out


# --------------------------------------------------------- virtual block
def virtual_inputs(hd, n, c, seed=0):
    g = torch.Generator().manual_seed(400 + seed)

    def t(*shape, s):
        return (torch.randn(*shape, generator=g) * s).to(DEV)

    k_in = 2 * hd + 1 + c
    params = [t(hd, k_in, s=1.5 / k_in ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2), t(hd, s=0.3),
              t(hd, hd, s=1.5 / hd ** 0.5), t(hd, s=0.2), t(hd, s=0.3)]
    data = [t(n, hd, s=0.7), t(n, 3, s=1.0), t(2, c, 3, s=1.0),
            t(2, c, hd, s=0.7), t(2, c, c, s=0.5)]
    batch = torch.cat([torch.zeros(n // 2, dtype=torch.long),
                       torch.ones(n - n // 2, dtype=torch.long)]).to(DEV)
    ptr = torch.tensor([0, n // 2, n], dtype=torch.long, device=DEV)
    return data, batch, ptr, params


@pytest.mark.parametrize("hd,c", [(32, 3), (64, 8), (128, 1)])
def test_virtual_block_no_grad_takes_fp32_kernel(hd, c, calls, capsys):
    n = 333
    data, batch, ptr, params = virtual_inputs(hd, n, c)
    params = [p.requires_grad_(True) for p in params]
    with fused_disabled(False), torch.no_grad():
        outs = ops.fused_virtual_block(*data, batch, ptr, None, *params)
    assert calls["virtual"] == 1
    assert "fused_virtual_block" not in capsys.readouterr().out
    want = VR.virtual_block(*[t.double() for t in data], batch,
                            *[p.detach().double() for p in params])
    for name, a, b, w in zip(("vmsg", "tv", "tx"), outs, want,
                             (hd, 3, 3)):
        assert a.shape == (n, c, w) and a.dtype == torch.float32, name
        assert rel_l2(a, b) <= GATE, name
    with fused_disabled(True), torch.no_grad():
        ops.fused_virtual_block(*data, batch, ptr, None, *params)
    assert calls["virtual"] == 1
    assert "fused_virtual_block" not in capsys.readouterr().out


def test_virtual_block_with_grad_takes_eager_and_differentiates(calls,
                                                                capsys):
    data, batch, ptr, params = virtual_inputs(64, 50, 3)
    data[0] = data[0].requires_grad_(True)
    params = [p.requires_grad_(True) for p in params]
    with fused_disabled(False):
        vmsg, tv, tx = ops.fused_virtual_block(*data, batch, ptr, None,
                                               *params)
        grads = torch.autograd.grad(
            vmsg.pow(2).sum() + tv.pow(2).sum() + tx.pow(2).sum(),
            [data[0]] + params)
    assert calls["virtual"] == 0
    assert "forward-only" in capsys.readouterr().out
    for g in grads:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_virtual_block_too_many_channels_names_them(calls, capsys):
    data, batch, ptr, params = virtual_inputs(64, 20, 9)
    with fused_disabled(False), torch.no_grad():
        ops.fused_virtual_block(*data, batch, ptr, None, *params)
    assert calls["virtual"] == 0
    assert "virtual_channels=9" in capsys.readouterr().out


# --------------------------------------------------------------- in model
_BATCH = {}


def model_batches():
    if not _BATCH:
        _BATCH["cpu"] = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                                    n_override=1200))
        _BATCH["gpu"] = collate(make_cutoff_dataset(
            "Water-3D", 2, seed=3, n_override=1200)).to(DEV)
    return _BATCH["cpu"], _BATCH["gpu"]


def run_model(m, bt, cast=None):
    f = (lambda t: t.to(cast)) if cast is not None else (lambda t: t)
    kw = dict(edge_attr=f(bt.edge_attr), rowptr=bt.rowptr, ptr=bt.ptr,
              counts=f(bt.counts), colptr=getattr(bt, "colptr", None),
              col_perm=getattr(bt, "col_perm", None))
    with torch.no_grad():
        return m(f(bt.x), f(bt.pos), f(bt.vel), f(bt.loc_mean),
                 bt.edge_index, bt.batch, **kw)


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_in_model_fp32_eval(hd, calls, capsys):
    """FastEGNN (L=4, C=3) under no_grad in fp32: the GPU run on the fused
    fp32 kernels and the GPU eager run against a CPU float64 copy. The
    displacement loc_pred - pos (|disp|/|pos| is 0.004 to 0.008, so fp32
    rounding of the position itself puts a CPU fp32 model at 1.1e-5 to
    2.3e-5) within 2^-12; virtual_loc (CPU fp32: about 4e-8) within 2^-17.
    One bf16 rounding inside a block would give >= 1e-3."""
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt_cpu, bt = model_batches()
    assert bt.num_nodes == 2400
    m = FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2,
                 hidden_nf=hd, virtual_channels=3, world_size=1, n_layers=4)
    loc64, vloc64 = run_model(copy.deepcopy(m).double(), bt_cpu,
                              cast=torch.float64)
    assert loc64.dtype == torch.float64
    disp64 = loc64 - bt_cpu.pos.double()
    mg = copy.deepcopy(m).to(DEV)
    with fused_disabled(False):
        loc_f, vloc_f = run_model(mg, bt)
    assert calls["edge"] == 4 and calls["virtual"] == 4
    out = capsys.readouterr().out
    assert "fused_edge_block" not in out and "fused_virtual_block" not in out
    with fused_disabled(True):
        loc_e, vloc_e = run_model(mg, bt)
    assert calls["edge"] == 4 and calls["virtual"] == 4
    pos = bt_cpu.pos.double()
    d_f = rel_l2(loc_f.cpu().double() - pos, disp64)
    d_e = rel_l2(loc_e.cpu().double() - pos, disp64)
    v_f = rel_l2(vloc_f.cpu(), vloc64)
    v_e = rel_l2(vloc_e.cpu(), vloc64)
    print(f"MODEL fp32 eval H={hd} disp fused={d_f:.3e} eager={d_e:.3e}  "
          f"virtual_loc fused={v_f:.3e} eager={v_e:.3e}")
    assert loc_f.dtype == torch.float32
    assert d_f <= 2.0 ** -12, d_f
    assert v_f <= GATE, v_f
