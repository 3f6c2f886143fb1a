"""GPU tests for the fused virtual-edge block at hidden_nf 32 and 128
(csrc/fused_virtual.hip instantiations next to the original H=64), against
the eager composition of the same math.

Every width keeps the 64-row tile of four 16-row wave sub-tiles, so the row
counts below (999 = 15 tiles + 39, 2664 = 41 tiles + 40, 5) leave a partial
tile and a partial wave sub-tile at each width."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops

WIDTHS = (32, 128)
SHAPES = ((333, 3), (333, 8), (5, 1))      # (N, C)
CASES = [(hd, n, c) for hd in WIDTHS for (n, c) in SHAPES]
PARAMS = ("w1", "b1", "w2", "b2", "wxv", "bxv", "wxvv", "wX", "bX", "wXv")


def dev():
    return torch.device("cuda:0")


def make_inputs(hd, n, c, seed=0):
    g = torch.Generator().manual_seed(seed)

    def t(*shape, s):
        return (torch.randn(*shape, generator=g) * s).to(dev())

    k_in = 2 * hd + 1 + c
    params = dict(
        w1=t(hd, k_in, s=0.1), b1=t(hd, s=0.1), w2=t(hd, hd, s=0.1),
        b2=t(hd, s=0.1), wxv=t(hd, hd, s=0.1), bxv=t(hd, s=0.1),
        wxvv=t(hd, s=0.1), wX=t(hd, hd, s=0.1), bX=t(hd, s=0.1),
        wXv=t(hd, s=0.1))
    data = dict(
        h=t(n, hd, s=0.5), coord=t(n, 3, s=1.0), vcoord=t(2, c, 3, s=1.0),
        vfeat=t(2, c, hd, s=0.5), gram=t(2, c, c, s=0.3))
    batch = torch.cat([torch.zeros(n // 2, dtype=torch.long),
                       torch.ones(n - n // 2, dtype=torch.long)]).to(dev())
    ptr = torch.tensor([0, n // 2, n], dtype=torch.long, device=dev())
    return params, data, batch, ptr


def run_block(params, data, batch, ptr, grad, mode):
    """mode: 'fused', 'eager' (bf16, DISTEGNN_DISABLE_FUSED=1) or 'fp32'
    (eager composition in fp32). Returns outputs, grads (or None) and
    whether the fused autograd node produced vmsg."""
    leaves = {k: v.detach().clone().requires_grad_(grad)
              for k, v in params.items()}
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    hh = data["h"].detach().clone().to(dt).requires_grad_(grad)
    rest = {k: data[k].detach().clone().requires_grad_(grad)
            for k in ("coord", "vcoord", "vfeat", "gram")}
    saved = os.environ.get("DISTEGNN_DISABLE_FUSED")
    if mode == "fused":
        os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
    else:
        os.environ["DISTEGNN_DISABLE_FUSED"] = "1"
    try:
        vmsg, tv, tx = ops.fused_virtual_block(
            hh, rest["coord"], rest["vcoord"], rest["vfeat"], rest["gram"],
            batch, ptr, None, *(leaves[k] for k in PARAMS))
    finally:
        if saved is None:
            os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
        else:
            os.environ["DISTEGNN_DISABLE_FUSED"] = saved
    took_kernel = (vmsg.grad_fn is not None
                   and "_FusedVirtualBlockFn" in type(vmsg.grad_fn).__name__)
    outs = (vmsg.detach().float(), tv.detach().float(), tx.detach().float())
    if not grad:
        return outs, None, took_kernel
    loss = vmsg.float().pow(2).sum() + tv.float().pow(2).sum() \
        + tx.float().pow(2).sum()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["h"] = hh.grad
    grads.update({k: v.grad for k, v in rest.items()})
    return outs, grads, took_kernel


_CACHE = {}


def arms(hd, n, c):
    """Fused and eager-bf16 arms (forward + backward), computed once per
    case and shared by the forward and backward tests."""
    key = (hd, n, c)
    if key not in _CACHE:
        inputs = make_inputs(hd, n, c)
        _CACHE[key] = (inputs,
                       run_block(*inputs, grad=True, mode="fused"),
                       run_block(*inputs, grad=True, mode="eager"))
    return _CACHE[key]


def relerr(a, b):
    return ((a.float() - b.float()).norm()
            / b.float().norm().clamp(min=1e-6)).item()


@pytest.mark.parametrize("hd,n,c", CASES)
def test_forward_matches_eager(hd, n, c):
    _, (out_f, _, fused_path), (out_e, _, eager_path) = arms(hd, n, c)
    assert fused_path, f"H={hd}: fused_virtual_block did not take the kernel"
    assert not eager_path
    (vm_f, tv_f, tx_f), (vm_e, tv_e, tx_e) = out_f, out_e
    assert vm_f.shape == (n, c, hd)
    assert tv_f.shape == tx_f.shape == (n, c, 3)
    print(f"H={hd} N={n} C={c}: vmsg max|d|={(vm_f - vm_e).abs().max():.4g}"
          f" tv rel={relerr(tv_f, tv_e):.4g} tx rel={relerr(tx_f, tx_e):.4g}")
    assert torch.allclose(vm_f, vm_e, atol=0.05, rtol=0.05), \
        (vm_f - vm_e).abs().max()
    for name, a, b in (("tv", tv_f, tv_e), ("tx", tx_f, tx_e)):
        rel = (a - b).norm() / b.norm().clamp(min=1e-9)
        assert rel < 0.05, (name, rel.item())


@pytest.mark.parametrize("hd,n,c", CASES)
def test_backward_matches_eager(hd, n, c):
    """Gate 0.08 on every gradient. At H=128 a gradient that misses it is
    compared, with the eager-bf16 one, against fp32 eager: both arms round
    the same math to bf16 at different points, so the fused arm may be at
    most 1.5x as far from fp32 as the eager-bf16 arm."""
    inputs, (_, g_f, fused_path), (_, g_e, _) = arms(hd, n, c)
    assert fused_path, f"H={hd}: fused_virtual_block did not take the kernel"
    assert set(g_e) == set(PARAMS) | {"h", "coord", "vcoord", "vfeat", "gram"}
    assert g_f["w1"].shape == (hd, 2 * hd + 1 + c)
    assert g_f["gram"].shape == (2, c, c)
    g_32 = None
    for k in sorted(g_e):
        assert g_f[k] is not None, k
        assert g_f[k].shape == g_e[k].shape, k
        rel = relerr(g_f[k], g_e[k])
        print(f"H={hd} N={n} C={c} grad {k}: rel={rel:.4g}")
        if rel < 0.08:
            continue
        assert hd == 128, (k, rel)
        if g_32 is None:
            g_32 = run_block(*inputs, grad=True, mode="fp32")[1]
        d_f, d_e = relerr(g_f[k], g_32[k]), relerr(g_e[k], g_32[k])
        print(f"  vs fp32: fused {d_f:.4g}, eager bf16 {d_e:.4g}")
        assert d_f <= 1.5 * d_e, (k, rel, d_f, d_e)


@pytest.mark.parametrize("hd", WIDTHS)
def test_direct_extension_call_inference(hd):
    ext = ops.hip_ext()
    params, data, batch, _ = make_inputs(hd, 333, 3)
    bf = {k: (v.bfloat16() if v.dim() == 2 else v) for k, v in params.items()}
    outs = ext.fused_virtual_forward(
        data["h"].bfloat16(), data["coord"], data["vcoord"],
        data["vfeat"].bfloat16(), data["gram"], batch,
        *(bf[k] for k in PARAMS), False, [])
    vmsg, tv, tx = outs[:3]
    assert vmsg.shape == (999, hd) and vmsg.dtype == torch.bfloat16
    assert tv.shape == tx.shape == (999, 3)
    assert torch.isfinite(vmsg.float()).all()
    for saved in outs[3:]:
        assert saved.size(0) == 0
    (ref, _, _), _, _ = run_block(params, data, batch, None, grad=False,
                                  mode="eager")
    assert torch.allclose(vmsg.float().view(333, 3, hd), ref,
                          atol=0.05, rtol=0.05)


def test_direct_extension_call_rejects_other_widths():
    ext = ops.hip_ext()
    params, data, batch, _ = make_inputs(48, 20, 3)
    bf = {k: (v.bfloat16() if v.dim() == 2 else v) for k, v in params.items()}
    with pytest.raises(RuntimeError, match=r"32, 64, 128"):
        ext.fused_virtual_forward(
            data["h"].bfloat16(), data["coord"], data["vcoord"],
            data["vfeat"].bfloat16(), data["gram"], batch,
            *(bf[k] for k in PARAMS), False, [])


def test_no_fallback_warning_for_compiled_widths(capsys):
    for hd in WIDTHS:
        inputs = make_inputs(hd, 5, 1)
        run_block(*inputs, grad=False, mode="fused")
    assert "fused_virtual_block" not in capsys.readouterr().out


_MODEL_REF = {}


def model_batches():
    from distegnn_amd.data.graph import collate
    from distegnn_amd.data.synthetic import make_cutoff_dataset

    if "bt" not in _MODEL_REF:
        bt_cpu = collate(make_cutoff_dataset("Water-3D", 2, seed=3,
                                             n_override=1200))
        _MODEL_REF["bt"] = (bt_cpu, collate(make_cutoff_dataset(
            "Water-3D", 2, seed=3, n_override=1200)).to(dev()))
    return _MODEL_REF["bt"]


@pytest.mark.parametrize("hd", WIDTHS)
def test_in_model_matches_cpu(hd):
    """FastEGNN (GPU bf16 autocast) with the fused blocks and with
    DISTEGNN_DISABLE_FUSED=1, each against the CPU fp32 forward: the fused
    arm's distance d_f must satisfy d_f <= max(0.02, 1.5 * d_e)."""
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    bt_cpu, bt = model_batches()
    m = FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2,
                 hidden_nf=hd, virtual_channels=3, world_size=1, n_layers=2)
    with torch.no_grad():
        loc_c, vloc_c = m(bt_cpu.x, bt_cpu.pos, bt_cpu.vel, bt_cpu.loc_mean,
                          bt_cpu.edge_index, bt_cpu.batch,
                          edge_attr=bt_cpu.edge_attr, rowptr=bt_cpu.rowptr,
                          ptr=bt_cpu.ptr, counts=bt_cpu.counts)
    mg = m.to(dev())

    def gpu_forward(disable):
        saved = os.environ.get("DISTEGNN_DISABLE_FUSED")
        if disable:
            os.environ["DISTEGNN_DISABLE_FUSED"] = "1"
        else:
            os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
        try:
            with torch.no_grad(), \
                    torch.autocast("cuda", dtype=torch.bfloat16):
                loc, vloc = mg(bt.x, bt.pos, bt.vel, bt.loc_mean,
                               bt.edge_index, bt.batch,
                               edge_attr=bt.edge_attr, rowptr=bt.rowptr,
                               ptr=bt.ptr, counts=bt.counts,
                               colptr=bt.colptr, col_perm=bt.col_perm)
        finally:
            if saved is None:
                os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
            else:
                os.environ["DISTEGNN_DISABLE_FUSED"] = saved
        return loc.float().cpu(), vloc.float().cpu()

    fused = gpu_forward(False)
    eager = gpu_forward(True)
    for name, ref, a_f, a_e in (("loc", loc_c, fused[0], eager[0]),
                                ("virtual_loc", vloc_c, fused[1], eager[1])):
        d_f = ((a_f - ref).norm() / ref.norm()).item()
        d_e = ((a_e - ref).norm() / ref.norm()).item()
        print(f"H={hd} {name}: d_f={d_f:.4g} d_e={d_e:.4g}")
        assert d_f <= max(0.02, 1.5 * d_e), (name, d_f, d_e)
