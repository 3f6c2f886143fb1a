"""GPU tests of the forward-only fp32 edge kernel (csrc/fused_edge_f32.hip)
and of the f32 MFMA operand layout it rests on.

Structure test: every element of msg against the float64
``edge_reference.edge_forward`` under a worst-case bound, u = 2^-23, ``mag``
= the same product over absolute values:

  a1 = (2(K_IN+1)+8) u mag1            fp32 accumulation of K_IN products and
                                       the bias; +8 for r2's own roundings
  e1 = 1.1 a1 + 2u|z1||t1| + u|t1|     silu stretches by <= 1.1; the fast
                                       exponential; the final division
  a2 = e1 |W2|^T + 2(H+1) u mag2       mag2 = (|t1|+e1)|W2|^T + |b2|
  e2 = 1.1 a2 + 2u|z2||msg| + u|msg|

trans is judged from the kernel's own msg under the ``forward_trans`` bound
of test_edge_block_gpu.py, u |d inv| (4(H+2) mag_p + 2 fx); a bound of 0
requires an error of 0. A plain fp32 CPU run of these stages stays below
0.3 % of the bounds, so this test catches wrong rows, columns, terms and
tiles, not lost precision. The precision test does that: relative L2 error
against float64 at most 2^-17 (a sequential fp32 fmaf chain gives 1.8e-7 to
5.2e-7, one bf16 rounding of t1 or msg 7e-4 to 3.6e-3).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires GPU", allow_module_level=True)

from distegnn_amd import ops
from distegnn_amd.data.graph import Data, collate
from distegnn_amd.ops import edge_reference as ER

U = 2.0 ** -23
GATE = 2.0 ** -17
DEV = "cuda:0"
EPS = float(torch.tensor(1e-8, dtype=torch.float32))
TILE = 64
GRID_CAP = 4096      # csrc/fused_edge_f32.hip


# ------------------------------------------------------------------ probe
def _probe(a, b):
    """a [16,4], b [4,16] exact small integers -> probe result, A @ B."""
    got = ops.hip_ext().mfma_probe_f32(a.to(DEV), b.t().contiguous().to(DEV))
    return got.cpu(), a.double() @ b.double()


def test_probe_identity_against_asymmetric_b():
    a = torch.zeros(16, 4)
    a[:4, :4] = torch.eye(4)
    b = (torch.arange(64, dtype=torch.float32).view(4, 16) * 3 - 50)
    got, want = _probe(a, b)
    assert torch.equal(got.double(), want)
    # rows 0..3 of D are rows 0..3 of B: k and column order both visible
    assert torch.equal(got[:4], b) and bool((got[4:] == 0).all())


def test_probe_general_asymmetric_pair():
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-9, 10, (16, 4), generator=g).float()
    b = torch.randint(-9, 10, (4, 16), generator=g).float()
    a[3, 1], b[2, 11] = 17.0, -13.0
    assert not torch.equal(a @ b, (a @ b).t())
    got, want = _probe(a, b)
    assert torch.equal(got.double(), want)


def test_probe_rejects_other_shapes():
    with pytest.raises(RuntimeError, match=r"\[16,4\]"):
        ops.hip_ext().mfma_probe_f32(torch.zeros(16, 8, device=DEV),
                                     torch.zeros(16, 8, device=DEV))


# ------------------------------------------------------------------ inputs
def make_params(hdim, seed):
    """fp32, not rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    k_in = 2 * hdim + 3
    w1 = torch.randn(hdim, k_in, generator=g) * 1.5 / k_in ** 0.5
    b1 = torch.randn(hdim, generator=g) * 0.2
    w2 = torch.randn(hdim, hdim, generator=g) * 1.5 / hdim ** 0.5
    b2 = torch.randn(hdim, generator=g) * 0.2
    w3 = torch.randn(hdim, hdim, generator=g) * 1.5 / hdim ** 0.5
    b3 = torch.randn(hdim, generator=g) * 0.2
    w3v = torch.randn(hdim, generator=g) * 0.3
    return [t.to(DEV) for t in (w1, b1, w2, b2, w3, b3, w3v)]


def _graph(n, row, col, seed, pos=None):
    g = torch.Generator().manual_seed(seed)
    if pos is None:
        pos = torch.randn(n, 3, generator=g)
    m = row.numel()
    return collate([Data(pos=pos, edge_index=torch.stack([row, col]),
                         edge_attr=torch.randn(m, 2, generator=g))])


def _random_edges(nodes, m, g):
    k = nodes.numel()
    a = torch.randint(0, k, (m,), generator=g)
    b = (a + torch.randint(1, k, (m,), generator=g)) % k
    return nodes[a], nodes[b]


def graph_random(m, n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + m)
    row, col = _random_edges(torch.arange(n), m, g)
    return _graph(n, row, col, seed + m)


HUB, HUB_DEG, ISO_N = 7, 200, 301
ISOLATED = (0, 150, 300)


def graph_iso_hub():
    """Isolated nodes at 0, in the middle and at N-1; node 7 is the row of
    200 edges; 150 more edges elsewhere."""
    g = torch.Generator().manual_seed(11)
    nodes = torch.tensor([i for i in range(ISO_N) if i not in ISOLATED])
    others = nodes[nodes != HUB]
    hub_col = others[torch.randint(0, others.numel(), (HUB_DEG,),
                                   generator=g)]
    row, col = _random_edges(others, 150, g)
    bt = _graph(ISO_N, torch.cat([torch.full((HUB_DEG,), HUB), row]),
                torch.cat([hub_col, col]), 12)
    for i in ISOLATED:
        assert not bool((bt.edge_index == i).any())
    assert int((bt.edge_index[0] == HUB).sum()) == HUB_DEG
    return bt


def graph_one_col():
    g = torch.Generator().manual_seed(13)
    row = torch.randint(0, 49, (150,), generator=g)
    return _graph(50, row, torch.full((150,), 49), 14)


COINC = (3, 4)


def graph_coincident():
    """Nodes 3 and 4 share a position; exactly one edge (3 -> 4) joins
    them, so that edge has r2 = 0."""
    g = torch.Generator().manual_seed(15)
    pos = torch.randn(10, 3, generator=g)
    pos[4] = pos[3]
    row, col = _random_edges(torch.arange(10), 60, g)
    keep = ~(((row == 3) & (col == 4)) | ((row == 4) & (col == 3)))
    row = torch.cat([row[keep], torch.tensor([COINC[0]])])
    col = torch.cat([col[keep], torch.tensor([COINC[1]])])
    return _graph(10, row, col, 16, pos=pos)


TILE_BOUNDARY_M = [1, 15, 16, 17, 63, 64, 65, 128]
TILE_COUNTS = [7, 8, 9, 15, 16, 17]
PAST_CAP_M = GRID_CAP * TILE + TILE * 10 + 5

GRAPHS = {}
for _m in TILE_BOUNDARY_M:
    GRAPHS[f"M{_m}"] = (lambda m=_m: graph_random(m, 24))
for _t in TILE_COUNTS:
    GRAPHS[f"tiles{_t}"] = (lambda t=_t: graph_random(TILE * t - 13, 97))
GRAPHS["iso_hub"] = graph_iso_hub
GRAPHS["one_col"] = graph_one_col
GRAPHS["coincident"] = graph_coincident


class _Case:
    def __init__(self, bt, hdim, normalize, seed=0):
        self.bt = bt.to(DEV)
        self.hdim, self.normalize = hdim, bool(normalize)
        self.n, self.m = bt.num_nodes, bt.num_edges
        self.row, self.col = self.bt.edge_index[0], self.bt.edge_index[1]
        g = torch.Generator().manual_seed(100 + seed)
        self.h = (torch.randn(self.n, hdim, generator=g) * 0.7).to(DEV)
        self.params = make_params(hdim, 200 + seed)

    def args(self):
        return (self.h, self.bt.pos, self.bt.edge_attr, self.row, self.col,
                *self.params, self.normalize, EPS)

    def forward(self):
        return ops.hip_ext().fused_edge_forward_f32(*self.args())

    def reference(self):
        return ER.edge_forward(
            self.h.double(), self.bt.pos.double(),
            self.bt.edge_attr.double(), self.row, self.col,
            *[p.double() for p in self.params], self.normalize, EPS)


# ------------------------------------------------------------------ bounds
def msg_bound(c, ref):
    H = c.hdim
    k_in = 2 * H + 3
    W1, b1, W2, b2 = [p.double() for p in c.params[:4]]
    mag1 = ref["ein"].abs() @ W1.abs().t() + b1.abs()
    a1 = (2 * (k_in + 1) + 8) * U * mag1
    t1 = ref["t1"].abs()
    e1 = 1.1 * a1 + 2 * U * ref["z1"].abs() * t1 + U * t1
    mag2 = (t1 + e1) @ W2.abs().t() + b2.abs()
    a2 = e1 @ W2.abs().t() + 2 * (H + 1) * U * mag2
    msg = ref["msg"].abs()
    return 1.1 * a2 + 2 * U * ref["z2"].abs() * msg + U * msg


def trans_ref_and_bound(c, ref, got_msg):
    """From the kernel's own msg: p = silu(msg W3^T + b3) . w3v in fp32,
    error (3.2H+2.2) u mag_p plus the fast-exponential term 2 u fx; d inv
    carries 8 roundings, the product 1: u |d inv| (4(H+2) mag_p + 2 fx)."""
    H = c.hdim
    W3, b3, w3v = [p.double() for p in c.params[4:]]
    x = got_msg.double()
    z3 = ER.preact(x, W3, b3)
    mag3 = x.abs() @ W3.abs().t() + b3.abs()
    s3 = ER.silu(z3)
    p = s3 @ w3v
    mag_p = mag3 @ w3v.abs()
    fx = (z3.abs() * s3.abs()) @ w3v.abs()
    dn = ref["d"] * ref["inv"].unsqueeze(1)
    return (dn * p.unsqueeze(1),
            U * dn.abs() * (4 * (H + 2) * mag_p + 2 * fx).unsqueeze(1))


def worst_ratio(got, want, bound):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    err = (got.double() - want).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


def check_structure(c, title):
    msg, trans = c.forward()
    assert msg.dtype == torch.float32 and msg.shape == (c.m, c.hdim)
    assert trans.dtype == torch.float32 and trans.shape == (c.m, 3)
    ref = c.reference()
    r_msg = worst_ratio(msg, ref["msg"], msg_bound(c, ref))
    r_trans = worst_ratio(trans, *trans_ref_and_bound(c, ref, msg))
    print(f"RATIO edge_f32 {title} msg={r_msg:.4f} trans={r_trans:.4f}")
    assert r_msg <= 1.0 and r_trans <= 1.0, (title, r_msg, r_trans)
    return msg, trans, ref


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_edge_f32_structure(gname, hdim, normalize):
    c = _Case(GRAPHS[gname](), hdim, normalize)
    if gname.startswith("M"):
        assert c.m == int(gname[1:])
    if gname.startswith("tiles"):
        assert (c.m + TILE - 1) // TILE == int(gname[5:])
        assert c.m % TILE != 0
    msg, trans, ref = check_structure(
        c, f"case={gname} H={hdim} norm={int(normalize)}")
    if gname == "coincident":
        e = ((c.row == COINC[0]) & (c.col == COINC[1])).nonzero().flatten()
        assert e.numel() == 1
        assert float(ref["r2"][e]) == 0.0
        assert bool((trans[e] == 0).all())


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
def test_edge_f32_empty(hdim, normalize):
    c = _Case(graph_random(5, 24), hdim, normalize)
    empty = c.row[:0]
    msg, trans = ops.hip_ext().fused_edge_forward_f32(
        c.h, c.bt.pos, c.bt.edge_attr[:0], empty, empty, *c.params,
        c.normalize, EPS)
    assert msg.shape == (0, hdim) and msg.dtype == torch.float32
    assert trans.shape == (0, 3) and trans.dtype == torch.float32


@pytest.mark.parametrize("normalize", [False, True])
def test_edge_f32_past_grid_cap(normalize):
    """The grid is capped at 4096 blocks: with M = 4096*64 + 64*10 + 5,
    blocks 0..10 walk a second tile, the last one ragged. H = 32: the tile
    loop does not depend on H. Every row is compared, on the device."""
    m = PAST_CAP_M
    assert (m + TILE - 1) // TILE == GRID_CAP + 11 and m % TILE == 5
    c = _Case(graph_random(m, 2048), 32, normalize)
    assert c.m == m
    check_structure(c, f"case=past_cap H=32 norm={int(normalize)}")


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
def test_edge_f32_precision_class(hdim, normalize):
    c = _Case(graph_random(1000, 97), hdim, normalize, seed=1)
    msg, trans = c.forward()
    ref = c.reference()
    e_msg, e_trans = rel_l2(msg, ref["msg"]), rel_l2(trans, ref["trans"])
    # the fp32 eager composition on the GPU, for information only
    bt = c.bt
    emsg, etrans = ops.eager_edge_block(
        c.h, bt.pos, bt.edge_attr, c.row, c.col, bt.rowptr, bt.colptr,
        bt.col_perm, *c.params, c.normalize, EPS)
    print(f"PRECISION edge_f32 H={hdim} norm={int(normalize)} "
          f"msg={e_msg:.3e} trans={e_trans:.3e} "
          f"(eager fp32: msg={rel_l2(emsg, ref['msg']):.3e} "
          f"trans={rel_l2(etrans, ref['trans']):.3e})")
    assert e_msg <= GATE and e_trans <= GATE, (e_msg, e_trans)
    msg2, trans2 = c.forward()
    assert torch.equal(msg, msg2) and torch.equal(trans, trans2)


def test_edge_f32_rejects_unsupported_inputs():
    ext = ops.hip_ext()
    c = _Case(graph_random(17, 24), 64, False)
    a = list(c.args())
    with pytest.raises(RuntimeError, match="fp32"):
        ext.fused_edge_forward_f32(a[0].bfloat16(), *a[1:])
    with pytest.raises(RuntimeError, match="fp32"):          # bf16 weight
        ext.fused_edge_forward_f32(*a[:5], a[5].bfloat16(), *a[6:])
    with pytest.raises(RuntimeError, match="edge_attr_nf=2"):
        ext.fused_edge_forward_f32(*a[:2], a[2][:, :1].contiguous(), *a[3:])
    c48 = _Case(graph_random(17, 24), 48, False)
    with pytest.raises(RuntimeError, match=r"32, 64, 128"):
        ext.fused_edge_forward_f32(*c48.args())
