"""GPU tests of the fused edge kernels (csrc/fused_edge.hip,
csrc/fused_edge_bwd.hip), one emitted tensor at a time.

Every stage is judged against a float64 reference of that ONE stage
(distegnn_amd/ops/edge_reference.py, itself checked on the CPU against
autograd), computed from the kernel's own output of the stage before, so a
check covers exactly one rounding step. The bounds come from the number
formats (u23 = 2^-23, u8 = 2^-8 = the bf16 unit roundoff, ``mag`` = the same
product over absolute values); each is derived where it is formed, in
``_Stages``. Every test prints its worst err/bound per stage;
docs/KERNELS.md ("Edge-path test bounds") records the measured values.

Building blocks of the bounds:

* fp32 MFMA accumulation of K bf16 products plus a bias: 2(K+1)*u23*mag
  (as in the linear-path tests).
* a pre-activation z that the backward stores as bf16 before the SiLU:
  |z_stored - z| <= zerr = u8*|z| + 2(K+1)*u23*mag.
* silu' lies in [-0.1, 1.1] and |silu''| <= 0.5, so an error e in z moves
  silu(z) by at most 1.1*e and silu'(z) by at most 0.5*e.
* the kernels' SiLU uses the fast exponential: exp(-z) carries a relative
  error of about (1 + |z|/2)*u23, silu(z) inherits at most that, relatively.
  Against a bf16 result that is absorbed by doubling the accumulation term;
  against an fp32 result it is the explicit term 2*u23*|z|*|silu(z)|.
  silu'(z) = s(1 + z(1-s)) then has an absolute error of at most
  6*u23*(1+|z|)^2.
"""

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

U23 = 2.0 ** -23
U8 = 2.0 ** -8
DEV = "cuda:0"
# the value the kernels see: eps is passed to them as an fp32 scalar
EPS = float(torch.tensor(1e-8, dtype=torch.float32))
TILE = 64
GRID_CAP = 16384


@pytest.fixture(scope="module", autouse=True)
def _fresh_weight_cache():
    prep.clear()
    yield
    prep.clear()


# ------------------------------------------------------------------ inputs
def _bf(t):
    """Round to bf16 values, keep fp32 storage."""
    return t.bfloat16().float()


def make_params(hdim, seed, round_all=False):
    """fp32 tensors; the three weight matrices hold bf16 values (with
    ``round_all`` the biases and w3v too, for the end-to-end comparison
    with the eager path, which casts them to bf16)."""
    g = torch.Generator().manual_seed(seed)
    k_in = 2 * hdim + 3
    w1 = _bf(torch.randn(hdim, k_in, generator=g) * 1.5 / k_in ** 0.5)
    b1 = torch.randn(hdim, generator=g) * 0.2
    w2 = _bf(torch.randn(hdim, hdim, generator=g) * 1.5 / hdim ** 0.5)
    b2 = torch.randn(hdim, generator=g) * 0.2
    w3 = _bf(torch.randn(hdim, hdim, generator=g) * 1.5 / hdim ** 0.5)
    b3 = torch.randn(hdim, generator=g) * 0.2
    w3v = torch.randn(hdim, generator=g) * 0.3
    if round_all:
        b1, b2, b3, w3v = _bf(b1), _bf(b2), _bf(b3), _bf(w3v)
    return [t.to(DEV) for t in (w1, b1, w2, b2, w3, b3, w3v)]


def _graph(n, row, col, seed, pos=None):
    g = torch.Generator().manual_seed(seed)
    if pos is None:
        pos = torch.randn(n, 3, generator=g)
    m = row.numel()
    return collate([Data(pos=pos, edge_index=torch.stack([row, col]),
                         edge_attr=torch.randn(m, 2, generator=g))])


def _random_edges(nodes, m, g):
    """m edges among ``nodes`` (a 1-D tensor of node ids), row != col."""
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
    """Isolated nodes at index 0, in the middle and at N-1; node 7 is the
    row of 200 edges (four tiles); 150 more edges elsewhere."""
    g = torch.Generator().manual_seed(11)
    nodes = torch.tensor([i for i in range(ISO_N) if i not in ISOLATED])
    others = nodes[nodes != HUB]
    hub_col = others[torch.randint(0, others.numel(), (HUB_DEG,),
                                   generator=g)]
    row, col = _random_edges(others, 150, g)
    bt = _graph(ISO_N, torch.cat([torch.full((HUB_DEG,), HUB), row]),
                torch.cat([hub_col, col]), 12)
    ei = bt.edge_index
    for i in ISOLATED:
        assert not bool((ei == i).any())
    hub_rows = (ei[0] == HUB).nonzero().flatten()
    assert hub_rows.numel() == HUB_DEG
    assert int(hub_rows[-1]) // TILE - int(hub_rows[0]) // TILE + 1 >= 4
    return bt


def graph_one_col():
    """Every edge points at node 49: colptr is one segment of length M."""
    g = torch.Generator().manual_seed(13)
    row = torch.randint(0, 49, (150,), generator=g)
    bt = _graph(50, row, torch.full((150,), 49), 14)
    assert int(bt.colptr[49]) == 0 and int(bt.colptr[50]) == 150
    return bt


COINC = (3, 4)


def graph_coincident():
    """Nodes 3 and 4 share one position; exactly one edge (3 -> 4) joins
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
SECOND_TRIP_M = GRID_CAP * TILE + TILE * 10 + 5

GRAPHS = {}
for _m in TILE_BOUNDARY_M:
    GRAPHS[f"M{_m}"] = (lambda m=_m: graph_random(m, 24))
for _t in TILE_COUNTS:
    GRAPHS[f"tiles{_t}"] = (lambda t=_t: graph_random(TILE * t - 13, 97))
GRAPHS["iso_hub"] = graph_iso_hub
GRAPHS["one_col"] = graph_one_col
GRAPHS["coincident"] = graph_coincident


# ------------------------------------------------------------ running
class _Case:
    """Inputs of one kernel call and the kernels' outputs."""

    def __init__(self, bt, hdim, normalize, seed=0):
        self.bt = bt.to(DEV)
        torch.cuda.synchronize()
        self.hdim, self.normalize = hdim, bool(normalize)
        self.n, self.m = bt.num_nodes, bt.num_edges
        self.row, self.col = self.bt.edge_index[0], self.bt.edge_index[1]
        g = torch.Generator().manual_seed(100 + seed)
        self.h = (torch.randn(self.n, hdim, generator=g) * 0.7) \
            .bfloat16().to(DEV)
        self.dmsg_n = (torch.randn(self.n, hdim, generator=g) * 0.5) \
            .bfloat16().to(DEV)
        self.dtrans_n = torch.randn(self.n, 3, generator=g).to(DEV)
        self.params = make_params(hdim, 200 + seed)

    def keep_cotangents(self, nodes):
        """Zero dmsg_n / dtrans_n except at ``nodes``."""
        mask = torch.zeros(self.n, 1, dtype=torch.bool, device=DEV)
        mask[nodes] = True
        self.dmsg_n = self.dmsg_n * mask
        self.dtrans_n = self.dtrans_n * mask

    def _weights(self):
        w1, b1, w2, b2, w3, b3, w3v = self.params
        return (w1.bfloat16(), b1, w2.bfloat16(), b2, w3.bfloat16(), b3, w3v)

    def forward(self):
        return ops.hip_ext().fused_edge_forward(
            self.h, self.bt.pos, self.bt.edge_attr, self.row, self.col,
            *self._weights(), self.normalize, EPS)

    def backward(self):
        return ops.hip_ext().fused_edge_backward(
            self.h, self.bt.pos, self.bt.edge_attr, self.row, self.col,
            self.dmsg_n, self.dtrans_n, *self._weights(),
            self.normalize, EPS)


class _Ratios(dict):
    """Worst err/bound per stage; where a bound is 0 the error must be 0."""

    def check(self, tag, got, want, bound):
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        assert bool(torch.isfinite(got.float()).all()), tag
        err = (got.double() - want).abs()
        zero = bound == 0
        if bool((err[zero] != 0).any()):
            r = float("inf")
        elif bool(zero.all()):
            r = 0.0
        else:
            r = float((err[~zero] / bound[~zero]).max())
        self[tag] = max(self.get(tag, 0.0), r)

    def equal(self, tag, got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, tag
        self[tag] = 0.0 if torch.equal(got, want) else float("inf")

    def report(self, title):
        print(f"RATIO edge {title} "
              + " ".join(f"{k}={v:.4f}" for k, v in self.items()))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, (title, bad)


class _Stages:
    """Per-stage float64 references and bounds of one case, each formed
    from the plain backward's emitted tensors (``outs``)."""

    def __init__(self, c, outs):
        (self.ein, self.t1, self.msg, self.dz1, self.dz2, self.dz3,
         self.dhr, self.dhc, self.dcd, self.dw3v, self.gb) = outs
        self.c = c
        H = self.H = c.hdim
        self.K_IN = 2 * H + 3
        self.K_OUT = (self.K_IN + 15) // 16 * 16
        (self.W1, self.b1, self.W2, self.b2, self.W3, self.b3,
         self.w3v) = [t.double() for t in c.params]
        self.d, self.r2, self.inv = ER.geometry(
            c.bt.pos.double(), c.row, c.col, c.normalize, EPS)
        self.dn = self.d * self.inv.unsqueeze(1)
        self.dtr = c.dtrans_n.double().index_select(0, c.row)
        self.refs = {}

    # z = x W^T + b, mag, and the error of its bf16-stored copy
    def _pre(self, x, W, b, K):
        z = ER.preact(x, W, b)
        mag = x.abs() @ W.abs().t() + b.abs()
        return z, mag, U8 * z.abs() + 2 * (K + 1) * U23 * mag

    def _layer(self, x, W, b, K):
        """bf16(silu(bf16(z))) of the backward. The stored z is off by
        zerr, which silu stretches by at most 1.1: 1.1*u8*|z| plus the
        accumulation term, doubled behind the fast-exp SiLU; u8*|want| is
        the rounding of the result."""
        z, mag, _ = self._pre(x, W, b, K)
        want = ER.silu(z)
        return want, (1.1 * U8 * z.abs() + U8 * want.abs()
                      + 4 * (K + 1) * U23 * mag)

    def _head(self, msg):
        """p = sum_c silu(z3_c) w3v_c with z3, silu and the sum in fp32.
        Error of p, in units of u23: silu stretches z3's accumulation
        error, 1.1*2(H+1)*mag3_c, the H-term sum adds H*|silu_c w3v_c| <=
        H*mag3_c|w3v_c|; together (3.2H + 2.2)*mag_p with mag_p =
        sum_c mag3_c |w3v_c|. The fast exponential adds fx =
        sum_c |z3_c silu_c w3v_c|, twice."""
        z3, mag3, zerr3 = self._pre(msg.double(), self.W3, self.b3, self.H)
        s3 = ER.silu(z3)
        w = self.w3v.abs()
        return dict(z3=z3, mag3=mag3, zerr3=zerr3, s3=s3, p=s3 @ self.w3v,
                    mag_p=mag3 @ w, fx=(z3.abs() * s3.abs()) @ w)

    def build(self):
        c, H, K_IN, R = self.c, self.H, self.K_IN, self.refs
        row = c.row
        ein64 = self.ein[:, :K_IN].double()

        # ein.r2: r2 is an fp32 sum of three squares of fp32 differences
        # (at most 8 roundings, contracted or not), then rounded to bf16
        R["ein.r2"] = (self.r2, (U8 + 8 * U23) * self.r2)

        # t1, msg of the backward: one K-term layer each, from ein / t1
        R["bwd.t1"] = self._layer(ein64, self.W1, self.b1, K_IN)
        R["bwd.msg"] = self._layer(self.t1.double(), self.W2, self.b2, H)

        # forward msg: two layers from ein (the forward stages ein with the
        # same code). Its t1 = bf16(silu(fp32 z1)) is not emitted: e1 is
        # its error, which |W2| carries into z2 and silu stretches by at
        # most 1.1; then the one-layer form without a stored z.
        z1, mag1, zerr1 = self._pre(ein64, self.W1, self.b1, K_IN)
        t1r = ER.silu(z1)
        e1 = U8 * t1r.abs() + 4 * (K_IN + 1) * U23 * mag1
        z2f = ER.preact(t1r, self.W2, self.b2)
        mag2f = (t1r.abs() + e1) @ self.W2.abs().t() + self.b2.abs()
        want = ER.silu(z2f)
        R["fwd.msg"] = (want, 1.1 * (e1 @ self.W2.abs().t())
                        + U8 * want.abs() + 4 * (H + 1) * U23 * mag2f)

        # backward head, from the backward's emitted msg
        hb = self.hb = self._head(self.msg)
        z3, zerr3, s3 = hb["z3"], hb["zerr3"], hb["s3"]
        # dp = (dtrans_i . d) inv in fp32: 3-term dot (3), d (1), inv =
        # 1/(sqrt(r2)+eps) (sqrt of a 4-rounding r2: 2, sqrt, add,
        # reciprocal, multiply: 4) -> 10*u23*mag_dp
        dp = ER.head_cotangent(self.dtr, self.d, self.inv)
        mag_dp = (self.dtr.abs() * self.d.abs()).sum(1) * self.inv
        dperr = 10 * U23 * mag_dp

        # dz3 = bf16(dp w3v silu'(z3 stored as bf16)): rounding of the
        # result (u8, plus 4*u23 for the two fp32 products), dp's error
        # times |w3v silu'| <= 1.1|w3v|, and |upstream| times the error of
        # silu': 0.5*zerr3 from the stored z3 and the fast-exp term
        up3 = dp.unsqueeze(1) * self.w3v
        want = up3 * ER.dsilu(z3)
        R["dz3"] = (want, (U8 + 4 * U23) * want.abs()
                    + 1.1 * dperr.unsqueeze(1) * self.w3v.abs()
                    + up3.abs() * (0.5 * zerr3
                                   + 6 * U23 * (1 + z3.abs()) ** 2))

        # dw3v = sum_e dp silu(z3 stored as bf16), fp32 in any order:
        # n*u23*sum|terms| with n the number of edges whose dp is not 0
        # (adding an exact zero rounds nothing; n = M when every node has
        # a cotangent), plus per term dp's error, the stored z3 through
        # silu (1.1*zerr3) and the fast exponential. (The proposed form
        # had the first term only; the kernel takes silu of the bf16-stored
        # z3, so the 1.1*zerr3 term is needed.)
        terms = dp.abs().unsqueeze(1) * s3.abs()
        n_dp = int((dp != 0).sum())
        R["dw3v"] = (ER.dw3v(dp, z3),
                     n_dp * U23 * terms.sum(0)
                     + (dperr.unsqueeze(1) * s3.abs()
                        + dp.abs().unsqueeze(1)
                        * (1.1 * zerr3 + 2 * U23 * z3.abs() * s3.abs())
                        ).sum(0))

        # dz2 = bf16((dmsg_i + dz3 W3) silu'(z2 stored)), dz1 likewise:
        # rounding of the result, the H-term accumulation of the upstream
        # (+1 for the add) times |silu'| <= 1.1, and |upstream| times the
        # error of silu' as for dz3
        def hidden(dz_next, W, extra, x_prev, Wf, bf, K):
            dzn = dz_next.double()
            up = dzn @ W
            mag_up = dzn.abs() @ W.abs()
            if extra is not None:
                up, mag_up = up + extra, mag_up + extra.abs()
            z, _, zerr = self._pre(x_prev, Wf, bf, K)
            want = up * ER.dsilu(z)
            return want, ((U8 + 4 * U23) * want.abs()
                          + 1.1 * 2 * (H + 1) * U23 * mag_up
                          + up.abs() * (0.5 * zerr
                                        + 6 * U23 * (1 + z.abs()) ** 2))

        R["dz2"] = hidden(self.dz3, self.W3,
                          c.dmsg_n.double().index_select(0, row),
                          self.t1.double(), self.W2, self.b2, H)
        R["dz1"] = hidden(self.dz2, self.W2, None, ein64, self.W1, self.b1,
                          K_IN)

        # dhr | dhc: the first 2H columns of dz1 W1, bf16 out, K = H
        dz1 = self.dz1.double()
        W1h = self.W1[:, :2 * H]
        dein = dz1 @ W1h
        bnd = U8 * dein.abs() + 2 * (H + 1) * U23 * (dz1.abs() @ W1h.abs())
        R["dhr"] = (dein[:, :H], bnd[:, :H])
        R["dhc"] = (dein[:, H:], bnd[:, H:])

        # dcd = p dtrans_i inv + 2 d dr2, all fp32. First product, in
        # units of u23*A with A = |dtrans_i| inv mag_p: p's (3.2H + 2.2),
        # inv (8), two products and the final add (3) <= 4(H+2), plus the
        # fast-exp term. Second product, B = 2|d| mag_dr2: dr2 is an
        # H-term fp32 accumulation, 2(H+1), d and the products 4.
        w_r2 = self.W1[:, 2 * H]
        dr2 = dz1 @ w_r2
        mag_dr2 = dz1.abs() @ w_r2.abs()
        A = (self.inv * hb["mag_p"]).unsqueeze(1) * self.dtr.abs()
        Afx = (self.inv * hb["fx"]).unsqueeze(1) * self.dtr.abs()
        B = 2 * self.d.abs() * mag_dr2.unsqueeze(1)
        R["dcd"] = (ER.dcoord_diff(hb["p"], self.dtr, self.inv, self.d, dr2),
                    U23 * (4 * (H + 2) * A + 2 * Afx
                           + (2 * (H + 1) + 4) * B))

        # gb: fp32 column sums of the emitted dz1 | dz2 | dz3, any order:
        # n*u23*sum|dz| with n the number of nonzero terms of the column
        # (M at most; zeros add exactly). gb3 is summed BEFORE dz3 is
        # rounded to bf16 (gb1, gb2 after): its terms are nonzero where dp
        # is, and against the emitted dz3 it carries one bf16 rounding per
        # term on top: u8*sum|dz3| (1.01 for |d3| vs |bf16|).
        dzs = [dz1, self.dz2.double(), self.dz3.double()]
        S = torch.cat([t.abs().sum(0) for t in dzs])
        cnt = torch.cat([(dz1 != 0).sum(0), (dzs[1] != 0).sum(0),
                         torch.full((H,), n_dp, device=S.device)])
        assert int(cnt.max()) <= c.m
        bnd = cnt.double() * U23 * S
        bnd[2 * H:] += 1.01 * U8 * S[2 * H:]
        R["gb"] = (torch.cat([t.sum(0) for t in dzs]), bnd)
        return self

    def forward_trans(self, fwd_msg):
        """trans = d inv p from the forward's own msg, fp32: p as in
        _head, d inv (8) and the product (1) -> 4(H+2)*u23*|d inv|*mag_p
        plus the fast-exp term. d = 0 gives bound 0: exactly 0."""
        hf = self._head(fwd_msg)
        return (self.dn * hf["p"].unsqueeze(1),
                U23 * self.dn.abs()
                * (4 * (self.H + 2) * hf["mag_p"] + 2 * hf["fx"]).unsqueeze(1))


def _check_plain(c, title):
    """Forward + plain backward of one case, every stage. Returns the
    stages and the forward outputs."""
    H, K_IN = c.hdim, 2 * c.hdim + 3
    fwd_msg, fwd_trans = c.forward()
    outs = c.backward()
    st = _Stages(c, outs).build()
    assert fwd_msg.dtype == torch.bfloat16 and fwd_msg.shape == (c.m, H)
    assert fwd_trans.dtype == torch.float32 and fwd_trans.shape == (c.m, 3)
    assert st.ein.shape == (c.m, st.K_OUT)
    R = _Ratios()
    R.equal("ein.h_row", st.ein[:, :H], c.h.index_select(0, c.row))
    R.equal("ein.h_col", st.ein[:, H:2 * H], c.h.index_select(0, c.col))
    R.equal("ein.attr", st.ein[:, 2 * H + 1:K_IN],
            c.bt.edge_attr.bfloat16())
    R.equal("ein.pad", st.ein[:, K_IN:],
            torch.zeros_like(st.ein[:, K_IN:]))
    got = {"ein.r2": st.ein[:, 2 * H], "bwd.t1": st.t1, "bwd.msg": st.msg,
           "fwd.msg": fwd_msg, "dz3": st.dz3, "dz2": st.dz2, "dz1": st.dz1,
           "dhr": st.dhr, "dhc": st.dhc, "dcd": st.dcd, "dw3v": st.dw3v,
           "gb": st.gb}
    for tag, g in got.items():
        R.check(tag, g, *st.refs[tag])
    R.check("fwd.trans", fwd_trans, *st.forward_trans(fwd_msg))
    R.report(title)
    return st, fwd_msg, fwd_trans


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hdim", [32, 64, 128])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_edge_stages(gname, hdim, normalize):
    c = _Case(GRAPHS[gname](), hdim, normalize)
    if gname.startswith("M"):
        assert c.m == int(gname[1:])
    if gname.startswith("tiles"):
        assert (c.m + TILE - 1) // TILE == int(gname[5:])
        assert c.m % TILE != 0
    st, fwd_msg, fwd_trans = _check_plain(
        c, f"case={gname} H={hdim} norm={int(normalize)}")
    if gname == "coincident":
        e = ((c.row == COINC[0]) & (c.col == COINC[1])).nonzero().flatten()
        assert e.numel() == 1
        assert float(st.r2[e]) == 0.0
        # d = 0: the translation is exactly 0 with and without normalize
        assert bool((fwd_trans[e] == 0).all())
        # dcd of that edge is p dtrans/eps under normalize (huge) and was
        # judged above per edge against a bound relative to its own size
        want, bound = st.refs["dcd"]
        assert bool((bound[e] > 0).all())
        assert bool(((st.dcd[e].double() - want[e]).abs() <= bound[e]).all())
        if normalize:
            assert float(want[e].abs().max()) > 1e3


@pytest.mark.parametrize("normalize", [False, True])
def test_edge_second_tile_trip(normalize):
    """M = 16384*64 + 64*10 + 5: the grids are capped at 16384 blocks, so
    blocks 0..10 walk a second tile (the last one ragged). Every row of
    every stage is compared, on the device. H = 32: the loop does not
    depend on H."""
    m, n = SECOND_TRIP_M, 2048
    assert (m + TILE - 1) // TILE == GRID_CAP + 11 and m % TILE == 5
    c = _Case(graph_random(m, n), 32, normalize)
    assert c.m == m
    _check_plain(c, f"case=second_trip H=32 norm={int(normalize)}")


def _second_trip_tiles(m):
    """Tiles a block reaches on its second trip, by the XCD remap of the
    kernels: virtual tile vt belongs to XCD vt & 7, which owns a contiguous
    range of tq + 1 (the first tr XCDs) or tq tiles."""
    ntile = (m + TILE - 1) // TILE
    tq, tr = ntile >> 3, ntile & 7
    tiles = []
    for vt in range(GRID_CAP, ntile):
        xcd, ti = vt & 7, vt >> 3
        start = xcd * (tq + 1) if xcd < tr else tr * (tq + 1) + (xcd - tr) * tq
        tiles.append(start + ti)
    return tiles


def test_edge_second_tile_trip_accumulators():
    """gb and dw3v are sums over ALL edges, and at a million dense terms
    their bound is too wide to miss eleven tiles. Here only the nodes
    whose rows own the second-trip tiles carry a cotangent, so every other
    edge contributes an exact zero: the sums then have some ten thousand
    nonzero terms, several percent of them from the second trip, against a
    bound of n*u23 ~ 1e-3 of sum|terms|."""
    m, n = SECOND_TRIP_M, 2048
    c = _Case(graph_random(m, n), 32, True)
    tiles = _second_trip_tiles(m)
    assert len(tiles) == 11 and len(set(tiles)) == 11
    assert max(tiles) == (m - 1) // TILE        # the ragged tile is one
    in_trip = torch.zeros(m, dtype=torch.bool, device=DEV)
    for t in tiles:
        in_trip[t * TILE:(t + 1) * TILE] = True
    nodes = torch.unique(c.row[in_trip])
    c.keep_cotangents(nodes)
    live = torch.isin(c.row, nodes)
    n_live = int(live.sum())
    share = int((live & in_trip).sum()) / n_live
    print(f"second-trip share of the {n_live} nonzero terms: {share:.3f}")
    assert share >= 0.03 and n_live * U23 <= share / 10
    st, _, _ = _check_plain(c, "case=second_trip_acc H=32 norm=1")
    assert float(st.refs["gb"][0].abs().min()) > 0
    # rows without a cotangent are exactly zero in every dz
    for dz in (st.dz1, st.dz2, st.dz3):
        assert bool((dz[~live] == 0).all())


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_direct_call_rejects_fp32_weights(which):
    """Without ``prepped`` the kernels read w1/w2/w3 as bf16; fp32 weights
    must raise instead of being reinterpreted."""
    c = _Case(graph_random(17, 24), 64, False)
    ext = ops.hip_ext()
    w1, b1, w2, b2, w3, b3, w3v = c.params
    assert w1.dtype == torch.float32
    geo = (c.h, c.bt.pos, c.bt.edge_attr, c.row, c.col)
    tail = (w1, b1, w2.bfloat16(), b2, w3.bfloat16(), b3, w3v, False, EPS)
    with pytest.raises(RuntimeError, match="must be bf16"):
        if which == "forward":
            ext.fused_edge_forward(*geo, *tail)
        else:
            ext.fused_edge_backward(*geo, c.dmsg_n, c.dtrans_n, *tail)


# ------------------------------------------------- end to end (python glue)
E2E_NAMES = ["agg_msg", "agg_trans", "h.grad", "coord.grad", "w1.grad",
             "b1.grad", "w2.grad", "b2.grad", "w3.grad", "b3.grad",
             "w3v.grad"]


def _e2e_graph(gname):
    if gname == "iso_hub":
        bt, normalize = graph_iso_hub(), False
    else:
        bt, normalize = collate(make_cutoff_dataset(
            "Water-3D", 1, seed=7, n_override=700)), True
    bt.edge_attr = _bf(bt.edge_attr)
    return bt, normalize


@pytest.mark.parametrize("hdim", [32, 64, 128])
@pytest.mark.parametrize("gname", ["iso_hub", "cutoff"])
def test_edge_block_end_to_end(gname, hdim):
    """ops.fused_edge_block forward + backward against a full float64
    reference (plain index_select / index_add_, mean over deg.clamp(1),
    autograd) from the same bf16-valued inputs. Per tensor, the relative
    L2 error of the fused path may be at most twice that of the bf16
    eager composition: both place the same bf16 roundings, the fused
    backward one more per layer (the bf16-stored pre-activation)."""
    bt, normalize = _e2e_graph(gname)
    bt = bt.to(DEV)
    row, col = bt.edge_index[0], bt.edge_index[1]
    n = bt.num_nodes
    params = make_params(hdim, 300, round_all=True)
    g = torch.Generator().manual_seed(301)
    h0 = (torch.randn(n, hdim, generator=g) * 0.7).bfloat16().to(DEV)
    gm = (torch.randn(n, hdim, generator=g) * 0.5).bfloat16().to(DEV)
    gt = torch.randn(n, 3, generator=g).to(DEV)

    def run(disable_fused):
        if disable_fused:
            os.environ["DISTEGNN_DISABLE_FUSED"] = "1"
        try:
            leaves = [h0.clone().requires_grad_(True),
                      bt.pos.clone().requires_grad_(True)] \
                + [p.clone().requires_grad_(True) for p in params]
            am, at = ops.fused_edge_block(
                leaves[0], leaves[1], bt.edge_attr, row, col, bt.rowptr,
                bt.colptr, bt.col_perm, *leaves[2:], normalize, EPS)
            grads = torch.autograd.grad((am, at), leaves,
                                        (gm.to(am.dtype), gt.to(at.dtype)))
        finally:
            os.environ.pop("DISTEGNN_DISABLE_FUSED", None)
        return [am.detach(), at.detach()] + list(grads)

    leaves = [h0.double().requires_grad_(True),
              bt.pos.double().requires_grad_(True)] \
        + [p.double().requires_grad_(True) for p in params]
    am, at = ER.edge_block_mean(leaves[0], leaves[1], bt.edge_attr.double(),
                                row, col, *leaves[2:], normalize, EPS)
    ref = [am.detach(), at.detach()] + list(torch.autograd.grad(
        (am, at), leaves, (gm.double(), gt.double())))

    fused, eager = run(False), run(True)
    bad = []
    for nm, r, f, e in zip(E2E_NAMES, ref, fused, eager):
        assert f.shape == r.shape and e.shape == r.shape, nm
        assert float(r.norm()) > 0, nm
        ef = float((f.double() - r).norm() / r.norm())
        ee = float((e.double() - r).norm() / r.norm())
        print(f"E2E graph={gname} H={hdim} {nm} err_fused={ef:.3e} "
              f"err_eager={ee:.3e} ratio={ef / ee:.3f}")
        if not ef <= 2 * ee:
            bad.append((nm, ef, ee))
    assert not bad, bad
