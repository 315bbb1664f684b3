"""GPU: the GATv2 baseline (bridged_gnn_amd.gatv2, models/backbones.py:302-358) on the one-pass HIP attention conv -- the kernels
against the edge-list fp64 restatement of tests/test_gatv2_host.py on adversarial graphs (duplicates, existing self loops, isolated
nodes, a hub row and a hub source of >= 30 000 edges, extreme logits), the two dropout laws, the model against the reference's fp64
fixtures (tools/gen_golden_gatv2.py) and `train_gatv2_noDTC` eager and graphed.
Bars: those of test_gpu_gat.py -- activations 1e-5 of the tensor's max + 1e-6, gradients 2e-5 of the max; Adam losses and parameters
1e-4; eager against graphed loss series rtol 2e-4.  At kernel level the restatement takes the kernel's own LeakyReLU sides,
(XL[src] + XR[dst]) > 0 formed on the host in fp32 from the same table -- exact, because the kernel's m is one IEEE add -- so there is
no kink allowance there.  At model level a gradient beyond 2e-5 must be within 2e-4 and then meet 2e-5 against the restatement
taken with the GPU's side pattern."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from test_gatv2_host import OFFICE_MODELS, SMALL_MODELS, conv_sparse, edge_list, params64, restate

pytestmark = pytest.mark.gpu

ACT_BAR, GRAD_BAR, KINK_CAP = 1e-5, 2e-5, 2e-4
TRAJ_RTOL = 2e-4
SHAPES = ((1, 1), (1, 2), (1, 5), (1, 31), (1, 64), (1, 128), (2, 5), (3, 8), (8, 16))


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _act_ok(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what + ": not finite"
    err = np.abs(got - ref).max()
    tol = ACT_BAR * np.abs(ref).max() + 1e-6
    print(f"{what}: max err {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _grad_ok(got, ref, what, rel=GRAD_BAR):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max()
    tol = rel * np.abs(ref).max()
    print(f"{what}: max err {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


# ---- kernel level ------------------------------------------------------------------------------------------------
def _graph(n, e, seed, hub=0):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    loops = np.arange(0, n, 7)
    extra = [ei, ei[:, : e // 20], np.stack([loops, loops]), np.stack([loops[:5], loops[:5]])]   # duplicates, self loops (5 twice)
    if hub:
        rng = np.random.default_rng(seed)
        extra.append(np.stack([rng.integers(0, n, hub), np.full(hub, 3)]))                  # node 3: >= hub in-edges
        extra.append(np.stack([np.full(hub, 5), rng.integers(0, n - n // 50, hub)]))        # node 5: >= hub out-edges
    return np.concatenate(extra, axis=1).astype(np.int64)


class _G:
    """a GatGraph and its edges in CSR order on the host (edge t of the kernels = element t of src / dst)"""

    def __init__(self, ei, n):
        from bridged_gnn_amd.gatv2 import GatGraph
        self.n = n
        self.g = GatGraph(torch.from_numpy(ei).to(_dev()), n)
        rp = self.g.rowptr.cpu().long()
        self.src = self.g.col.cpu().long()
        self.dst = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
        keep = ei[0] != ei[1]
        assert self.src.shape[0] == int(keep.sum()) + n                            # input self loops dropped, one per node
        self.indeg = np.bincount(ei[1][keep], minlength=n)
        self.outdeg = np.bincount(ei[0][keep], minlength=n)
        self.bwd = (self.g.rowptr, self.g.col, self.g.t_rowptr, self.g.t_eid, self.g.t_dst)


_GRAPHS = {}


def _shared_graph(key):
    """the graphs of the kernel tests, built once: (n, e, seed, hub)"""
    if key not in _GRAPHS:
        n, e, seed, hub = key
        _GRAPHS[key] = _G(_graph(n, e, seed, hub), n)
    return _GRAPHS[key]


SMALLG, HUBG, LAWG = (3000, 30000, 1, 0), (40000, 40000, 2, 30000), (20000, 200000, 10, 0)


def _inputs(n, H, C, seed):
    """the one table [n, 2P] (XL | XR), att [1, H, C], bias [P], dy [n, P]; pad columns 0"""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(seed)
    HC, P = H * C, ops.pad4(H * C)
    T = torch.zeros(n, 2 * P)
    T[:, :HC] = torch.from_numpy(rng.standard_normal((n, HC)).astype(np.float32))
    T[:, P:P + HC] = torch.from_numpy(rng.standard_normal((n, HC)).astype(np.float32))
    att = torch.from_numpy((rng.standard_normal((1, H, C)) / np.sqrt(C)).astype(np.float32))
    b = torch.zeros(P)
    b[:HC] = torch.from_numpy(rng.standard_normal(HC).astype(np.float32))
    dy = torch.zeros(n, P)
    dy[:, :HC] = torch.from_numpy(rng.standard_normal((n, HC)).astype(np.float32))
    return T, att, b, dy


def _halves(T, H, C):
    """(XL, XR) [n, H, C] views of the table"""
    from bridged_gnn_amd import ops
    HC, P = H * C, ops.pad4(H * C)
    return T[:, :HC].reshape(-1, H, C), T[:, P:P + HC].reshape(-1, H, C)


def _kernel_sides(T, H, C, src, dst):
    """the LeakyReLU side of every (edge, head, column) as the kernels take it: one fp32 add of the table's own values"""
    XL, XR = _halves(T, H, C)
    return (XL[src] + XR[dst]) > 0


def _epi64(z, epi):
    return F.elu(z) if epi == "elu" else torch.log_softmax(z, 1) if epi == "log_softmax" else z


def _epilogues(H):
    return (None, "elu", "log_softmax") if H == 1 else (None, "elu")


def _forward_shape(G, H, C, seed):
    from bridged_gnn_amd import ops
    dev, n, HC = _dev(), G.n, H * C
    T, att, b, _ = _inputs(n, H, C, seed)
    Td, bd, ad = T.to(dev), b.to(dev), att.to(dev)
    sides = _kernel_sides(T, H, C, G.src, G.dst)
    assert bool(sides.any()) and bool((~sides).any()), "the pre-activations must straddle 0"
    XL, XR = _halves(T.double(), H, C)
    ref, rstate = conv_sparse(XL, XR, att.double(), G.src, G.dst, sides=sides, want_state=True)
    what = f"H={H} C={C}"
    for epi in _epilogues(H):
        for bias in (bd, None):
            out, state, pre, alpha = ops.gatv2_aggregate(Td, ad, G.g.rowptr, G.g.col, n, H, C, bias=bias, epilogue=epi, want_pre=True,
                                                         return_alpha=True)
            z64 = ref + (b[:HC].double() if bias is not None else 0.0)
            tag = f"{what} epi={epi} bias={bias is not None}"
            _act_ok(out[:, :HC].cpu(), _epi64(z64, epi), tag)
            _act_ok(pre[:, :HC].cpu(), z64, tag + " pre")
            if out.shape[1] > HC:
                assert torch.count_nonzero(out[:, HC:]).item() == 0 and torch.count_nonzero(pre[:, HC:]).item() == 0, "pad columns must be 0"
            lean = ops.gatv2_aggregate(Td, ad, G.g.rowptr, G.g.col, n, H, C, bias=bias, epilogue=epi)
            assert lean[2] is None and lean[3] is None and torch.equal(lean[0], out) and torch.equal(lean[1], state)
    _act_ok(state[..., 0].cpu(), rstate[..., 0], what + " softmax max")
    _act_ok(state[..., 1].cpu(), rstate[..., 1], what + " softmax denominator")
    assert float(state[..., 1].min().item()) >= 1.0                      # the shifted denominator holds the maximum's own 1
    sums = torch.zeros(n, H, dtype=torch.float64).index_add_(0, G.dst, alpha.cpu().double())
    _act_ok(sums, torch.ones(n, H, dtype=torch.float64), what + " coefficients of a row sum to 1")


def _backward_case(G, H, C, seed, epilogues, att_mask=None, p_att=0.0, seed_att=0):
    """kernel backward against fp64 autograd of the restatement with XL, XR, att and the bias as leaves (the kernel returns exactly
    those gradients); the LeakyReLU side of every (edge, head, column) is the kernel's own"""
    from bridged_gnn_amd import ops
    dev, n, HC, P = _dev(), G.n, H * C, ops.pad4(H * C)
    T, att, b, dy = _inputs(n, H, C, seed)
    Td, bd, dyd, ad = T.to(dev), b.to(dev), dy.to(dev), att.to(dev)
    sides = _kernel_sides(T, H, C, G.src, G.dst)
    for epi in epilogues:
        out, state, pre, _ = ops.gatv2_aggregate(Td, ad, G.g.rowptr, G.g.col, n, H, C, bias=bd, epilogue=epi, p_att=p_att,
                                                 seed_att=seed_att, want_pre=True)
        args = (Td, ad, state, pre, dyd, *G.bwd, H, C)
        kw = dict(bias=bd, epilogue=epi, p_att=p_att, seed_att=seed_att)
        got = ops.gatv2_aggregate_bwd(*args, **kw)
        again = ops.gatv2_aggregate_bwd(*args, **kw)
        assert all(torch.equal(a, b2) for a, b2 in zip(got, again)), f"H={H} C={C} epi={epi}: two calls differ"
        xl, xr = (t.clone().requires_grad_(True) for t in _halves(T.double(), H, C))
        a64, b64 = att.double().requires_grad_(True), b[:HC].double().requires_grad_(True)
        r = _epi64(conv_sparse(xl, xr, a64, G.src, G.dst, bias=b64, sides=sides, edge_scale=att_mask), epi)
        if att_mask is not None:
            _act_ok(out[:, :HC].cpu(), r.detach(), f"H={H} C={C} epi={epi} forward under the recovered mask")
        rl, rr, ra, rb = torch.autograd.grad((r * dy[:, :HC].double()).sum(), [xl, xr, a64, b64])
        what = f"n={n} H={H} C={C} epi={epi}"
        dT = got[0].cpu()
        assert tuple(dT.shape) == (n, 2 * P)
        _grad_ok(dT[:, :HC], rl.reshape(n, HC), what + " dXL")
        _grad_ok(dT[:, P:P + HC], rr.reshape(n, HC), what + " dXR")
        _grad_ok(got[1].cpu(), ra.reshape(HC), what + " datt")
        _grad_ok(got[2].cpu(), rb, what + " grad_bias")
        if P > HC:
            assert torch.count_nonzero(dT[:, HC:P]).item() == 0 and torch.count_nonzero(dT[:, P + HC:]).item() == 0


@pytest.mark.parametrize("H,C", SHAPES)
def test_forward_kernel_every_shape_epilogue_and_bias(H, C):
    G = _shared_graph(SMALLG)
    assert (G.indeg == 0).any()                                                     # isolated nodes: their row is the self loop alone
    _forward_shape(G, H, C, seed=10 + H * 131 + C)


@pytest.mark.parametrize("H,C", SHAPES)
def test_backward_kernel_matches_fp64_autograd_and_is_deterministic(H, C):
    _backward_case(_shared_graph(SMALLG), H, C, seed=500 + H * 131 + C, epilogues=_epilogues(H))


@pytest.mark.parametrize("H,C", [(1, 64), (1, 2)])
def test_hub_row_and_hub_source_forward_and_backward(H, C):
    G = _shared_graph(HUBG)
    assert G.indeg.max() >= 30000 and G.outdeg.max() >= 30000 and (G.indeg == 0).any()
    if C == 64:
        # bgnn_gatv2.hip launch_dst: the persistent grid, never more than DATT_BLOCKS = 2048 blocks, over tiles of 4 * (64 // LF) = 16
        # rows at C = 64 (lf_ladder: LF = 16, EP = 1); bgnn_conv_common.h launch_rows: 2048 blocks of 256 // LF = 16 (node, head) rows
        assert -(-G.n // 16) > 2048 and G.n * H > 2048 * 16
    _forward_shape(G, H, C, seed=900 + C)
    _backward_case(G, H, C, seed=950 + C, epilogues=("elu",))


def test_out_of_envelope_requests_raise_shape_errors():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gatv2 import GATv2Conv
    dev = _dev()
    G = _shared_graph(SMALLG)
    for H, C in ((9, 4), (1, 129)):
        P = ops.pad4(H * C)
        T = torch.zeros(G.n, 2 * P, device=dev)
        att = torch.zeros(H * C, device=dev)
        with pytest.raises(RuntimeError, match="shape"):
            ops.gatv2_aggregate(T, att, G.g.rowptr, G.g.col, G.n, H, C)
        with pytest.raises(RuntimeError, match="shape"):
            ops.gatv2_aggregate_bwd(T, att, torch.zeros(G.n, H, 2, device=dev), T[:, :P], T[:, :P], *G.bwd, H, C)
        with pytest.raises(RuntimeError, match="shape"):
            GATv2Conv(8, C, heads=H).to(dev)(torch.zeros(G.n, 8, device=dev), G.g)
    with pytest.raises(RuntimeError, match="shape"):                               # the fused log_softmax is for one head
        ops.gatv2_aggregate(torch.zeros(G.n, 16, device=dev), torch.zeros(8, device=dev), G.g.rowptr, G.g.col, G.n, 2, 4,
                            epilogue="log_softmax")


@pytest.mark.parametrize("H,C", [(3, 8), (1, 2)])
def test_extreme_logits_stay_finite_and_follow_the_fp64_softmax(H, C):
    """Integer-valued tables in [-8, 8], integer att scaled by 2^7 and negative_slope = 0.25: every product and partial sum of a
    logit is a multiple of 32 below 2^24 * 32, so the fp32 logit is exact in any summation order and equals the fp64 one.  What is
    under test is the online softmax -- the running maximum, the rescaling, the merge of the sub-groups -- at |e| up to 1e4 and
    beyond, with both signs inside one row."""
    from bridged_gnn_amd import ops
    dev = _dev()
    G = _shared_graph(SMALLG)
    n, HC, P = G.n, H * C, ops.pad4(H * C)
    rng = np.random.default_rng(77)
    T = torch.zeros(n, 2 * P)
    T[:, :HC] = torch.from_numpy(rng.integers(-8, 9, (n, HC)).astype(np.float32))
    T[:, P:P + HC] = torch.from_numpy(rng.integers(-8, 9, (n, HC)).astype(np.float32))
    att = torch.from_numpy((rng.integers(-8, 9, (1, H, C)) * 128.0).astype(np.float32))
    att[0, :, 0] = 8 * 128.0
    XL, XR = _halves(T.double(), H, C)
    e64 = (F.leaky_relu(XL[G.src] + XR[G.dst], 0.25) * att.double()).sum(-1)
    idx = G.dst.unsqueeze(1).expand(-1, H)
    hi = torch.full((n, H), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, e64, "amax")
    lo = torch.full((n, H), float("inf"), dtype=torch.float64).scatter_reduce(0, idx, e64, "amin")
    assert float(e64.abs().max()) >= 1e4 and bool(((hi > 1e3) & (lo < -1e3)).any())
    assert torch.equal(e64.float().double(), e64)
    ref, rstate = conv_sparse(XL, XR, att.double(), G.src, G.dst, want_state=True, slope=0.25)
    out, state, _, alpha = ops.gatv2_aggregate(T.to(dev), att.to(dev), G.g.rowptr, G.g.col, n, H, C, negative_slope=0.25,
                                               return_alpha=True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(state).all())
    _act_ok(out[:, :HC].cpu(), ref, f"extreme H={H} C={C}")
    assert torch.equal(state[..., 0].cpu(), rstate[..., 0].float())                 # the maximum of the same exact logits
    _act_ok(state[..., 1].cpu(), rstate[..., 1], f"extreme H={H} C={C} denominator")


def test_attention_dropout_law_and_backward_under_the_recovered_mask():
    from bridged_gnn_amd import ops
    dev = _dev()
    H, C, n, p = 3, 8, 20000, 0.5
    G = _shared_graph(LAWG)
    E = G.src.shape[0]
    T, att, b, _ = _inputs(n, H, C, seed=21)
    Td, ad = T.to(dev), att.to(dev)
    args = (G.g.rowptr, G.g.col, n, H, C)
    alpha = ops.gatv2_aggregate(Td, ad, *args, return_alpha=True)[3]
    assert float(alpha.min().item()) > 0.0
    at = ops.gatv2_aggregate(Td, ad, *args, p_att=p, seed_att=1234, return_alpha=True)[3]
    keep = at != 0                                                       # the zero pattern of a~ is the mask
    cnt, tot = int(keep.sum().item()), E * H
    sd = (tot * p * (1 - p)) ** 0.5
    print(f"kept {cnt} of {tot}: {(cnt - (1 - p) * tot) / sd:+.2f} sd from {1 - p}")
    assert abs(cnt - (1 - p) * tot) <= 6 * sd, f"kept {cnt} of {tot}"
    torch.testing.assert_close(at[keep], alpha[keep] / (1 - p), rtol=1e-6, atol=0)
    # the mask is a function of (seed, edge position, head): other tables and another att, the same mask
    T2, a2 = torch.roll(Td, 1, 0), torch.flip(ad, (2,))
    assert torch.equal(ops.gatv2_aggregate(T2, a2, *args, p_att=p, seed_att=1234, return_alpha=True)[3] != 0, keep)
    assert not torch.equal(ops.gatv2_aggregate(Td, ad, *args, p_att=p, seed_att=1235, return_alpha=True)[3] != 0, keep)
    word = torch.tensor([1000], dtype=torch.int64, device=dev)
    o1 = ops.gatv2_aggregate(Td, ad, *args, p_att=p, seed_att=1234, return_alpha=True)
    o2 = ops.gatv2_aggregate(Td, ad, *args, p_att=p, seed_att=234, seed_att_dev=word, return_alpha=True)
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[3], o2[3]) and torch.equal(o1[3], at), "seed + device word is the seed"
    # forward and backward with the recovered mask in the fp64 restatement: both backward passes redraw the same mask
    mask = keep.cpu().double() / (1 - p)
    _backward_case(G, H, C, seed=21, epilogues=(None, "elu"), att_mask=mask, p_att=p, seed_att=1234)


def test_feature_dropout_law_backward_and_seeds():
    """att = 0 here: every logit is 0, so on the graph of self loops only the coefficient is exactly 1, de multiplies att = 0, and
    dXL is g itself, element by element"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gatv2 import GatGraph
    dev = _dev()
    n = 20000
    G = _shared_graph(LAWG)
    eye = GatGraph(torch.zeros(2, 0, dtype=torch.int64, device=dev), n)             # self loops only: alpha = 1, out = XL + bias
    ebwd = (eye.rowptr, eye.col, eye.t_rowptr, eye.t_eid, eye.t_dst)
    for H, C in ((3, 8), (1, 31)):
        HC, P = H * C, ops.pad4(H * C)
        gen = torch.Generator().manual_seed(11)
        tbl = torch.zeros(n, 2 * P)
        tbl[:, :HC] = torch.rand(n, HC, generator=gen)
        tbl[:, P:P + HC] = torch.rand(n, HC, generator=gen)
        tbl = tbl.to(dev)
        bias = (10.0 + torch.rand(P, generator=gen)).to(dev)             # pre-activation > 0 everywhere: ELU is the identity, y > 0 <=> kept
        att = torch.zeros(HC, device=dev)

        def run(g, bias=bias, tbl=tbl, **kw):
            return ops.gatv2_aggregate(tbl, att, g.rowptr, g.col, n, H, C, bias=bias, epilogue="elu", want_pre=True, **kw)
        z = run(G.g)[0][:, :HC]
        y, state, pre, _ = run(G.g, p_drop=0.5, seed=1234)
        keep = y[:, :HC] > 0
        cnt, tot = int(keep.sum().item()), n * HC
        assert abs(cnt - tot / 2) <= 6 * (tot * 0.25) ** 0.5, f"H={H} C={C}: kept {cnt} of {tot}"
        torch.testing.assert_close(y[:, :HC][keep], 2.0 * z[keep], rtol=1e-6, atol=0)
        assert torch.count_nonzero(y[:, :HC][~keep]).item() == 0 and torch.count_nonzero(y[:, HC:]).item() == 0
        # the gradient: g = keep ? 2 dy : 0, seen through grad_bias = column sums of g
        dy = torch.randn(n, P, generator=gen)
        dy[:, HC:] = 0
        dy = dy.to(dev)
        want = torch.where(keep, 2.0 * dy[:, :HC], torch.zeros_like(dy[:, :HC]))
        gb = ops.gatv2_aggregate_bwd(tbl, att, state, pre, dy, *G.bwd, H, C, bias=bias, epilogue="elu", p_drop=0.5, seed=1234)[2]
        torch.testing.assert_close(gb.double(), want.double().sum(0), rtol=1e-5, atol=1e-4)
        # element by element through dXL of the graph of self loops only
        y1, st1, pre1, _ = run(eye, p_drop=0.5, seed=1234)
        assert torch.equal(y1[:, :HC] > 0, keep), "the mask depends on (seed, row, column) alone"
        gt = ops.gatv2_aggregate_bwd(tbl, att, st1, pre1, dy, *ebwd, H, C, bias=bias, epilogue="elu", p_drop=0.5, seed=1234)[0]
        torch.testing.assert_close(gt[:, :HC], want, rtol=0, atol=0)
        # rows whose pre-activation is exactly 0 (zero features, zero bias): y is 0 kept or not, the gradient of a kept element is 2 dy
        zero_tbl, zero_bias = torch.zeros_like(tbl), torch.zeros_like(bias)
        y0, st0, pre0, _ = run(eye, bias=zero_bias, tbl=zero_tbl, p_drop=0.5, seed=1234)
        assert torch.count_nonzero(y0).item() == 0 and torch.count_nonzero(pre0).item() == 0
        g0 = ops.gatv2_aggregate_bwd(zero_tbl, att, st0, pre0, dy, *ebwd, H, C, bias=zero_bias, epilogue="elu", p_drop=0.5, seed=1234)[0]
        torch.testing.assert_close(g0[:, :HC], want, rtol=0, atol=0)
        assert bool((g0[:, :HC][keep] == 2.0 * dy[:, :HC][keep]).all()) and int(keep[:, 0].sum().item()) > 0
        # seeds
        assert not torch.equal(run(G.g, p_drop=0.5, seed=1235)[0][:, :HC] > 0, keep), "two seeds gave the same mask"
        assert torch.equal(run(G.g, p_drop=0.5, seed=1234)[0], y)
        word = torch.tensor([1000], dtype=torch.int64, device=dev)
        assert torch.equal(run(G.g, p_drop=0.5, seed=234, seed_dev=word)[0], y), "seed + device word is the seed"


# ---- model level -------------------------------------------------------------------------------------------------
def _case(fixture, variant):
    from bridged_gnn_amd.data import Data
    dev = _dev()
    if fixture == "office":
        g, fx, models = load_golden("office_a2d_graph.npz"), load_golden("gatv2_office_a2d.npz"), OFFICE_MODELS
    else:
        g = fx = load_golden("gatv2_small.npz")
        models = SMALL_MODELS
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(dev)          # the driver's mask (y == -1 cleared, :404)
    dims = (g["x"].shape[1], int(g["y"].max()) + 1)
    return data, tm, dims, fx, models


def _model(dims, fx, name, hidden, heads, layers, seed):
    """the fixture's model: the generator's seed and PyG's initialisers, checked against the stored parameters / their sums"""
    from bridged_gnn_amd.gatv2 import GATv2
    torch.manual_seed(seed)
    m = GATv2(dims[0], hidden, dims[1], layers, heads, 0.6, 0.5)
    full, sums = sub(fx, f"{name}/param/"), sub(fx, f"{name}/param_sum/")
    assert sorted(full or sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        if full:
            assert np.array_equal(v.numpy(), full[k]), k
        else:
            vd = v.double()
            np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-6, atol=1e-300, err_msg=k)
    return m.to(_dev()).eval()


@pytest.mark.parametrize("variant", ["raw", "und"])
@pytest.mark.parametrize("fixture", ["office", "small"])
def test_forward_matches_reference(fixture, variant):
    data, _, dims, fx, models = _case(fixture, variant)
    rows = torch.from_numpy(fx["rows"])
    x64 = data.x.double().cpu()
    edges = edge_list(data.edge_index.cpu(), x64.shape[0])
    for name, hidden, heads, layers, seed in models:
        m = _model(dims, fx, name, hidden, heads, layers, seed)
        P = params64(m.state_dict())
        pre = f"{variant}/{name}/"
        with torch.no_grad():
            logp = m(data).cpu()
            r_logp = restate(P, x64, edges)
        _act_ok(logp[rows], fx[pre + "logp"], pre + "logp")                          # the reference, at the fixture's rows
        _act_ok(logp, r_logp, pre + "logp (every row, fp64 restatement)")
        # the autograd path (grad enabled, eval mode) computes the same outputs
        _act_ok(m(data).detach().cpu()[rows], fx[pre + "logp"], pre + "logp (autograd path)")


def _gpu_sides(m, data, edges):
    """the LeakyReLU side the GPU takes for every (edge, head, column) of every conv: the sign of its own fp32 x_l[j] + x_r[i]"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gatv2 import _cat_params, _transform_cat
    sides = {}
    src, dst = edges[0].to(_dev()), edges[1].to(_dev())
    with torch.no_grad():
        g = m.graph(data.edge_index, data.x.shape[0])
        h = data.x.float()
        for i, conv in enumerate(m.convs):
            H, C = conv.heads, conv.out_channels
            HC, P = H * C, ops.pad4(H * C)
            T = _transform_cat(h, *_cat_params(conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, conv.lin_r.bias, HC))
            sides[i] = ((T[:, :HC][src] + T[:, P:P + HC][dst]) > 0).view(-1, H, C).cpu()
            h = conv.run(h, g, epilogue="elu")
    return sides


def _joined(fx, prefix, name, k, got, full_ref):
    """(got, reference) with the fixture's values where it holds them: a tensor it keeps whole is compared with the fixture, one it
    keeps sampled rows of is compared with the fp64 restatement (tests/test_gatv2_host.py pins it to the fixture's rows and sums at
    1e-9) with the fixture's rows put in their places"""
    if f"{prefix}/{k}" not in fx:
        return got, full_ref
    if f"{prefix}_sum/{k}" not in fx:
        return got, fx[f"{prefix}/{k}"]
    ref = np.array(full_ref, np.float64)
    ref[fx[f"wrows/{name}"]] = fx[f"{prefix}/{k}"]
    return got, ref


def _ref_grads(fx, pre, name, P, x64, edges, y, tm, sides=None):
    """key, got -> (tensor to compare, reference): the fixture's gradients where it holds them, else the fp64 restatement's"""
    loss = F.nll_loss(restate(P, x64, edges, sides=sides)[tm], y[tm])
    grads = {k: g.numpy() for k, g in zip(P, torch.autograd.grad(loss, list(P.values())))}
    if sides is not None:
        return lambda k, got: (got, grads[k])
    return lambda k, got: _joined(fx, pre + "grad", name, k, got, grads[k])


@pytest.mark.parametrize("variant", ["raw", "und"])
@pytest.mark.parametrize("fixture", ["office", "small"])
def test_gradients_match_reference(fixture, variant):
    data, tm, dims, fx, models = _case(fixture, variant)
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    edges = edge_list(data.edge_index.cpu(), x64.shape[0])
    for name, hidden, heads, layers, seed in models:
        m = _model(dims, fx, name, hidden, heads, layers, seed)
        P = params64(m.state_dict())
        pre = f"{variant}/{name}/"
        ref = _ref_grads(fx, pre, name, P, x64, edges, y, tmc)
        loss = F.nll_loss(m(data)[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        named = {k: p for k, p in m.named_parameters() if p.grad is not None}
        assert sorted(named) == sorted(P)                                # every conv tensor, and no BatchNorm, receives a gradient
        bad = []
        for k, prm in named.items():
            got, want = ref(k, prm.grad.double().cpu().numpy())
            err = np.abs(got - want).max()
            print(f"{pre}{k}: grad err {err / np.abs(want).max():.3e} of max")
            if err > GRAD_BAR * np.abs(want).max():
                assert err <= KINK_CAP * np.abs(want).max(), f"{pre}{k}: {err:.3e} beyond any LeakyReLU kink flip"
                bad.append(k)
        if bad:
            # LeakyReLU kink flips: an fp32 x_l[j] + x_r[i] within rounding of zero may take the other side.  The fp64 restatement
            # with the GPU's side pattern must then meet the ordinary bar on every tensor.
            ref = _ref_grads(fx, pre, name, P, x64, edges, y, tmc, sides=_gpu_sides(m, data, edges))
            for k, prm in named.items():
                _grad_ok(*ref(k, prm.grad.double().cpu().numpy()), f"{pre}{k} (GPU LeakyReLU pattern)")
            print(f"{pre}: LeakyReLU kink flips explained for {bad}")


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_adam_trajectory_matches_reference(fixture):
    for variant in ("raw", "und"):
        data, tm, dims, fx, models = _case(fixture, variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        edges = edge_list(data.edge_index.cpu(), x64.shape[0])
        for name, hidden, heads, layers, seed in models:
            m = _model(dims, fx, name, hidden, heads, layers, seed)
            pre = f"{variant}/{name}/"
            P = params64(m.state_dict())                    # the fp64 restatement's five steps: whatever the fixture does not hold
            named = {k: p for k, p in m.named_parameters() if k in P}
            if pre + "adam/convs.0.att" not in fx or pre + "adam_sum/convs.0.lin_l.weight" in fx:
                ropt = torch.optim.Adam(list(P.values()), lr=1e-3, weight_decay=5e-3)
                for _ in range(5):
                    ropt.zero_grad()
                    F.nll_loss(restate(P, x64, edges)[tmc], y[tmc]).backward()
                    ropt.step()
            ref = lambda k, got: _joined(fx, pre + "adam", name, k, got, P[k].detach().numpy())      # noqa: E731
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(m(data)[tm], data.y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            np.testing.assert_allclose(losses, fx[pre + "adam_loss"], rtol=1e-4, err_msg=pre)
            for k, prm in named.items():
                _grad_ok(*ref(k, prm.detach().double().cpu().numpy()), pre + "adam/" + k, rel=1e-4)


# ---- driver ------------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(dataset_name="office")


def _office_data():
    from bridged_gnn_amd.data import Data
    og = load_golden("office_a2d_graph.npz")
    dev = _dev()
    d = Data(x=torch.from_numpy(og["x"]).to(dev), edge_index=torch.from_numpy(og["edge_index"]).long().to(dev),
             y=torch.from_numpy(og["y"]).long().to(dev),
             **{k: torch.from_numpy(og[k]).to(dev) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False                    # main_graph_knowledge_transfer.py:404
    d.to_undirected_()                                 # :411
    return d


def _run(data, graphed, hist, **kw):
    from bridged_gnn_amd import gatv2, transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, seed=0, hidden=16, heads=1, verbose=False)
    cfg.update(kw)
    return gatv2.train_gatv2_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def _check_history(h, epochs=8):
    assert len(h["loss_train"]) == epochs and len(h["eval_res"]) == epochs and all(len(r) == 3 for r in h["eval_res"])
    assert np.isfinite(h["loss_train"]).all() and 0 <= h["best_epoch"] < epochs


def test_driver_returns_none_fills_history_and_graphed_run_equals_eager_run():
    data = _office_data()
    he, hg = {}, {}
    assert _run(data, False, he) is None and _run(data, True, hg) is None
    for h in (he, hg):
        _check_history(h)
    e, g = np.array(he["loss_train"]), np.array(hg["loss_train"])
    print("GATv2 dropout run, eager", e, "graphed", g, "max rel dev", (np.abs(g - e) / np.abs(e)).max())
    assert np.allclose(g, e, rtol=TRAJ_RTOL), (g, e)
    assert hg["eval_res"] == he["eval_res"] and hg["best_epoch"] == he["best_epoch"]


def test_driver_runs_three_layers_and_two_heads():
    data = _office_data()
    he, hg = {}, {}
    assert _run(data, False, he, num_layer=3, heads=2) is None and _run(data, True, hg, num_layer=3, heads=2) is None
    _check_history(he)
    _check_history(hg)
    assert np.allclose(hg["loss_train"], he["loss_train"], rtol=TRAJ_RTOL), (hg["loss_train"], he["loss_train"])


def test_save_writes_a_checkpoint_that_loads_back(tmp_path, monkeypatch):
    """the checkpoint of the best epoch, loaded strict=True into a fresh GATv2, gives bit for bit the log-probabilities of the
    training model at the moment it was saved (taken there by a wrapper round torch.save: an eval forward under no_grad, which
    draws no seed)"""
    from bridged_gnn_amd import gatv2, transfer
    data = _office_data()
    built, at_save = [], []

    class Recorded(gatv2.GATv2):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    real_save = torch.save

    def save(obj, path, *a, **kw):
        m = built[-1]
        was_training = m.training
        m.eval()
        with torch.no_grad():
            at_save.append(m(data).clone())
        m.train(was_training)
        return real_save(obj, path, *a, **kw)

    monkeypatch.setattr(gatv2, "GATv2", Recorded)
    monkeypatch.setattr(torch, "save", save)
    hist = {}
    _run(data, False, hist, save=True, ckpt_dir=str(tmp_path), num_epoch=4)
    monkeypatch.undo()
    path = os.path.join(str(tmp_path), "model_GATv2_office_share_best.ckpt")
    assert os.path.exists(path) and len(built) == 1 and len(at_save) >= 1
    ds = transfer.pyg_dataset(data)
    m = gatv2.GATv2(ds.num_features, 16, ds.num_classes, 2, 1, 0.6, 0.5).to(_dev()).eval()
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    with torch.no_grad():
        assert torch.equal(m(data), at_save[-1])                                   # the last save is the best epoch's
    assert transfer.test_noDTC(data, m) == hist["eval_res"][hist["best_epoch"]]
