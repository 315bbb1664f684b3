"""GPU: the GAT baseline (bridged_gnn_amd.gat, models/backbones.py:404-438) on the HIP attention aggregation -- the kernels against
the edge-list fp64 restatement of tests/test_gat_host.py on adversarial graphs (duplicates, existing self loops, isolated nodes, a
hub row and a hub source of >= 30 000 edges, extreme scores), the two dropout laws, the model against the reference's fp64
fixtures (tools/gen_golden_gat.py) and `train_gat_noDTC` eager and graphed.
Bars: those of test_gpu_gcn.py -- activations 1e-5 of the tensor's max + 1e-6, gradients 2e-5 of the max; a gradient beyond that
must be within 2e-4 and then meet 2e-5 against the fp64 restatement taken with the GPU's own LeakyReLU side pattern; Adam losses
and parameters 1e-4; eager against graphed loss series rtol 2e-4."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from test_gat_host import OFFICE_MODELS, SMALL_MODELS, SLOPE, conv_sparse, edge_list, params64, restate

pytestmark = pytest.mark.gpu

ACT_BAR, GRAD_BAR, KINK_CAP = 1e-5, 2e-5, 2e-4
TRAJ_RTOL = 2e-4
SHAPES = ((1, 1), (1, 2), (1, 5), (1, 31), (1, 128), (2, 5), (3, 8), (3, 64), (8, 16))


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
        from bridged_gnn_amd.gat import GatGraph
        self.n = n
        self.g = GatGraph(torch.from_numpy(ei).to(_dev()), n)
        rp = self.g.rowptr.cpu().long()
        self.src = self.g.col.cpu().long()
        self.dst = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
        keep = ei[0] != ei[1]
        assert self.src.shape[0] == int(keep.sum()) + n                            # input self loops dropped, one per node
        self.indeg = np.bincount(ei[1][keep], minlength=n)
        self.outdeg = np.bincount(ei[0][keep], minlength=n)


_GRAPHS = {}


def _shared_graph(key):
    """the graphs of the kernel tests, built once: (n, e, seed, hub)"""
    if key not in _GRAPHS:
        n, e, seed, hub = key
        _GRAPHS[key] = _G(_graph(n, e, seed, hub), n)
    return _GRAPHS[key]


SMALLG, HUBG = (3000, 30000, 1, 0), (40000, 40000, 2, 30000)


def _inputs(n, H, C, seed, att_scale=1.0):
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(seed)
    W = ops.pad4(H * C)
    T = torch.zeros(n, W)
    T[:, :H * C] = torch.from_numpy(rng.standard_normal((n, H * C)).astype(np.float32))
    a_s = torch.from_numpy((att_scale * rng.standard_normal((1, H, C)) / np.sqrt(C)).astype(np.float32))
    a_d = torch.from_numpy((att_scale * rng.standard_normal((1, H, C)) / np.sqrt(C)).astype(np.float32))
    b = torch.zeros(W)
    b[:H * C] = torch.from_numpy(rng.standard_normal(H * C).astype(np.float32))
    dy = torch.zeros(n, W)
    dy[:, :H * C] = torch.from_numpy(rng.standard_normal((n, H * C)).astype(np.float32))
    return T, a_s, a_d, b, dy


def _epi64(z, epi):
    return F.elu(z) if epi == "elu" else torch.log_softmax(z, 1) if epi == "log_softmax" else z


def _epilogues(H):
    return (None, "elu", "log_softmax") if H == 1 else (None, "elu")


def _forward_shape(G, H, C, seed):
    from bridged_gnn_amd import ops
    dev, n, HC = _dev(), G.n, H * C
    T, a_s, a_d, b, _ = _inputs(n, H, C, seed)
    Td, bd = T.to(dev), b.to(dev)
    s_src, s_dst = ops.gat_scores(Td, a_s.to(dev), a_d.to(dev), H, C)
    T64 = T[:, :HC].double().view(n, H, C)
    r_src, r_dst = (T64 * a_s.double()).sum(-1), (T64 * a_d.double()).sum(-1)
    what = f"H={H} C={C}"
    _act_ok(s_src.cpu(), r_src, what + " s_src")
    _act_ok(s_dst.cpu(), r_dst, what + " s_dst")
    z = r_src[G.src] + r_dst[G.dst]
    assert bool((z > 0).any()) and bool((z < 0).any()), "the scores must straddle 0"
    ref, rstate = conv_sparse(T64, a_s.double(), a_d.double(), G.src, G.dst, want_state=True)
    for epi in _epilogues(H):
        for bias in (bd, None):
            out, state, pre, alpha = ops.gat_aggregate(Td, s_src, s_dst, G.g.rowptr, G.g.col, n, H, C, bias=bias, epilogue=epi,
                                                       want_pre=True, return_alpha=True)
            z64 = ref + (b[:HC].double() if bias is not None else 0.0)
            tag = f"{what} epi={epi} bias={bias is not None}"
            _act_ok(out[:, :HC].cpu(), _epi64(z64, epi), tag)
            _act_ok(pre[:, :HC].cpu(), z64, tag + " pre")
            if out.shape[1] > HC:
                assert torch.count_nonzero(out[:, HC:]).item() == 0 and torch.count_nonzero(pre[:, HC:]).item() == 0, "pad columns must be 0"
    _act_ok(state[..., 0].cpu(), rstate[..., 0], what + " softmax max")
    _act_ok(state[..., 1].cpu(), rstate[..., 1], what + " softmax denominator")
    assert float(state[..., 1].min().item()) >= 1.0                      # the self loop: the shifted denominator is >= 1
    sums = torch.zeros(n, H, dtype=torch.float64).index_add_(0, G.dst, alpha.cpu().double())
    _act_ok(sums, torch.ones(n, H, dtype=torch.float64), what + " coefficients of a row sum to 1")


@pytest.mark.parametrize("H,C", SHAPES)
def test_forward_kernel_every_shape_epilogue_and_bias(H, C):
    G = _shared_graph(SMALLG)
    assert (G.indeg == 0).any()                                                     # isolated nodes: their row is the self loop alone
    _forward_shape(G, H, C, seed=10 + H * 131 + C)


def test_scores_past_the_grid_cap():
    """bgnn_gat_scores_f32 launches at most 4096 blocks of 256 (node, head) pairs and walks the rest in a grid-stride loop (DESIGN
    section 20); the other kernel tests stay at n * H <= 120 000"""
    from bridged_gnn_amd import ops
    dev, n, H, C = _dev(), 350_000, 3, 4
    assert n * H > 4096 * 256
    T, a_s, a_d, _, _ = _inputs(n, H, C, seed=4242)
    s_src, s_dst = ops.gat_scores(T.to(dev), a_s.to(dev), a_d.to(dev), H, C)
    T64 = T[:, :H * C].double().view(n, H, C)
    assert s_src.shape == s_dst.shape == (n, H)
    _act_ok(s_src.cpu(), (T64 * a_s.double()).sum(-1), "scores past the cap: s_src")
    _act_ok(s_dst.cpu(), (T64 * a_d.double()).sum(-1), "scores past the cap: s_dst")


def test_wide_requests_raise_shape_errors():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gat import GATConv
    dev = _dev()
    G = _shared_graph(SMALLG)
    for H, C in ((9, 4), (1, 129)):
        T = torch.zeros(G.n, ops.pad4(H * C), device=dev)
        with pytest.raises(RuntimeError, match="shape"):
            ops.gat_scores(T, torch.zeros(H * C, device=dev), torch.zeros(H * C, device=dev), H, C)
        with pytest.raises(RuntimeError, match="shape"):
            ops.gat_aggregate(T, torch.zeros(G.n, H, device=dev), torch.zeros(G.n, H, device=dev), G.g.rowptr, G.g.col, G.n, H, C)
        with pytest.raises(RuntimeError, match="shape"):
            GATConv(8, C, heads=H).to(dev)(torch.zeros(G.n, 8, device=dev), G.g)
    with pytest.raises(RuntimeError, match="shape"):                               # the fused log_softmax is for one head
        ops.gat_aggregate(torch.zeros(G.n, 8, device=dev), torch.zeros(G.n, 2, device=dev), torch.zeros(G.n, 2, device=dev),
                          G.g.rowptr, G.g.col, G.n, 2, 4, epilogue="log_softmax")


@pytest.mark.parametrize("H,C", [(3, 8), (1, 2)])
def test_extreme_scores_stay_finite_and_follow_the_fp64_softmax(H, C):
    """att scaled until |z| reaches 1e4.  The fp64 softmax is taken over the logits the kernel itself forms, e = leaky_relu(s_src[j]
    + s_dst[i]) in fp32 from its own fp32 scores (two IEEE operations, reproduced here on the host): at |e| ~ 2e3 one fp32 rounding
    of e is 1e-4, which no softmax can undo; what is under test is the shift by the row maximum, the exponentials and the
    normalisation at such logits."""
    from bridged_gnn_amd import ops
    dev = _dev()
    G = _shared_graph(SMALLG)
    n, HC = G.n, H * C
    T, a_s, a_d, b, _ = _inputs(n, H, C, seed=77, att_scale=3000.0)
    Td = T.to(dev)
    s_src, s_dst = ops.gat_scores(Td, a_s.to(dev), a_d.to(dev), H, C)
    z32 = s_src.cpu()[G.src] + s_dst.cpu()[G.dst]
    assert float(z32.abs().max()) >= 1e4 and bool((z32 > 1e3).any()) and bool((z32 < -1e3).any())
    e32 = torch.where(z32 > 0, z32, torch.tensor(SLOPE, dtype=torch.float32) * z32)
    ref, rstate = conv_sparse(T[:, :HC].double().view(n, H, C), None, None, G.src, G.dst, logits=e32.double(), want_state=True)
    out, state, _, alpha = ops.gat_aggregate(Td, s_src, s_dst, G.g.rowptr, G.g.col, n, H, C, return_alpha=True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(state).all())
    _act_ok(out[:, :HC].cpu(), ref, f"extreme H={H} C={C}")
    assert torch.equal(state[..., 0].cpu(), rstate[..., 0].float())                 # the maximum of the same fp32 logits: exact
    _act_ok(state[..., 1].cpu(), rstate[..., 1], f"extreme H={H} C={C} denominator")


def _backward_case(G, H, C, seed, epilogues, att_mask=None, p_att=0.0, seed_att=0):
    """kernel backward against fp64 autograd of the restatement with T, the two score tables and the bias as separate leaves
    (the kernel returns exactly those four gradients); the LeakyReLU side of every edge is the kernel's own (fp32 z > 0)"""
    from bridged_gnn_amd import ops
    dev, n, HC = _dev(), G.n, H * C
    T, a_s, a_d, b, dy = _inputs(n, H, C, seed)
    Td, bd, dyd = T.to(dev), b.to(dev), dy.to(dev)
    s_src, s_dst = ops.gat_scores(Td, a_s.to(dev), a_d.to(dev), H, C)
    sides = (s_src.cpu()[G.src] + s_dst.cpu()[G.dst]) > 0
    for epi in epilogues:
        out, state, pre, alpha = ops.gat_aggregate(Td, s_src, s_dst, G.g.rowptr, G.g.col, n, H, C, bias=bd, epilogue=epi, p_att=p_att,
                                                   seed_att=seed_att, want_pre=True, return_alpha=True)
        args = (Td, s_src, s_dst, state, alpha, pre, dyd, G.g.rowptr, G.g.col, G.g.t_rowptr, G.g.t_eid, G.g.t_dst, H, C)
        kw = dict(bias=bd, epilogue=epi, p_att=p_att, seed_att=seed_att)
        got = ops.gat_aggregate_bwd(*args, **kw)
        again = ops.gat_aggregate_bwd(*args, **kw)
        assert all(torch.equal(a, b2) for a, b2 in zip(got, again)), f"H={H} C={C} epi={epi}: two calls differ"
        t64 = T[:, :HC].double().view(n, H, C).requires_grad_(True)
        ss, sd = s_src.cpu().double().requires_grad_(True), s_dst.cpu().double().requires_grad_(True)
        b64 = b[:HC].double().requires_grad_(True)
        r = _epi64(conv_sparse(t64, None, None, G.src, G.dst, bias=b64, scores=(ss, sd), sides=sides, edge_scale=att_mask), epi)
        if att_mask is not None:
            _act_ok(out[:, :HC].cpu(), r.detach(), f"H={H} C={C} epi={epi} forward under the recovered mask")
        rt, rs, rd, rb = torch.autograd.grad((r * dy[:, :HC].double()).sum(), [t64, ss, sd, b64])
        what = f"n={n} H={H} C={C} epi={epi}"
        _grad_ok(got[0][:, :HC].cpu(), rt.reshape(n, HC), what + " dT")
        _grad_ok(got[1].cpu(), rs, what + " ds_src")
        _grad_ok(got[2].cpu(), rd, what + " ds_dst")
        _grad_ok(got[3].cpu(), rb, what + " grad_bias")
        if got[0].shape[1] > HC:
            assert torch.count_nonzero(got[0][:, HC:]).item() == 0


@pytest.mark.parametrize("H,C", SHAPES)
def test_backward_kernel_matches_fp64_autograd_and_is_deterministic(H, C):
    _backward_case(_shared_graph(SMALLG), H, C, seed=500 + H * 131 + C, epilogues=_epilogues(H))


@pytest.mark.parametrize("H,C", [(3, 64), (1, 2)])
def test_hub_row_and_hub_source_forward_and_backward(H, C):
    G = _shared_graph(HUBG)
    assert G.indeg.max() >= 30000 and G.outdeg.max() >= 30000 and (G.indeg == 0).any()
    if C == 64:
        # bgnn_conv_common.h launch_rows (attn_bwd_rows_kernel): at most 2048 blocks of 256 // LF (node, head) rows, lf_ladder: LF = 16
        # at C = 64 -- the backward's row pass takes a second trip here; at C = 2 (LF = 1) the cap is 524 288
        assert G.n * H > 2048 * (256 // 16)
    _forward_shape(G, H, C, seed=900 + C)
    _backward_case(G, H, C, seed=950 + C, epilogues=("elu",))


def test_attention_dropout_law_and_backward_under_the_recovered_mask():
    from bridged_gnn_amd import ops
    dev = _dev()
    H, C, n, p = 3, 8, 20000, 0.6
    G = _shared_graph((n, 200000, 10, 0))
    E = G.src.shape[0]
    T, a_s, a_d, b, _ = _inputs(n, H, C, seed=21)
    Td = T.to(dev)
    s_src, s_dst = ops.gat_scores(Td, a_s.to(dev), a_d.to(dev), H, C)
    args = (G.g.rowptr, G.g.col, n, H, C)
    alpha = ops.gat_aggregate(Td, s_src, s_dst, *args, return_alpha=True)[3]
    assert float(alpha.min().item()) > 0.0
    at = ops.gat_aggregate(Td, s_src, s_dst, *args, p_att=p, seed_att=1234, return_alpha=True)[3]
    keep = at != 0                                                       # the zero pattern of a~ is the mask
    cnt, tot = int(keep.sum().item()), E * H
    sd = (tot * 0.4 * 0.6) ** 0.5
    print(f"kept {cnt} of {tot}: {(cnt - 0.4 * tot) / sd:+.2f} sd from 0.4")
    assert abs(cnt - 0.4 * tot) <= 6 * sd, f"kept {cnt} of {tot}"
    torch.testing.assert_close(at[keep], alpha[keep] / 0.4, rtol=1e-6, atol=0)
    # the mask is a function of (seed, edge position, head): other tables and scores, the same mask
    T2 = torch.roll(Td, 1, 0)
    s2 = ops.gat_scores(T2, a_d.to(dev), a_s.to(dev), H, C)
    assert torch.equal(ops.gat_aggregate(T2, s2[0], s2[1], *args, p_att=p, seed_att=1234, return_alpha=True)[3] != 0, keep)
    assert not torch.equal(ops.gat_aggregate(Td, s_src, s_dst, *args, p_att=p, seed_att=1235, return_alpha=True)[3] != 0, keep)
    word = torch.tensor([1000], dtype=torch.int64, device=dev)
    o1 = ops.gat_aggregate(Td, s_src, s_dst, *args, p_att=p, seed_att=1234, return_alpha=True)
    o2 = ops.gat_aggregate(Td, s_src, s_dst, *args, p_att=p, seed_att=234, seed_att_dev=word, return_alpha=True)
    assert torch.equal(o1[0], o2[0]) and torch.equal(o1[3], o2[3]) and torch.equal(o1[3], at), "seed + device word is the seed"
    # forward and backward with the recovered mask in the fp64 restatement: the by-source pass reaches the same draws through t_eid
    mask = keep.cpu().double() / 0.4
    _backward_case(G, H, C, seed=21, epilogues=(None, "elu"), att_mask=mask, p_att=p, seed_att=1234)


def test_feature_dropout_law_backward_and_seeds():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gat import GatGraph
    dev = _dev()
    n = 20000
    G = _shared_graph((n, 200000, 10, 0))
    eye = GatGraph(torch.zeros(2, 0, dtype=torch.int64, device=dev), n)             # self loops only: alpha = 1, out = T + bias
    for H, C in ((3, 8), (1, 31)):
        HC, W = H * C, ops.pad4(H * C)
        gen = torch.Generator().manual_seed(11)
        tbl = torch.rand(n, W, generator=gen)
        tbl[:, HC:] = 0
        tbl = tbl.to(dev)
        bias = (10.0 + torch.rand(W, generator=gen)).to(dev)             # pre-activation > 0 everywhere: ELU is the identity, y > 0 <=> kept
        a = torch.randn(HC, generator=gen).to(dev)
        s_src, s_dst = ops.gat_scores(tbl, a, a, H, C)

        def run(g, bias=bias, tbl=tbl, **kw):
            return ops.gat_aggregate(tbl, s_src, s_dst, g.rowptr, g.col, n, H, C, bias=bias, epilogue="elu", want_pre=True,
                                     return_alpha=True, **kw)
        z = run(G.g)[0][:, :HC]
        y, state, pre, alpha = run(G.g, p_drop=0.5, seed=1234)
        keep = y[:, :HC] > 0
        cnt, tot = int(keep.sum().item()), n * HC
        assert abs(cnt - tot / 2) <= 6 * (tot * 0.25) ** 0.5, f"H={H} C={C}: kept {cnt} of {tot}"
        torch.testing.assert_close(y[:, :HC][keep], 2.0 * z[keep], rtol=1e-6, atol=0)
        assert torch.count_nonzero(y[:, :HC][~keep]).item() == 0 and torch.count_nonzero(y[:, HC:]).item() == 0
        # the gradient: g = keep ? 2 dy : 0, seen through grad_bias = column sums of g
        dy = torch.randn(n, W, generator=gen)
        dy[:, HC:] = 0
        dy = dy.to(dev)
        want = torch.where(keep, 2.0 * dy[:, :HC], torch.zeros_like(dy[:, :HC]))
        gb = ops.gat_aggregate_bwd(tbl, s_src, s_dst, state, alpha, pre, dy, G.g.rowptr, G.g.col, G.g.t_rowptr, G.g.t_eid, G.g.t_dst, H, C,
                                   bias=bias, epilogue="elu", p_drop=0.5, seed=1234)[3]
        torch.testing.assert_close(gb.double(), want.double().sum(0), rtol=1e-5, atol=1e-4)
        # element by element through dT of the graph of self loops only (coefficient 1: the gather part of dT is g itself)
        y1, st1, pre1, al1 = run(eye, p_drop=0.5, seed=1234)
        assert torch.equal(y1[:, :HC] > 0, keep), "the mask depends on (seed, row, column) alone"
        ebwd = (eye.rowptr, eye.col, eye.t_rowptr, eye.t_eid, eye.t_dst, H, C)
        gt = ops.gat_aggregate_bwd(tbl, s_src, s_dst, st1, al1, pre1, dy, *ebwd, bias=bias, epilogue="elu", p_drop=0.5, seed=1234)[0]
        torch.testing.assert_close(gt[:, :HC], want, rtol=0, atol=0)
        # rows whose pre-activation is exactly 0 (zero features, zero bias): y is 0 kept or not, the gradient of a kept element is 2 dy
        zero_tbl, zero_bias = torch.zeros_like(tbl), torch.zeros_like(bias)
        s0 = ops.gat_scores(zero_tbl, a, a, H, C)
        y0, st0, pre0, al0 = ops.gat_aggregate(zero_tbl, s0[0], s0[1], eye.rowptr, eye.col, n, H, C, bias=zero_bias, epilogue="elu",
                                               p_drop=0.5, seed=1234, want_pre=True, return_alpha=True)
        assert torch.count_nonzero(y0).item() == 0 and torch.count_nonzero(pre0).item() == 0
        g0 = ops.gat_aggregate_bwd(zero_tbl, s0[0], s0[1], st0, al0, pre0, dy, *ebwd, bias=zero_bias, epilogue="elu", p_drop=0.5,
                                   seed=1234)[0]
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
        g, fx, models = load_golden("office_a2d_graph.npz"), load_golden("gat_office_a2d.npz"), OFFICE_MODELS
    else:
        g = fx = load_golden("gat_small.npz")
        models = SMALL_MODELS
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(dev)          # the driver's mask (y == -1 cleared, :404)
    ds = types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1)
    return data, tm, ds, fx, models


def _model(ds, fx, name, hidden, head, dropout=0.0):
    """the fixture's model: torch.manual_seed(0) and PyG's initialisers, checked against the stored parameters / their sums"""
    from bridged_gnn_amd.gat import GAT
    torch.manual_seed(0)
    m = GAT(ds, hidden=hidden, head=head, dropout=dropout)
    full, sums = sub(fx, f"{name}/param/"), sub(fx, f"{name}/param_sum/")
    assert sorted(full or sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        if full:
            assert np.array_equal(v.numpy(), full[k]), k
        else:
            vd = v.double()
            np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-6, atol=1e-300, err_msg=k)
    return m.to(_dev())


@pytest.mark.parametrize("variant", ["raw", "und"])
@pytest.mark.parametrize("fixture", ["office", "small"])
def test_forward_matches_reference(fixture, variant):
    data, _, ds, fx, models = _case(fixture, variant)
    rows, erows = torch.from_numpy(fx["rows"]), torch.from_numpy(fx["emb_rows"])
    x64 = data.x.double().cpu()
    edges = edge_list(data.edge_index.cpu(), x64.shape[0])
    for name, hidden, head in models:
        m = _model(ds, fx, name, hidden, head).eval()
        P = params64(m.state_dict())
        pre = f"{variant}/{name}/"
        with torch.no_grad():
            logp, emb = m(data).cpu(), m.get_emb(data).cpu()
            r_logp, r_emb = restate(P, x64, edges), restate(P, x64, edges, emb=True)
        _act_ok(logp[rows], fx[pre + "logp"], pre + "logp")                          # the reference, at the fixture's rows
        _act_ok(emb[erows], fx[pre + "emb"], pre + "emb")
        _act_ok(logp, r_logp, pre + "logp (every row, fp64 restatement)")
        _act_ok(emb, r_emb, pre + "emb (every row, fp64 restatement)")
        # the autograd path (grad enabled, eval mode) computes the same outputs
        _act_ok(m(data).detach().cpu()[rows], fx[pre + "logp"], pre + "logp (autograd path)")


def _gpu_sides(m, data, edges):
    """the LeakyReLU side the GPU takes for every edge and head of both convs: the sign of its own fp32 z"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gat import _aligned_rows, _pad_rows, _transform
    sides = {}
    with torch.no_grad():
        g = m.graph(data.edge_index, data.x.shape[0])
        h = data.x
        for name, conv in (("conv1", m.conv1), ("conv2", m.conv2)):
            H, C = conv.heads, conv.out_channels
            T = _aligned_rows(_transform(h.float(), _pad_rows(conv.lin_src.weight.detach())), H * C)
            s_src, s_dst = ops.gat_scores(T, conv.att_src.detach(), conv.att_dst.detach(), H, C)
            sides[name] = (s_src.cpu()[edges[0]] + s_dst.cpu()[edges[1]]) > 0
            h = conv.run(h, g, epilogue="elu")
    return sides


def _joined(fx, prefix, name, k, got, full_ref):
    """(got, reference) with the fixture's values where it holds them: a tensor it keeps whole is compared with the fixture, one it
    keeps sampled rows of is compared with the fp64 restatement (tests/test_gat_host.py pins it to the fixture's rows and sums at
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
    data, tm, ds, fx, models = _case(fixture, variant)
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    edges = edge_list(data.edge_index.cpu(), x64.shape[0])
    for name, hidden, head in models:
        m = _model(ds, fx, name, hidden, head).eval()
        P = params64(m.state_dict())
        pre = f"{variant}/{name}/"
        ref = _ref_grads(fx, pre, name, P, x64, edges, y, tmc)
        loss = F.nll_loss(m(data)[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        named = dict(m.named_parameters())
        assert sorted(named) == sorted(P)                                # the shared lin weight receives ONE gradient
        bad = []
        for k, prm in named.items():
            got, want = ref(k, prm.grad.double().cpu().numpy())
            err = np.abs(got - want).max()
            print(f"{pre}{k}: grad err {err / np.abs(want).max():.3e} of max")
            if err > GRAD_BAR * np.abs(want).max():
                assert err <= KINK_CAP * np.abs(want).max(), f"{pre}{k}: {err:.3e} beyond any LeakyReLU kink flip"
                bad.append(k)
        if bad:
            # LeakyReLU kink flips: an fp32 z within rounding of zero may take the other side.  The fp64 restatement with the
            # GPU's side pattern must then meet the ordinary bar on every tensor.
            ref = _ref_grads(fx, pre, name, P, x64, edges, y, tmc, sides=_gpu_sides(m, data, edges))
            for k, prm in named.items():
                _grad_ok(*ref(k, prm.grad.double().cpu().numpy()), f"{pre}{k} (GPU LeakyReLU pattern)")
            print(f"{pre}: LeakyReLU kink flips explained for {bad}")


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_adam_trajectory_matches_reference(fixture):
    for variant in ("raw", "und"):
        data, tm, ds, fx, models = _case(fixture, variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        edges = edge_list(data.edge_index.cpu(), x64.shape[0])
        for name, hidden, head in models:
            m = _model(ds, fx, name, hidden, head, dropout=0.0).eval()
            pre = f"{variant}/{name}/"
            named = dict(m.named_parameters())
            P = params64(m.state_dict())                    # the fp64 restatement's five steps: whatever the fixture does not hold
            if pre + "adam/conv1.att_src" not in fx or pre + "adam_sum/conv1.lin_src.weight" in fx:
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
    from bridged_gnn_amd import gat, transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, seed=0, hidden=16, head=3, dropout=0.6, verbose=False)
    cfg.update(kw)
    return gat.train_gat_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def test_driver_returns_none_fills_history_and_graphed_run_equals_eager_run():
    data = _office_data()
    he, hg = {}, {}
    assert _run(data, False, he) is None and _run(data, True, hg) is None
    for h in (he, hg):
        assert len(h["loss_train"]) == 8 and len(h["eval_res"]) == 8 and all(len(r) == 3 for r in h["eval_res"])
        assert np.isfinite(h["loss_train"]).all() and 0 <= h["best_epoch"] < 8
    e, g = np.array(he["loss_train"]), np.array(hg["loss_train"])
    print("GAT dropout run, eager", e, "graphed", g, "max rel dev", (np.abs(g - e) / np.abs(e)).max())
    assert np.allclose(g, e, rtol=TRAJ_RTOL), (g, e)
    assert hg["eval_res"] == he["eval_res"] and hg["best_epoch"] == he["best_epoch"]


def test_save_writes_a_checkpoint_that_loads_back(tmp_path, monkeypatch):
    """the checkpoint of the best epoch, loaded into a fresh GAT, gives bit for bit the log-probabilities of the training model at
    the moment it was saved (taken there by a wrapper round torch.save: an eval forward under no_grad, which draws no seed)"""
    from bridged_gnn_amd import gat, transfer
    data = _office_data()
    built, at_save = [], []

    class Recorded(gat.GAT):
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

    monkeypatch.setattr(gat, "GAT", Recorded)
    monkeypatch.setattr(torch, "save", save)
    hist = {}
    _run(data, False, hist, save=True, ckpt_dir=str(tmp_path), num_epoch=4)
    monkeypatch.undo()
    path = os.path.join(str(tmp_path), "model_GAT_office_share_best.ckpt")
    assert os.path.exists(path) and len(built) == 1 and len(at_save) >= 1
    m = gat.GAT(transfer.pyg_dataset(data), hidden=16, head=3).to(_dev()).eval()
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert m.conv1.lin_src.weight is m.conv1.lin_dst.weight
    with torch.no_grad():
        assert torch.equal(m(data), at_save[-1])                                   # the last save is the best epoch's
    assert transfer.test_noDTC(data, m) == hist["eval_res"][hist["best_epoch"]]
