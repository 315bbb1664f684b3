"""GPU: the APPNP baseline (bridged_gnn_amd.appnp, models/backbones.py:110-128) on the fused HIP K-step propagation -- the kernel
against an fp64 restatement of the recurrence on two adversarial graphs (duplicates, input self loops, isolated nodes,
asymmetric; one with a hub row and a hub source), its identities against the already-verified GCN aggregation, the backward
(the same call over the by-source view) against fp64 autograd, the feature-dropout passes, the model on the office graph and
`train_appnp_noDTC` (eager; `graphed=True` is refused, tests/test_appnp_host.py).
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max).  A plain fp32 torch
restatement of the recurrence stays within 1e-6 of max|ref| of fp64 on these graphs, so the bars leave about 10x for another
summation order.
Past the caps: graph C (70 000 nodes: more row tiles than a persistent grid has blocks at 8 and at 32 rows per
tile; two hubs of 30 000 edges, some 235 segments each, so the FINISH launch's edge loop takes 8 to 30 trips) forward at
D in {2, 31, 128}, K in {1, 2, 10}, both epilogues, with and without the hub tables, and backward against the recurrence over the
by-source view in fp64 (`_grad64`, pinned to fp64 autograd on graphs A and B).  A hub row there is a 30 000-term sum and a
sequential fp32 restatement is 2e-6 to 5e-6 of max off, so fp32 is no yardstick on graph C; the bars are the ones
test_gpu_gcn.py holds the same segmented summation to on its own 30 000-edge hub.  Measured on an MI355X, worst error as a share
of its bar: forward 0.044 / 0.257 / 0.382 at D = 2 / 31 / 128, backward 0.007 / 0.008 / 0.015.
Feature dropout: the ragged last quad (n * D % 4 != 0) at five shapes, [8193, 1025] past the 4096-block cap, and the keep mask
against a host restatement of the hash.  APPNP_Net: forward and parameter gradients with both dropout sites live
(`test_model_gradients_under_dropout`)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev, _gcn_graph, _graph, _sparse_parts

pytestmark = pytest.mark.gpu

GRAPHS = {"A": dict(n=3000, e=30000, seed=21, hub=0), "B": dict(n=2000, e=20000, seed=22, hub=700),
          "C": dict(n=70000, e=350000, seed=23, hub=30000)}
_CACHE = {}


def _case(name):
    """(n, GcnGraph, fp64 parts) of graph A (no hub), B (node 3: >= 700 in-edges, node 5: >= 700 out-edges) or C (more row tiles than
    the persistent grid has blocks, at every width; the two hubs have 30 000 edges, some 235 segments each); built once"""
    if name not in _CACHE:
        cfg = GRAPHS[name]
        n, hub = cfg["n"], cfg["hub"]
        if name == "C":
            # bgnn_conv_common.h persistent_grid: at most 8 blocks per CU; bgnn_appnp.hip appnp_step_kernel: RPB = 4 * (64 / (LF * EP))
            # rows per tile, lf_ladder: (LF, EP) = (32, 1) at D = 128 -> 8 rows, (1, 8) at D = 2 and (8, 1) at D = 31 -> 32 rows
            cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
            for rows_per_tile in (8, 32):
                ntiles = -(-n // rows_per_tile)
                assert ntiles > cap, f"graph C must have more tiles of {rows_per_tile} rows than the {cap} blocks of a persistent grid"
        ei = _graph(n, cfg["e"], seed=cfg["seed"], hub=hub)
        nl = ei[:, ei[0] != ei[1]]
        indeg, outdeg = np.bincount(nl[1], minlength=n), np.bincount(nl[0], minlength=n)
        assert (indeg == 0).any() and not np.array_equal(indeg, outdeg)                 # isolated nodes; asymmetric
        assert (ei[0] == ei[1]).any()                                                    # input self loops
        g = _gcn_graph(ei, n)
        if hub:
            assert indeg[3] >= hub and outdeg[5] >= hub
            assert g.hubs is not None and g.t_hubs is not None
            from bridged_gnn_amd import ops
            assert (ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT) == (256, 128)
            for tables in (g.hubs, g.t_hubs):                                            # several full segments and a ragged last one
                b = tables[3].cpu().numpy().reshape(-1, 2)
                lens = b[:, 1] - b[:, 0]
                assert (lens == 128).sum() >= 3 and (lens < 128).any()
                if name == "C":                                                          # the FINISH launch adds EP * U <= 32 partial rows per
                    nseg = np.diff(tables[2].cpu().numpy())                              # trip of its edge loop (bgnn_appnp.hip: niter): a hub
                    assert nseg.max() > 64, nseg                                         # of > 64 segments takes three trips at the least
        else:
            assert g.hubs is None and g.t_hubs is None
        _CACHE[name] = (n, g, _sparse_parts(torch.from_numpy(ei), n))
    return _CACHE[name]


def _step64(z, h, parts, alpha, transposed=False):
    src, dst, dinv = parts
    if transposed:
        src, dst = dst, src
    w = (dinv[src] * dinv[dst]).unsqueeze(1)
    return (1.0 - alpha) * torch.zeros_like(h).index_add_(0, dst, z[src] * w) + alpha * h


def _prop64(h, parts, K, alpha, epi=None, transposed=False):
    """the recurrence in fp64: z_0 = h, z_{k+1} = (1 - alpha) A^ z_k + alpha h, out = epi(z_K)"""
    z = h
    for _ in range(K):
        z = _step64(z, h, parts, alpha, transposed)
    return torch.log_softmax(z, 1) if epi == "log_softmax" else z


def _propagate(h, g, n, D, K, alpha, epi=None, hubs="own", view="dst"):
    from bridged_gnn_amd import ops
    if view == "dst":
        return ops.appnp_propagate(h, g.csr.rowptr, g.col, g.dinv, n, D, K, alpha, epilogue=epi, hubs=g.hubs if hubs == "own" else None)
    return ops.appnp_propagate(h, g.t_rowptr, g.t_dst, g.dinv, n, D, K, alpha, epilogue=epi, hubs=g.t_hubs if hubs == "own" else None)


DS = (1, 2, 3, 4, 5, 31, 32, 100, 128)
KS = (0, 1, 2, 10)


# ---- kernel level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_every_width_step_count_alpha_and_epilogue(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, parts = _case(name)
    rng = np.random.default_rng(31)
    worst = 0.0
    for D in DS:
        Dp = ops.pad4(D)
        h = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32))
        hd, h64 = h.to(dev), h[:, :D].double()
        for alpha in (0.1, 0.5):
            z, refs = h64, {}
            for k in range(max(KS) + 1):
                if k in KS:
                    refs[k] = z
                z = _step64(z, h64, parts, alpha)
            for K in KS:
                for epi in (None, "log_softmax"):
                    got = _propagate(hd, g, n, D, K, alpha, epi)
                    ref = torch.log_softmax(refs[K], 1) if epi else refs[K]
                    what = f"graph {name} D={D} K={K} alpha={alpha} epi={epi}"
                    _bar_ok(got[:, :D].cpu(), ref.numpy(), ACT_BAR, what)
                    worst = max(worst, (got[:, :D].cpu().double() - ref).abs().max().item() / (ACT_BAR * ref.abs().max().item() + 1e-6))
                    if Dp > D:
                        assert torch.count_nonzero(got[:, D:]).item() == 0, what + ": pad columns must be 0"
    print(f"graph {name}: worst forward error {worst:.3f} of its bar")


def test_hub_graph_walked_without_hub_tables():
    from bridged_gnn_amd import ops
    n, g, parts = _case("B")
    rng = np.random.default_rng(32)
    for D in (2, 31, 128):
        h = torch.from_numpy(rng.standard_normal((n, ops.pad4(D))).astype(np.float32))
        for epi in (None, "log_softmax"):
            got = _propagate(h.to(_dev()), g, n, D, 10, 0.1, epi, hubs=None)
            _bar_ok(got[:, :D].cpu(), _prop64(h[:, :D].double(), parts, 10, 0.1, epi).numpy(), ACT_BAR,
                    f"graph B without hub tables D={D} epi={epi}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_identities(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, _ = _case(name)
    rng = np.random.default_rng(33)
    for D in (2, 5, 31, 128):
        Dp = ops.pad4(D)
        h = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32)).to(dev)
        # alpha = 1: the teleport term alone, bit for bit, whatever K
        for K in (1, 2, 10):
            assert torch.equal(_propagate(h, g, n, D, K, 1.0)[:, :D], h[:, :D]), f"D={D} K={K}: alpha = 1 must return h"
        # K = 0: h, or its log_softmax
        assert torch.equal(_propagate(h, g, n, D, 0, 0.1)[:, :D], h[:, :D])
        _bar_ok(_propagate(h, g, n, D, 0, 0.1, "log_softmax")[:, :D].cpu(), torch.log_softmax(h[:, :D].double().cpu(), 1).numpy(),
                ACT_BAR, f"graph {name} D={D} K=0 log_softmax")
        # K = 1, alpha = 0: the GCN aggregation without bias
        agg = ops.gcn_aggregate(h, g.csr.rowptr, g.col, g.dinv, n, D, hubs=g.hubs)
        _bar_ok(_propagate(h, g, n, D, 1, 0.0)[:, :D].cpu(), agg[:, :D].cpu().numpy(), ACT_BAR, f"graph {name} D={D} K=1 alpha=0 vs gcn_aggregate")
        # K = 10 against ten gcn_aggregate calls plus torch mul / add
        z = h
        for _ in range(10):
            z = ops.gcn_aggregate(z, g.csr.rowptr, g.col, g.dinv, n, D, hubs=g.hubs).mul_(0.9).add_(h, alpha=0.1)
        _bar_ok(_propagate(h, g, n, D, 10, 0.1)[:, :D].cpu(), z[:, :D].cpu().numpy(), ACT_BAR, f"graph {name} D={D} K=10 vs the composition")
        _bar_ok(_propagate(h, g, n, D, 10, 0.1, "log_softmax")[:, :D].cpu(), F.log_softmax(z[:, :D], 1).cpu().numpy(), ACT_BAR,
                f"graph {name} D={D} K=10 log_softmax vs the composition")


@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_matches_fp64_autograd_and_is_deterministic(name):
    from bridged_gnn_amd.appnp import APPNP
    dev = _dev()
    n, g, parts = _case(name)
    rng = np.random.default_rng(34)
    prop = APPNP(10, 0.1)
    for D in (2, 31, 128):
        h = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
        dy = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
        for epi in (None, "log_softmax"):
            grads = []
            for _ in range(2):
                hd = h.to(dev).requires_grad_(True)
                out = prop.run(hd, g, epilogue=epi)
                grads.append(torch.autograd.grad((out * dy.to(dev)).sum(), hd)[0])
            assert torch.equal(grads[0], grads[1]), f"D={D} epi={epi}: two calls differ"
            h64 = h.double().requires_grad_(True)
            ref = torch.autograd.grad((_prop64(h64, parts, 10, 0.1, epi) * dy.double()).sum(), h64)[0]
            _bar_ok(grads[0].cpu(), ref.numpy(), GRAD_BAR, f"graph {name} D={D} epi={epi} grad_h")
            # the wrong view is visible on this graph: the by-destination walk of dy is far from the gradient
            if epi is None:
                wrong = _prop64(dy.double(), parts, 10, 0.1)
                assert (wrong - ref).abs().max().item() > 100 * GRAD_BAR * ref.abs().max().item()


# ---- graph C: past the persistent grid's cap, hubs of many segments ----------------------------------------------
CD = (2, 31, 128)
_C_REF = {}


def _c_ref(D):
    """graph C at width D, computed once and left unchanged: h (fp32 [n, pad4(D)], the pad columns hold deviates too), dy (fp32 [n, D])
    and the fp64 states z_1, z_2, z_10 of the recurrence at alpha = 0.1"""
    if D not in _C_REF:
        from bridged_gnn_amd import ops
        n, _, parts = _case("C")
        rng = np.random.default_rng([35, D])
        h = torch.from_numpy(rng.standard_normal((n, ops.pad4(D))).astype(np.float32))
        dy = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
        z, refs = h[:, :D].double(), {}
        for k in range(1, 11):
            z = _step64(z, h[:, :D].double(), parts, 0.1)
            if k in (1, 2, 10):
                refs[k] = z
        _C_REF[D] = (h, dy, refs)
    return _C_REF[D]


def _grad64(h64, dy64, parts, K, alpha, epi, zK=None):
    """d <epi(P h), dy> / dh in fp64 without autograd (ten saved steps of graph C at D = 128 are gigabytes): the operator is linear,
    so the gradient is the recurrence over the by-source view applied to g = dy or, under log_softmax, g = dy - exp(y) rowsum(dy)
    with y from the fp64 forward (zK: that forward's z_K where the caller has it)"""
    g = dy64
    if epi == "log_softmax":
        y = torch.log_softmax(_prop64(h64, parts, K, alpha) if zK is None else zK, 1)
        g = dy64 - torch.exp(y) * dy64.sum(1, keepdim=True)
    return _prop64(g, parts, K, alpha, transposed=True)


@pytest.mark.parametrize("name", ["A", "B"])
def test_gradient_by_linearity_equals_fp64_autograd(name):
    """the yardstick of graph C's backward, pinned to autograd where autograd is affordable"""
    n, _, parts = _case(name)
    rng = np.random.default_rng(36)
    for D in (2, 31):
        h64, dy64 = (torch.from_numpy(rng.standard_normal((n, D))) for _ in range(2))
        for epi in (None, "log_softmax"):
            hg = h64.clone().requires_grad_(True)
            ref = torch.autograd.grad((_prop64(hg, parts, 10, 0.1, epi) * dy64).sum(), hg)[0]
            got = _grad64(h64, dy64, parts, 10, 0.1, epi)
            assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), (name, D, epi)


@pytest.mark.parametrize("D", CD)
def test_forward_past_the_persistent_cap_with_many_segment_hubs(D):
    """every block of every launch walks more than one tile, and the FINISH launch's edge loop more than one trip: K in {1, 2, 10},
    both epilogues, with the graph's hub tables, and K = 10 once without them"""
    from bridged_gnn_amd import ops
    n, g, _ = _case("C")
    h, _, refs = _c_ref(D)
    hd = h.to(_dev())
    worst = 0.0
    for K, hubs in ((1, "own"), (2, "own"), (10, "own"), (10, None)):
        for epi in (None, "log_softmax"):
            got = _propagate(hd, g, n, D, K, 0.1, epi, hubs=hubs)
            ref = torch.log_softmax(refs[K], 1) if epi else refs[K]
            what = f"graph C D={D} K={K} epi={epi} hubs={hubs}"
            _bar_ok(got[:, :D].cpu(), ref.numpy(), ACT_BAR, what)
            worst = max(worst, (got[:, :D].cpu().double() - ref).abs().max().item() / (ACT_BAR * ref.abs().max().item() + 1e-6))
            if ops.pad4(D) > D:
                assert torch.count_nonzero(got[:, D:]).item() == 0, what + ": pad columns must be 0"
    print(f"graph C D={D}: worst forward error {worst:.3f} of its bar")


@pytest.mark.parametrize("D", CD)
def test_backward_past_the_persistent_cap_with_many_segment_hubs(D):
    """`APPNP(10, 0.1).run` under autograd on graph C (the by-source view: node 5's 30 000 out-edges are the hub row), both
    epilogues, twice with equal bits, against `_grad64`"""
    from bridged_gnn_amd.appnp import APPNP
    dev = _dev()
    n, g, parts = _case("C")
    if D >= 31:
        # bgnn_conv_common.h launch_bwd_rows (the log_softmax rule, conv_bwd_rows_kernel): at most 2048 blocks of 256 // LF rows,
        # lf_ladder: LF = 8 at D = 31, 32 at D = 128; at D = 2 (LF = 1) the cap is 524 288 rows and graph C stays under it
        assert n > 2048 * (256 // (8 if D == 31 else 32))
    h, dy, refs = _c_ref(D)
    prop = APPNP(10, 0.1)
    worst = 0.0
    for epi in (None, "log_softmax"):
        grads = []
        for _ in range(2):
            hd = h[:, :D].to(dev).requires_grad_(True)
            out = prop.run(hd, g, epilogue=epi)
            grads.append(torch.autograd.grad((out * dy.to(dev)).sum(), hd)[0])
        assert torch.equal(grads[0], grads[1]), f"D={D} epi={epi}: two calls differ"
        ref = _grad64(h[:, :D].double(), dy.double(), parts, 10, 0.1, epi, zK=refs[10])
        _bar_ok(grads[0].cpu(), ref.numpy(), GRAD_BAR, f"graph C D={D} epi={epi} grad_h")
        worst = max(worst, (grads[0].cpu().double() - ref).abs().max().item() / (GRAD_BAR * ref.abs().max().item() + 1e-6))
    print(f"graph C D={D}: worst backward error {worst:.3f} of its bar")


def test_envelope():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, _ = _case("A")
    h = torch.zeros(n, 132, device=dev)
    args = (g.csr.rowptr, g.col, g.dinv, n)
    with pytest.raises(RuntimeError, match="(?i)shape"):
        ops.appnp_propagate(h, *args, 129, 10, 0.1)
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|K must"):
        ops.appnp_propagate(h, *args, 4, -1, 0.1)
    for alpha in (-0.01, 1.01, float("nan")):
        with pytest.raises((RuntimeError, ValueError), match="(?i)shape|alpha"):
            ops.appnp_propagate(h, *args, 4, 10, alpha)
    with pytest.raises((RuntimeError, ValueError), match="(?i)align|stride"):
        ops.appnp_propagate(torch.zeros(n, 6, device=dev), *args, 5, 10, 0.1)            # row stride 6: not a multiple of 4
    with pytest.raises((RuntimeError, ValueError), match="(?i)align|stride"):
        ops.appnp_propagate(torch.zeros(n, 9, device=dev)[:, 1:], *args, 4, 10, 0.1)     # base 4 bytes off
    with pytest.raises((RuntimeError, ValueError), match="(?i)align|stride"):
        ops.appnp_propagate(h, *args, 4, 10, 0.1, out=torch.zeros(n, 6, device=dev))
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|epilogue"):
        ops.appnp_propagate(h, *args, 4, 10, 0.1, epilogue="relu")
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|rows"):
        ops.appnp_propagate(h[:-1], *args, 4, 10, 0.1)                                   # the graph is square


# ---- feature dropout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 64, 300])
def test_feature_dropout(D):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, p = 1000, 0.5
    gen = torch.Generator().manual_seed(41 + D)
    x = torch.randn(n, D, generator=gen).to(dev)
    b = torch.randn(D, generator=gen).to(dev)
    dy = torch.randn(n, D, generator=gen).to(dev)
    tot = n * D
    sd = (tot * p * (1 - p)) ** 0.5
    ones = torch.ones(n, D, device=dev)
    keep = ops.feature_dropout(ones, p, 1234) > 0                                        # the mask of (seed 1234, element index)
    cnt = int(keep.sum().item())
    print(f"D={D}: kept {cnt} of {tot}")
    assert abs(cnt - tot * (1 - p)) <= 3 * sd
    for relu in (False, True):
        for bias in (None, b):
            act = x if bias is None else x + bias
            act = torch.relu(act) if relu else act
            y = ops.feature_dropout(x, p, 1234, bias=bias, relu=relu)
            assert torch.equal(y, torch.where(keep, act / (1 - p), torch.zeros_like(act))), f"relu={relu} bias={bias is not None}"
            assert torch.equal(ops.feature_dropout(x, 0.0, 1234, bias=bias, relu=relu), act)       # p = 0: act(x + b)
        y = ops.feature_dropout(x, p, 1234, relu=relu)
        gx = ops.feature_dropout_bwd(dy, p, 1234, y=y if relu else None, relu=relu)
        want = torch.where(keep & (y > 0) if relu else keep, dy / (1 - p), torch.zeros_like(dy))
        assert torch.equal(gx, want), f"backward relu={relu}"
    assert torch.equal(ops.feature_dropout(x, 0.0, 7), x) and torch.equal(ops.feature_dropout_bwd(dy, 0.0, 7), dy)
    # seeds: the same seed the same mask, another seed or a device word another one, seed + word composes
    assert torch.equal(ops.feature_dropout(ones, p, 1234) > 0, keep)
    assert not torch.equal(ops.feature_dropout(ones, p, 1235) > 0, keep)
    word = torch.tensor([1000], dtype=torch.int64, device=dev)
    assert not torch.equal(ops.feature_dropout(ones, p, 1234, seed_dev=word) > 0, keep)
    assert torch.equal(ops.feature_dropout(ones, p, 234, seed_dev=word) > 0, keep)
    assert torch.equal(ops.feature_dropout_bwd(dy, p, 234, seed_dev=word), torch.where(keep, dy / (1 - p), torch.zeros_like(dy)))
    # in place, and the mask is the one the other dropout sites draw for (seed, row * D + column)
    xc = x.clone()
    assert ops.feature_dropout(xc, p, 1234, out=xc) is xc and torch.equal(xc, torch.where(keep, x / (1 - p), torch.zeros_like(x)))
    if D % 4 == 0:
        from test_gpu_gcn import _gcn_graph as gg
        eye = gg(np.zeros((2, 0), dtype=np.int64), n)
        big = torch.full((D,), 10.0, device=dev)
        y1 = ops.gcn_aggregate(torch.rand(n, D, device=dev), eye.csr.rowptr, eye.col, eye.dinv, n, D, bias=big, epilogue="relu",
                               p_drop=p, seed=1234)
        assert torch.equal(y1 > 0, keep)


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def _keep_by_hash(total, p, seed):
    """the keep mask of elements 0 .. total-1 restated on the host (bgnn_common.h drop_words, drop_consts): element e takes 16 bits of
    the word pair of quad e / 4 -- w0 low, w0 high, w1 low, w1 high -- and is kept when they reach round(p * 65536)"""
    nq = (total + 3) // 4
    assert nq < 2 ** 32 and 0 <= seed < 2 ** 64
    with np.errstate(over="ignore"):
        q = np.arange(nq, dtype=np.uint32)
        a = _fmix32(q * np.uint32(0x9E3779B1) + np.uint32(seed & 0xFFFFFFFF))
        b = _fmix32(np.uint32(seed >> 32) + a)                                           # the quad's high word is 0 below 2^32 quads
        w0 = _fmix32(a ^ b ^ np.uint32(0x2C1B3C6D))
        w1 = _fmix32(w0 + b + np.uint32(0x297A2D39))
    bits = np.stack([w0 & np.uint32(0xFFFF), w0 >> np.uint32(16), w1 & np.uint32(0xFFFF), w1 >> np.uint32(16)], axis=1).reshape(-1)
    return torch.from_numpy(bits[:total] >= np.uint32(int(p * 65536.0 + 0.5)))


def _feature_dropout_cases(n, D, p, cases, seed=1234):
    """forward and backward of `cases` = [(relu, bias present)] on an [n, D] activation against the mask read off
    `feature_dropout(ones)` and torch.where, bit for bit; outputs start as NaN, so an element no lane reaches is seen -> keep"""
    from bridged_gnn_amd import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(43 + n + D)
    x = torch.randn(n, D, generator=gen).to(dev)
    b = torch.randn(D, generator=gen).to(dev)
    dy = torch.randn(n, D, generator=gen).to(dev)

    def nan():
        return torch.full((n, D), float("nan"), device=dev)
    keep = ops.feature_dropout(torch.ones(n, D, device=dev), p, seed, out=nan()) > 0
    scale = 1.0 / (1.0 - p)                                                              # p in {0, 0.5}: exactly 1 or 2
    for relu, with_bias in cases:
        bias = b if with_bias else None
        act = x if bias is None else x + bias
        act = torch.relu(act) if relu else act
        y = ops.feature_dropout(x, p, seed, bias=bias, relu=relu, out=nan())
        assert torch.equal(y, torch.where(keep, act * scale, torch.zeros_like(act))), f"[{n}, {D}] p={p} relu={relu} bias={with_bias}"
        gx = ops.feature_dropout_bwd(dy, p, seed, y=y if relu else None, relu=relu, out=nan())
        want = torch.where(keep & (y > 0) if relu else keep, dy * scale, torch.zeros_like(dy))
        assert torch.equal(gx, want), f"[{n}, {D}] p={p} backward relu={relu} bias={with_bias}"
    return keep


@pytest.mark.parametrize("n,D", [(1001, 2), (1001, 3), (1001, 5), (3, 1), (1, 7)])
def test_feature_dropout_ragged_last_quad(n, D):
    """n * D % 4 != 0: the last quad goes element by element.  ReLU x bias x p in {0, 0.5}, forward and backward; the bias cases pin
    the column wrap inside a quad.  The tail draws the bits a full quad would: the mask is the first n * D entries of the mask of
    one row of pad4(n * D) ones, and both are the host restatement of the hash."""
    from bridged_gnn_amd import ops
    tot = n * D
    assert tot % 4 != 0                                                                  # bgnn_appnp.hip feature_dropout_kernel: `full = e + 3 < p.total`
    cases = [(relu, bias) for relu in (False, True) for bias in (False, True)]
    assert bool(_feature_dropout_cases(n, D, 0.0, cases).all())
    keep = _feature_dropout_cases(n, D, 0.5, cases)
    row = ops.feature_dropout(torch.ones(1, ops.pad4(tot), device=_dev()), 0.5, 1234) > 0
    assert torch.equal(keep.reshape(-1), row[0, :tot])
    assert torch.equal(keep.reshape(-1).cpu(), _keep_by_hash(tot, 0.5, 1234))


def test_feature_dropout_past_the_grid_cap():
    """more quads than 4096 blocks of 256 lanes hold, and a ragged last one: forward with bias and ReLU, backward with and without
    ReLU, the kept count, and the mask against the host restatement of the hash"""
    n, D, p = 8193, 1025, 0.5
    tot = n * D
    # bgnn_appnp.hip launch_fdrop: `if (grid > 4096) grid = 4096`, 256 lanes per block, one quad per lane and trip
    assert (tot + 3) // 4 > 4096 * 256 and tot % 4 == 1
    keep = _feature_dropout_cases(n, D, p, [(True, True), (False, False)])
    cnt = int(keep.sum().item())
    print(f"[{n}, {D}]: kept {cnt} of {tot}")
    assert abs(cnt - tot * (1 - p)) <= 3 * (tot * p * (1 - p)) ** 0.5
    assert torch.equal(keep.reshape(-1).cpu(), _keep_by_hash(tot, p, 1234))


# ---- model level -------------------------------------------------------------------------------------------------
ARGS =types.SimpleNamespace(dataset_name="office")


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


def _restate(P, x, parts, K=10, alpha=0.1, relu_mask=None):
    """fp64 APPNP_Net forward (no dropout); relu_mask: the ReLU pattern to use instead of the restatement's own"""
    z = x @ P["lin1.weight"].t() + P["lin1.bias"]
    z = torch.relu(z) if relu_mask is None else z * relu_mask
    z = z @ P["lin2.weight"].t() + P["lin2.bias"]
    return _prop64(z, parts, K, alpha, "log_softmax")


def _params64(m):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}


def test_model_forward_and_gradients_on_the_office_graph():
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.appnp import APPNP_Net
    data = _office_data()
    ds = transfer.pyg_dataset(data)
    n = data.x.shape[0]
    parts = _sparse_parts(data.edge_index.cpu(), n)
    torch.manual_seed(0)
    m = APPNP_Net(ds, hidden=64, dropout=0).to(_dev()).train()
    P = _params64(m)
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    seen = []
    hook = m.lin1.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
    lp = m(data)
    hook.remove()
    assert lp.shape == (n, ds.num_classes)
    _bar_ok(lp.detach().cpu(), _restate(P, x64, parts).detach().numpy(), ACT_BAR, "APPNP_Net forward (training mode, dropout 0)")
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(data), lp.detach()), "eval under no_grad must equal the training-mode forward at dropout 0"
    # gradients under the masked NLL, the fp64 restatement on the kernel's ReLU pattern
    F.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    mask = (seen[0] > 0).double().cpu()
    loss = F.nll_loss(_restate(P, x64, parts, relu_mask=mask)[tm], y[tm])
    ref = dict(zip(P, torch.autograd.grad(loss, list(P.values()))))
    for k, prm in m.named_parameters():
        _bar_ok(prm.grad.cpu(), ref[k].numpy(), GRAD_BAR, f"APPNP_Net grad {k}")


def test_model_gradients_under_dropout(monkeypatch):
    """APPNP_Net in training mode at dropout 0.5 (keep scale exactly 2): the two sites' patterns are read off their recorded
    (input, output) pairs -- site 1 keeps where `out != 0` (or the input is 0), site 2's ReLU-and-keep pattern is `out > 0` -- and
    the fp64 restatement applies them with the factor 2: forward at the activation bar, the four parameter gradients under the
    masked NLL at the gradient bar; a second forward draws other masks."""
    from bridged_gnn_amd import appnp, transfer
    data = _office_data()
    ds = transfer.pyg_dataset(data)
    n = data.x.shape[0]
    parts = _sparse_parts(data.edge_index.cpu(), n)
    torch.manual_seed(0)
    m = appnp.APPNP_Net(ds, hidden=64, dropout=0.5).to(_dev()).train()
    P = _params64(m)
    sites = []
    real = appnp._feature_drop

    def recording(x, p, relu):
        y = real(x, p, relu)
        sites.append((relu, p, x.detach(), y.detach()))
        return y
    monkeypatch.setattr(appnp, "_feature_drop", recording)
    lp = m(data)
    assert [(s[0], s[1]) for s in sites] == [(False, 0.5), (True, 0.5)]
    (_, _, x_in, x_out), (_, _, h_in, h_out) = sites
    keep1 = (x_out != 0) | (x_in == 0)
    open2 = h_out > 0
    assert torch.equal(x_out, torch.where(keep1, x_in * 2, torch.zeros_like(x_in)))
    assert torch.equal(h_out, torch.where(open2, h_in * 2, torch.zeros_like(h_in))) and bool((h_in[open2] > 0).all())
    for kept, among in ((keep1, x_in != 0), (open2, h_in > 0)):                           # each site drops about half of what it could drop
        k, t = int((kept & among).sum()), int(among.sum())
        assert t > 1000 and abs(k - 0.5 * t) <= 6 * (0.25 * t) ** 0.5, (k, t)
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    x1 = torch.where(keep1.cpu(), 2.0 * x64, torch.zeros_like(x64))
    mask2 = 2.0 * open2.double().cpu()
    _bar_ok(lp.detach().cpu(), _restate(P, x1, parts, relu_mask=mask2).detach().numpy(), ACT_BAR, "APPNP_Net forward (training mode, dropout 0.5)")
    F.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    loss = F.nll_loss(_restate(P, x1, parts, relu_mask=mask2)[tm], y[tm])
    ref = dict(zip(P, torch.autograd.grad(loss, list(P.values()))))
    for k, prm in m.named_parameters():
        _bar_ok(prm.grad.cpu(), ref[k].numpy(), GRAD_BAR, f"APPNP_Net grad {k} at dropout 0.5")
    m(data)
    assert len(sites) == 4
    assert not torch.equal(sites[2][3] != 0, x_out != 0) and not torch.equal(sites[3][3] > 0, open2), "a second forward draws other masks"


# ---- driver ------------------------------------------------------------------------------------------------------
def _run(data, graphed, hist, **kw):
    from bridged_gnn_amd import appnp, transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, seed=0, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return appnp.train_appnp_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def test_driver_follows_the_fp64_adam_run():
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.appnp import APPNP_Net
    data = _office_data()
    hist = {}
    assert _run(data, False, hist, dropout=0.0, use_scheduler=False) is None
    assert len(hist["loss_train"]) == 8 and len(hist["eval_res"]) == 8 and all(len(r) == 3 for r in hist["eval_res"])
    transfer.set_random_seed(0)
    P = _params64(APPNP_Net(transfer.pyg_dataset(data), hidden=64))
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    parts = _sparse_parts(data.edge_index.cpu(), x64.shape[0])
    opt = torch.optim.Adam(list(P.values()), lr=1e-3, weight_decay=5e-3)
    ref = []
    for _ in range(8):
        opt.zero_grad()
        loss = F.nll_loss(_restate(P, x64, parts)[tm], y[tm])
        loss.backward()
        opt.step()
        ref.append(loss.item())
    print("driver losses", hist["loss_train"], "fp64", ref)
    np.testing.assert_allclose(hist["loss_train"], ref, rtol=1e-5)
    assert hist["best_epoch"] == int(np.argmin(ref))


def test_dropout_run_is_seeded_and_differs_from_the_dropout_free_run():
    data = _office_data()
    h1, h2, h0 = {}, {}, {}
    assert _run(data, False, h1) is None and _run(data, False, h2) is None and _run(data, False, h0, dropout=0.0) is None
    a, b, c = (np.array(h["loss_train"]) for h in (h1, h2, h0))
    assert a.shape == (8,) and np.array_equal(a, b) and h1["eval_res"] == h2["eval_res"]      # the host generator's seeds, no atomics
    assert not np.allclose(c, a, rtol=1e-3)                                                     # the masks are drawn


def test_save_writes_a_checkpoint_that_loads_back(tmp_path):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.appnp import APPNP_Net
    data = _office_data()
    hist = {}
    _run(data, False, hist, save=True, ckpt_dir=str(tmp_path), num_epoch=4)
    path = os.path.join(str(tmp_path), "model_APPNP_office_share_best.ckpt")
    assert os.path.exists(path)
    m = APPNP_Net(transfer.pyg_dataset(data), hidden=64).to(_dev())
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert transfer.test_noDTC(data, m) == hist["eval_res"][hist["best_epoch"]]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    assert np.isfinite(transfer.train_noDTC(data, m, opt))
