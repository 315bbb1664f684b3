"""GPU: the GCN baseline (bridged_gnn_amd.gcn, models/backbones.py:246-300) on the HIP normalised aggregation -- the kernels
against an fp64 restatement on adversarial graphs (duplicates, existing self loops, isolated nodes, a hub row and a hub source of
>= 30 000 edges), the model against the reference's fp64 fixtures (tools/gen_golden_gcn.py) and, on every row, against the dense
fp64 restatement tests/test_gcn_host.py pins to those fixtures, and `train_gnn_noDTC(gnn='GCN')` eager and graphed.
Bars: those of test_gpu_graphsage.py (activations 1e-5, gradients 2e-5 of each tensor's max, Adam parameters 1e-4)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from test_gcn_host import OFFICE_MODELS, SMALL_MODELS, norm_adj, restate

pytestmark = pytest.mark.gpu

ACT_BAR, GRAD_BAR, KINK_CAP = 1e-5, 2e-5, 2e-4
TRAJ_RTOL = 2e-4         # eager against graphed loss trajectories: the bar test_gpu_transfer_graphed.py uses for GraphSAGE


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _bar_ok(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max()
    tol = rel * np.abs(ref).max() + 1e-6
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


def _sparse_parts(ei, n):
    """(src, dst, dinv) of A' + I in fp64: input self loops dropped, one per node, duplicates kept"""
    keep = ei[0] != ei[1]
    loops = torch.arange(n)
    src, dst = torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64))
    return src, dst, deg.pow(-0.5)


def _fp64_forward(tbl, bias, parts, epi):
    src, dst, dinv = parts
    z = torch.zeros(dinv.shape[0], tbl.shape[1], dtype=torch.float64).index_add_(0, dst, tbl[src] * (dinv[src] * dinv[dst]).unsqueeze(1))
    if bias is not None:
        z = z + bias
    if epi == "relu":
        return torch.relu(z)
    if epi == "log_softmax":
        return torch.log_softmax(z, 1)
    return z


def _gcn_graph(ei, n):
    from bridged_gnn_amd.gcn import GcnGraph
    return GcnGraph(torch.from_numpy(ei).to(_dev()), n)


DS = (1, 2, 3, 4, 5, 31, 64, 100, 128)


def _forward_cases(n, e, seed, hub):
    from bridged_gnn_amd import ops
    dev = _dev()
    ei = _graph(n, e, seed=seed, hub=hub)
    indeg = np.bincount(ei[1][ei[0] != ei[1]], minlength=n)
    assert (indeg == 0).any()                                                   # isolated nodes: their row is the self loop alone
    if hub:
        assert indeg.max() >= hub and np.bincount(ei[0], minlength=n).max() >= hub
    g = _gcn_graph(ei, n)
    assert (g.hubs is not None) == bool(hub) and (g.t_hubs is not None) == bool(hub)
    parts = _sparse_parts(torch.from_numpy(ei), n)
    torch.testing.assert_close(g.dinv.cpu().double(), parts[2], rtol=1e-7, atol=0)
    rng = np.random.default_rng(seed + 1)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(Dp).astype(np.float32))
        Td, bd = T.to(dev), b.to(dev)
        for epi in (None, "relu", "log_softmax"):
            for bias in (bd, None):
                got = ops.gcn_aggregate(Td, g.csr.rowptr, g.col, g.dinv, n, D, bias=bias, epilogue=epi, hubs=g.hubs)
                ref = _fp64_forward(T[:, :D].double(), b[:D].double() if bias is not None else None, parts, epi)
                _bar_ok(got[:, :D].cpu(), ref.numpy(), ACT_BAR, f"hub={hub} D={D} epi={epi} bias={bias is not None}")
                if Dp > D:
                    assert torch.count_nonzero(got[:, D:]).item() == 0, "pad columns must be 0"
    return g, parts


def test_forward_kernel_every_width_epilogue_and_bias():
    _forward_cases(3000, 30000, seed=1, hub=0)


def test_forward_kernel_hub_row_and_hub_source():
    from bridged_gnn_amd import ops
    g, parts = _forward_cases(40000, 200000, seed=2, hub=30000)
    # the hub tables change how a row is walked, not what it sums: without them (one lane group per row) the bar holds as well
    n, D = 40000, 64
    T = torch.from_numpy(np.random.default_rng(3).standard_normal((n, D)).astype(np.float32))
    got = ops.gcn_aggregate(T.to(_dev()), g.csr.rowptr, g.col, g.dinv, n, D)
    _bar_ok(got.cpu(), _fp64_forward(T.double(), None, parts, None).numpy(), ACT_BAR, "hub graph walked without hub tables")


def test_wide_rows_run_as_slices_and_wide_log_softmax_raises():
    from bridged_gnn_amd import ops
    n, D = 3000, 200
    ei = _graph(n, 30000, seed=4)
    g = _gcn_graph(ei, n)
    parts = _sparse_parts(torch.from_numpy(ei), n)
    rng = np.random.default_rng(5)
    T = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(D).astype(np.float32))
    got = ops.gcn_aggregate(T.to(_dev()), g.csr.rowptr, g.col, g.dinv, n, D, bias=b.to(_dev()), epilogue="relu")
    _bar_ok(got.cpu(), _fp64_forward(T.double(), b.double(), parts, "relu").numpy(), ACT_BAR, "D=200 relu")
    with pytest.raises(RuntimeError, match="shape"):
        ops.gcn_aggregate(T.to(_dev()), g.csr.rowptr, g.col, g.dinv, n, D, epilogue="log_softmax")


def test_forward_kernel_large_graph_on_sampled_rows():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 200_000
    ei = _graph(n, 2_000_000, seed=6, hub=30000)
    g = _gcn_graph(ei, n)
    rowptr = g.csr.rowptr.cpu().numpy().astype(np.int64)
    colv = g.col.cpu().numpy()
    dinv = 1.0 / np.sqrt((rowptr[1:] - rowptr[:-1]).astype(np.float64))
    rng = np.random.default_rng(7)
    rows = np.unique(np.concatenate([rng.choice(n, 4096, replace=False), [3, 5]]))
    for D, epi in ((3, "log_softmax"), (64, "relu")):
        Dp = ops.pad4(D)
        T = rng.standard_normal((n, Dp)).astype(np.float32)
        b = rng.standard_normal(Dp).astype(np.float32)
        got = ops.gcn_aggregate(torch.from_numpy(T).to(dev), g.csr.rowptr, g.col, g.dinv, n, D, bias=torch.from_numpy(b).to(dev),
                                epilogue=epi, hubs=g.hubs)
        T64 = T[:, :D].astype(np.float64)
        ref = np.stack([dinv[r] * (dinv[colv[rowptr[r]:rowptr[r + 1]], None] * T64[colv[rowptr[r]:rowptr[r + 1]]]).sum(0) + b[:D]
                        for r in rows])
        ref = torch.from_numpy(ref)
        ref = torch.relu(ref) if epi == "relu" else torch.log_softmax(ref, 1)
        _bar_ok(got[torch.from_numpy(rows).to(dev), :D].cpu(), ref.numpy(), ACT_BAR, f"N=200k D={D}")


@pytest.mark.parametrize("hub", [0, 30000])
def test_backward_kernel_matches_fp64_autograd_and_is_deterministic(hub):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, e = (40000, 200000) if hub else (3000, 30000)
    ei = _graph(n, e, seed=8, hub=hub)
    g = _gcn_graph(ei, n)
    parts = _sparse_parts(torch.from_numpy(ei), n)
    rng = np.random.default_rng(9)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal(Dp).astype(np.float32))
        dy = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32))
        dy[:, D:] = 0
        Td, bd, dyd = T.to(dev), b.to(dev), dy.to(dev)
        for epi in (None, "relu", "log_softmax"):
            y = ops.gcn_aggregate(Td, g.csr.rowptr, g.col, g.dinv, n, D, bias=bd, epilogue=epi, hubs=g.hubs)
            gt, gb = ops.gcn_aggregate_bwd(y, dyd, g.t_rowptr, g.t_dst, g.dinv, n, D, epilogue=epi, hubs=g.t_hubs)
            gt2, gb2 = ops.gcn_aggregate_bwd(y, dyd, g.t_rowptr, g.t_dst, g.dinv, n, D, epilogue=epi, hubs=g.t_hubs)
            assert torch.equal(gt, gt2) and torch.equal(gb, gb2), f"D={D} epi={epi}: two calls differ"
            t64 = T[:, :D].double().requires_grad_(True)
            b64 = b[:D].double().requires_grad_(True)
            if epi == "relu":     # the kernel's ReLU pattern is the fp32 output's (y > 0)
                out = _fp64_forward(t64, b64, parts, None) * (y[:, :D].cpu() > 0).double()
            else:
                out = _fp64_forward(t64, b64, parts, epi)
            rt, rb = torch.autograd.grad((out * dy[:, :D].double()).sum(), [t64, b64])
            what = f"hub={hub} D={D} epi={epi}"
            _bar_ok(gt[:, :D].cpu(), rt.numpy(), GRAD_BAR, what + " grad_tbl")
            _bar_ok(gb.cpu(), rb.numpy(), GRAD_BAR, what + " grad_bias")
            if Dp > D:
                assert torch.count_nonzero(gt[:, D:]).item() == 0


def test_dropout_mask_law_backward_and_seeds():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 20000
    ei = _graph(n, 200000, seed=10)
    g = _gcn_graph(ei, n)
    for D in (64, 31):
        Dp = ops.pad4(D)
        gen = torch.Generator().manual_seed(11)
        tbl = torch.rand(n, Dp, generator=gen).to(dev)
        bias = (10.0 + torch.rand(Dp, generator=gen)).to(dev)           # pre-activation > 0 everywhere: y > 0 <=> kept
        args = (tbl, g.csr.rowptr, g.col, g.dinv, n, D)
        z = ops.gcn_aggregate(*args, bias=bias)[:, :D]
        y = ops.gcn_aggregate(*args, bias=bias, epilogue="relu", p_drop=0.5, seed=1234)
        keep = y[:, :D] > 0
        cnt, tot = int(keep.sum().item()), n * D
        sd = (tot * 0.25) ** 0.5
        assert abs(cnt - tot / 2) <= 6 * sd, f"D={D}: kept {cnt} of {tot}"
        torch.testing.assert_close(y[:, :D][keep], 2.0 * z[keep], rtol=1e-6, atol=0)
        assert torch.count_nonzero(y[:, :D][~keep]).item() == 0
        # the gradient: with a unit upstream gradient on ONE row pattern, g = keep ? 2 dy : 0, seen through grad_bias = column sums of g
        dy = torch.randn(n, Dp, generator=gen).to(dev)
        dy[:, D:] = 0
        _, gb = ops.gcn_aggregate_bwd(y, dy, g.t_rowptr, g.t_dst, g.dinv, n, D, epilogue="relu", p_drop=0.5)
        want = torch.where(keep, 2.0 * dy[:, :D], torch.zeros_like(dy[:, :D])).double().sum(0)
        torch.testing.assert_close(gb.double(), want, rtol=1e-5, atol=1e-4)
        # and element by element, through grad_tbl of a graph of self loops only (A^ = I: grad_tbl = g)
        eye = _gcn_graph(np.zeros((2, 0), dtype=np.int64), n)
        y1 = ops.gcn_aggregate(tbl, eye.csr.rowptr, eye.col, eye.dinv, n, D, bias=bias, epilogue="relu", p_drop=0.5, seed=1234)
        assert torch.equal(y1[:, :D] > 0, keep), "the mask depends on (seed, row, column) alone"
        gt, _ = ops.gcn_aggregate_bwd(y1, dy, eye.t_rowptr, eye.t_dst, eye.dinv, n, D, epilogue="relu", p_drop=0.5)
        torch.testing.assert_close(gt[:, :D], torch.where(keep, 2.0 * dy[:, :D], torch.zeros_like(dy[:, :D])), rtol=0, atol=0)
        y2 = ops.gcn_aggregate(*args, bias=bias, epilogue="relu", p_drop=0.5, seed=1235)
        assert not torch.equal(y2[:, :D] > 0, keep), "two seeds gave the same mask"
        y3 = ops.gcn_aggregate(*args, bias=bias, epilogue="relu", p_drop=0.5, seed=1234)
        assert torch.equal(y3, y)
        word = torch.tensor([1000], dtype=torch.int64, device=dev)
        y4 = ops.gcn_aggregate(*args, bias=bias, epilogue="relu", p_drop=0.5, seed=234, seed_dev=word)
        assert torch.equal(y4, y), "seed + device word is the seed"


# ---- model level -------------------------------------------------------------------------------------------------
def _case(fixture, variant):
    from bridged_gnn_amd.data import Data
    dev = _dev()
    if fixture == "office":
        g, fx, models = load_golden("office_a2d_graph.npz"), load_golden("gcn_office_a2d.npz"), OFFICE_MODELS
    else:
        g = fx = load_golden("gcn_small.npz")
        models = SMALL_MODELS
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(dev)          # the driver's mask (y == -1 cleared, :404)
    ds = types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1)
    return data, tm, ds, fx, models


def _model(ds, fx, name, L, hidden, dropout=0.5):
    """the fixture's model: torch.manual_seed(0) and PyG's initialisers, checked against the stored parameters / their sums"""
    from bridged_gnn_amd.gcn import GCNNet
    torch.manual_seed(0)
    m = GCNNet(ds, layer_num=L, hidden=hidden, dropout=dropout)
    full, sums = sub(fx, f"{name}/param/"), sub(fx, f"{name}/param_sum/")
    assert sorted(full or sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        if full:
            assert np.array_equal(v.numpy(), full[k]), k
        else:
            vd = v.double()
            np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
    return m.to(_dev())


def _params64(m):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("variant", ["raw", "und"])
@pytest.mark.parametrize("fixture", ["office", "small"])
def test_forward_matches_reference(fixture, variant):
    data, _, ds, fx, models = _case(fixture, variant)
    rows = torch.from_numpy(fx["rows"])
    x64 = data.x.double().cpu()
    A = norm_adj(data.edge_index.cpu(), x64.shape[0])
    for name, L, hidden in models:
        m = _model(ds, fx, name, L, hidden).eval()
        P = _params64(m)
        pre = f"{variant}/{name}/"
        with torch.no_grad():
            outs = {"logp": (m(data), restate(P, x64, A)), "logits": (m.get_logits(data), restate(P, x64, A, log_softmax=False))}
            if L > 1:
                outs["emb"] = (m.get_emb(data), restate(P, x64, A, n_convs=L - 1))
        for what, (got, ref) in outs.items():
            got = got.cpu()
            _bar_ok(got[rows], fx[pre + what], ACT_BAR, pre + what)                     # the reference, at the fixture's rows
            _bar_ok(got, ref.detach().numpy(), ACT_BAR, pre + what + " (every row, fp64 restatement)")
        # the autograd path (grad enabled, eval mode) computes the same outputs
        _bar_ok(m(data).detach().cpu()[rows], fx[pre + "logp"], ACT_BAR, pre + "logp (autograd path)")


def _ref_grads(fx, pre, P, x64, A, y, tm, relu_masks=None):
    """the fixture's gradients where it holds them, else those of the fp64 restatement"""
    if relu_masks is None and pre + "grad/convs.0.lin.weight" in fx:
        return {k: fx[pre + "grad/" + k] for k in P}
    loss = F.nll_loss(restate(P, x64, A, relu_masks=relu_masks)[tm], y[tm])
    return {k: g.numpy() for k, g in zip(P, torch.autograd.grad(loss, list(P.values())))}


@pytest.mark.parametrize("variant", ["raw", "und"])
@pytest.mark.parametrize("fixture", ["office", "small"])
def test_gradients_match_reference(fixture, variant):
    data, tm, ds, fx, models = _case(fixture, variant)
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    A = norm_adj(data.edge_index.cpu(), x64.shape[0])
    for name, L, hidden in models:
        m = _model(ds, fx, name, L, hidden).eval()
        P = _params64(m)
        pre = f"{variant}/{name}/"
        ref = _ref_grads(fx, pre, P, x64, A, y, tmc)
        loss = F.nll_loss(m(data)[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        bad = []
        for k, prm in m.named_parameters():
            got = prm.grad.double().cpu().numpy()
            err = np.abs(got - ref[k]).max()
            print(f"{pre}{k}: grad err {err / np.abs(ref[k]).max():.3e} of max")
            if err > GRAD_BAR * np.abs(ref[k]).max():
                assert err <= KINK_CAP * np.abs(ref[k]).max(), f"{pre}{k}: {err:.3e} beyond any ReLU kink flip"
                bad.append(k)
        if bad:
            # ReLU kink flips: an fp32 pre-activation within rounding of zero may take the other side.  The fp64 restatement
            # with the GPU's ReLU pattern must then meet the ordinary bar on every tensor.
            with torch.no_grad():
                g = m.graph(data.edge_index, data.x.shape[0])
                h, masks = data.x, []
                for conv in m.convs[:-1]:
                    h = conv.run(h, g, epilogue="relu")
                    masks.append(torch.from_numpy((h.cpu().numpy() > 0).astype(np.float64)))
            ref = _ref_grads(fx, pre, P, x64, A, y, tmc, relu_masks=masks)
            for k, prm in m.named_parameters():
                _bar_ok(prm.grad.cpu(), ref[k], GRAD_BAR, f"{pre}{k} (GPU ReLU pattern)")
            print(f"{pre}: ReLU kink flips explained for {bad}")


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_adam_trajectory_matches_reference(fixture):
    for variant in ("raw", "und"):
        data, tm, ds, fx, models = _case(fixture, variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        A = norm_adj(data.edge_index.cpu(), x64.shape[0])
        for name, L, hidden in models:
            m = _model(ds, fx, name, L, hidden, dropout=0.0).train()
            pre = f"{variant}/{name}/"
            if pre + "adam/convs.0.lin.weight" in fx:
                ref = {k: fx[pre + "adam/" + k] for k, _ in m.named_parameters()}
            else:                                            # the fp64 restatement's five steps
                P = _params64(m)
                ropt = torch.optim.Adam(list(P.values()), lr=1e-3, weight_decay=5e-3)
                for _ in range(5):
                    ropt.zero_grad()
                    F.nll_loss(restate(P, x64, A)[tmc], y[tmc]).backward()
                    ropt.step()
                ref = {k: v.detach().numpy() for k, v in P.items()}
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(m(data)[tm], data.y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            np.testing.assert_allclose(losses, fx[pre + "adam_loss"], rtol=1e-5, err_msg=pre)
            for k, prm in m.named_parameters():
                _bar_ok(prm.detach().cpu(), ref[k], 1e-4, pre + "adam/" + k)


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
    from bridged_gnn_amd import transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, gnn="GCN", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return transfer.train_gnn_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def test_driver_default_backbone_trains_gcn_and_follows_fp64():
    """`train_gnn_noDTC` with its own default `gnn` (GCN), dropout off: the loss series against the fp64 restatement's Adam run"""
    from bridged_gnn_amd import transfer
    data = _office_data()
    hist = {}
    assert transfer.train_gnn_noDTC(ARGS, transfer.pyg_dataset(data), data, repeat=1, num_epoch=6, seed=0, num_layer=2, hidden=64,
                                    use_scheduler=False, dropout=0.0, verbose=False, history=hist) is None
    assert len(hist["loss_train"]) == 6 and len(hist["eval_res"]) == 6 and all(len(r) == 3 for r in hist["eval_res"])
    from bridged_gnn_amd.gcn import GCNNet
    transfer.set_random_seed(0)
    m = GCNNet(transfer.pyg_dataset(data), 2, hidden=64)
    P = _params64(m)
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    A = norm_adj(data.edge_index.cpu(), x64.shape[0])
    opt = torch.optim.Adam(list(P.values()), lr=1e-3, weight_decay=5e-3)
    ref = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.nll_loss(restate(P, x64, A)[tm], y[tm])
        loss.backward()
        opt.step()
        ref.append(loss.item())
    print("driver losses", hist["loss_train"], "fp64", ref)
    np.testing.assert_allclose(hist["loss_train"], ref, rtol=1e-5)
    assert hist["best_epoch"] == int(np.argmin(ref))


def test_graphed_dropout_run_equals_the_eager_run():
    data = _office_data()
    he, hg = {}, {}
    assert _run(data, False, he) is None and _run(data, True, hg) is None
    e, g = np.array(he["loss_train"]), np.array(hg["loss_train"])
    print("GCN dropout run, max rel dev", (np.abs(g - e) / np.abs(e)).max())
    assert g.shape == (8,) and np.allclose(g, e, rtol=TRAJ_RTOL), (g, e)
    assert hg["eval_res"] == he["eval_res"] and hg["best_epoch"] == he["best_epoch"]


def test_save_writes_a_checkpoint_that_loads_back(tmp_path):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.gcn import GCNNet
    data = _office_data()
    hist = {}
    _run(data, False, hist, save=True, ckpt_dir=str(tmp_path), num_epoch=4)
    path = os.path.join(str(tmp_path), "model_GCN_office_share_best.ckpt")
    assert os.path.exists(path)
    m = GCNNet(transfer.pyg_dataset(data), 2, hidden=64).to(_dev())
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert transfer.test_noDTC(data, m) == hist["eval_res"][hist["best_epoch"]]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    assert np.isfinite(transfer.train_noDTC(data, m, opt))
