"""GPU: GraphSAGE (bridged_gnn_amd.sage, the --no_dtc model of models/backbones.py:440-498) on the HIP mean aggregation --
model outputs, gradients and a short Adam run against the reference's fp64 fixtures (tools/gen_golden_graphsage.py) and, on
every row and for what the office fixture leaves out, against an fp64 restatement (the one tests/test_graphsage_host.py pins to
the fixtures); then the two kernels against fp64 restatements on adversarial graphs."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub

pytestmark = pytest.mark.gpu

OFFICE_MODELS = (("l2h64", 2, 64), ("l1", 1, 16), ("l3h32", 3, 32))
ACT_BAR, GRAD_BAR, KINK_CAP = 1e-5, 2e-5, 2e-4


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _bar_ok(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max()
    tol = rel * np.abs(ref).max() + 1e-6
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _office(variant):
    from bridged_gnn_amd.data import Data
    dev = _dev()
    g = load_golden("office_a2d_graph.npz")
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(g["train_mask"]).to(dev)
    tm[data.y == -1] = False                                 # :404
    ds = types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1)
    return data, tm, ds


def _model(ds, fx, name, L, hidden, dropout=0.5):
    """the fixture's model: torch.manual_seed(0) and the reference's initialisers, checked against the stored parameter sums"""
    from bridged_gnn_amd.sage import GraphSAGE
    torch.manual_seed(0)
    m = GraphSAGE(ds, layer_num=L, hidden=hidden, root_weight=True, dropout=dropout)
    sums = sub(fx, f"{name}/param_sum/")
    assert sorted(sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, err_msg=k)
    return m.to(_dev())


def _restate(params, x, ei, n_convs=None, out_neighbours=False, log_softmax=True, relu_masks=None):
    """fp64 GraphSAGE on the CPU (eval); relu_masks: force the ReLU pattern of the hidden layers (kink flips)."""
    L = 1 + max(int(k.split(".")[1]) for k in params)
    src, dst = (ei[1], ei[0]) if out_neighbours else (ei[0], ei[1])
    n = x.shape[0]
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64)).clamp(min=1)
    n_convs = L if n_convs is None else n_convs
    h = x
    for i in range(n_convs):
        c = f"convs.{i}."
        agg = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add_(0, dst, h[src]) / cnt.unsqueeze(1)
        h = agg @ params[c + "lin_l.weight"].t() + params[c + "lin_l.bias"] + h @ params[c + "lin_r.weight"].t()
        if i < L - 1:
            h = h * relu_masks[i] if relu_masks is not None else torch.relu(h)
    return torch.log_softmax(h, 1) if (log_softmax and n_convs == L) else h


def _params64(m):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("variant", ["raw", "und"])
def test_office_forward_matches_reference(variant):
    fx = load_golden("graphsage_office_a2d.npz")
    rows = torch.from_numpy(fx["rows"])
    data, _, ds = _office(variant)
    x64, ei = data.x.double().cpu(), data.edge_index.cpu()
    for name, L, hidden in OFFICE_MODELS:
        m = _model(ds, fx, name, L, hidden).eval()
        P = _params64(m)
        pre = f"{variant}/{name}/"
        with torch.no_grad():
            outs = {"logp": (m(data), _restate(P, x64, ei)),
                    "logits": (m.get_logits(data), _restate(P, x64, ei, out_neighbours=True, log_softmax=False))}
            if L > 1:
                outs["emb"] = (m.get_emb(data), _restate(P, x64, ei, n_convs=L - 1, out_neighbours=True))
        for what, (got, ref) in outs.items():
            got = got.cpu()
            _bar_ok(got[rows], fx[pre + what], ACT_BAR, pre + what)                     # the reference, at the fixture's rows
            _bar_ok(got, ref.detach().numpy(), ACT_BAR, pre + what + " (every row, fp64 restatement)")
        # the autograd path (grad enabled, eval mode) computes the same outputs
        _bar_ok(m(data).detach().cpu()[rows], fx[pre + "logp"], ACT_BAR, pre + "logp (autograd path)")


def _ref_grads(fx, pre, P, x64, ei, y, tm, relu_masks=None):
    """the fixture's gradients where it holds them (graph as shipped), else those of the fp64 restatement"""
    if relu_masks is None and pre + "grad/convs.0.lin_l.weight" in fx:
        return {k: fx[pre + "grad/" + k] for k in P}
    loss = F.nll_loss(_restate(P, x64, ei, relu_masks=relu_masks)[tm], y[tm])
    return {k: g.numpy() for k, g in zip(P, torch.autograd.grad(loss, list(P.values())))}


@pytest.mark.parametrize("variant", ["raw", "und"])
def test_office_gradients_match_reference(variant):
    fx = load_golden("graphsage_office_a2d.npz")
    data, tm, ds = _office(variant)
    x64, ei, y, tmc = data.x.double().cpu(), data.edge_index.cpu(), data.y.cpu(), tm.cpu()
    for name, L, hidden in OFFICE_MODELS:
        m = _model(ds, fx, name, L, hidden).eval()
        P = _params64(m)
        pre = f"{variant}/{name}/"
        ref = _ref_grads(fx, pre, P, x64, ei, y, tmc)
        loss = F.nll_loss(m(data)[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        bad = []
        for k, prm in m.named_parameters():
            got = prm.grad.double().cpu().numpy()
            err = np.abs(got - ref[k]).max()
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
            ref = _ref_grads(fx, pre, P, x64, ei, y, tmc, relu_masks=masks)
            for k, prm in m.named_parameters():
                _bar_ok(prm.grad.cpu(), ref[k], GRAD_BAR, f"{pre}{k} (GPU ReLU pattern)")
            print(f"{pre}: ReLU kink flips explained for {bad}")


def test_office_adam_trajectory_matches_reference():
    fx = load_golden("graphsage_office_a2d.npz")
    for variant in ("raw", "und"):
        data, tm, ds = _office(variant)
        x64, ei, y, tmc = data.x.double().cpu(), data.edge_index.cpu(), data.y.cpu(), tm.cpu()
        for name, L, hidden in OFFICE_MODELS:
            m = _model(ds, fx, name, L, hidden, dropout=0.0).train()
            pre = f"{variant}/{name}/"
            ref = {}
            if pre + "adam/convs.0.lin_l.weight" in fx:
                ref = {k: fx[pre + "adam/" + k] for k, _ in m.named_parameters()}
            else:                                            # the fp64 restatement's five steps
                P = _params64(m)
                ropt = torch.optim.Adam(list(P.values()), lr=1e-3, weight_decay=5e-3)
                for _ in range(5):
                    ropt.zero_grad()
                    F.nll_loss(_restate(P, x64, ei)[tmc], y[tmc]).backward()
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


# ---- kernel level ------------------------------------------------------------------------------------------------
def _graph(n, e, seed, hubs=False):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    extra = [ei, ei[:, : e // 20], np.stack([np.arange(0, n, 7), np.arange(0, n, 7)])]   # duplicates + self loops
    if hubs:
        rng = np.random.default_rng(seed)
        extra.append(np.stack([rng.integers(0, n, 6000), np.full(6000, 3)]))     # node 3: >= 5000 in-edges
        extra.append(np.stack([np.full(6000, 5), rng.integers(0, n - n // 50, 6000)]))   # node 5: >= 5000 out-edges
    return np.concatenate(extra, axis=1).astype(np.int64)


def _fp64_forward(tbl, root, ei, n, epi, out_neighbours):
    src, dst = (ei[1], ei[0]) if out_neighbours else (ei[0], ei[1])
    s = torch.zeros(n, tbl.shape[1], dtype=torch.float64).index_add_(0, dst, tbl[src])
    c = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64))
    z = s / c.clamp(min=1).unsqueeze(1) + root
    if epi == "relu":
        return torch.relu(z)
    if epi == "log_softmax":
        return torch.log_softmax(z, 1)
    return z


def _views(ei_t, n):
    from bridged_gnn_amd.sage import SageGraph
    return SageGraph(ei_t, n)


DS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 100, 128, 200)


def test_forward_kernel_every_width_epilogue_direction():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 3000
    ei = _graph(n, 30000, seed=1, hubs=True)
    assert np.bincount(ei[1], minlength=n).max() >= 5000 and np.bincount(ei[0], minlength=n).max() >= 5000
    assert (np.bincount(ei[1], minlength=n) == 0).any()
    g = _views(torch.from_numpy(ei).to(dev), n)
    ei64 = torch.from_numpy(ei)
    rng = np.random.default_rng(2)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.from_numpy(rng.standard_normal((n, 2 * Dp)).astype(np.float32))
        tl, tr = T[:, :D].double(), T[:, Dp:Dp + D].double()
        Td = T.to(dev)
        for out_nb in (False, True):
            rowptr, col = g.view(out_nb)[:2]
            for epi in (None, "relu", "log_softmax"):
                if epi == "log_softmax" and D > 128:
                    continue
                got = ops.sage_mean_aggregate(Td[:, :Dp], rowptr, col, n, D, root=Td[:, Dp:], epilogue=epi)
                ref = _fp64_forward(tl, tr, ei64, n, epi, out_nb)
                _bar_ok(got[:, :D].cpu(), ref.numpy(), ACT_BAR, f"D={D} epi={epi} out_neighbours={out_nb}")
                if Dp > D:
                    assert torch.count_nonzero(got[:, D:]).item() == 0, "pad columns must be 0"


def test_forward_kernel_large_graph():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 200_000
    ei = _graph(n, 2_000_000, seed=3, hubs=True)
    g = _views(torch.from_numpy(ei).to(dev), n)
    ei64 = torch.from_numpy(ei)
    rng = np.random.default_rng(4)
    for D in (3, 64):
        T = torch.from_numpy(rng.standard_normal((n, 2 * ops.pad4(D))).astype(np.float32))
        Dp = ops.pad4(D)
        for out_nb in (False, True):
            rowptr, col = g.view(out_nb)[:2]
            epi = "log_softmax" if D == 3 else "relu"
            got = ops.sage_mean_aggregate(T[:, :Dp].to(dev), rowptr, col, n, D, root=T[:, Dp:].to(dev), epilogue=epi)
            ref = _fp64_forward(T[:, :D].double(), T[:, Dp:Dp + D].double(), ei64, n, epi, out_nb)
            _bar_ok(got[:, :D].cpu(), ref.numpy(), ACT_BAR, f"N=200k D={D} out_neighbours={out_nb}")


def test_backward_kernel_matches_fp64_autograd_and_is_deterministic():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 3000
    ei = _graph(n, 30000, seed=5, hubs=True)
    g = _views(torch.from_numpy(ei).to(dev), n)
    ei64 = torch.from_numpy(ei)
    rng = np.random.default_rng(6)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.from_numpy(rng.standard_normal((n, 2 * Dp)).astype(np.float32))
        dy = torch.from_numpy(rng.standard_normal((n, Dp)).astype(np.float32))
        dy[:, D:] = 0
        Td = T.to(dev)
        for out_nb in (False, True):
            rowptr, col, t_rowptr, t_col = g.view(out_nb)
            for epi in (None, "relu", "log_softmax"):
                if epi == "log_softmax" and D > 128:
                    continue
                y = ops.sage_mean_aggregate(Td[:, :Dp], rowptr, col, n, D, root=Td[:, Dp:], epilogue=epi)
                gt, gr = ops.sage_mean_aggregate_bwd(y, dy.to(dev), rowptr, t_rowptr, t_col, n, D, epilogue=epi)
                gt2, gr2 = ops.sage_mean_aggregate_bwd(y, dy.to(dev), rowptr, t_rowptr, t_col, n, D, epilogue=epi)
                assert torch.equal(gt, gt2) and torch.equal(gr, gr2), f"D={D} epi={epi}: two calls differ"
                tl = T[:, :D].double().requires_grad_(True)
                tr = T[:, Dp:Dp + D].double().requires_grad_(True)
                if epi == "relu":     # the kernel's ReLU pattern is the fp32 output's (y > 0)
                    out = _fp64_forward(tl, tr, ei64, n, None, out_nb) * (y[:, :D].cpu() > 0).double()
                else:
                    out = _fp64_forward(tl, tr, ei64, n, epi, out_nb)
                rl, rr = torch.autograd.grad((out * dy[:, :D].double()).sum(), [tl, tr])
                what = f"D={D} epi={epi} out_neighbours={out_nb}"
                _bar_ok(gt[:, :D].cpu(), rl.numpy(), GRAD_BAR, what + " dT_l")
                _bar_ok(gr[:, :D].cpu(), rr.numpy(), GRAD_BAR, what + " dT_r")


def test_dropout_mask_law_backward_and_seeds():
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 20000
    ei = _graph(n, 200000, seed=7)
    g = _views(torch.from_numpy(ei).to(dev), n)
    rowptr, col, t_rowptr, t_col = g.view(False)
    for D in (64, 31):
        Dp = ops.pad4(D)
        gen = torch.Generator().manual_seed(8)
        tbl = torch.rand(n, Dp, generator=gen).to(dev)
        root = (10.0 + torch.rand(n, Dp, generator=gen)).to(dev)      # pre-activation > 0 everywhere: y > 0 <=> kept
        z = ops.sage_mean_aggregate(tbl, rowptr, col, n, D, root=root)[:, :D]
        y = ops.sage_mean_aggregate(tbl, rowptr, col, n, D, root=root, epilogue="relu", p_drop=0.5, seed=1234)
        keep = y[:, :D] > 0
        cnt, tot = int(keep.sum().item()), n * D
        sd = (tot * 0.25) ** 0.5
        assert abs(cnt - tot / 2) <= 6 * sd, f"D={D}: kept {cnt} of {tot}"
        torch.testing.assert_close(y[:, :D][keep], 2.0 * z[keep], rtol=1e-6, atol=0)
        dy = torch.randn(n, Dp, generator=gen).to(dev)
        dy[:, D:] = 0
        _, gr = ops.sage_mean_aggregate_bwd(y, dy, rowptr, t_rowptr, t_col, n, D, epilogue="relu", p_drop=0.5)
        torch.testing.assert_close(gr[:, :D], torch.where(keep, 2.0 * dy[:, :D], torch.zeros_like(dy[:, :D])), rtol=0, atol=0)
        y2 = ops.sage_mean_aggregate(tbl, rowptr, col, n, D, root=root, epilogue="relu", p_drop=0.5, seed=1235)
        assert not torch.equal(y2[:, :D] > 0, keep), "two seeds gave the same mask"
        y3 = ops.sage_mean_aggregate(tbl, rowptr, col, n, D, root=root, epilogue="relu", p_drop=0.5, seed=1234)
        assert torch.equal(y3, y)


def test_c4_shaped_graph_forward_on_sampled_rows():
    from bridged_gnn_amd import synth
    from bridged_gnn_amd.sage import GraphSAGE
    dev = _dev()
    n = 1_000_000
    ei, _ = synth.bridged_graph(n // 2, n - n // 2, k_within=6, k_cross=20, n_extra=4_000_000, cluster=1024, seed=0)
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=9)).to(dev)
    data = types.SimpleNamespace(x=x, edge_index=torch.from_numpy(ei).to(dev))
    torch.manual_seed(0)
    m = GraphSAGE(types.SimpleNamespace(num_features=128, num_classes=2), layer_num=2, hidden=64).to(dev).eval()
    with torch.no_grad():
        logp = m(data)
        g = m.graph(data.edge_index, n)
        h1 = m.convs[0].run(x, g, epilogue="relu")
    rows = np.sort(np.random.default_rng(10).choice(n, 4096, replace=False))
    rowptr = g.csr.rowptr.cpu().numpy().astype(np.int64)
    colv = g.csr.col.cpu().numpy()
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}

    def conv(inp, i, rows_):            # fp64 conv on `rows_` from their in-neighbours only
        c = f"convs.{i}."
        out = []
        for r in rows_:
            nb = colv[rowptr[r]: rowptr[r + 1]]
            mean = inp(nb).mean(0) if nb.size else torch.zeros(P[c + "lin_l.weight"].shape[1], dtype=torch.float64)
            out.append(mean @ P[c + "lin_l.weight"].t() + P[c + "lin_l.bias"] + inp(np.array([r]))[0] @ P[c + "lin_r.weight"].t())
        return torch.stack(out)

    xs = lambda idx: x[torch.from_numpy(idx).to(dev)].double().cpu()
    ref1 = torch.relu(conv(xs, 0, rows))
    _bar_ok(h1[torch.from_numpy(rows).to(dev)].cpu(), ref1.numpy(), ACT_BAR, "C4 layer 1")
    hs = lambda idx: h1[torch.from_numpy(idx).to(dev)].double().cpu()
    ref2 = torch.log_softmax(conv(hs, 1, rows), 1)
    _bar_ok(logp[torch.from_numpy(rows).to(dev)].cpu(), ref2.numpy(), ACT_BAR, "C4 log-probs")
