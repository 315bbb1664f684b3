"""GPU: the GCNII baseline (bridged_gnn_amd.gcn2, models/backbones.py:163-197) on the fused HIP propagate-and-mix conv -- the
forward entry against an fp64 restatement of PyG's formula (index_add_ for A^, then addmm(m, m, weight1, beta=1-beta, alpha=beta))
on the adversarial graphs of test_gpu_appnp.py (A: 3000 nodes, no hub; B: 2000 nodes, a hub row and a hub source of >= 700 edges;
both with duplicates, input self loops, isolated nodes, asymmetric), its identities, graph C past the persistent grid's cap, the
backward dense entry, the layer's gradients under autograd, the model on the office graph and `train_gcn2_noDTC`.
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max).  A plain fp32 torch restatement stays
within 7.5e-7 (activations) and 7.1e-7 (gradients) of fp64 on graphs A and B at H in {5, 64, 128} with 1 and 4 layers, so the
bars leave more than 10x for another summation order; on graph C fp32 is 2.4e-6 to 4.3e-6 off in the forward and its gradients
differ by up to 6e-3 because a ReLU sign flips on a hub row.  Hence: every layer-level gradient check takes the ReLU and dropout
state from the GPU forward's own y (mask = y_gpu > 0, scale = 1 / (1 - p): the backward's contract), and graph C is forward-only.
At p = 0.5 the forward's reference applies the host restatement of the dropout hash (test_gpu_appnp._keep_by_hash).
Measured on an MI355X, worst error as a share of its bar (each test prints its own): forward 0.045 (y) / 0.013 (m) on graph A and
0.050 / 0.013 on graph B; graph C 0.014 / 0.031 / 0.040 (y) at H = 5 / 64 / 128; backward dense entry 0.023 at 3000 rows and 0.026
at 3001; layer gradients 0.022 on graph A and 0.018 on graph B."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_appnp import _case, _keep_by_hash, _office_data, _params64
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev, _sparse_parts

pytestmark = pytest.mark.gpu

HS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 100, 128)
MIXES = ((0.1, math.log(1.5)), (0.5, math.log(2.0)), (0.0, 0.0), (1.0, 1.0), (0.1, 0.0))
SEED = 1234


def _agg64(x, parts):
    src, dst, dinv = parts
    return torch.zeros_like(x).index_add_(0, dst, x[src] * (dinv[src] * dinv[dst]).unsqueeze(1))


def _conv64(a, x0, w, alpha, beta):
    """PyG's GCN2Conv with shared weights from a = A^ x: (m, (1 - beta) m + beta m weight1)"""
    m = (1.0 - alpha) * a + alpha * x0
    return m, torch.addmm(m, m, w, beta=1.0 - beta, alpha=beta)


def _mix_matrix(w, beta, pad=0.0):
    """M = (1 - beta) I + beta w as fp32 [pad4(H), pad4(H)]; `pad`: what the pad rows and columns hold"""
    from bridged_gnn_amd import ops
    H = w.shape[0]
    M = torch.full((ops.pad4(H), ops.pad4(H)), pad, dtype=torch.float32)
    M[:H, :H] = (1.0 - beta) * torch.eye(H) + beta * w
    return M


def _share(got, ref, bar):
    return (got.double() - ref).abs().max().item() / (bar * ref.abs().max().item() + 1e-6)


def _conv(x, x0, M, g, n, H, alpha, p=0.0, hubs="own", m_out=None):
    from bridged_gnn_amd import ops
    return ops.gcn2_conv(x, x0, M, g.csr.rowptr, g.col, g.dinv, n, H, alpha, p_drop=p, seed=SEED,
                         hubs=g.hubs if hubs == "own" else None, m_out=m_out)


# ---- forward entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_every_width_mix_and_dropout(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, parts = _case(name)
    rng = np.random.default_rng(51)
    worst_y = worst_m = 0.0
    for H in HS:
        Hp = ops.pad4(H)
        x, x0 = (torch.from_numpy(rng.standard_normal((n, Hp)).astype(np.float32)) for _ in range(2))
        w = torch.from_numpy((rng.standard_normal((H, H)) / math.sqrt(H)).astype(np.float32))
        a64 = _agg64(x[:, :H].double(), parts)
        keep = _keep_by_hash(n * H, 0.5, SEED).reshape(n, H)
        # x as a view of a wider buffer, once per width: what surrounds the view, the pad columns of x and x0 and the pad rows and
        # columns of M hold NaN, which must not reach y or m
        wide = torch.full((n, Hp + 8), float("nan"))
        wide[:, 4:4 + H] = x[:, :H]
        xv = wide.to(dev)[:, 4:4 + Hp]
        x0v = torch.full((n, Hp), float("nan"))
        x0v[:, :H] = x0[:, :H]
        xd, x0d = x.to(dev), x0.to(dev)
        for k, (alpha, beta) in enumerate(MIXES):
            m64, z64 = _conv64(a64, x0[:, :H].double(), w.double(), alpha, beta)
            Md = _mix_matrix(w, beta).to(dev)
            for p in (0.0, 0.5):
                what = f"graph {name} H={H} alpha={alpha} beta={beta:.3f} p={p}"
                mo = torch.full((n, Hp), float("nan"), device=dev)
                if k == 0:
                    y = _conv(xv, x0v.to(dev), _mix_matrix(w, beta, pad=float("nan")).to(dev), g, n, H, alpha, p, m_out=mo)
                else:
                    y = _conv(xd, x0d, Md, g, n, H, alpha, p, m_out=mo)
                ref = torch.relu(z64)
                if p > 0:
                    ref = torch.where(keep, 2.0 * ref, torch.zeros_like(ref))
                _bar_ok(y[:, :H].cpu(), ref.numpy(), ACT_BAR, what + " y")
                _bar_ok(mo[:, :H].cpu(), m64.numpy(), ACT_BAR, what + " m")
                worst_y, worst_m = max(worst_y, _share(y[:, :H].cpu(), ref, ACT_BAR)), max(worst_m, _share(mo[:, :H].cpu(), m64, ACT_BAR))
                if p > 0:
                    # the mask is the hash's: every element the reference keeps well above 0 is kept, every dropped one is 0
                    yc = y[:, :H].cpu()
                    assert torch.count_nonzero(yc[~keep]).item() == 0, what + ": a dropped element is not 0"
                    assert bool((yc[keep & (ref > 1e-3)] > 0).all()), what + ": a kept element is 0"
                if Hp > H:
                    assert torch.count_nonzero(y[:, H:]).item() == 0 and torch.count_nonzero(mo[:, H:]).item() == 0, what + ": pad columns must be 0"
    print(f"graph {name}: worst forward error {worst_y:.3f} (y) and {worst_m:.3f} (m) of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_identities(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, _ = _case(name)
    _, other, _ = _case("B" if name == "A" else "A")
    rng = np.random.default_rng(52)
    for H in (3, 5, 32, 64, 100, 128):
        Hp = ops.pad4(H)
        x, x0 = (torch.from_numpy(rng.standard_normal((n, Hp)).astype(np.float32)).to(dev) for _ in range(2))
        w = torch.from_numpy((rng.standard_normal((H, H)) / math.sqrt(H)).astype(np.float32))
        # beta = 0 and alpha = 0: M = I, y = relu(A^ x)
        eye = _mix_matrix(w, 0.0).to(dev)
        agg = ops.gcn_aggregate(x, g.csr.rowptr, g.col, g.dinv, n, H, hubs=g.hubs)
        _bar_ok(_conv(x, x0, eye, g, n, H, 0.0)[:, :H].cpu(), torch.relu(agg[:, :H]).cpu().numpy(), ACT_BAR, f"graph {name} H={H} vs relu(gcn_aggregate)")
        # alpha = 1: y = relu(x0 M), whatever the graph
        M = _mix_matrix(w, math.log(1.5)).to(dev)
        y1 = _conv(x, x0, M, g, n, H, 1.0)
        _bar_ok(y1[:, :H].cpu(), torch.relu(x0[:, :H].double().cpu() @ M[:H, :H].double().cpu()).numpy(), ACT_BAR, f"graph {name} H={H} alpha=1")
        k = min(n, other.num_nodes)
        if name == "A":                                   # graph B has fewer nodes: its rows against the same rows here
            y2 = _conv(x[:k].contiguous(), x0[:k].contiguous(), M, other, k, H, 1.0)
            assert torch.equal(y1[:k], y2), f"H={H}: alpha = 1 must not depend on the graph"
        # evaluation (no m written) and training forwards: the same bits; two calls: the same bits
        for p in (0.0, 0.5):
            ye = _conv(x, x0, M, g, n, H, 0.1, p)
            mo = torch.empty(n, Hp, device=dev)
            yt = _conv(x, x0, M, g, n, H, 0.1, p, m_out=mo)
            assert torch.equal(ye, yt), f"H={H} p={p}: evaluation and training forwards differ"
            assert torch.equal(ye, _conv(x, x0, M, g, n, H, 0.1, p)), f"H={H} p={p}: two calls differ"
        if name == "B":                                   # without the hub tables the hub rows are walked whole: within the bar
            yo, yn = _conv(x, x0, M, g, n, H, 0.1), _conv(x, x0, M, g, n, H, 0.1, hubs=None)
            _bar_ok(yn[:, :H].cpu(), yo[:, :H].cpu().numpy(), ACT_BAR, f"graph B H={H} without hub tables")


@pytest.mark.parametrize("H", [5, 64, 128])
def test_forward_past_the_persistent_cap(H):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, parts = _case("C")
    # bgnn_gcn2.hip Tile: TR = RPB * NB rows per tile, RPB = 4 * (64 / (LF * EP)), NB = 2 where RPB = 8; lf_ladder: (LF, EP) = (2, 4) at
    # H = 5 -> 32 rows, (16, 1) at H = 64 -> 16 rows, (32, 1) at H = 128 -> 2 * 8 rows; bgnn_conv_common.h persistent_grid: at most 8
    # blocks per CU
    rpb = {5: 32, 64: 16, 128: 16}[H]
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // rpb) > cap, f"graph C must have more tiles of {rpb} rows than the {cap} blocks of a persistent grid"
    rng = np.random.default_rng([53, H])
    Hp = ops.pad4(H)
    x, x0 = (torch.from_numpy(rng.standard_normal((n, Hp)).astype(np.float32)) for _ in range(2))
    w = torch.from_numpy((rng.standard_normal((H, H)) / math.sqrt(H)).astype(np.float32))
    alpha, beta = 0.1, math.log(1.5)
    m64, z64 = _conv64(_agg64(x[:, :H].double(), parts), x0[:, :H].double(), w.double(), alpha, beta)
    mo = torch.empty(n, Hp, device=dev)
    y = _conv(x.to(dev), x0.to(dev), _mix_matrix(w, beta).to(dev), g, n, H, alpha, m_out=mo)
    _bar_ok(y[:, :H].cpu(), torch.relu(z64).numpy(), ACT_BAR, f"graph C H={H} y")
    _bar_ok(mo[:, :H].cpu(), m64.numpy(), ACT_BAR, f"graph C H={H} m")
    print(f"graph C H={H}: worst forward error {_share(y[:, :H].cpu(), torch.relu(z64), ACT_BAR):.3f} (y) and "
          f"{_share(mo[:, :H].cpu(), m64, ACT_BAR):.3f} (m) of the bar")
    if Hp > H:
        assert torch.count_nonzero(y[:, H:]).item() == 0


# ---- backward dense entry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3000, 3001])
def test_backward_dense_entry(n):
    from bridged_gnn_amd import ops
    dev = _dev()
    rng = np.random.default_rng(54 + n)
    worst = 0.0
    for H in HS:
        Hp = ops.pad4(H)
        y = torch.from_numpy(np.maximum(rng.standard_normal((n, Hp)), 0.0).astype(np.float32))
        gy = torch.from_numpy(rng.standard_normal((n, Hp)).astype(np.float32))
        w = torch.from_numpy((rng.standard_normal((H, H)) / math.sqrt(H)).astype(np.float32))
        M = _mix_matrix(w, math.log(1.5))
        for p in (0.0, 0.5):
            gz, t, gx0 = ops.gcn2_conv_bwd(y.to(dev), gy.to(dev), M.to(dev), H, 0.1, p)
            gz64 = gy[:, :H].double() * (y[:, :H] > 0) / (1.0 - p)
            gm64 = gz64 @ M[:H, :H].double().t()
            for got, ref, what in ((gz, gz64, "gz"), (t, 0.9 * gm64, "t"), (gx0, 0.1 * gm64, "gx0")):
                _bar_ok(got[:, :H].cpu(), ref.numpy(), GRAD_BAR, f"n={n} H={H} p={p} {what}")
                worst = max(worst, _share(got[:, :H].cpu(), ref, GRAD_BAR))
                if Hp > H:
                    assert torch.count_nonzero(got[:, H:]).item() == 0, f"n={n} H={H} {what}: pad columns must be 0"
    print(f"n={n}: worst backward dense error {worst:.3f} of the bar")


# ---- the layer under autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_layer_gradients(name):
    from bridged_gnn_amd.gcn2 import GCN2Conv
    dev = _dev()
    n, g, parts = _case(name)
    rng = np.random.default_rng(55)
    worst = 0.0
    for H in (5, 64, 128):
        torch.manual_seed(H)
        conv = GCN2Conv(H, 0.1, 0.5, 1).to(dev)
        x, x0, dy = (torch.from_numpy(rng.standard_normal((n, H)).astype(np.float32)) for _ in range(3))
        for p in (0.0, 0.5):
            xd, x0d = x.to(dev).requires_grad_(True), x0.to(dev).requires_grad_(True)
            y = conv.run(xd, x0d, g, p_drop=p)
            got = torch.autograd.grad((y * dy.to(dev)).sum(), [xd, x0d, conv.weight1])
            # rule 1: the ReLU and dropout state is the GPU forward's own
            mask = (y.detach() > 0).double().cpu() / (1.0 - p)
            x64, x064, w64 = (v.double().requires_grad_(True) for v in (x, x0, conv.weight1.detach().cpu()))
            m64, z64 = _conv64(_agg64(x64, parts), x064, w64, conv.alpha, conv.beta)
            _bar_ok(y.detach().cpu(), (z64 * mask).detach().numpy(), ACT_BAR, f"graph {name} H={H} p={p} layer forward")
            ref = torch.autograd.grad((z64 * mask * dy.double()).sum(), [x64, x064, w64])
            for gg, rr, what in zip(got, ref, ("grad_x", "grad_x0", "grad_weight1")):
                _bar_ok(gg.cpu(), rr.numpy(), GRAD_BAR, f"graph {name} H={H} p={p} {what}")
                worst = max(worst, _share(gg.cpu(), rr, GRAD_BAR))
            with torch.no_grad():                                         # no_grad: nothing saved, no m written, the same bits at p = 0
                if p == 0:
                    assert torch.equal(conv.run(xd, x0d, g), y.detach())
            # PyG parity of forward(): the bare conv output, no ReLU
            if p == 0:
                _bar_ok(conv(xd.detach(), x0d.detach(), g).detach().cpu(), z64.detach().numpy(), ACT_BAR, f"graph {name} H={H} GCN2Conv.forward")
    print(f"graph {name}: worst layer gradient error {worst:.3f} of the bar")


# ---- model level -------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(dataset_name="office")


def _model64(P, L, alpha, betas, x, parts, masks=None):
    """fp64 GCN2 forward.  masks: None (no dropout, the restatement's own ReLU) or (keep0, relu0, keep1, [conv l's y > 0]) as
    multipliers that carry the keep scale"""
    if masks is not None:
        x = x * masks[0]
    h = x @ P["lins.0.weight"].t() + P["lins.0.bias"]
    x0 = torch.relu(h) if masks is None else h * masks[1]
    x = x0 if masks is None else x0 * masks[2]
    for l in range(L):
        _, z = _conv64(_agg64(x, parts), x0, P[f"convs.{l}.weight1"], alpha, betas[l])
        x = torch.relu(z) if masks is None else z * masks[3][l]
    return torch.log_softmax(x @ P["lins.1.weight"].t() + P["lins.1.bias"], 1)


@pytest.mark.parametrize("L,hidden", [(1, 64), (4, 64), (1, 20), (4, 20), (2, 132)])
def test_model_forward_and_gradients_with_every_dropout_site_live(L, hidden, monkeypatch):
    """GCN2 in training mode at dropout 0.5 (keep scale exactly 2): sites 0 and 1 are read off the recorded (input, output) pairs of
    the feature-dropout passes, the conv sites off each conv's output (y > 0), and the fp64 restatement applies them.  hidden = 132
    runs the composed route (outside the kernel's envelope)."""
    from bridged_gnn_amd import gcn2, transfer
    data = _office_data()
    ds = transfer.pyg_dataset(data)
    n = data.x.shape[0]
    parts = _sparse_parts(data.edge_index.cpu(), n)
    torch.manual_seed(0)
    m = gcn2.GCN2(ds, hidden, L, 0.1, 0.5, dropout=0.5).to(_dev()).train()
    assert list(m.state_dict()) == ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias"] + [f"convs.{l}.weight1" for l in range(L)]
    P = _params64(m)
    betas = [c.beta for c in m.convs]
    sites, outs = [], []
    real_drop, real_run = gcn2._feature_drop, gcn2.GCN2Conv.run

    def rec_drop(x, p, relu):
        y = real_drop(x, p, relu)
        sites.append((relu, p, x.detach(), y.detach()))
        return y

    def rec_run(self, x, x0, graph, p_drop=0.0):
        y = real_run(self, x, x0, graph, p_drop)
        outs.append(y.detach())
        return y
    monkeypatch.setattr(gcn2, "_feature_drop", rec_drop)
    monkeypatch.setattr(gcn2.GCN2Conv, "run", rec_run)
    lp = m(data)
    top = [s for s in sites if not (s[0] and s[1] > 0)]                   # the composed route's own ReLU + dropout passes aside
    assert [(s[0], s[1]) for s in top] == [(False, 0.5), (True, 0.0), (False, 0.5)] and len(outs) == L
    (_, _, a_in, a_out), (_, _, _, x0_out), (_, _, b_in, b_out) = top
    keep0, keep1 = (a_out != 0) | (a_in == 0), (b_out != 0) | (b_in == 0)
    assert torch.equal(a_out, torch.where(keep0, a_in * 2, torch.zeros_like(a_in)))
    assert torch.equal(b_out, torch.where(keep1, b_in * 2, torch.zeros_like(b_in))) and torch.equal(b_in, x0_out)
    assert all(0 < int((y > 0).sum()) < y.numel() for y in outs)
    masks = (2.0 * keep0.double().cpu(), (x0_out > 0).double().cpu(), 2.0 * keep1.double().cpu(), [2.0 * (y > 0).double().cpu() for y in outs])
    x64, yl, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    ref_lp = _model64(P, L, 0.1, betas, x64, parts, masks)
    _bar_ok(lp.detach().cpu(), ref_lp.detach().numpy(), ACT_BAR, f"GCN2 L={L} hidden={hidden} forward at dropout 0.5")
    F.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    ref = dict(zip(P, torch.autograd.grad(F.nll_loss(ref_lp[tm], yl[tm]), list(P.values()))))
    for k, prm in m.named_parameters():
        _bar_ok(prm.grad.cpu(), ref[k].numpy(), GRAD_BAR, f"GCN2 L={L} hidden={hidden} grad {k}")
    # evaluation: no dropout, no m written, nothing saved
    m.eval()
    with torch.no_grad():
        le = m(data)
    _bar_ok(le.cpu(), _model64(P, L, 0.1, betas, x64, parts).detach().numpy(), ACT_BAR, f"GCN2 L={L} hidden={hidden} eval forward")
    # the state_dict round-trips
    torch.manual_seed(1)
    m2 = gcn2.GCN2(ds, hidden, L, 0.1, 0.5).to(_dev()).eval()
    m2.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(m2(data), le)


# ---- driver ------------------------------------------------------------------------------------------------------
def _run(data, hist, **kw):
    from bridged_gnn_amd import gcn2, transfer
    cfg = dict(repeat=1, num_epoch=6, use_scheduler=False, seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return gcn2.train_gcn2_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, **cfg)


def test_driver_loss_falls_and_runs_are_seeded():
    data = _office_data()
    h0, h1, h2 = {}, {}, {}
    assert _run(data, h0, dropout=0.0, lr=1e-2) is None
    assert len(h0["loss_train"]) == 6 and len(h0["eval_res"]) == 6 and all(len(r) == 3 for r in h0["eval_res"])
    assert 0 <= h0["best_epoch"] < 6
    print("GCN2 driver losses", h0["loss_train"])
    assert all(np.isfinite(h0["loss_train"])) and h0["loss_train"][-1] < h0["loss_train"][0]
    assert _run(data, h1) is None and _run(data, h2) is None
    assert h1["loss_train"] == h2["loss_train"] and h1["eval_res"] == h2["eval_res"]        # the host generator's seeds, no atomics


def test_save_writes_a_checkpoint_that_loads_back(tmp_path):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.gcn2 import GCN2
    data = _office_data()
    hist = {}
    _run(data, hist, save=True, ckpt_dir=str(tmp_path), num_epoch=4)
    path = os.path.join(str(tmp_path), "model_GCN2_office_share_best.ckpt")
    assert os.path.exists(path)
    m = GCN2(transfer.pyg_dataset(data), 64, 2, 0.1, 0.5).to(_dev())
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert transfer.test_noDTC(data, m) == hist["eval_res"][hist["best_epoch"]]
