"""GPU: the DeeperGCN baseline (bridged_gnn_amd.deepergcn, models/backbones.py:130-161) on the fused HIP softmax aggregation -- the
forward entry against an fp64 torch restatement of PyG 2.0.x's GENConv(aggr='softmax', learn_t=True) formulas (scatter_reduce amax,
index_add_) on the generator of test_gpu_gcn.py with the shapes of test_gpu_appnp.py, the edges EXACTLY as generated (no self loop
added or dropped; A: 3000 nodes, no hub; B: 2000 nodes, node 3 with >= 700 in-edges and node 5 with >= 700 out-edges; both with
duplicates, self loops, rows without in-edges, asymmetric; C: past the persistent grid's cap, forward only; A2: 20 000 nodes, no
hub, past the backward's grid at H = 128), its identities, the
backward entry against fp64 autograd, the layers under autograd, the model on the office graph and `train_deepergcn_noDTC`.
Inputs are 2 * randn, so t * v reaches a few hundred at t = 40 and would overflow without the running maximum.
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max); grad_t: |dt - dt64| <= 2e-5 * sum |g * w64|
with w64 = E_alpha[v^2] - o^2 in fp64.  Layer- and model-level references take every ReLU / dropout state, and the sign pattern of
each conv's input (the message is relu(x) + 1e-7), from the GPU forward's own tensors, as test_gpu_gcn2.py explains and does.
A plain fp32 torch restatement (same formulas, CPU, torch autograd) on graphs A and B at H in {5, 64, 128, 200} and t in
{1, 0.05, -0.7, 0, 40} is within FP32_FWD = 2.2e-6 of fp64 in the forward (worst: graph B at t = 1) and within FP32_GX = 9.7e-6 in
grad_x (worst: t = 40); its grad_t, which autograd forms through the uncentred softmax backward, is up to FP32_GT = 2.1e-4 of
sum |g w64| away at t = 40 and so misses the grad_t bar -- the reason the kernel sums the centred form.  The kernel's own
algorithm restated in fp32 on the CPU (one rounded lse per row and channel, a = exp(t v - lse), centred grad_t) takes 0.22 of the
forward bar, 0.41 of the grad_x bar (t = 40: half an ulp of lse, up to 1.5e-5 relative at |t v| in [256, 512), scales every alpha of
its row) and 0.003 of the grad_t bar, which leaves 2.4x and more for another summation order.
Measured on an MI355X, worst error as a share of its bar (each test prints its own): forward 0.026 (z) / 0.021 (lse) / 0.034 (o) on
graph A and 0.022 / 0.018 / 0.042 on graph B; identities 0.016 and 0.017; graph C 0.020 at H = 5 and 0.033 at H = 128 (its row of
30 000 in-edges was 1.4 of the bar in o before the running sums became compensated adds); backward 0.495 (grad_x) / 0.004 (grad_t)
on graph A, 0.365 / 0.005 on graph B, 0.325 / 0.001 at 3001 rows, 0.025 / 0.000 on graph A2; layers 0.293 on graph A and 0.099 on graph B; the model 0.050 at
1 layer and 0.067 at 3."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_appnp import GRAPHS, _office_data
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev, _graph

pytestmark = pytest.mark.gpu

# worst error of the plain fp32 CPU restatement as a share of max |ref| (forward, grad_x) and of sum |g w64| (grad_t), graphs A and B
FP32_FWD, FP32_GX, FP32_GT = 2.2e-6, 9.7e-6, 2.1e-4

HS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 100, 128, 129, 200)
TS = (1.0, 0.05, -0.7, 0.0, 40.0)
_CACHE = {}
_EXTRA = {"A1": dict(n=3001, e=30000, seed=24, hub=0), "A2": dict(n=20000, e=120000, seed=25, hub=0)}


def _case(name):
    """(n, SageGraph, src, dst) of graph A, B, C (test_gpu_appnp.GRAPHS) or A1 (3001 rows), edges as generated; built once"""
    if name not in _CACHE:
        from bridged_gnn_amd.sage import SageGraph
        cfg = GRAPHS.get(name) or _EXTRA[name]
        n, hub = cfg["n"], cfg["hub"]
        ei = _graph(n, cfg["e"], seed=cfg["seed"], hub=hub)
        indeg, outdeg = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
        assert (indeg == 0).any() and not np.array_equal(indeg, outdeg)                 # rows without in-edges; asymmetric
        assert (ei[0] == ei[1]).any()                                                    # self loops, ordinary edges here
        pairs = ei[0] * n + ei[1]
        assert np.unique(pairs).shape[0] < pairs.shape[0]                                # duplicates
        if hub:
            assert indeg[3] >= hub and outdeg[5] >= hub
        eid = torch.from_numpy(ei).to(_dev())
        g = SageGraph(eid, n)
        assert g.csr.num_edges == ei.shape[1]                                            # nothing added, nothing dropped
        _CACHE[name] = (n, g, eid[0], eid[1])
    return _CACHE[name]


def _agg64(x, src, dst, t, n, pos=None):
    """fp64 restatement -> (z, o, lse, w = E_alpha[v^2] - o^2); pos: the sign pattern to use for relu(x) instead of x's own"""
    v = (torch.relu(x) if pos is None else x * pos) + 1e-7
    vs = v[src]
    a = t * vs
    idx = dst.unsqueeze(1).expand_as(a)
    m = torch.full_like(x, float("-inf")).scatter_reduce(0, idx, a.detach(), "amax", include_self=True)
    has = torch.zeros(n, dtype=torch.bool, device=x.device).index_fill_(0, dst, True).unsqueeze(1)
    m = torch.where(has, m, torch.zeros_like(m))
    e = torch.exp(a - m[dst])
    s = torch.zeros_like(x).index_add_(0, dst, e)
    s1 = s + (~has)
    o = torch.zeros_like(x).index_add_(0, dst, e * vs) / s1
    v2 = torch.zeros_like(x).index_add_(0, dst, e * vs * vs) / s1
    lse = torch.where(has, m + torch.log(s1), torch.zeros_like(m))
    return o + x, o, lse, v2 - o * o


def _share(got, ref, bar):
    return (got.double() - ref).abs().max().item() / (bar * ref.abs().max().item() + 1e-6)


def _ok(got, ref, bar, what):
    _bar_ok(got.double().cpu(), ref.detach().cpu().numpy(), bar, what)
    return _share(got, ref.detach(), bar)


def _x(rng, n, Hp, dev):
    return torch.from_numpy((2.0 * rng.standard_normal((n, Hp))).astype(np.float32)).to(dev)


def _tt(t, dev):
    return torch.tensor([t], dtype=torch.float32, device=dev)


def _fwd(x, g, t, n, H, save=False):
    from bridged_gnn_amd import ops
    tabs = None
    if save:
        tabs = tuple(torch.full((n, ops.pad4(H)), float("nan"), device=x.device) for _ in range(2))
    z = ops.gen_softmax_aggregate(x, g.by_dst[0], g.by_dst[1], t, n, H, save=tabs)
    return z, tabs


# ---- forward entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_every_width_and_temperature(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(61)
    worst = [0.0, 0.0, 0.0]
    for H in HS:
        Hp = ops.pad4(H)
        x = _x(rng, n, Hp, dev)
        # x as a view of a wider buffer, once per width: what surrounds the view and the pad columns hold NaN
        wide = torch.full((n, Hp + 8), float("nan"), device=dev)
        wide[:, 4:4 + H] = x[:, :H]
        xv = wide[:, 4:4 + Hp]
        x64 = x[:, :H].double()
        for k, t in enumerate(TS):
            what = f"graph {name} H={H} t={t}"
            z64, o64, lse64, _ = _agg64(x64, src, dst, t, n)
            td = _tt(t, dev)
            ze, _ = _fwd(xv if k == 0 else x, g, td, n, H)
            zt, (lse, o) = _fwd(xv if k == 0 else x, g, td, n, H, save=True)
            assert torch.equal(ze, zt), what + ": evaluation and training forwards differ"
            worst[0] = max(worst[0], _ok(ze[:, :H], z64, ACT_BAR, what + " z"))
            worst[1] = max(worst[1], _ok(lse[:, :H], lse64, ACT_BAR, what + " lse"))
            worst[2] = max(worst[2], _ok(o[:, :H], o64, ACT_BAR, what + " o"))
            assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(o).all()), what
            if Hp > H:
                assert all(torch.count_nonzero(v[:, H:]).item() == 0 for v in (ze, lse, o)), what + ": pad columns must be 0"
    print(f"graph {name}: worst forward error {worst[0]:.3f} (z), {worst[1]:.3f} (lse), {worst[2]:.3f} (o) of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_identities(name):
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.sage import SageGraph
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(62)
    has = torch.zeros(n, dtype=torch.bool, device=dev).index_fill_(0, dst, True)
    assert 0 < int((~has).sum()) < n
    g2 = SageGraph(torch.stack([torch.cat([src, src]), torch.cat([dst, dst])]), n)      # every edge twice
    worst = 0.0
    for H in (3, 5, 32, 64, 100, 128, 200):
        Hp = ops.pad4(H)
        x = _x(rng, n, Hp, dev)
        # t = 0: the mean of the messages plus x
        v = (torch.relu(x) + 1e-7).contiguous()
        mean = ops.sage_mean_aggregate(v, g.by_dst[0], g.by_dst[1], n, H, root=x, mean=True)
        z0, _ = _fwd(x, g, _tt(0.0, dev), n, H)
        worst = max(worst, _ok(z0[:, :H], mean[:, :H].double(), ACT_BAR, f"graph {name} H={H} t=0 vs sage_mean_aggregate"))
        row = x[7:8, :].clone()
        same = row.expand(n, Hp).contiguous()
        for t in TS:
            td = _tt(t, dev)
            z, (lse, o) = _fwd(x, g, td, n, H, save=True)
            # rows without in-edges: x_i bit for bit, lse = 0 and o = 0
            assert torch.equal(z[~has][:, :H], x[~has][:, :H]), f"graph {name} H={H} t={t}: an isolated row is not x_i"
            assert torch.count_nonzero(o[~has]).item() == 0 and torch.count_nonzero(lse[~has]).item() == 0
            # two runs: the same bits
            z2, (lse2, o2) = _fwd(x, g, td, n, H, save=True)
            assert torch.equal(z, z2) and torch.equal(lse, lse2) and torch.equal(o, o2), f"graph {name} H={H} t={t}: two runs differ"
            # every edge doubled: the same softmax
            zd, _ = _fwd(x, g2, td, n, H)
            worst = max(worst, _ok(zd[:, :H], z[:, :H].double(), ACT_BAR, f"graph {name} H={H} t={t} doubled edges"))
            # neighbours that carry equal rows: that row's message, whatever t
            zs, _ = _fwd(same, g, td, n, H)
            want = torch.where(has.unsqueeze(1), torch.relu(same.double()) + 1e-7, torch.zeros_like(same, dtype=torch.float64)) + same.double()
            worst = max(worst, _ok(zs[:, :H], want[:, :H], ACT_BAR, f"graph {name} H={H} t={t} equal rows"))
    print(f"graph {name}: worst identity error {worst:.3f} of the bar")


@pytest.mark.parametrize("H", [5, 128])
def test_forward_past_the_persistent_cap(H):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("C")
    # bgnn_gen.hip gen_fwd_kernel: RPB = 4 * (64 / (LF * EP)) rows per tile; lf_ladder: (LF, EP) = (2, 4) at H = 5 -> 32 rows, (32, 1) at
    # H = 128 -> 8 rows; bgnn_conv_common.h persistent_grid: at most 8 blocks per CU
    rpb = {5: 32, 128: 8}[H]
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // rpb) > cap, f"graph C must have more tiles of {rpb} rows than the {cap} blocks of a persistent grid"
    rng = np.random.default_rng([63, H])
    x = _x(rng, n, ops.pad4(H), dev)
    worst = 0.0
    for t in (1.0, 40.0):
        z64, o64, lse64, _ = _agg64(x[:, :H].double(), src, dst, t, n)
        z, (lse, o) = _fwd(x, g, _tt(t, dev), n, H, save=True)
        worst = max(worst, _ok(z[:, :H], z64, ACT_BAR, f"graph C H={H} t={t} z"), _ok(lse[:, :H], lse64, ACT_BAR, f"graph C H={H} t={t} lse"),
                    _ok(o[:, :H], o64, ACT_BAR, f"graph C H={H} t={t} o"))
        if ops.pad4(H) > H:
            assert torch.count_nonzero(z[:, H:]).item() == 0
    print(f"graph C H={H}: worst forward error {worst:.3f} of the bar")


# ---- backward entry ----------------------------------------------------------------------------------------------
def _grads64(x64, g64, src, dst, t, n):
    xr = x64.clone().requires_grad_(True)
    tr = torch.tensor(t, dtype=torch.float64, device=x64.device, requires_grad=True)
    z, _, _, w = _agg64(xr, src, dst, tr, n)
    gx, gt = torch.autograd.grad((z * g64).sum(), [xr, tr])
    return gx, gt.item(), (g64 * w.detach()).abs().sum().item()


def _backward_case(name, H, t, rng, worst):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    Hp = ops.pad4(H)
    x = _x(rng, n, Hp, dev)
    td = _tt(t, dev)
    _, tabs = _fwd(x, g, td, n, H, save=True)
    t_rowptr, t_dst = g.by_dst[2], g.by_dst[3]
    first = None
    for rep in range(2):                                                                   # a second call with another g: nothing carried over
        gz = torch.from_numpy(rng.standard_normal((n, Hp)).astype(np.float32)).to(dev)
        what = f"graph {name} H={H} t={t} call {rep}"
        gx, gt = ops.gen_softmax_aggregate_bwd(x, gz, tabs, t_rowptr, t_dst, td, H)
        gx2, gt2 = ops.gen_softmax_aggregate_bwd(x, gz, tabs, t_rowptr, t_dst, td, H)
        assert torch.equal(gx, gx2) and torch.equal(gt, gt2), what + ": two runs differ"
        gx64, gt64, scale = _grads64(x[:, :H].double(), gz[:, :H].double(), src, dst, t, n)
        worst[0] = max(worst[0], _ok(gx[:, :H], gx64, GRAD_BAR, what + " grad_x"))
        err, tol = abs(gt.item() - gt64), GRAD_BAR * scale
        print(f"{what} grad_t: err {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"{what} grad_t: {gt.item()} vs {gt64}, err {err:.3e} > {tol:.3e}"
        worst[1] = max(worst[1], err / tol)
        if Hp > H:
            assert torch.count_nonzero(gx[:, H:]).item() == 0, what + ": pad columns must be 0"
        if rep == 0:
            first = gt.clone()
    assert not torch.equal(first, gt)


@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_matches_fp64_autograd_and_is_deterministic(name):
    rng = np.random.default_rng(64)
    worst = [0.0, 0.0]
    for H in (5, 64, 128, 200):
        for t in (1.0, -0.7, 40.0):
            _backward_case(name, H, t, rng, worst)
    print(f"graph {name}: worst backward error {worst[0]:.3f} (grad_x), {worst[1]:.3f} (grad_t) of the bar")


def test_backward_at_3001_rows():
    rng = np.random.default_rng(65)
    worst = [0.0, 0.0]
    for H, t in ((5, 1.0), (64, 40.0), (200, -0.7)):
        _backward_case("A1", H, t, rng, worst)
    print(f"3001 rows: worst backward error {worst[0]:.3f} (grad_x), {worst[1]:.3f} (grad_t) of the bar")


def test_backward_past_the_persistent_cap():
    """graph A2 (20 000 nodes, no hub): at H = 128 more tiles than the backward's grid has blocks, so blocks walk several tiles and
    several blocks' partial sums of grad_t are made of more than one tile"""
    n = _EXTRA["A2"]["n"]
    # bgnn_gen.hip launch_bwd: RPB = 4 * (64 / (LF * EP)) = 8 rows per tile at H = 128 (lf_ladder: LF = 32, EP = 1); the grid is
    # bgnn_conv_common.h persistent_grid (at most 8 blocks per CU), and never more than GEN_MAX_BLOCKS = 4096
    cap = min(8 * torch.cuda.get_device_properties(0).multi_processor_count, 4096)
    assert -(-n // 8) > cap, f"graph A2 must have more tiles of 8 rows than the {cap} blocks of the backward's grid"
    worst = [0.0, 0.0]
    _backward_case("A2", 128, 1.0, np.random.default_rng(66), worst)
    print(f"graph A2 H=128: worst backward error {worst[0]:.3f} (grad_x), {worst[1]:.3f} (grad_t) of the bar")


# ---- the layers under autograd -----------------------------------------------------------------------------------
def _ln64(x, w, b):
    return F.layer_norm(x, (x.shape[1],), w, b, 1e-5)


def _conv64(P, pre, x, src, dst, n, pos, mask):
    """fp64 GENConv from the parameters P[pre + ...]; pos: the sign pattern of x, mask: the ReLU state of the mlp, both the GPU's"""
    z = _agg64(x, src, dst, P[pre + "t"].reshape(()), n, pos=pos)[0]
    h = _ln64(z @ P[pre + "mlp.0.weight"].t() + P[pre + "mlp.0.bias"], P[pre + "mlp.1.weight"], P[pre + "mlp.1.bias"]) * mask
    return h @ P[pre + "mlp.4.weight"].t() + P[pre + "mlp.4.bias"]


def _record(monkeypatch):
    """record every ReLU / dropout site as (p, output) and every conv input, in forward order"""
    from bridged_gnn_amd import deepergcn
    sites, inputs = [], []
    real_drop, real_agg = deepergcn._feature_drop, deepergcn.GENConv.aggregate

    def rec_drop(x, p, relu, row_ids=None):
        y = real_drop(x, p, relu, row_ids)
        assert relu
        sites.append((p, y.detach()))
        return y

    def rec_agg(self, x, graph):
        inputs.append(x.detach())
        return real_agg(self, x, graph)
    monkeypatch.setattr(deepergcn, "_feature_drop", rec_drop)
    monkeypatch.setattr(deepergcn.GENConv, "aggregate", rec_agg)
    return sites, inputs


def _mult(site):
    p, y = site
    return (y > 0).double() / (1.0 - p)


def _to64(m, dev):
    return {k: v.detach().double().to(dev).requires_grad_(True) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", ["A", "B"])
def test_genconv_and_res_layer_gradients(name, monkeypatch):
    from bridged_gnn_amd.deepergcn import DeepGCNLayer, GENConv
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(66)
    sites, inputs = _record(monkeypatch)
    worst = 0.0
    for H in (5, 64, 128):
        torch.manual_seed(H)
        conv = GENConv(H, H, aggr="softmax", t=1.0, learn_t=True, num_layers=2, norm="layer").to(dev)
        with torch.no_grad():
            conv.t.fill_(1.7)
        x = _x(rng, n, H, dev)
        dy = torch.from_numpy(rng.standard_normal((n, H)).astype(np.float32)).to(dev)
        # the bare conv
        del sites[:], inputs[:]
        xd = x.clone().requires_grad_(True)
        y = conv(xd, g)
        names = [k for k, _ in conv.named_parameters()]
        got = torch.autograd.grad((y * dy).sum(), [xd] + [p for _, p in conv.named_parameters()])
        assert len(sites) == 1 and sites[0][0] == 0.0 and len(inputs) == 1
        P = _to64(conv, dev)
        x64 = x.double().requires_grad_(True)
        y64 = _conv64(P, "", x64, src, dst, n, (inputs[0] > 0).double(), _mult(sites[0]))
        worst = max(worst, _ok(y.detach(), y64, ACT_BAR, f"graph {name} H={H} GENConv forward"))
        ref = torch.autograd.grad((y64 * dy.double()).sum(), [x64] + [P[k] for k in names])
        for gg, rr, what in zip(got, ref, ["x"] + names):
            worst = max(worst, _ok(gg.reshape(rr.shape), rr, GRAD_BAR, f"graph {name} H={H} GENConv grad {what}"))
        with torch.no_grad():
            _ok(conv(x, g), y64, ACT_BAR, f"graph {name} H={H} GENConv under no_grad")
        # the res+ layer in training mode at dropout 0.5 (keep scale exactly 2)
        layer = DeepGCNLayer(conv, torch.nn.LayerNorm(H).to(dev), torch.nn.ReLU(inplace=True), block="res+", dropout=0.5, ckpt_grad=1).train()
        del sites[:], inputs[:]
        xd = x.clone().requires_grad_(True)
        y = layer(xd, g)
        lnames = [k for k, _ in layer.named_parameters()]
        got = torch.autograd.grad((y * dy).sum(), [xd] + [p for _, p in layer.named_parameters()])
        assert [s[0] for s in sites] == [0.5, 0.0] and len(inputs) == 1
        assert 0 < int((sites[0][1] > 0).sum()) < sites[0][1].numel()
        P = _to64(layer, dev)
        x64 = x.double().requires_grad_(True)
        h64 = _ln64(x64, P["norm.weight"], P["norm.bias"]) * _mult(sites[0])
        y64 = x64 + _conv64(P, "conv.", h64, src, dst, n, (inputs[0] > 0).double(), _mult(sites[1]))
        worst = max(worst, _ok(y.detach(), y64, ACT_BAR, f"graph {name} H={H} res+ forward"))
        ref = torch.autograd.grad((y64 * dy.double()).sum(), [x64] + [P[k] for k in lnames])
        for gg, rr, what in zip(got, ref, ["x"] + lnames):
            worst = max(worst, _ok(gg.reshape(rr.shape), rr, GRAD_BAR, f"graph {name} H={H} res+ grad {what}"))
    print(f"graph {name}: worst layer error {worst:.3f} of the bar")


# ---- model level -------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(dataset_name="office")


def _model64(P, L, x, src, dst, n, sites, inputs):
    """fp64 DeeperGCN forward on the GPU forward's ReLU / dropout states (in forward order) and conv-input sign patterns"""
    s, pos = iter(sites), iter(inputs)
    x = x @ P["node_encoder.weight"].t() + P["node_encoder.bias"]
    x = _conv64(P, "layers.0.conv.", x, src, dst, n, (next(pos) > 0).double(), _mult(next(s)))
    for l in range(1, L):
        h = _ln64(x, P[f"layers.{l}.norm.weight"], P[f"layers.{l}.norm.bias"]) * _mult(next(s))
        x = x + _conv64(P, f"layers.{l}.conv.", h, src, dst, n, (next(pos) > 0).double(), _mult(next(s)))
    x = _ln64(x, P["layers.0.norm.weight"], P["layers.0.norm.bias"]) * _mult(next(s))
    return torch.log_softmax(x @ P["lin.weight"].t() + P["lin.bias"], 1)


@pytest.mark.parametrize("L", [1, 3])
def test_model_forward_and_gradients_on_the_office_graph(L, monkeypatch):
    from bridged_gnn_amd import deepergcn, transfer
    dev = _dev()
    data = _office_data()
    ds = transfer.pyg_dataset(data)
    n = data.x.shape[0]
    src, dst = data.edge_index[0], data.edge_index[1]
    torch.manual_seed(0)
    m = deepergcn.DeeperGCN(ds, 64, L, dropout=0.0).to(dev).train()
    with torch.no_grad():
        for i, layer in enumerate(m.layers):
            layer.conv.t.fill_(1.0 + 0.5 * i)
    sites, inputs = _record(monkeypatch)
    lp = m(data)
    assert lp.shape == (n, ds.num_classes) and len(sites) == 2 * L and len(inputs) == L and all(s[0] == 0.0 for s in sites)
    train_sites, train_inputs = list(sites), list(inputs)
    P = _to64(m, dev)
    x64 = data.x.double()
    ref_lp = _model64(P, L, x64, src, dst, n, train_sites, train_inputs)
    worst = _ok(lp.detach(), ref_lp, ACT_BAR, f"DeeperGCN L={L} forward (training mode, dropout 0)")
    F.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    ref = dict(zip(P, torch.autograd.grad(F.nll_loss(ref_lp[data.train_mask], data.y[data.train_mask]), list(P.values()))))
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k
        worst = max(worst, _ok(prm.grad.reshape(ref[k].shape), ref[k], GRAD_BAR, f"DeeperGCN L={L} grad {k}"))
    # evaluation against training at dropout 0: nothing saved, no tables written
    m.eval()
    with torch.no_grad():
        le = m(data)
    worst = max(worst, _ok(le, lp.detach().double(), ACT_BAR, f"DeeperGCN L={L} eval against train at dropout 0"))
    print(f"DeeperGCN L={L}: worst error {worst:.3f} of the bar")
    # the state_dict round-trips
    torch.manual_seed(1)
    m2 = deepergcn.DeeperGCN(ds, 64, L).to(dev).eval()
    m2.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(m2(data), le)


# ---- driver ------------------------------------------------------------------------------------------------------
def _run(data, hist, **kw):
    from bridged_gnn_amd import deepergcn, transfer
    cfg = dict(repeat=1, num_epoch=6, use_scheduler=False, seed=0, num_layer=3, hidden=64, dropout=0.1, verbose=False)
    cfg.update(kw)
    return deepergcn.train_deepergcn_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, **cfg)


def test_driver_loss_falls_and_runs_are_seeded():
    data = _office_data()
    h0, h1, h2 = {}, {}, {}
    assert _run(data, h0, dropout=0.0, lr=1e-2) is None
    assert len(h0["loss_train"]) == 6 and len(h0["eval_res"]) == 6 and all(len(r) == 3 for r in h0["eval_res"])
    assert 0 <= h0["best_epoch"] < 6
    print("DeeperGCN driver losses", h0["loss_train"])
    assert all(np.isfinite(h0["loss_train"])) and h0["loss_train"][-1] < h0["loss_train"][0]
    assert _run(data, h1) is None and _run(data, h2) is None
    assert all(np.isfinite(h1["loss_train"]))
    assert h1["loss_train"] == h2["loss_train"] and h1["eval_res"] == h2["eval_res"]        # the host generator's seeds, no atomics
    with pytest.raises(NotImplementedError, match="graphed"):
        _run(data, {}, graphed=True)
