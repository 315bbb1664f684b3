"""CPU: the GCN fixtures (tools/gen_golden_gcn.py, made by the reference's GCNNet class, models/backbones.py:246-300) against an
fp64 DENSE restatement written here (A^ = D^-1/2 (A' + I) D^-1/2, A' without self loops, multiplicities kept) -- the checker of the
GPU tests --, the module's state_dict layout and seeded parameters, the command line, and the refusal of host tensors."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_golden, sub

OFFICE_MODELS = (("l2h64", 2, 64), ("l1", 1, 16), ("l3h32", 3, 32))
SMALL_MODELS = (("l2h8", 2, 8), ("l1", 1, 16), ("l3h6", 3, 6))


def norm_adj(ei, n):
    """A^ [n, n] fp64 (row = destination): self loops of the input dropped, one of weight 1 per node, duplicates counted"""
    A = torch.zeros(n, n, dtype=torch.float64)
    keep = ei[0] != ei[1]
    A.index_put_((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=torch.float64), accumulate=True)
    A += torch.eye(n, dtype=torch.float64)
    dinv = A.sum(1).pow(-0.5)
    return dinv.unsqueeze(1) * A * dinv.unsqueeze(0)


def restate(params, x, A, n_convs=None, log_softmax=True, relu_masks=None):
    """fp64 GCNNet forward (eval: no dropout); params: name -> tensor (convs.{i}.lin.weight, convs.{i}.bias)"""
    L = 1 + max(int(k.split(".")[1]) for k in params)
    n_convs = L if n_convs is None else n_convs
    for i in range(n_convs):
        x = A @ (x @ params[f"convs.{i}.lin.weight"].t()) + params[f"convs.{i}.bias"]
        if i < L - 1:
            x = x * relu_masks[i] if relu_masks is not None else torch.relu(x)
    return torch.log_softmax(x, dim=1) if (log_softmax and n_convs == L) else x


def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("gcn_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("gcn_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def fixture_params(d, name, F_in, C, L, hidden):
    """the fixture's initial parameters: stored (small fixture) or the seeded model rebuilt and checked against the stored
    fp64 (sum, sum of squares) of every tensor (office fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.gcn import GCNNet
    torch.manual_seed(0)
    sd = GCNNet(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden).state_dict()
    sums = sub(d, f"{name}/param_sum/")
    assert sorted(sums) == sorted(sd)
    for k, v in sd.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
    return {k: v.clone() for k, v in sd.items()}


def undirected(ei, n):
    """ToUndirected(merge=True): the coalesced union of both directions"""
    both = torch.cat([ei, ei.flip(0)], 1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


def _close(got, ref, rel=1e-10):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= rel * max(np.abs(ref).max(), 1e-30), f"max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})"


def test_small_fixture_graph_has_the_cases_it_is_for():
    d = load_golden("gcn_small.npz")
    ei, n = d["edge_index"], d["x"].shape[0]
    assert 24 <= n <= 60
    loops = ei[0][ei[0] == ei[1]]
    assert loops.size >= 3 and np.bincount(loops).max() >= 2                       # existing self loops, one duplicated
    pairs = ei[0][ei[0] != ei[1]] * n + ei[1][ei[0] != ei[1]]
    assert np.unique(pairs).size < pairs.size                                      # duplicate edges
    assert (np.bincount(ei[1][ei[0] != ei[1]], minlength=n) == 0).any()            # nodes without in-edges


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_dense_restatement_reproduces_fixture(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x = torch.from_numpy(x).double()
    y = torch.from_numpy(y).long()
    tm = torch.from_numpy(d["train_mask"])
    rows = torch.from_numpy(d["rows"])
    assert not bool((y[tm] == -1).any())
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        A = norm_adj(e, n)
        for name, L, hidden in models:
            params = {k: v.double().requires_grad_(True) for k, v in fixture_params(d, name, F_in, C, L, hidden).items()}
            pre = f"{var}/{name}/"
            logp = restate(params, x, A)
            _close(logp.detach()[rows], d[pre + "logp"])
            _close(restate(params, x, A, log_softmax=False).detach()[rows], d[pre + "logits"])
            if L > 1:
                _close(restate(params, x, A, n_convs=L - 1).detach()[rows], d[pre + "emb"])
            loss = F.nll_loss(logp[tm], y[tm])
            assert abs(loss.item() - float(d[pre + "loss"])) <= 1e-12 * abs(float(d[pre + "loss"]))
            if pre + "grad/convs.0.lin.weight" in d:
                grads = torch.autograd.grad(loss, list(params.values()))
                for (k, _), g in zip(params.items(), grads):
                    _close(g, d[pre + "grad/" + k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_dense_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        A = norm_adj(e, n)
        for name, L, hidden in models:
            params = {k: v.double().requires_grad_(True) for k, v in fixture_params(d, name, F_in, C, L, hidden).items()}
            opt = torch.optim.Adam(list(params.values()), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(restate(params, x, A)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            pre = f"{var}/{name}/"
            np.testing.assert_allclose(losses, d[pre + "adam_loss"], rtol=1e-10)
            for k, p in params.items():
                if pre + "adam/" + k in d:
                    _close(p.detach(), d[pre + "adam/" + k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_module_state_dict_matches_fixture(fixture):
    from bridged_gnn_amd.gcn import GCNNet
    d, x, y, _, models = _inputs(fixture)
    ds = types.SimpleNamespace(num_features=x.shape[1], num_classes=int(y.max()) + 1)
    for name, L, hidden in models:
        # same initialisers in the same order as PyG's GCNConv: the seeded model IS the fixture's (office: via its sums)
        ref = fixture_params(d, name, x.shape[1], int(y.max()) + 1, L, hidden)
        torch.manual_seed(0)
        m = GCNNet(ds, layer_num=L, hidden=hidden)
        sd = m.state_dict()
        assert sorted(sd) == sorted(ref)
        assert sorted(sd) == sorted(f"convs.{i}.{leaf}" for i in range(L) for leaf in ("bias", "lin.weight"))
        for k in ref:
            assert sd[k].shape == ref[k].shape and sd[k].dtype == torch.float32
            assert torch.equal(sd[k], ref[k]), k
        m.load_state_dict(ref, strict=True)


def test_package_exports_and_unsupported_constructor_arguments():
    import bridged_gnn_amd
    from bridged_gnn_amd import GCNConv, GCNNet
    from bridged_gnn_amd import gcn
    assert GCNNet is gcn.GCNNet and GCNConv is gcn.GCNConv and bridged_gnn_amd.GCNNet is GCNNet
    for kw in ({"improved": True}, {"cached": True}, {"add_self_loops": False}, {"normalize": False}):
        with pytest.raises(NotImplementedError):
            GCNConv(4, 4, **kw)
    assert sorted(GCNConv(4, 3).state_dict()) == ["bias", "lin.weight"]
    assert sorted(GCNConv(4, 3, bias=False).state_dict()) == ["lin.weight"]


def test_command_line_baseline_flag():
    from bridged_gnn_amd.transfer import build_parser
    ap = build_parser()
    a = ap.parse_args(["--no_dtc"])
    assert a.no_dtc and a.baseline == "GraphSAGE"                   # --no_dtc alone still trains GraphSAGE
    assert ap.parse_args(["--no_dtc", "--model_name", "GCN"]).baseline == "GraphSAGE"    # --model_name is ignored there
    assert ap.parse_args(["--no_dtc", "--baseline", "GCN"]).baseline == "GCN"
    assert ap.parse_args([]).baseline == "GraphSAGE"
    with pytest.raises(SystemExit):
        ap.parse_args(["--no_dtc", "--baseline", "GAT"])


@pytest.mark.parametrize("gnn", ["MLP", "GAT", "GATv2", "KTGNN", "nonsense"])
def test_unbuilt_baselines_still_raise(gnn):
    from bridged_gnn_amd.transfer import train_gnn_noDTC
    with pytest.raises(NotImplementedError):
        train_gnn_noDTC(types.SimpleNamespace(gpu=0, dataset_name="x"), None, None, gnn=gnn)


def test_train_gnn_with_gcn_still_raises():
    from bridged_gnn_amd.transfer import train_gnn
    with pytest.raises(NotImplementedError):
        train_gnn(types.SimpleNamespace(gpu=0, dataset_name="x"), None, None, gnn="GCN")


def test_gcn_ops_refuse_host_tensors():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gcn import GCNNet
    tbl = torch.zeros(4, 8)
    rowptr = torch.arange(5, dtype=torch.int32)
    col = torch.arange(4, dtype=torch.int32)
    dinv = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gcn_aggregate(tbl, rowptr, col, dinv, 4, 8, bias=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gcn_aggregate_bwd(tbl, tbl, rowptr, col, dinv, 4, 8, epilogue="relu")
    m = GCNNet(types.SimpleNamespace(num_features=8, num_classes=3), layer_num=2, hidden=8)
    data = types.SimpleNamespace(x=tbl, edge_index=torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(data)


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_gcn.py"), "--out", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    for name in ("gcn_office_a2d.npz", "gcn_small.npz"):
        a, b = dict(np.load(os.path.join(GOLDEN, name))), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
