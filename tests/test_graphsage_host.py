"""CPU: the GraphSAGE fixtures (tools/gen_golden_graphsage.py, made from the reference's models/backbones.py:440-498) against an
fp64 restatement written here, the module's state_dict layout, and the refusal of host tensors by the new ops."""
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


def mean_agg(x, src, dst, n):
    """torch_sparse matmul(adj_t, x, reduce='mean') with adj_t[dst, src]: duplicates count, empty rows give 0"""
    s = torch.zeros(n, x.shape[1], dtype=x.dtype).index_add_(0, dst, x[src])
    c = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(dst.shape[0], dtype=x.dtype))
    return s / c.clamp(min=1).unsqueeze(1)


def restate(params, x, ei, n_convs=None, out_neighbours=False, log_softmax=True):
    """fp64 GraphSAGE forward (eval: no dropout); params: name -> tensor (convs.{i}.lin_l.weight, ...)."""
    L = 1 + max(int(k.split(".")[1]) for k in params)
    src, dst = (ei[1], ei[0]) if out_neighbours else (ei[0], ei[1])
    n = x.shape[0]
    n_convs = L if n_convs is None else n_convs
    for i in range(n_convs):
        p = f"convs.{i}."
        x = (mean_agg(x, src, dst, n) @ params[p + "lin_l.weight"].t() + params[p + "lin_l.bias"]
             + x @ params[p + "lin_r.weight"].t())
        if i < L - 1:
            x = torch.relu(x)
    return torch.log_softmax(x, dim=1) if (log_softmax and n_convs == L) else x


def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("graphsage_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("graphsage_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def fixture_params(d, name, F_in, C, L, hidden):
    """the fixture's initial parameters: stored (small fixture) or the seeded model rebuilt and checked against the stored
    fp64 (sum, sum of squares) of every tensor (office fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.sage import GraphSAGE
    torch.manual_seed(0)
    sd = GraphSAGE(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden).state_dict()
    sums = sub(d, f"{name}/param_sum/")
    assert sorted(sums) == sorted(sd)
    for k, v in sd.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, err_msg=k)
    return {k: v.clone() for k, v in sd.items()}


def undirected(ei, n):
    """ToUndirected(merge=True): the coalesced union of both directions"""
    both = torch.cat([ei, ei.flip(0)], 1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


def _close(got, ref, rel=2e-6):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= rel * max(np.abs(ref).max(), 1e-30) + 1e-7, f"max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})"


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_restatement_reproduces_fixture(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x = torch.from_numpy(x).double()
    y = torch.from_numpy(y).long()
    tm = torch.from_numpy(d["train_mask"])
    rows = torch.from_numpy(d["rows"])
    assert not bool((y[tm] == -1).any())
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        for name, L, hidden in models:
            params = {k: v.double().requires_grad_(True) for k, v in fixture_params(d, name, F_in, C, L, hidden).items()}
            pre = f"{var}/{name}/"
            logp = restate(params, x, e)
            _close(logp.detach()[rows], d[pre + "logp"])
            _close(restate(params, x, e, out_neighbours=True, log_softmax=False).detach()[rows], d[pre + "logits"])
            if L > 1:
                _close(restate(params, x, e, n_convs=L - 1, out_neighbours=True).detach()[rows], d[pre + "emb"])
            loss = F.nll_loss(logp[tm], y[tm])
            assert abs(loss.item() - float(d[pre + "loss"])) <= 1e-12 * abs(float(d[pre + "loss"]))
            if pre + "grad/convs.0.lin_l.weight" in d:
                grads = torch.autograd.grad(loss, list(params.values()))
                for (k, _), g in zip(params.items(), grads):
                    _close(g, d[pre + "grad/" + k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        for name, L, hidden in models:
            params = {k: v.double().requires_grad_(True) for k, v in fixture_params(d, name, F_in, C, L, hidden).items()}
            opt = torch.optim.Adam(list(params.values()), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(restate(params, x, e)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            pre = f"{var}/{name}/"
            np.testing.assert_allclose(losses, d[pre + "adam_loss"], rtol=1e-12)
            for k, p in params.items():
                if pre + "adam/" + k in d:
                    _close(p.detach(), d[pre + "adam/" + k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_module_state_dict_matches_fixture(fixture):
    from bridged_gnn_amd.sage import GraphSAGE
    d, x, y, _, models = _inputs(fixture)
    ds = types.SimpleNamespace(num_features=x.shape[1], num_classes=int(y.max()) + 1)
    for name, L, hidden in models:
        # same initialisers in the same order as PyG's SAGEConv: the seeded model IS the fixture's (office: via its sums)
        ref = fixture_params(d, name, x.shape[1], int(y.max()) + 1, L, hidden)
        torch.manual_seed(0)
        m = GraphSAGE(ds, layer_num=L, hidden=hidden, root_weight=True)
        sd = m.state_dict()
        assert sorted(sd) == sorted(ref)
        for k in ref:
            assert sd[k].shape == ref[k].shape and sd[k].dtype == torch.float32
            assert torch.equal(sd[k], ref[k]), k
        m.load_state_dict(ref, strict=True)


def test_sage_ops_refuse_host_tensors():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.sage import GraphSAGE
    tbl = torch.zeros(4, 8)
    rowptr = torch.zeros(5, dtype=torch.int32)
    col = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.sage_mean_aggregate(tbl, rowptr, col, 4, 8, root=tbl)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.sage_mean_aggregate_bwd(tbl, tbl, rowptr, rowptr, col, 4, 8, epilogue="relu")
    m = GraphSAGE(types.SimpleNamespace(num_features=8, num_classes=3), layer_num=2, hidden=8)
    data = types.SimpleNamespace(x=tbl, edge_index=torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(data)


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_graphsage.py"), "--out", str(tmp_path)],
                          cwd=ROOT)
    for name in ("graphsage_office_a2d.npz", "graphsage_small.npz"):
        a, b = dict(np.load(os.path.join(GOLDEN, name))), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
