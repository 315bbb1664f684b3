"""CPU: the GIN baseline's host side (bridged_gnn_amd.gin, models/backbones.py:26-57) -- the three new C entries are declared, bound
and argument-counted at ABI 116 and cite the reference, eps is a device pointer in both kernels' declarations, the new source
uses no float atomics and is built and hashed at one position, GINNet carries the reference's state_dict (tools/gen_golden_gin.py)
at 1, 2 and 3 layers with eps a buffer in the single-layer model and a Parameter otherwise, seeded initial parameters equal the
fixture's, every configuration the layers do not implement is refused, the ops refuse a host or float eps and host tensors,
`graphed=True` is refused, the CLI has step 2's flags plus --dropout, and a dense fp64 restatement (an [N, N] multiplicity matrix)
reproduces the fixtures' outputs, losses, gradients and Adam trajectories."""
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bgnn_gin_aggregate_f32", "bgnn_gin_aggregate_bwd_workspace_bytes", "bgnn_gin_aggregate_bwd_f32")
OFFICE_MODELS = (("l2h64", 2, 64), ("l1", 1, 16), ("l3h32", 3, 32))
SMALL_MODELS = (("l2h8", 2, 8), ("l1", 1, 16), ("l3h6", 3, 6))
DS = types.SimpleNamespace(num_features=37, num_classes=5)


# ---- C ABI -------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_cite_the_reference():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in bgnn.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(",") if a.strip()]), name
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if "bgnn_gin_aggregate_bwd_f32 (" in b]
    assert blocks and all(b.count("backbones.py:26-57") >= 2 for b in blocks)        # the forward's and the backward's citation
    assert all("(1 + eps)" in b for b in blocks)                                     # and their formulas
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)          # additive: the revision stays
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_gin.hip")).read()
    for name in ENTRIES:
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    for piece in ("bgnn_conv_common.h", "lf_ladder", "persistent_grid", "ep_sum", "drop4", "log_softmax4", "clamp_row", "epi_switch",
                  "epi_check", "tbl_ok", "dispatch_bwd_rows<false>"):
        assert piece in src, piece
    assert "atomicAdd" not in src and "atomic" not in re.sub(r"//.*", "", src)
    # eps is a device pointer in both kernels' declarations
    for name in (ENTRIES[0], ENTRIES[2]):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert re.search(r"const\s+float\s*\*\s*eps\b", decl), name


def test_source_is_built_and_hashed_in_the_same_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "bgnn_gin.hip" in srcs and "bgnn_gin.hip" in _lib._HASHED_SOURCES
    assert srcs.index("bgnn_gin.hip") == _lib._HASHED_SOURCES.index("bgnn_gin.hip")
    assert list(_lib._HASHED_SOURCES[:len(srcs)]) == srcs


# ---- model -------------------------------------------------------------------------------------------------------
def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("gin_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("gin_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def _want_keys(F_in, C, L, hidden):
    dims = [(F_in, C)] if L == 1 else [(F_in, hidden)] + [(hidden, hidden)] * (L - 2) + [(hidden, C)]
    want = []
    for i, (a, b) in enumerate(dims):
        want += [(f"convs.{i}.eps", (1,)), (f"convs.{i}.nn.weight", (b, a)), (f"convs.{i}.nn.bias", (b,))]
    return want


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_state_dict_eps_kind_and_seeded_parameters_match_the_fixture(fixture):
    import bridged_gnn_amd
    from bridged_gnn_amd.gin import GINConv, GINNet
    d, x, y, _, models = _inputs(fixture)
    ds = types.SimpleNamespace(num_features=x.shape[1], num_classes=int(y.max()) + 1)
    assert sorted(L for _, L, _ in models) == [1, 2, 3]
    for name, L, hidden in models:
        torch.manual_seed(0)
        m = GINNet(ds, layer_num=L, hidden=hidden)
        sd = m.state_dict()
        # the reference's keys, shapes and order: a module's own eps before its child's weight and bias
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == _want_keys(ds.num_features, ds.num_classes, L, hidden)
        full, sums = sub(d, f"{name}/param/"), sub(d, f"{name}/param_sum/")
        assert sorted(full or sums) == sorted(sd)
        for k, v in sd.items():
            if full:
                assert v.dtype == torch.float32 and np.array_equal(v.numpy(), full[k]), k
            else:
                vd = v.double()
                np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
        params = dict(m.named_parameters())
        buffers = dict(m.named_buffers())
        for i, conv in enumerate(m.convs):
            assert isinstance(conv, GINConv) and float(conv.eps.detach()) == 0.0 and conv.initial_eps == 0.0
            if L == 1:                                   # GINConv(Linear(F, C)): train_eps=False, a buffer
                assert f"convs.{i}.eps" in buffers and f"convs.{i}.eps" not in params and not conv.eps.requires_grad
            else:
                assert f"convs.{i}.eps" in params and f"convs.{i}.eps" not in buffers and conv.eps.requires_grad
        assert m.dropout == 0.5
        # reset_parameters: nn, then eps back to its initial value; the same seed, the same draw as one more reset of each Linear
        with torch.no_grad():
            for conv in m.convs:
                conv.eps.fill_(0.7)
        torch.manual_seed(3)
        m.reset_parameters()
        torch.manual_seed(3)
        for conv in m.convs:
            from bridged_gnn_amd.ktgnn import Linear
            ref = Linear(conv.in_channels, conv.out_channels)
            assert torch.equal(conv.nn.weight, ref.weight) and torch.equal(conv.nn.bias, ref.bias) and float(conv.eps.detach()) == 0.0
    assert bridged_gnn_amd.GINNet is GINNet and bridged_gnn_amd.GINConv is GINConv
    assert bridged_gnn_amd.train_gin_noDTC.__module__ == "bridged_gnn_amd.gin"


def test_eps_argument_and_train_eps():
    from bridged_gnn_amd.gin import GINConv
    from bridged_gnn_amd.ktgnn import Linear
    c = GINConv(Linear(6, 4), eps=0.25, train_eps=True)
    assert isinstance(c.eps, torch.nn.Parameter) and tuple(c.eps.shape) == (1,) and float(c.eps.detach()) == 0.25
    assert list(c.state_dict()) == ["eps", "nn.weight", "nn.bias"]
    c = GINConv(torch.nn.Linear(6, 4), eps=-1.0)
    assert not isinstance(c.eps, torch.nn.Parameter) and float(c.eps.detach()) == -1.0 and list(c.state_dict()) == ["eps", "nn.weight", "nn.bias"]
    assert (c.in_channels, c.out_channels) == (6, 4)


def test_unsupported_configurations_raise():
    from bridged_gnn_amd.gin import GINConv
    from bridged_gnn_amd.ktgnn import Linear
    for bad in (torch.nn.Sequential(Linear(4, 4), torch.nn.ReLU(), Linear(4, 4)), torch.nn.Sequential(Linear(4, 4)), torch.nn.ReLU(),
                torch.nn.Identity()):
        with pytest.raises(NotImplementedError, match="single Linear"):
            GINConv(bad)
    with pytest.raises(NotImplementedError):
        GINConv(Linear(4, 4), aggr="mean")
    conv = GINConv(Linear(4, 4), train_eps=True)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError, match="edge attributes"):
        conv(torch.zeros(2, 4), ei, edge_attr=torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="bipartite"):
        conv(torch.zeros(2, 4), ei, size=(2, 2))
    with pytest.raises(NotImplementedError, match="bipartite"):
        conv((torch.zeros(2, 4), torch.zeros(2, 4)), ei)


def test_host_tensors_and_host_eps_are_refused():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.gin import GINConv, GINNet
    from bridged_gnn_amd.ktgnn import Linear
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU"):
        GINConv(Linear(4, 4), train_eps=True)(torch.zeros(2, 4), ei)
    with pytest.raises(RuntimeError, match="no CPU"):
        GINNet(DS, 2, 8).eval()(Data(x=torch.zeros(2, 37), edge_index=ei))
    rowptr, col = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    T = torch.zeros(2, 4)
    # eps: a Python number is refused as such, a host tensor as a host tensor -- both before the table is looked at
    for fn, args in ((ops.gin_aggregate, lambda e: (T, rowptr, col, e, 2, 4)),
                     (ops.gin_aggregate_bwd, lambda e: (T, T, T, rowptr, col, e, 2, 4))):
        for bad in (0.3, 0, np.float32(0.3)):
            with pytest.raises(ValueError, match="eps must be a float32 tensor"):
                fn(*args(bad))
        for bad in (torch.zeros(1), torch.zeros(1, dtype=torch.float64), torch.zeros(2)):
            with pytest.raises((RuntimeError, ValueError), match="no CPU|eps must be"):
                fn(*args(bad))
        with pytest.raises(RuntimeError, match="no CPU"):
            fn(*args(None))                                # eps=None is taken; the host table is not


def test_ops_validate_what_needs_no_device():
    from bridged_gnn_amd import ops
    with pytest.raises(ValueError, match="D >= 1"):
        ops.gin_aggregate(None, None, None, None, 2, 0)
    with pytest.raises(ValueError, match="D >= 1"):
        ops.gin_aggregate_bwd(None, None, None, None, None, None, 2, 0)
    with pytest.raises(ValueError, match="epilogue"):
        ops.gin_aggregate(None, None, None, None, 2, 4, epilogue="elu")
    with pytest.raises(ValueError, match="D <= 128"):
        ops.gin_aggregate(None, None, None, None, 2, 129, epilogue="log_softmax")
    with pytest.raises(ValueError, match="D <= 128"):
        ops.gin_aggregate_bwd(None, None, None, None, None, None, 2, 129, epilogue="log_softmax")
    for p, epi in ((0.5, None), (0.5, "log_softmax"), (1.0, "relu"), (-0.1, "relu")):
        with pytest.raises(ValueError, match="p_drop"):
            ops.gin_aggregate(None, None, None, None, 2, 4, epilogue=epi, p_drop=p)
    sig = inspect.signature(ops.gin_aggregate).parameters
    assert list(sig) == ["tbl", "rowptr", "col", "eps", "n_rows", "D", "bias", "epilogue", "p_drop", "seed", "seed_dev", "out", "row_ids"]
    sig = inspect.signature(ops.gin_aggregate_bwd).parameters
    assert list(sig) == ["tbl", "y", "grad_y", "t_rowptr", "t_col", "eps", "n_src", "D", "epilogue", "p_drop", "want_bias", "want_eps",
                         "grad_tbl"]
    assert sig["want_bias"].default is True and sig["want_eps"].default is True
    for fn in (ops.gin_aggregate, ops.gin_aggregate_bwd):
        assert "backbones.py:26-57" in fn.__doc__ and "bgnn.h" in fn.__doc__


def test_cli_defaults_are_step_twos_with_two_layers_of_64():
    from bridged_gnn_amd import gin, transfer
    a = gin.build_parser().parse_args([])
    assert (a.num_layer, a.hidden_dim, a.dropout) == (2, 64, 0.5)
    base = transfer.build_parser().parse_args([])
    for k, v in vars(base).items():
        if k not in ("num_layer", "hidden_dim"):
            assert getattr(a, k) == v, k
    b = gin.build_parser().parse_args(["--path_data", "x_bridged_graph.dat", "--to_undirected", "--graphed", "--num_layer", "3",
                                       "--hidden_dim", "128", "--dropout", "0.2"])
    assert b.to_undirected and b.graphed and (b.num_layer, b.hidden_dim, b.dropout, b.path_data) == (3, 128, 0.2, "x_bridged_graph.dat")
    # step 2's own command line is as it was: no GIN among its baselines
    assert "GIN" not in (transfer._FLAGS["baseline"][2] or ())


def test_graphed_driver_is_refused():
    from bridged_gnn_amd import gin
    with pytest.raises(NotImplementedError, match="graphed"):
        gin.train_gin_noDTC(types.SimpleNamespace(dataset_name="x"), DS, None, graphed=True)
    sig = inspect.signature(gin.train_gin_noDTC).parameters
    assert (sig["num_layer"].default, sig["hidden"].default, sig["dropout"].default, sig["graphed"].default,
            sig["history"].default) == (2, 64, 0.5, False, None)


# ---- the dense fp64 restatement ----------------------------------------------------------------------------------
def mult_adj(ei, n):
    """A [n, n] fp64 (row = destination): A[i, j] = how many times the edge j -> i is listed; self loops are ordinary entries"""
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    return A


def restate(params, x, A, relu_masks=None):
    """fp64 GINNet forward (eval: no dropout), aggregate first as PyG does; params: name -> tensor (convs.{i}.eps, .nn.weight, .nn.bias)"""
    L = 1 + max(int(k.split(".")[1]) for k in params)
    for i in range(L):
        h = (1.0 + params[f"convs.{i}.eps"]) * x + A @ x
        x = h @ params[f"convs.{i}.nn.weight"].t() + params[f"convs.{i}.nn.bias"]
        if i < L - 1:
            x = x * relu_masks[i] if relu_masks is not None else torch.relu(x)
    return torch.log_softmax(x, dim=1)


def fixture_params(d, name, F_in, C, L, hidden):
    """the fixture's initial parameters: stored (small fixture) or the seeded model rebuilt (office fixture; checked against the
    stored sums by test_state_dict_eps_kind_and_seeded_parameters_match_the_fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.gin import GINNet
    torch.manual_seed(0)
    sd = GINNet(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden).state_dict()
    return {k: v.clone() for k, v in sd.items()}


def undirected(ei, n):
    """ToUndirected(merge=True): the coalesced union of both directions"""
    both = torch.cat([ei, ei.flip(0)], 1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


def params64(d, name, F_in, C, L, hidden):
    """fp64 leaves; a buffer eps (the single-layer model) takes no gradient"""
    P = {k: v.double() for k, v in fixture_params(d, name, F_in, C, L, hidden).items()}
    return {k: v.requires_grad_(not (L == 1 and k.endswith(".eps"))) for k, v in P.items()}


def _close(got, ref, rel=1e-10):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= rel * max(np.abs(ref).max(), 1e-30), f"max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})"


def test_small_fixture_graph_has_the_cases_it_is_for():
    d = load_golden("gin_small.npz")
    ei, n = d["edge_index"], d["x"].shape[0]
    assert 24 <= n <= 60
    loops = ei[0][ei[0] == ei[1]]
    assert loops.size >= 3 and np.bincount(loops).max() >= 2                       # self loops, one of them twice
    pairs = ei[0] * n + ei[1]
    assert np.unique(pairs).size < pairs.size                                      # duplicate edges
    assert (np.bincount(ei[1], minlength=n) == 0).any()                            # rows without in-edges
    for k, v in d.items():
        assert v.dtype.kind in "fiub", k                                           # numeric arrays only


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
        A = mult_adj(e, n)
        for name, L, hidden in models:
            params = params64(d, name, F_in, C, L, hidden)
            pre = f"{var}/{name}/"
            logp = restate(params, x, A)
            _close(logp.detach()[rows], d[pre + "logp"])
            loss = F.nll_loss(logp[tm], y[tm])
            assert abs(loss.item() - float(d[pre + "loss"])) <= 1e-12 * abs(float(d[pre + "loss"]))
            leaves = {k: v for k, v in params.items() if v.requires_grad}
            assert sorted(leaves) == sorted(sub(d, pre + "grad/")) or not sub(d, pre + "grad/")
            if sub(d, pre + "grad/"):
                for (k, _), g in zip(leaves.items(), torch.autograd.grad(loss, list(leaves.values()))):
                    _close(g, d[pre + "grad/" + k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_dense_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        A = mult_adj(e, n)
        for name, L, hidden in models:
            params = params64(d, name, F_in, C, L, hidden)
            leaves = {k: v for k, v in params.items() if v.requires_grad}
            opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(restate(params, x, A)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            pre = f"{var}/{name}/"
            np.testing.assert_allclose(losses, d[pre + "adam_loss"], rtol=1e-10)
            for k, p in leaves.items():
                if pre + "adam/" + k in d:
                    _close(p.detach(), d[pre + "adam/" + k])


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_gin.py"), "--out", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    for name in ("gin_office_a2d.npz", "gin_small.npz"):
        a, b = load_golden(name), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
