"""CPU: the JKNet baseline's host side (bridged_gnn_amd.jknet, models/backbones.py:60-107) -- the five new C entries are declared,
bound and argument-counted at ABI 116 and cite the reference, the new source uses no float atomics and is built and hashed at one
position, JKNet carries the reference's state_dict (tools/gen_golden_jknet.py) and its seeded initial parameters, a dense fp64
restatement written here from the operator's closed form (A2_ij = s_i s_j m_ij, A2_ii = 1 / d2_i) reproduces the fixtures' outputs,
losses, gradients and Adam trajectories for every model (the `renormalize=False` model from the single normalisation), the
operator facts hold on the small graph, `JKGraph.scales` (the fp64 formula the device graph rounds once) equals the closed form,
and JumpingKnowledge('lstm'), `graphed=True`, CPU tensors and malformed op arguments raise without touching a device."""
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
ENTRIES = ("bgnn_jk_gcn_aggregate_f32", "bgnn_jk_gcn_aggregate_bwd_f32", "bgnn_jk_head_supported", "bgnn_jk_head_f32",
           "bgnn_jk_max_route_f32")
# (name, mode, layers, hidden, renormalize)
OFFICE_MODELS = (("cat_l2h32", "cat", 2, 32, True), ("max_l2h20", "max", 2, 20, True), ("cat_l3h16", "cat", 3, 16, True),
                 ("max_l3h10", "max", 3, 10, True))
SMALL_MODELS = (("cat_l2h8", "cat", 2, 8, True), ("max_l2h8", "max", 2, 8, True), ("cat_l3h6", "cat", 3, 6, True),
                ("max_l3h6", "max", 3, 6, True), ("single_cat_l2h8", "cat", 2, 8, False))


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
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if "bgnn_jk_head_f32 (" in b]
    assert len(blocks) == 1 and blocks[0].count("backbones.py:60-107") >= 4          # conv, its backward, head, route
    assert "w_i * tbl_i + s_i * sum" in blocks[0] and "lowest l on ties" in blocks[0]
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)          # additive: the revision stays
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_jk.hip")).read()
    for name in ENTRIES:
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    for piece in ("bgnn_conv_common.h", "lf_ladder", "persistent_grid", "ep_sum", "drop4", "clamp_row", "epi_check", "tbl_ok",
                  "dispatch_bwd_rows<false>", "xcd_pos_range", "__builtin_amdgcn_mfma_f32_16x16x4f32"):
        assert piece in src, piece
    assert "atomicAdd" not in src and "atomic_add" not in re.sub(r"//.*", "", src)


def test_source_is_built_and_hashed_in_the_same_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "bgnn_jk.hip" in srcs and srcs.index("bgnn_jk.hip") == _lib._HASHED_SOURCES.index("bgnn_jk.hip")
    assert list(_lib._HASHED_SOURCES[:len(srcs)]) == srcs


# ---- model -------------------------------------------------------------------------------------------------------
def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("jknet_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("jknet_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def _want_keys(F_in, C, L, hidden, mode):
    want = []
    for i in range(L):
        want += [(f"convs.{i}.bias", (hidden,)), (f"convs.{i}.lin.weight", (hidden, F_in if i == 0 else hidden))]
    return want + [("lin.weight", (C, L * hidden if mode == "cat" else hidden)), ("lin.bias", (C,))]


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_state_dict_and_seeded_parameters_match_the_fixture(fixture):
    import bridged_gnn_amd
    from bridged_gnn_amd.jknet import JKGraph, JKNet, JumpingKnowledge
    d, x, y, _, models = _inputs(fixture)
    F_in, C = x.shape[1], int(y.max()) + 1
    assert sorted({(m, L) for _, m, L, _, r in models if r}) == [("cat", 2), ("cat", 3), ("max", 2), ("max", 3)]
    for name, mode, L, hidden, renorm in models:
        torch.manual_seed(0)
        m = JKNet(F_in, hidden, C, L, 0.5, mode=mode, renormalize=renorm)
        sd = m.state_dict()
        assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == sorted(_want_keys(F_in, C, L, hidden, mode))
        full, sums = sub(d, f"{name}/param/"), sub(d, f"{name}/param_sum/")
        assert sorted(full or sums) == sorted(sd)
        for k, v in sd.items():
            if full:
                assert v.dtype == torch.float32 and np.array_equal(v.numpy(), full[k]), k
            else:
                vd = v.double()
                np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
        assert m.dropout == 0.5 and len(m.convs) == L and not list(m.jump.parameters())
    assert bridged_gnn_amd.JKNet is JKNet and bridged_gnn_amd.JKGraph is JKGraph and bridged_gnn_amd.JumpingKnowledge is JumpingKnowledge
    assert bridged_gnn_amd.train_jknet_noDTC.__module__ == "bridged_gnn_amd.jknet"
    assert "never" in JKNet.__doc__ and "adj_t_cache" in JKNet.__doc__


def test_jumping_knowledge_modes():
    from bridged_gnn_amd.jknet import JKNet, JumpingKnowledge
    with pytest.raises(NotImplementedError, match="lstm.*LSTM"):
        JumpingKnowledge("lstm", channels=8, num_layers=2)
    with pytest.raises(NotImplementedError, match="lstm"):
        JKNet(4, 8, 3, 2, 0.5, mode="lstm")
    with pytest.raises(ValueError, match="mode"):
        JumpingKnowledge("sum")
    xs = [torch.tensor([[1.0, 0.0, 2.0]]), torch.tensor([[1.0, 3.0, -1.0]]), torch.tensor([[0.5, 3.0, 2.0]])]
    assert torch.equal(JumpingKnowledge("cat")(xs), torch.cat(xs, 1))
    assert torch.equal(JumpingKnowledge("max")(xs), torch.tensor([[1.0, 3.0, 2.0]]))
    assert not list(JumpingKnowledge("max").parameters()) and not list(JumpingKnowledge("cat", 8, 3).parameters())


def test_host_tensors_are_refused_and_graphed_driver_too():
    from bridged_gnn_amd import jknet, ops
    from bridged_gnn_amd.data import Data
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU"):
        jknet.JKNet(5, 8, 3, 2, 0.5).eval()(Data(x=torch.zeros(2, 5), edge_index=ei))
    rowptr, col = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32)
    T, s = torch.zeros(2, 4), torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.jk_gcn_aggregate(T, rowptr, col, s, s, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.jk_gcn_aggregate_bwd(T, T, rowptr, col, s, s, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.jk_head(torch.zeros(2, 8), 2, 4, "cat", torch.zeros(3, 8), None, 3)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.jk_head_bwd(torch.zeros(2, 8), 2, 4, "cat", torch.zeros(3, 8), 3, torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="graphed"):
        jknet.train_jknet_noDTC(types.SimpleNamespace(dataset_name="x"), types.SimpleNamespace(num_features=5, num_classes=3), None,
                                graphed=True)
    sig = inspect.signature(jknet.train_jknet_noDTC).parameters
    assert (sig["num_layer"].default, sig["hidden"].default, sig["dropout"].default, sig["mode"].default, sig["graphed"].default) == \
        (2, 64, 0.5, "cat", False)


def test_ops_validate_what_needs_no_device():
    from bridged_gnn_amd import ops
    with pytest.raises(ValueError, match="D >= 1"):
        ops.jk_gcn_aggregate(None, None, None, None, None, 2, 0)
    with pytest.raises(ValueError, match="D >= 1"):
        ops.jk_gcn_aggregate_bwd(None, None, None, None, None, None, 2, 0)
    for epi in ("elu", "log_softmax"):
        with pytest.raises(ValueError, match="epilogue"):
            ops.jk_gcn_aggregate(None, None, None, None, None, 2, 4, epilogue=epi)
    for p, epi in ((0.5, None), (1.0, "relu"), (-0.1, "relu")):
        with pytest.raises(ValueError, match="p_drop"):
            ops.jk_gcn_aggregate(None, None, None, None, None, 2, 4, epilogue=epi, p_drop=p)
        with pytest.raises(ValueError, match="p_drop"):
            ops.jk_gcn_aggregate_bwd(None, None, None, None, None, None, 2, 4, epilogue=epi, p_drop=p)
    with pytest.raises(ValueError, match="mode"):
        ops.jk_head(None, 2, 4, "lstm", None, None, 3)
    with pytest.raises(ValueError, match="mode"):
        ops.jk_head_bwd(None, 2, 4, "sum", None, 3, None, None)
    with pytest.raises(ValueError, match=">= 1"):
        ops.jk_head(None, 2, 0, "cat", None, None, 3)
    with pytest.raises(ValueError, match="envelope"):
        ops.jk_head(None, 2, 64, "cat", None, None, 33)
    with pytest.raises(ValueError, match="weight must be"):
        ops.jk_pack_weight(torch.zeros(3, 7), 2, 4, "cat")
    # the packed weight: the layer buffer's padded columns, pad columns 0
    w = torch.arange(1.0, 13.0).reshape(2, 6)
    wp = ops.jk_pack_weight(w, 2, 3, "cat")
    assert tuple(wp.shape) == (2, 8) and torch.equal(wp[:, :3], w[:, :3]) and torch.equal(wp[:, 4:7], w[:, 3:])
    assert torch.count_nonzero(wp[:, 3]) == 0 and torch.count_nonzero(wp[:, 7]) == 0
    assert tuple(ops.jk_pack_weight(w[:, :3], 2, 3, "max").shape) == (2, 4)
    for fn in (ops.jk_gcn_aggregate, ops.jk_gcn_aggregate_bwd, ops.jk_head, ops.jk_head_bwd):
        assert "backbones.py:60-107" in fn.__doc__ and "bgnn.h" in fn.__doc__
    assert list(inspect.signature(ops.jk_gcn_aggregate).parameters) == ["tbl", "rowptr", "col", "s", "w", "n_rows", "D", "bias", "epilogue",
                                                                        "p_drop", "seed", "seed_dev", "out"]


def test_head_envelope():
    from bridged_gnn_amd import ops
    assert ops.jk_head_supported(4, 128, 32, "cat") and ops.jk_head_supported(4, 128, 32, "max")    # the widest product: 512 x 32
    assert ops.jk_head_supported(1, 1, 1, "cat") and ops.jk_head_supported(8, 128, 16, "cat")
    assert not ops.jk_head_supported(2, 64, 33, "cat") and not ops.jk_head_supported(2, 64, 0, "max")
    assert not ops.jk_head_supported(5, 128, 32, "cat") and ops.jk_head_supported(5, 128, 32, "max")  # max keeps K = pad4(H)
    assert not ops.jk_head_supported(9, 4, 2, "cat") and not ops.jk_head_supported(2, 64, 2, "lstm")
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_jk.hip")).read()
    assert int(re.search(r"JK_HEAD_LDS_BYTES\s*=\s*(\d+)", src).group(1)) == ops.JK_HEAD_LDS_BYTES
    assert int(re.search(r"JK_MAX_LAYERS\s*=\s*(\d+)", src).group(1)) == ops.JK_MAX_LAYERS


def test_cli_defaults():
    from bridged_gnn_amd import jknet, transfer
    a = jknet.build_parser().parse_args([])
    assert (a.num_layer, a.hidden_dim, a.dropout, a.mode, a.no_renormalize) == (2, 64, 0.5, "cat", False)
    base = transfer.build_parser().parse_args([])
    for k, v in vars(base).items():
        if k not in ("num_layer", "hidden_dim"):
            assert getattr(a, k) == v, k
    b = jknet.build_parser().parse_args(["--path_data", "x.dat", "--to_undirected", "--num_layer", "3", "--hidden_dim", "128",
                                         "--dropout", "0.2", "--mode", "max", "--no_renormalize"])
    assert b.to_undirected and (b.num_layer, b.hidden_dim, b.dropout, b.mode, b.no_renormalize) == (3, 128, 0.2, "max", True)
    with pytest.raises(SystemExit):
        jknet.build_parser().parse_args(["--mode", "lstm"])


# ---- the dense fp64 restatement ----------------------------------------------------------------------------------
def mult_adj(ei, n):
    """m [n, n] fp64 (row = destination): m[i, j] = how many times the edge j -> i is listed, self loops dropped"""
    keep = ei[0] != ei[1]
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=torch.float64), accumulate=True)
    return A


def operator(m, renormalize=True):
    """the operator the convs apply, dense fp64, from its closed form; -> (A2, dinv, d2)"""
    n = m.shape[0]
    d = 1.0 + m.sum(1)
    dinv = d.pow(-0.5)
    if not renormalize:
        return dinv[:, None] * (m + torch.eye(n, dtype=torch.float64)) * dinv[None, :], dinv, None
    d2 = 1.0 + dinv * (m @ dinv)
    s = dinv * d2.pow(-0.5)
    return s[:, None] * m * s[None, :] + torch.diag(1.0 / d2), dinv, d2


def restate(params, x, A, mode, masks=None):
    """fp64 JKNet forward (eval: no dropout); params: name -> tensor; masks: per layer, the ReLU pattern to impose (None: relu)"""
    L = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("convs."))
    xs = []
    for i in range(L):
        z = A @ (x @ params[f"convs.{i}.lin.weight"].t()) + params[f"convs.{i}.bias"]
        x = z * masks[i] if masks is not None else torch.relu(z)
        xs.append(x)
    j = torch.cat(xs, 1) if mode == "cat" else torch.stack(xs, 0).max(0)[0]
    return torch.log_softmax(j @ params["lin.weight"].t() + params["lin.bias"], dim=1)


def fixture_params(d, name, F_in, C, mode, L, hidden):
    """the fixture's initial parameters: stored (small fixture) or the seeded model rebuilt (office fixture; checked against the
    stored sums by test_state_dict_and_seeded_parameters_match_the_fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.jknet import JKNet
    torch.manual_seed(0)
    return {k: v.clone() for k, v in JKNet(F_in, hidden, C, L, 0.5, mode=mode).state_dict().items()}


def undirected(ei, n):
    """ToUndirected(merge=True): the coalesced union of both directions"""
    both = torch.cat([ei, ei.flip(0)], 1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


def params64(d, name, F_in, C, mode, L, hidden):
    return {k: v.double().requires_grad_(True) for k, v in fixture_params(d, name, F_in, C, mode, L, hidden).items()}


def _close(got, ref, rel=1e-10):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= rel * max(np.abs(ref).max(), 1e-30), f"max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})"


def test_small_fixture_graph_has_the_cases_it_is_for():
    d = load_golden("jknet_small.npz")
    ei, n = d["edge_index"], d["x"].shape[0]
    assert n == 40
    loops = ei[0][ei[0] == ei[1]]
    assert loops.size >= 3 and np.bincount(loops).max() >= 2                       # self loops, one of them twice
    pairs = ei[0] * n + ei[1]
    assert np.unique(pairs).size < pairs.size                                      # duplicate edges
    assert (np.bincount(ei[1], minlength=n) == 0).any()                            # rows without in-edges
    for name in ("jknet_small.npz", "jknet_office_a2d.npz"):
        for k, v in load_golden(name).items():
            assert v.dtype.kind in "fiub", k                                       # numeric arrays only
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jknet_office_a2d.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "gin_office_a2d.npz"))
    # the tool's fp32 run of the reference stayed inside GRAD_BAR for every tensor: no model gradient may lean on KINK_CAP
    for name in ("jknet_small.npz", "jknet_office_a2d.npz"):
        dd = load_golden(name)
        assert all(v.size == 0 for k, v in dd.items() if k.endswith("/flipped"))


def test_operator_facts_on_the_small_graph():
    from bridged_gnn_amd.jknet import JKGraph
    d = load_golden("jknet_small.npz")
    n = d["x"].shape[0]
    raw = torch.from_numpy(d["edge_index"]).long()
    for e in (raw, undirected(raw, n)):
        m = mult_adj(e, n)
        A2, dinv, d2 = operator(m)
        assert torch.equal(torch.diagonal(A2), 1.0 / d2)                                 # the diagonal is 1 / d2 ...
        s = dinv * d2.pow(-0.5)
        assert not torch.allclose(torch.diagonal(A2), s * s, rtol=1e-6)                  # ... which is not s^2
        assert torch.equal(A2, A2.t()) == torch.equal(m, m.t())                          # symmetric exactly when m is
        lonely = torch.nonzero(m.sum(1) == 0).reshape(-1)
        assert lonely.numel() > 0 or e is not raw                                        # the raw graph has rows without in-edges
        assert torch.equal(torch.diagonal(A2)[lonely], torch.ones(lonely.numel(), dtype=torch.float64))
        # the same matrix by the reference's route: normalise, put 1 on the diagonal, normalise again
        B = dinv[:, None] * (m + torch.eye(n, dtype=torch.float64)) * dinv[None, :]
        B = B - torch.diag(torch.diagonal(B)) + torch.eye(n, dtype=torch.float64)
        r = B.sum(1).pow(-0.5)
        _close(r[:, None] * B * r[None, :], A2, rel=1e-14)
        # JKGraph.scales, the fp64 formula the device graph rounds once, from the loop-free CSR
        keep = e[0] != e[1]
        src, dst = e[0][keep], e[1][keep]
        order = torch.sort(dst, stable=True).indices
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
        s64, w64 = JKGraph.scales(rowptr, src[order])
        _close(s64, s, rel=1e-14)
        _close(w64, 1.0 / d2, rel=1e-14)
        # renormalize=False rebuilds GcnGraph's dinv: (in-degree without loops + 1)^-1/2
        s1, w1 = JKGraph.scales(rowptr, src[order], renormalize=False)
        assert torch.equal(s1, (1.0 + m.sum(1)).rsqrt()) and torch.equal(w1, s1 * s1)
    assert not torch.equal(mult_adj(raw, n), mult_adj(raw, n).t())                       # the raw graph is the asymmetric case


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
        m = mult_adj(e, n)
        ops_ = {True: operator(m, True)[0], False: operator(m, False)[0]}
        for name, mode, L, hidden, renorm in models:
            params = params64(d, name, F_in, C, mode, L, hidden)
            pre = f"{var}/{name}/"
            logp = restate(params, x, ops_[renorm], mode)
            _close(logp.detach()[rows], d[pre + "logp"])
            loss = F.nll_loss(logp[tm], y[tm])
            assert abs(loss.item() - float(d[pre + "loss"])) <= 1e-12 * abs(float(d[pre + "loss"]))
            want = sub(d, pre + "grad/")
            assert sorted(params) == sorted(want) or not want
            if want:
                for (k, _), g in zip(params.items(), torch.autograd.grad(loss, list(params.values()))):
                    _close(g, want[k])


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_dense_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        m = mult_adj(e, n)
        ops_ = {True: operator(m, True)[0], False: operator(m, False)[0]}
        for name, mode, L, hidden, renorm in models:
            params = params64(d, name, F_in, C, mode, L, hidden)
            opt = torch.optim.Adam(list(params.values()), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(restate(params, x, ops_[renorm], mode)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            pre = f"{var}/{name}/"
            np.testing.assert_allclose(losses, d[pre + "adam_loss"], rtol=1e-10)
            for k, p in params.items():
                if pre + "adam/" + k in d:
                    _close(p.detach(), d[pre + "adam/" + k])


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_jknet.py"), "--out", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    for name in ("jknet_office_a2d.npz", "jknet_small.npz"):
        a, b = load_golden(name), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
