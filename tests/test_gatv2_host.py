"""CPU: the GATv2 fixtures (tools/gen_golden_gatv2.py, made by the reference's GATv2 class, models/backbones.py:302-358) against an
fp64 edge-list restatement written here -- the checker of the GPU tests --, the module's state_dict layout and seeded parameters,
the command line and driver signature, the refusal of host tensors and of shapes outside the envelope, and the three new symbols."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_golden, sub

OFFICE_MODELS = (("h64x1l2", 64, 1, 2, 4), ("h16x3l3", 16, 3, 3, 8))    # (name, hidden, heads, num_layers, seed): the generator's
SMALL_MODELS = (("h8x3l2", 8, 3, 2, 0), ("h6x1l3", 6, 1, 3, 0), ("h5x2l2", 5, 2, 2, 0))
BIG = ("convs.0.lin_l.weight", "convs.0.lin_r.weight")
SLOPE = 0.2


def edge_list(ei, n):
    """(src, dst) of the graph the convs walk: self loops of the input dropped, kept edges in input order, then the n self loops"""
    keep = ei[0] != ei[1]
    loops = torch.arange(n)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


def conv_sparse(XL, XR, att, src, dst, bias=None, edge_scale=None, sides=None, want_state=False, logits=None, slope=SLOPE):
    """fp64 GATv2 attention aggregation over an edge list.  XL, XR [N, H, C]; att [1, H, C]; edge_scale [E, H]: multiplies the
    coefficients (the dropout mask); sides [E, H, C] bool: the LeakyReLU side to take per edge, head and column instead of m > 0 (a
    GPU's own pattern); logits [E, H]: the softmax's inputs given directly (exact ones).
    -> out [N, H*C] (and (max, denominator) [N, H, 2] with want_state)"""
    N, H, C = XL.shape
    if logits is not None:
        e = logits
    else:
        m = XL[src] + XR[dst]
        lk = F.leaky_relu(m, slope) if sides is None else m * torch.where(sides, 1.0, slope).to(m.dtype)
        e = (lk * att).sum(-1)
    idx = dst.unsqueeze(1).expand(-1, H)
    mx = torch.full((N, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    ex = (e - mx[dst]).exp()
    den = torch.zeros(N, H, dtype=e.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    if edge_scale is not None:
        a = a * edge_scale
    out = torch.zeros(N, H, C, dtype=e.dtype).index_add_(0, dst, XL[src] * a.unsqueeze(-1)).reshape(N, H * C)
    if bias is not None:
        out = out + bias
    return (out, torch.stack([mx, den.detach()], dim=-1)) if want_state else out


def n_convs(p):
    return sum(1 for k in p if k.startswith("convs.") and k.endswith(".att"))


def restate(params, x, graph, sides=None):
    """fp64 GATv2 forward (eval: no dropout; the registered BatchNorms are not applied) -> log-probabilities.  graph: (src, dst);
    sides: None, or {conv index: [E, H, C] bool}"""
    src, dst = graph
    L = n_convs(params)
    h = x
    for i in range(L):
        c = f"convs.{i}."
        att = params[c + "att"]
        H, C = att.shape[1], att.shape[2]
        XL = (h @ params[c + "lin_l.weight"].t() + params[c + "lin_l.bias"]).view(-1, H, C)
        XR = (h @ params[c + "lin_r.weight"].t() + params[c + "lin_r.bias"]).view(-1, H, C)
        h = conv_sparse(XL, XR, att, src, dst, bias=params[c + "bias"], sides=None if sides is None else sides.get(i))
        if i < L - 1:
            h = F.elu(h)
    return torch.log_softmax(h, dim=1)


def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("gatv2_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("gatv2_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def fixture_params(d, name, F_in, C, hidden, heads, layers, seed):
    """the fixture's initial state_dict: stored (small fixture) or the seeded model rebuilt and checked against the stored fp64
    (sum, sum of squares) of every tensor to 1e-6 relative (office fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.gatv2 import GATv2
    torch.manual_seed(seed)
    sd = GATv2(F_in, hidden, C, layers, heads, 0.6, 0.5).state_dict()
    sums = sub(d, f"{name}/param_sum/")
    assert sorted(sums) == sorted(sd)
    for k, v in sd.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-6, atol=1e-300, err_msg=k)
    return {k: v.clone() for k, v in sd.items()}


def params64(sd):
    """fp64 leaves of a state_dict: the convs' tensors (the BatchNorms are registered and never applied: no gradient)"""
    return {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("convs.")}


def undirected(ei, n):
    """ToUndirected(merge=True): the coalesced union of both directions"""
    both = torch.cat([ei, ei.flip(0)], 1)
    key = torch.unique(both[0] * n + both[1])
    return torch.stack([key // n, key % n])


def close(got, ref, rel=1e-9, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= rel * max(np.abs(ref).max(), 1e-30), f"{what}: max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})"


def stored(d, prefix, name, k, full_tensor, sums_rtol=1e-9):
    """a whole tensor against what the fixture keeps of it -> (part to compare, stored part): all of it, or sampled rows after its
    (sum, sum of squares) met `sums_rtol`"""
    ref = d[f"{prefix}/{k}"]
    t = np.asarray(full_tensor, np.float64)
    if f"{prefix}_sum/{k}" in d:
        if sums_rtol is not None:
            np.testing.assert_allclose([t.sum(), (t * t).sum()], d[f"{prefix}_sum/{k}"], rtol=sums_rtol, err_msg=f"{prefix}_sum/{k}")
        t = t[d[f"wrows/{name}"]]
    return t, ref


def test_small_fixture_graph_has_the_cases_it_is_for():
    d = load_golden("gatv2_small.npz")
    ei, n = d["edge_index"], d["x"].shape[0]
    assert n == 40
    loops = ei[0][ei[0] == ei[1]]
    assert loops.size >= 3 and np.bincount(loops).max() >= 2                       # existing self loops, one duplicated
    pairs = ei[0][ei[0] != ei[1]] * n + ei[1][ei[0] != ei[1]]
    assert np.unique(pairs).size < pairs.size                                      # duplicate edges
    assert (np.bincount(ei[1][ei[0] != ei[1]], minlength=n) == 0).any()            # nodes without in-edges
    assert any(h * c % 4 for _, c, h, _, _ in SMALL_MODELS)                           # a width that is no multiple of 4
    assert {m[3] for m in SMALL_MODELS} == {2, 3} and {m[3] for m in OFFICE_MODELS} == {2, 3}
    for f in ("gatv2_small.npz", "gatv2_office_a2d.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20)
        assert all(v.dtype.kind in "fiub" for v in load_golden(f).values())           # numeric arrays only


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
        edges = edge_list(e, n)
        for name, hidden, heads, layers, seed in models:
            params = params64(fixture_params(d, name, F_in, C, hidden, heads, layers, seed))
            assert n_convs(params) == max(layers, 2)
            pre = f"{var}/{name}/"
            logp = restate(params, x, edges)
            loss = F.nll_loss(logp[tm], y[tm])
            close(logp.detach()[rows], d[pre + "logp"], what=pre + "logp")
            close(loss.item(), float(d[pre + "loss"]), what=pre + "loss")
            if pre + "grad/convs.0.att" not in d:
                continue
            grads = dict(zip(params, torch.autograd.grad(loss, list(params.values()))))
            assert sorted(sub(d, pre + "grad/")) == sorted(grads)
            for k, g in grads.items():
                close(*stored(d, pre + "grad", name, k, g.numpy()), what=pre + "grad/" + k)


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        graph = edge_list(e, n)
        for name, hidden, heads, layers, seed in models:
            params = params64(fixture_params(d, name, F_in, C, hidden, heads, layers, seed))
            opt = torch.optim.Adam(list(params.values()), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(restate(params, x, graph)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            pre = f"{var}/{name}/"
            np.testing.assert_allclose(losses, d[pre + "adam_loss"], rtol=1e-9)
            for k, p in params.items():
                if pre + "adam/" + k in d:
                    got, ref = stored(d, pre + "adam", name, k, p.detach().numpy())
                    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9, err_msg=pre + "adam/" + k)


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_module_state_dict_matches_fixture(fixture):
    from bridged_gnn_amd.gatv2 import GATv2
    d, x, y, _, models = _inputs(fixture)
    F_in, C = x.shape[1], int(y.max()) + 1
    for name, hidden, heads, layers, seed in models:
        # same initialisers in the same order as PyG's GATv2Conv: the seeded model IS the fixture's (office: via its sums)
        ref = fixture_params(d, name, F_in, C, hidden, heads, layers, seed)
        torch.manual_seed(seed)
        m = GATv2(F_in, hidden, C, layers, heads, 0.6, 0.5)
        sd = m.state_dict()
        L = max(layers, 2)
        assert len(m.convs) == L and len(m.bns) == L - 1 and m.adj_t_cache is None
        want = [f"convs.{i}.{leaf}" for i in range(L)
                for leaf in ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")]
        want += [f"bns.{i}.{leaf}" for i in range(L - 1)
                 for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        assert sorted(sd) == sorted(ref) == sorted(want)
        HC = heads * hidden
        shapes = {"convs.0.att": (1, heads, hidden), "convs.0.bias": (HC,), "convs.0.lin_l.weight": (HC, F_in),
                  "convs.0.lin_r.bias": (HC,), f"convs.{L - 1}.att": (1, 1, C), f"convs.{L - 1}.bias": (C,),
                  f"convs.{L - 1}.lin_r.weight": (C, HC), "bns.0.weight": (HC,)}
        if L == 3:
            shapes["convs.1.lin_l.weight"] = (HC, HC)
        for k, shp in shapes.items():
            assert tuple(sd[k].shape) == shp, k
        for k in ref:
            assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype
            if fixture == "small":
                assert torch.equal(sd[k], ref[k]), k
        assert float(sd["convs.0.lin_l.bias"].abs().max()) > 0 and float(sd["convs.0.bias"].abs().max()) == 0
        m.load_state_dict(ref, strict=True)
        for conv in m.convs:
            assert conv.lin_l.weight is not conv.lin_r.weight


def test_num_layers_one_builds_two_convs_as_two_does():
    from bridged_gnn_amd.gatv2 import GATv2
    a, b = GATv2(6, 4, 3, 1, 2, 0.6, 0.5), GATv2(6, 4, 3, 2, 2, 0.6, 0.5)
    assert len(a.convs) == len(b.convs) == 2 and sorted(a.state_dict()) == sorted(b.state_dict())
    assert not hasattr(a, "get_emb") and not hasattr(a, "get_logits")


def test_package_exports_and_unsupported_constructor_arguments():
    import bridged_gnn_amd
    from bridged_gnn_amd import gat, gatv2
    assert bridged_gnn_amd.GATv2 is gatv2.GATv2 and bridged_gnn_amd.GATv2Conv is gatv2.GATv2Conv
    assert gatv2.GatGraph is gat.GatGraph
    for kw in ({"share_weights": True}, {"edge_dim": 4}, {"add_self_loops": False}, {"heads": 2, "concat": False}):
        with pytest.raises(NotImplementedError):
            gatv2.GATv2Conv(4, 4, **kw)
    with pytest.raises(NotImplementedError):
        gatv2.GATv2Conv((4, 4), 4)
    keys = ["att", "bias", "lin_l.bias", "lin_l.weight", "lin_r.bias", "lin_r.weight"]
    assert sorted(gatv2.GATv2Conv(4, 3, heads=2).state_dict()) == keys
    assert tuple(gatv2.GATv2Conv(4, 3, heads=2).bias.shape) == (6,) and tuple(gatv2.GATv2Conv(4, 3, concat=False).bias.shape) == (3,)
    assert sorted(gatv2.GATv2Conv(4, 3, bias=False).state_dict()) == ["att", "lin_l.weight", "lin_r.weight"]


def test_seeded_draw_order_is_lin_l_lin_r_twice_then_att():
    """Linear.__init__ draws lin_l (weight, bias) and lin_r, reset_parameters draws both again and then att"""
    import math
    from bridged_gnn_amd.gatv2 import GATv2Conv
    torch.manual_seed(3)
    conv = GATv2Conv(5, 3, heads=2)
    torch.manual_seed(3)
    for _ in range(2):                                     # the first round is overwritten by the second
        ws, bs = [], []
        for _ in range(2):
            a = math.sqrt(6.0 / (6 + 5))
            ws.append(torch.empty(6, 5).uniform_(-a, a))
            bs.append(torch.empty(6).uniform_(-1 / math.sqrt(5), 1 / math.sqrt(5)))
    a = math.sqrt(6.0 / (2 + 3))
    att = torch.empty(1, 2, 3).uniform_(-a, a)
    assert torch.equal(conv.lin_l.weight, ws[0]) and torch.equal(conv.lin_r.weight, ws[1])
    assert torch.equal(conv.lin_l.bias, bs[0]) and torch.equal(conv.lin_r.bias, bs[1]) and torch.equal(conv.att, att)


def test_command_line_takes_the_step2_flags():
    from bridged_gnn_amd.gatv2 import build_parser
    a = build_parser().parse_args(["--path_data", "office_bridged_graph.dat", "--to_undirected", "--graphed", "--dataset_name", "office",
                                   "--num_epoch", "7", "--hidden_dim", "16", "--eval_metric", "auc", "--gpu", "0", "--save",
                                   "--num_layer", "3", "--heads", "2"])
    assert a.path_data == "office_bridged_graph.dat" and a.to_undirected and a.graphed and a.save
    assert (a.num_epoch, a.hidden_dim, a.eval_metric, a.heads, a.num_layer) == (7, 16, "auc", 2, 3)
    d = build_parser().parse_args([])
    assert not d.to_undirected and not d.graphed and d.num_epoch == 300 and d.hidden_dim == 64 and d.heads == 1


def test_driver_signature_is_train_gnn_noDTC_plus_heads_and_att_dropout():
    from bridged_gnn_amd.gatv2 import train_gatv2_noDTC
    from bridged_gnn_amd.transfer import train_gnn_noDTC
    ours, theirs = inspect.signature(train_gatv2_noDTC).parameters, inspect.signature(train_gnn_noDTC).parameters
    assert set(ours) == (set(theirs) - {"gnn"}) | {"heads", "att_dropout"}
    assert (ours["heads"].default, ours["dropout"].default, ours["att_dropout"].default, ours["num_layer"].default,
            ours["hidden"].default) == (1, 0.6, 0.5, 2, 64)                         # main_graph_knowledge_transfer.py:330
    for k in set(theirs) - {"gnn", "dropout"}:
        assert ours[k].default == theirs[k].default, k
    with pytest.raises(NotImplementedError, match="train_gatv2_noDTC"):            # the plain driver points here and keeps refusing
        train_gnn_noDTC(None, None, None, gnn="GATv2")


def test_gatv2_ops_refuse_host_tensors():
    import types
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gatv2 import GATv2
    tbl = torch.zeros(4, 16)
    rowptr = torch.arange(5, dtype=torch.int32)
    col = torch.arange(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gatv2_aggregate(tbl, torch.zeros(8), rowptr, col, 4, 2, 4, bias=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gatv2_aggregate_bwd(tbl, torch.zeros(8), torch.zeros(4, 2, 2), tbl[:, :8], tbl[:, :8], rowptr, col, rowptr, col, col, 2, 4)
    m = GATv2(8, 4, 3, 2, 2, 0.6, 0.5)
    data = types.SimpleNamespace(x=torch.zeros(4, 8), edge_index=torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(data)


def test_library_exports_the_new_symbols_and_refuses_shapes_outside_the_envelope():
    """the shape check of the C entries precedes every access: host buffers never reach a kernel"""
    from bridged_gnn_amd import _lib
    raw = ctypes.CDLL(_lib.SO_PATH)
    for n in ("bgnn_gatv2_aggregate_workspace_bytes", "bgnn_gatv2_aggregate_f32", "bgnn_gatv2_aggregate_bwd_f32"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.bgnn_version() == 116
    assert lib.bgnn_gatv2_aggregate_workspace_bytes(100, 10, 2, 8) >= 2 * 100 * 2 * 4 + 10 * 2 * 4 + 2 * 8 * 4
    buf = np.zeros(64, np.float32)
    P = ctypes.c_void_p(buf.ctypes.data)
    for H, C in ((9, 4), (0, 4), (1, 129), (1, 0)):
        assert lib.bgnn_gatv2_aggregate_workspace_bytes(100, 10, H, C) == 0
        rc = lib.bgnn_gatv2_aggregate_f32(P, 8, 1, P, None, P, P, 1, 1, H, C, 0.2, 0.0, 0, None, 0, 0.0, 0, None, None, None, P, None, None,
                                          0, P, 8, None)
        assert rc == -2, (H, C, rc)
        rc = lib.bgnn_gatv2_aggregate_bwd_f32(P, 8, 1, P, None, P, P, 8, P, 8, P, P, P, P, P, 1, 1, H, C, 0.2, 0.0, 0, None, 0, 0.0, 0,
                                              None, P, 64, None, None, P, 8, P, 8, P, None)
        assert rc == -2, (H, C, rc)

    def fwd(tbl=P, epi=0, p_drop=0.0, row_id=None, edge_base=None):
        return lib.bgnn_gatv2_aggregate_f32(tbl, 16, 1, P, None, P, P, 1, 1, 2, 4, 0.2, 0.0, 0, None, epi, p_drop, 0, None, row_id,
                                            edge_base, P, None, None, 0, P, 8, None)

    def bwd(n_src=1, n_rows=1, row_id=None, edge_base=None):
        return lib.bgnn_gatv2_aggregate_bwd_f32(P, 16, n_src, P, None, P, P, 8, P, 8, P, P, P, P, P, 1, n_rows, 2, 4, 0.2, 0.0, 0, None,
                                                0, 0.0, 0, None, P, 64, row_id, edge_base, P, 8, P, 16, P, None)

    # the fused log_softmax is for one head; dropout only after the ELU
    assert fwd(epi=2) == -2
    assert fwd(p_drop=0.5) == -2
    assert fwd(tbl=None) == -1
    # the ids are given together, and the sources include the destination rows: refused before any launch
    assert fwd(row_id=P) == -1 and fwd(edge_base=P) == -1
    assert bwd(row_id=P) == -1 and bwd(edge_base=P) == -1
    assert bwd(n_src=0, n_rows=1) == -2 and bwd(n_src=1, n_rows=2) == -2


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_gatv2.py"), "--out", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    for name in ("gatv2_office_a2d.npz", "gatv2_small.npz"):
        a, b = dict(np.load(os.path.join(GOLDEN, name))), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
