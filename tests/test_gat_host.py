"""CPU: the GAT fixtures (tools/gen_golden_gat.py, made by the reference's GAT class, models/backbones.py:404-438) against an fp64
DENSE restatement written here (softmax over a masked [N, N] score matrix with edge multiplicities) -- the checker of the GPU
tests --, the module's state_dict layout and seeded parameters, the command line, and the refusal of host tensors.

The dense form holds an [N, N] matrix per head and per autograd intermediate; on the 3408-node office graph it checks the
forward outputs and the loss.  The office gradients and Adam steps are checked through the edge-list (sparse) fp64 restatement,
which this file first pins to the dense one on the small fixture (outputs, gradients) and on the office forward."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_golden, sub

OFFICE_MODELS = (("h64x3", 64, 3), ("h16x8", 16, 8))
SMALL_MODELS = (("h8x3", 8, 3), ("h6x1", 6, 1), ("h5x2", 5, 2))
BIG = "conv1.lin_src.weight"
SLOPE = 0.2


def multiplicity(ei, n):
    """M [n, n] fp64 (row = destination): self loops of the input dropped, one per node, duplicate edges counted"""
    M = torch.zeros(n, n, dtype=torch.float64)
    keep = ei[0] != ei[1]
    M.index_put_((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=torch.float64), accumulate=True)
    return M + torch.eye(n, dtype=torch.float64)


def edge_list(ei, n):
    """(src, dst) of the same edge set as a list: kept edges in input order, then the n self loops"""
    keep = ei[0] != ei[1]
    loops = torch.arange(n)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


def _heads(p, conv):
    att = p[conv + ".att_src"]
    return att.shape[1], att.shape[2]


def conv_dense(p, conv, x, M):
    """fp64 GATConv over the multiplicity matrix, one head at a time"""
    H, C = _heads(p, conv)
    T = (x @ p[conv + ".lin_src.weight"].t()).view(-1, H, C)
    s_src = (T * p[conv + ".att_src"]).sum(-1)
    s_dst = (T * p[conv + ".att_dst"]).sum(-1)
    outs = []
    for h in range(H):
        E = F.leaky_relu(s_dst[:, h].unsqueeze(1) + s_src[:, h].unsqueeze(0), SLOPE)
        E = E.masked_fill(M == 0, -float("inf"))
        W = M * (E - E.max(dim=1, keepdim=True).values.detach()).exp()
        outs.append((W / W.sum(1, keepdim=True)) @ T[:, h, :])
    return torch.cat(outs, dim=1) + p[conv + ".bias"]


def conv_sparse(T, att_src, att_dst, src, dst, bias=None, edge_scale=None, sides=None, want_state=False, scores=None, logits=None):
    """fp64 attention aggregation over an edge list.  T [N, H, C]; edge_scale [E, H]: multiplies the coefficients (the dropout
    mask); sides [E, H] bool: the LeakyReLU side to take per edge and head instead of z > 0 (a GPU's own pattern); scores =
    (s_src, s_dst) [N, H]: per-node scores given as inputs of their own instead of <T, att>; logits [E, H]: the softmax's inputs
    given directly.  -> out [N, H*C] (and (max, denominator) [N, H, 2] with want_state)"""
    N, H, C = T.shape
    if logits is not None:
        e = logits
    else:
        s_src, s_dst = scores if scores is not None else ((T * att_src).sum(-1), (T * att_dst).sum(-1))
        z = s_src[src] + s_dst[dst]
        e = F.leaky_relu(z, SLOPE) if sides is None else z * torch.where(sides, 1.0, SLOPE).to(z.dtype)
    idx = dst.unsqueeze(1).expand(-1, H)
    m = torch.full((N, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    ex = (e - m[dst]).exp()
    den = torch.zeros(N, H, dtype=e.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    if edge_scale is not None:
        a = a * edge_scale
    out = torch.zeros(N, H, C, dtype=e.dtype).index_add_(0, dst, T[src] * a.unsqueeze(-1)).reshape(N, H * C)
    if bias is not None:
        out = out + bias
    return (out, torch.stack([m, den.detach()], dim=-1)) if want_state else out


def _conv_edges(p, conv, x, src, dst, sides=None):
    H, C = _heads(p, conv)
    T = (x @ p[conv + ".lin_src.weight"].t()).view(-1, H, C)
    return conv_sparse(T, p[conv + ".att_src"], p[conv + ".att_dst"], src, dst, bias=p[conv + ".bias"], sides=sides)


def restate(params, x, graph, emb=False, sides=None):
    """fp64 GAT forward (eval: no dropout) -> log-probabilities, or get_emb.  graph: the dense multiplicity matrix, or (src, dst).
    sides: None, or {conv: [E, H] bool} for the edge-list form"""
    dense = torch.is_tensor(graph)
    conv = (lambda c, h: conv_dense(params, c, h, graph)) if dense else \
        (lambda c, h: _conv_edges(params, c, h, graph[0], graph[1], None if sides is None else sides.get(c)))
    h = F.elu(conv("conv1", x))
    return h if emb else torch.log_softmax(conv("conv2", h), dim=1)


def _inputs(name):
    if name == "office":
        g = load_golden("office_a2d_graph.npz")
        return load_golden("gat_office_a2d.npz"), g["x"], g["y"], g["edge_index"], OFFICE_MODELS
    d = load_golden("gat_small.npz")
    return d, d["x"], d["y"], d["edge_index"], SMALL_MODELS


def fixture_params(d, name, F_in, C, hidden, head):
    """the fixture's initial parameters: stored (small fixture) or the seeded model rebuilt and checked against the stored
    fp64 (sum, sum of squares) of every tensor to 1e-6 relative (office fixture)"""
    full = sub(d, f"{name}/param/")
    if full:
        return {k: torch.from_numpy(v) for k, v in full.items()}
    from bridged_gnn_amd.gat import GAT
    torch.manual_seed(0)
    sd = GAT(types.SimpleNamespace(num_features=F_in, num_classes=C), hidden=hidden, head=head).state_dict()
    sums = sub(d, f"{name}/param_sum/")
    assert sorted(sums) == sorted(sd)
    for k, v in sd.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-6, atol=1e-300, err_msg=k)
    return {k: v.clone() for k, v in sd.items()}


def params64(sd):
    """fp64 leaves of a state_dict; lin_dst.weight IS lin_src.weight (one leaf, one gradient)"""
    P = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in sd.items() if ".lin_dst." not in k}
    return P


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
    (sum, sum of squares) met `sums_rtol` (None: not checked -- an fp32 result; its other rows are the caller's to cover)"""
    ref = d[f"{prefix}/{k}"]
    t = np.asarray(full_tensor, np.float64)
    if f"{prefix}_sum/{k}" in d:
        if sums_rtol is not None:
            np.testing.assert_allclose([t.sum(), (t * t).sum()], d[f"{prefix}_sum/{k}"], rtol=sums_rtol, err_msg=f"{prefix}_sum/{k}")
        t = t[d[f"wrows/{name}"]]
    return t, ref


def test_small_fixture_graph_has_the_cases_it_is_for():
    d = load_golden("gat_small.npz")
    ei, n = d["edge_index"], d["x"].shape[0]
    assert n == 40
    loops = ei[0][ei[0] == ei[1]]
    assert loops.size >= 3 and np.bincount(loops).max() >= 2                       # existing self loops, one duplicated
    pairs = ei[0][ei[0] != ei[1]] * n + ei[1][ei[0] != ei[1]]
    assert np.unique(pairs).size < pairs.size                                      # duplicate edges
    assert (np.bincount(ei[1][ei[0] != ei[1]], minlength=n) == 0).any()            # nodes without in-edges
    assert any(h * c % 4 for _, h, c in SMALL_MODELS)                              # a width that is no multiple of 4


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_restatement_reproduces_fixture(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x = torch.from_numpy(x).double()
    y = torch.from_numpy(y).long()
    tm = torch.from_numpy(d["train_mask"])
    rows, erows = torch.from_numpy(d["rows"]), torch.from_numpy(d["emb_rows"])
    assert not bool((y[tm] == -1).any())
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        M, edges = multiplicity(e, n), edge_list(e, n)
        for name, hidden, head in models:
            params = params64(fixture_params(d, name, F_in, C, hidden, head))
            pre = f"{var}/{name}/"
            with torch.no_grad():                       # the dense form: outputs and loss on both fixtures
                emb = restate(params, x, M, emb=True)
                logp = torch.log_softmax(conv_dense(params, "conv2", emb, M), dim=1)
                close(logp[rows], d[pre + "logp"], what=pre + "logp")
                close(emb[erows], d[pre + "emb"], what=pre + "emb")
                close(F.nll_loss(logp[tm], y[tm]).item(), float(d[pre + "loss"]), what=pre + "loss")
                close(restate(params, x, edges), logp, what=pre + "edge-list form against dense")
            if pre + "grad/conv1.att_src" not in d:
                continue
            loss = F.nll_loss(restate(params, x, edges)[tm], y[tm])
            grads = dict(zip(params, torch.autograd.grad(loss, list(params.values()))))
            if fixture == "small":                      # dense gradients too, where [N, N] intermediates are small
                dl = F.nll_loss(restate(params, x, M)[tm], y[tm])
                for k, g in zip(params, torch.autograd.grad(dl, list(params.values()))):
                    close(g, grads[k], what=pre + k + " dense against edge-list gradient")
            for k, g in grads.items():
                close(*stored(d, pre + "grad", name, k, g.numpy()), what=pre + "grad/" + k)


@pytest.mark.parametrize("fixture", ["office", "small"])
def test_fp64_restatement_reproduces_adam_trajectory(fixture):
    d, x, y, ei, models = _inputs(fixture)
    n, F_in, C = x.shape[0], x.shape[1], int(y.max()) + 1
    x, y, tm = torch.from_numpy(x).double(), torch.from_numpy(y).long(), torch.from_numpy(d["train_mask"])
    raw = torch.from_numpy(np.asarray(ei)).long()
    for var, e in (("raw", raw), ("und", undirected(raw, n))):
        graph = multiplicity(e, n) if fixture == "small" else edge_list(e, n)
        for name, hidden, head in models:
            params = params64(fixture_params(d, name, F_in, C, hidden, head))
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
    from bridged_gnn_amd.gat import GAT
    d, x, y, _, models = _inputs(fixture)
    F_in, C = x.shape[1], int(y.max()) + 1
    ds = types.SimpleNamespace(num_features=F_in, num_classes=C)
    for name, hidden, head in models:
        # same initialisers in the same order as PyG's GATConv: the seeded model IS the fixture's (office: via its sums)
        ref = fixture_params(d, name, F_in, C, hidden, head)
        torch.manual_seed(0)
        m = GAT(ds, hidden=hidden, head=head)
        sd = m.state_dict()
        assert sorted(sd) == sorted(ref)
        assert sorted(sd) == sorted(f"conv{i}.{leaf}" for i in (1, 2)
                                    for leaf in ("att_dst", "att_src", "bias", "lin_dst.weight", "lin_src.weight"))
        shapes = {"conv1.att_src": (1, head, hidden), "conv1.bias": (head * hidden,), "conv1.lin_src.weight": (head * hidden, F_in),
                  "conv2.att_dst": (1, 1, C), "conv2.bias": (C,), "conv2.lin_dst.weight": (C, head * hidden)}
        for k, shp in shapes.items():
            assert tuple(sd[k].shape) == shp, k
        for k in ref:
            assert sd[k].shape == ref[k].shape and sd[k].dtype == torch.float32
            if fixture == "small":
                assert torch.equal(sd[k], ref[k]), k
        m.load_state_dict(ref, strict=True)
        for conv in (m.conv1, m.conv2):
            assert conv.lin_src.weight is conv.lin_dst.weight
        names = [k for k, _ in m.named_parameters()]
        assert len(names) == 8 and not any(".lin_dst." in k for k in names)          # the shared Linear is yielded once


def test_package_exports_and_unsupported_constructor_arguments():
    import bridged_gnn_amd
    from bridged_gnn_amd import gat
    assert bridged_gnn_amd.GAT is gat.GAT and bridged_gnn_amd.GATConv is gat.GATConv
    for kw in ({"edge_dim": 4}, {"add_self_loops": False}, {"heads": 2, "concat": False}):
        with pytest.raises(NotImplementedError):
            gat.GATConv(4, 4, **kw)
    with pytest.raises(NotImplementedError):
        gat.GATConv((4, 4), 4)
    assert sorted(gat.GATConv(4, 3, heads=2).state_dict()) == ["att_dst", "att_src", "bias", "lin_dst.weight", "lin_src.weight"]
    assert tuple(gat.GATConv(4, 3, heads=2).bias.shape) == (6,) and tuple(gat.GATConv(4, 3, concat=False).bias.shape) == (3,)
    assert "bias" not in gat.GATConv(4, 3, bias=False).state_dict()
    assert not hasattr(gat.GAT, "get_logits")


def test_command_line_takes_the_step2_flags():
    from bridged_gnn_amd.gat import build_parser
    a = build_parser().parse_args(["--path_data", "office_bridged_graph.dat", "--to_undirected", "--graphed", "--dataset_name", "office",
                                   "--num_epoch", "7", "--hidden_dim", "16", "--eval_metric", "auc", "--gpu", "0", "--save"])
    assert a.path_data == "office_bridged_graph.dat" and a.to_undirected and a.graphed and a.save
    assert (a.num_epoch, a.hidden_dim, a.eval_metric, a.head) == (7, 16, "auc", 3)
    d = build_parser().parse_args([])
    assert not d.to_undirected and not d.graphed and d.num_epoch == 300 and d.hidden_dim == 64


def test_driver_signature_is_train_gnn_noDTC_plus_head():
    import inspect
    from bridged_gnn_amd.gat import train_gat_noDTC
    from bridged_gnn_amd.transfer import train_gnn_noDTC
    ours, theirs = inspect.signature(train_gat_noDTC).parameters, inspect.signature(train_gnn_noDTC).parameters
    assert set(ours) == (set(theirs) - {"gnn"}) | {"head"} and ours["head"].default == 3
    for k in set(theirs) - {"gnn", "dropout"}:
        assert ours[k].default == theirs[k].default, k


def test_gat_ops_refuse_host_tensors_and_wide_shapes():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gat import GAT
    tbl = torch.zeros(4, 8)
    s = torch.zeros(4, 2)
    rowptr = torch.arange(5, dtype=torch.int32)
    col = torch.arange(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gat_scores(tbl, torch.zeros(8), torch.zeros(8), 2, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gat_aggregate(tbl, s, s, rowptr, col, 4, 2, 4, bias=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gat_aggregate_bwd(tbl, s, s, torch.zeros(4, 2, 2), torch.zeros(4, 2), tbl, tbl, rowptr, col, rowptr, col, col, 2, 4)
    m = GAT(types.SimpleNamespace(num_features=8, num_classes=3), hidden=4, head=2)
    data = types.SimpleNamespace(x=tbl, edge_index=torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(data)


@pytest.mark.skipif(not __import__("oracle.ref_import").ref_import.reference_available(), reason="reference tree not present")
def test_generator_reproduces_fixtures(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_gat.py"), "--out", str(tmp_path)],
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    for name in ("gat_office_a2d.npz", "gat_small.npz"):
        a, b = dict(np.load(os.path.join(GOLDEN, name))), dict(np.load(tmp_path / name))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{name}:{k}"
