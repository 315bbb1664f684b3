"""GPU: the atomic-free aggregation backward for 128 < D <= 256 (the wave-per-row route of bgnn_adaptedconv_aggregate_bwd_pull_f32,
csrc/bgnn_aggregate_bwd_wide.hip): ABI envelope and the border to the D <= 128 routes, fp64 autograd on the same tables, the atomic
scatter form, hub rows against the plain walk, bitwise reproducibility and the route `ops.adaptedconv_aggregate_bwd` takes; and
for both pull entries, that the advertised workspace is the accepted one."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from oracle import oracle_torch as OT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.1
# D -> (nodes, frac_src): 129 = one live column in lane 32, lanes 33..63 dead; 255 = a pad column inside the last live lane;
# 256 = every lane and all eight sign words; 600 nodes = 150 tiles (more than one block per XCD), 40 nodes = fewer tiles than blocks
CASES = {129: (40, 0.3), 132: (150, 0.7), 160: (600, 0.3), 192: (333, 0.7), 255: (257, 0.3), 256: (600, 0.7)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _inputs(ei, mask, n, D, seed, ld=None):
    """tables (pad columns 0), attention vectors, the forward's out / alpha and dL/dout on the GPU, the numpy originals beside them"""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(seed)
    ld = ops.pad4(D) if ld is None else ld
    tabs = []
    for _ in range(2):
        t = np.zeros((n, ld), np.float32)
        t[:, :D] = rng.standard_normal((n, D)).astype(np.float32)
        tabs.append(t)
    a = (rng.standard_normal((2, D)) * 0.3).astype(np.float32)
    w = np.zeros((n, ld), np.float32)
    w[:, :D] = rng.standard_normal((n, D)).astype(np.float32)
    c = dict(ei=ei, mask=mask, n=n, D=D, ld=ld, tabs=tabs, a=a, w=w)
    c["csr"] = ops.build_dst_csr(_t(ei), n)
    c["m8"] = _t(mask).to(torch.uint8)
    c["hS"], c["hT"], c["a1"], c["a2"], c["g"] = _t(tabs[0]), _t(tabs[1]), _t(a[0]), _t(a[1]), _t(w)
    return c


def _forward(c):
    from bridged_gnn_amd import ops
    c["out"], c["alpha"] = ops.adaptedconv_aggregate(c["hS"], c["hT"], c["a1"], c["a2"], c["csr"], c["m8"], c["D"], SLOPE, want_alpha=True)
    return c


def _op(c):
    from bridged_gnn_amd import ops
    return ops.adaptedconv_aggregate_bwd(c["hS"], c["hT"], c["a1"], c["a2"], c["csr"], c["m8"], c["D"], c["out"], c["alpha"], c["g"], SLOPE)


def _hub_args(csr, hubs=True):
    """the hub-table argument group of the pull entries (bgnn.h) and the two segment counts"""
    from bridged_gnn_amd import _lib, ops
    P = _lib.ptr
    args, nseg = [ops.HUB_THRESHOLD], []
    for tables in ((csr.hub_tables(), csr.transposed_hub_tables()) if hubs else (None, None)):
        rows, seg_ptr, bounds, node = tables if tables is not None else (None, None, None, None)
        nseg.append(0 if tables is None else int(node.numel()))
        args += [P(rows), 0 if tables is None else int(rows.numel()), P(seg_ptr), P(bounds), P(node), nseg[-1]]
    return args, nseg[0], nseg[1]


def _direct(c, D=None, ld=None, hubs=True, ws_bytes=None, ws_short=0):
    """bgnn_adaptedconv_aggregate_bwd_pull_f32 called through ctypes -> (rc, (dh_t2s, dh_s2t, da_t2s, da_s2t)); the workspace
    size claimed is `ws_bytes`, by default the advertised one less `ws_short`.  Outputs are NaN-prefilled (every element must be
    written), but da for D <= 128, which is accumulated into, is zeroed as its contract says."""
    from bridged_gnn_amd import _lib
    L = _lib.lib()
    P = _lib.ptr
    csr, n = c["csr"], c["n"]
    D = c["D"] if D is None else D
    ld = c["ld"] if ld is None else ld
    t_rowptr, t_eid, t_dst = csr.transposed()
    hub_args, nd, ns = _hub_args(csr, hubs)
    wsb = L.bgnn_aggregate_bwd_pull_workspace_bytes(n, csr.num_edges, ld, D, nd, ns)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    d1, d2 = torch.full_like(c["hS"], float("nan")), torch.full_like(c["hT"], float("nan"))
    fill = float("nan") if D > 128 else 0.0
    da1, da2 = torch.full((max(D, 1),), fill, device=DEV), torch.full((max(D, 1),), fill, device=DEV)
    rc = L.bgnn_adaptedconv_aggregate_bwd_pull_f32(
        P(c["hS"]), P(c["hT"]), ld, P(c["a1"]), P(c["a2"]), P(csr.rowptr), P(csr.col), P(c["m8"]), P(t_rowptr), P(t_eid), P(t_dst),
        n, csr.num_edges, D, SLOPE, P(c["out"]), ld, P(c["alpha"]), P(c["g"]), ld, P(d1), P(d2), P(da1), P(da2), *hub_args,
        P(ws), wsb - ws_short if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, (d1, d2, da1, da2)


def _fp64(c):
    """autograd in fp64 ON THE SAME fp32 TABLES (the oracle of test_aggregation_backward_exact_on_the_same_tables)"""
    n, D = c["n"], c["D"]
    mo = torch.from_numpy(c["mask"])
    e1, e2 = OT.graph_partition(torch.from_numpy(c["ei"]), mo)
    t1 = torch.from_numpy(c["tabs"][0][:, :D]).double().requires_grad_(True)
    t2 = torch.from_numpy(c["tabs"][1][:, :D]).double().requires_grad_(True)
    b1 = torch.from_numpy(c["a"][0]).double().requires_grad_(True)
    b2 = torch.from_numpy(c["a"][1]).double().requires_grad_(True)
    al = OT.segment_softmax(torch.cat((F.leaky_relu(t1[e1[0]] + t1[e1[1]], SLOPE) @ b1, F.leaky_relu(t2[e2[0]] + t2[e2[1]], SLOPE) @ b2)),
                            torch.cat((e1[1], e2[1])), n)
    o = torch.zeros(n, D, dtype=torch.float64)
    o = o.index_add(0, e1[1], t1[e1[0]] * al[: e1.shape[1], None]).index_add(0, e2[1], t2[e2[0]] * al[e1.shape[1]:, None])
    (o * torch.from_numpy(c["w"][:, :D]).double()).sum().backward()
    return t1.grad, t2.grad, b1.grad, b2.grad


@functools.lru_cache(maxsize=None)
def _random_case(D):
    """one seeded case per width, shared by the fp64 and the scatter-form tests: inputs, the op's result, the fp64 gradients"""
    from bridged_gnn_amd import synth
    n, frac = CASES[D]
    ei, mask = synth.random_multigraph(n, 6 * n, frac_src=frac, n_isolated=2, seed=D)          # duplicate edges, self loops
    c = _forward(_inputs(ei, mask, n, D, seed=1000 + D))
    c["got"] = _op(c)
    c["ref"] = _fp64(c)
    return c


def _hub_case(D):
    """one destination with 193 in-edges (three full 64-edge segments and a 1-edge tail), one with exactly 128 (on the threshold),
    one source with 200 out-edges, 300 ordinary nodes; the counts include the rewritten self loop"""
    rng = np.random.default_rng(77)
    n = 303
    bg = rng.integers(3, n, size=(2, 1800))
    e_a = np.stack([rng.integers(3, n, size=192), np.zeros(192, np.int64)])
    e_b = np.stack([rng.integers(3, n, size=127), np.ones(127, np.int64)])
    e_c = np.stack([np.full(199, 2, np.int64), rng.integers(3, n, size=199)])
    ei = np.concatenate([bg, e_a, e_b, e_c], axis=1).astype(np.int64)
    mask = rng.random(n) < 0.5
    mask[0], mask[1], mask[2] = True, False, True
    c = _forward(_inputs(ei, mask, n, D, seed=2000 + D))
    csr = c["csr"]
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).cpu()
    t_rp = csr.transposed()[0].cpu()
    assert int(deg[0]) == 193 and int(deg[1]) == 128 and int(t_rp[3] - t_rp[2]) == 200
    d_rows, d_ptr, d_bounds, _ = csr.hub_tables()
    s_rows = csr.transposed_hub_tables()[0]
    assert d_rows.cpu().tolist() == [0, 1] and s_rows.cpu().tolist() == [2]
    assert d_ptr.cpu().tolist() == [0, 4, 6] and int(d_bounds[7] - d_bounds[6]) == 1        # 64 + 64 + 64 + 1 | 64 + 64
    return c


def _tiny_case(D):
    ei = np.array([[0, 1, 2, 3, 0, 0], [1, 2, 3, 0, 2, 2]], np.int64)
    return _forward(_inputs(ei, np.array([True, False, True, False]), 4, D, seed=D))


def _assert_whole_and_fp64(c, got):
    D = c["D"]
    for t in got:
        assert bool(torch.isfinite(t).all())
    for name, a, b in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), got, _fp64(c)):
        assert _rel(a[..., :D].double().cpu(), b) < 2e-5, name


def test_abi_envelope():
    """0 inside the envelope (D = 132 on a 4-node graph, every output element written); BGNN_E_SHAPE at D = 0, D = 260 and
    ldh = 134; BGNN_E_WORKSPACE with a 16-byte workspace."""
    c = _tiny_case(132)
    rc, got = _direct(c)
    assert rc == 0
    _assert_whole_and_fp64(c, got)
    # the refusals come before any launch, so the same 132-column buffers serve (the claimed widths are never walked)
    assert _direct(c, ws_bytes=16)[0] == -3
    assert _direct(c, D=0)[0] == -2
    assert _direct(c, D=260, ld=260)[0] == -2
    assert _direct(c, ld=134)[0] == -2


@pytest.mark.parametrize("D", [128, 129])
def test_entry_at_the_border_of_the_wide_route(D):
    """the one entry on either side of D = 128 (lane groups of 32 | a wave per row) on the 4-node graph: 0, every element of the
    NaN-prefilled outputs written (da of D = 128, which is accumulated into, zeroed beforehand), fp64 at 2e-5"""
    c = _tiny_case(D)
    rc, got = _direct(c)
    assert rc == 0
    _assert_whole_and_fp64(c, got)


def _untouched(got, D):
    return all(bool(torch.isnan(t).all()) for t in got[:2]) and all(bool((torch.isnan(t) if D > 128 else t == 0).all()) for t in got[2:])


@pytest.mark.parametrize("graph,D", [("tiny", 2), ("tiny", 16), ("tiny", 100), ("tiny", 160), ("hub", 100), ("hub", 160)])
def test_advertised_workspace_is_the_accepted_workspace(graph, D):
    """bgnn_aggregate_bwd_pull_workspace_bytes is exactly what the entry accepts: one byte less is BGNN_E_WORKSPACE with
    nothing launched (the prefilled outputs stay as they were), the advertised size runs"""
    c = _tiny_case(D) if graph == "tiny" else _hub_case(D)
    rc, got = _direct(c, ws_short=1)
    assert rc == -3 and _untouched(got, D)
    rc, got = _direct(c)
    assert rc == 0 and bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("graph", ["tiny", "hub"])
def test_advertised_heads_workspace_is_the_accepted_workspace(graph):
    """the same for bgnn_aggregate_heads_bwd_workspace_bytes / bgnn_adaptedconv_aggregate_heads_bwd_f32 at heads = 3, D = 2"""
    from bridged_gnn_amd import _lib, ops
    L, P, heads, D = _lib.lib(), _lib.ptr, 3, 2
    base = _tiny_case(4) if graph == "tiny" else _hub_case(4)          # (the graph; the tables below are the heads' own)
    csr, m8, n = base["csr"], base["m8"], base["n"]
    g = torch.Generator(device=DEV).manual_seed(5)
    t2s, s2t, gr = (torch.zeros(n, heads * 4, device=DEV) for _ in range(3))
    for t in (t2s, s2t, gr):
        for h in range(heads):
            t[:, 4 * h:4 * h + D] = torch.randn(n, D, device=DEV, generator=g)
    a1, a2 = torch.randn(heads, D, device=DEV, generator=g) * 0.3, torch.randn(heads, D, device=DEV, generator=g) * 0.3
    ms = torch.zeros(n, heads, 2, device=DEV)
    out = ops.adaptedconv_aggregate(t2s, s2t, a1, a2, csr, m8, D, SLOPE, heads=heads, log_softmax=True, state_ms=ms, part=3)
    t_rowptr, _, t_dst = csr.transposed()
    hub_args, nd, ns = _hub_args(csr)
    assert (nd > 0 and ns > 0) == (graph == "hub")
    wsb = L.bgnn_aggregate_heads_bwd_workspace_bytes(n, csr.num_edges, heads, nd, ns)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    for claimed, want in ((wsb - 1, -3), (wsb, 0)):
        d1, d2 = torch.full_like(t2s, float("nan")), torch.full_like(s2t, float("nan"))
        da1, da2 = torch.zeros(heads, D, device=DEV), torch.zeros(heads, D, device=DEV)
        rc = L.bgnn_adaptedconv_aggregate_heads_bwd_f32(
            P(t2s), P(s2t), P(a1), P(a2), P(csr.rowptr), P(csr.col), P(m8), P(t_rowptr), P(t_dst), n, csr.num_edges, D, heads, SLOPE,
            P(out), P(ms), P(gr), 1, P(d1), P(d2), P(da1), P(da2), *hub_args, P(ws), claimed, _lib.stream())
        torch.cuda.synchronize()
        assert rc == want
        if want == 0:
            assert bool(torch.isfinite(d1).all()) and bool(torch.isfinite(d2).all())
        else:
            assert bool(torch.isnan(d1).all()) and bool(torch.isnan(d2).all()) and not bool(da1.any()) and not bool(da2.any())


@pytest.mark.parametrize("D", sorted(CASES))
def test_wide_pull_backward_matches_fp64(D):
    """all four gradients against fp64 autograd at 2e-5 of each tensor's max (the bar of the D <= 128 pull tests); pad columns
    of both dH tables exactly 0"""
    c = _random_case(D)
    for t in c["tabs"]:
        assert (t[:, 128:D] > 0).any() and (t[:, 128:D] < 0).any(), "columns >= 128 must carry both signs (upper four sign words)"
    for name, a, b in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), c["got"], c["ref"]):
        err = _rel(a[..., :D].double().cpu(), b)
        print(f"D={D} {name}: {err:.3e} of max")
        assert err < 2e-5, (name, D, err)
    assert c["got"][0].shape[1] == c["ld"]
    assert not bool(c["got"][0][:, D:].any()) and not bool(c["got"][1][:, D:].any()), "pad columns"


@pytest.mark.parametrize("D", sorted(CASES))
def test_wide_pull_backward_equals_atomic_backward(D):
    """the same seeds through bgnn_adaptedconv_aggregate_bwd_f32 (the scatter form) called directly"""
    from bridged_gnn_amd import _lib
    c = _random_case(D)
    L, P, ld, n = _lib.lib(), _lib.ptr, c["ld"], c["n"]
    d1, d2 = torch.zeros_like(c["hS"]), torch.zeros_like(c["hT"])
    da1, da2 = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    rc = L.bgnn_adaptedconv_aggregate_bwd_f32(P(c["hS"]), P(c["hT"]), ld, P(c["a1"]), P(c["a2"]), P(c["csr"].rowptr), P(c["csr"].col),
                                              P(c["m8"]), 0, n, D, SLOPE, P(c["out"]), ld, P(c["alpha"]), P(c["g"]), ld,
                                              P(d1), P(d2), P(da1), P(da2), _lib.stream())
    assert rc == 0
    for name, a, b in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), c["got"], (d1, d2, da1, da2)):
        err = _rel(a.double().cpu(), b.double().cpu())
        print(f"D={D} {name}: {err:.3e} of max")
        assert err < 2e-5, (name, D, err)


@pytest.mark.parametrize("D", [160, 256])
def test_wide_pull_hub_rows_equal_the_plain_walk(D, monkeypatch):
    """hub rows as segments + merges against the same call with BGNN_HUB_ROWS=0 (every row one chain), default bar"""
    c = _hub_case(D)
    hub = _op(c)
    monkeypatch.setenv("BGNN_HUB_ROWS", "0")
    plain = _op(c)
    monkeypatch.delenv("BGNN_HUB_ROWS")
    ref = _fp64(c)
    for name, a, b, r in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), hub, plain, ref):
        print(f"D={D} {name}: hub vs fp64 {_rel(a[..., :D].double().cpu(), r):.3e}, plain vs fp64 {_rel(b[..., :D].double().cpu(), r):.3e}")
        assert_close(a.cpu().numpy(), b.cpu().numpy(), what=name)
        assert _rel(a[..., :D].double().cpu(), r) < 2e-5, name


def test_wide_pull_is_reproducible_and_is_the_ops_route():
    """two calls on the hub graph at D = 256 give equal bits in all four outputs, and `ops.adaptedconv_aggregate_bwd` gives the
    bits of the direct ABI call (so the op routes here; the scatter form's atomics would not reproduce them)"""
    c = _hub_case(256)
    first, again = _op(c), _op(c)
    rc, direct = _direct(c)
    assert rc == 0
    for name, a, b, d in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), first, again, direct):
        assert torch.equal(a, b), name
        assert torch.equal(a, d), name
