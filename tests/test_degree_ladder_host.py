"""Host side of the degree-ladder tests (no GPU): the ladder builder's coverage on both sides for every
rewrite variant, its determinism, its duplicates, the restated (LF, EP, U) tables against the kernel sources, and every fp64
restatement of tests/degree_ladder.py that test_gpu_degree_ladder.py compares a kernel with against a DENSE formulation
(A @ X with A the matrix of edge counts, dense softmaxes) on the ladder graph, so that reference and kernel cannot be wrong
together.  The restatements are edge lists under index_add; the dense forms never touch an edge list."""
import os
import re

import numpy as np
import pytest
import torch

import degree_ladder as dl

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bridged_gnn_amd", "csrc")
TIGHT = 1e-12        # fp64 against fp64 over at most 97 terms a row


def _views(variant):
    g = dl.Ladder(variant)
    src, dst = g.walked()
    return g, dl.csr_by(dst, src, g.N), dl.csr_by(src, dst, g.N)


def _close(a, b, what, scale=None):
    s = (b.abs().max().item() if scale is None else scale) + 1e-300
    assert (a - b).abs().max().item() <= TIGHT * s, what


def test_ladder_degrees_and_batch_sizes():
    L = dl.ladder_degrees()
    assert L[0] == 0 and L[-1] == 97 and len(L) == 30, L
    assert dl.batch_sizes() == {4, 8, 16, 32}
    dl.assert_batches_bracketed(L)
    assert [dl.rung(D) for D in dl.WIDTHS] == [(1, 8, 4), (2, 4, 4), (4, 2, 4), (8, 1, 8), (16, 1, 8), (32, 1, 8)]
    assert [dl.rung(D)[1] * dl.rung(D)[2] for D in dl.WIDTHS] == [32, 16, 8, 8, 8, 8]
    assert [dl.rows_per_wave(D) for D in dl.WIDTHS] == [8, 8, 8, 8, 4, 2]
    assert [dl.rung(D, dl.ADAPTED_LADDER) for D in dl.ADAPTED_WIDTHS] == [(4, 1, 8), (8, 1, 4), (16, 1, 4), (32, 1, 4)]


def test_restated_tables_are_the_kernels_own():
    """lf_ladder of bgnn_conv_common.h, aggregate()'s switch of bgnn_aggregate.hip and the fixed U of the attention files, read
    from the sources: a changed table fails here (and in the GPU tests' coverage assertions), it does not silence them"""
    src = open(os.path.join(CSRC, "bgnn_conv_common.h")).read()
    got = re.findall(r"if \(nv <= (\d+)\) return f\(int_c<(\d+)>\{\}, int_c<(\d+)>\{\}, int_c<(\d+)>\{\}\);", src)
    last = re.search(r"return f\(int_c<(\d+)>\{\}, int_c<(\d+)>\{\}, int_c<(\d+)>\{\}\);\n\}", src)
    table = [(int(a), (int(b), int(c), int(d))) for a, b, c, d in got] + [(32, tuple(int(v) for v in last.groups()))]
    assert tuple(table) == dl.LF_LADDER, table
    agg = open(os.path.join(CSRC, "bgnn_aggregate.hip")).read()
    narrow = re.findall(r"if \(nv <= (\d+)\) return launch<(\d+), (\d+), (\d+)>\(p, st\);", agg)
    assert [(int(a), (int(b), int(c), int(d))) for a, b, c, d in narrow[:4]] == list(dl.ADAPTED_LADDER[:4]), narrow
    wide = re.findall(r"if \(nv <= (\d+)\) return launch_wide<(\d+), (\d+)>\(p, st\);", agg)
    assert [(int(a), (int(b), 1, int(c))) for a, b, c in wide] == list(dl.ADAPTED_LADDER[4:]), wide
    assert re.search(r"constexpr int U = 4;", agg)                                   # agg_wide_fast_kernel's depth
    gat = open(os.path.join(CSRC, "bgnn_gat.hip")).read()
    assert "gat_alpha_kernel<8, 4, EDGE_ID>" in gat and dl.GAT_ALPHA_SWEEP == 32
    assert "launch_edge<LF, EP, 4, EDGE_ID>" in gat
    gen = open(os.path.join(CSRC, "bgnn_gen.hip")).read()
    assert "constexpr int UB = U > 4 ? 4 : U;" in gen and "gen_bwd_kernel<LF, EP, UB>" in gen and dl.GEN_BWD_U_CAP == 4
    v2 = open(os.path.join(CSRC, "bgnn_gatv2.hip")).read()
    assert all(s in v2 for s in ("launch_fwd<LF, EP, 4, EPI, IDS>", "launch_dst<LF, EP, 4, true>", "launch_src<LF, EP, 4, false>"))


@pytest.mark.parametrize("variant", dl.VARIANTS)
def test_both_views_carry_the_ladder_at_every_position(variant):
    g, (rp_d, _), (rp_s, _) = _views(variant)
    assert g.n % 8 and g.N % 8 and g.N % 32 and g.N % 128, "the last tile must be ragged at every mapping"
    assert (0 in g.degrees) == (variant != "loops_rewritten")
    dl.assert_batches_bracketed(g.degrees + ([0] if variant == "loops_rewritten" else []), variant)
    for rpw in (16, 8, 4, 2):
        seen_d = dl.assert_coverage(rp_d, g.degrees, rpw, f"{variant} by destination")
        seen_s = dl.assert_coverage(rp_s, g.degrees, rpw, f"{variant} by source")
        assert set(seen_d) == set(seen_s) == set(g.degrees) | ({1} if variant == "loops_rewritten" else {0})
    # the same multiset on both sides, the other side's rows carry the bare minimum (no edge, or the self loop alone)
    own = 1 if variant == "loops_rewritten" else 0
    deg_d, deg_s = rp_d[1:] - rp_d[:-1], rp_s[1:] - rp_s[:-1]
    assert sorted(deg_d[: g.n]) == sorted(deg_s[g.n:]) and (deg_d[g.n:] == own).all() and (deg_s[: g.n] == own).all()
    assert rp_d[-1] == rp_s[-1] < 20000 and g.N < 1100
    assert g.duplicates() > 0, "duplicate edges must occur"


@pytest.mark.parametrize("variant", dl.VARIANTS)
def test_builder_is_deterministic_under_its_seed(variant):
    a, b, c = dl.Ladder(variant), dl.Ladder(variant), dl.Ladder(variant, seed=dl.SEED + 1)
    assert np.array_equal(a.ei, b.ei) and a.ei.shape == c.ei.shape and not np.array_equal(a.ei, c.ei)
    assert np.array_equal(np.sort(a.deg_dst), np.sort(c.deg_dst))
    if variant != "plain":
        assert (a.ei[0] == a.ei[1]).sum() > a.N // 7, "raw self loops, some doubled, for the graph class to rewrite"


def test_virtual_rows_of_the_attention_kernels_are_covered():
    """a lane group of the attention kernels owns the virtual row v = i * H + h: every degree at every position v % rpw, H = 1, 3"""
    g, (rp_d, _), (rp_s, _) = _views("loops_rewritten")
    for H in (1, 3):
        for rpw in (8, 4, 2):
            dl.assert_coverage(rp_d, g.degrees, rpw, f"H={H} by destination", heads=H)
            dl.assert_coverage(rp_s, g.degrees, rpw, f"H={H} by source", heads=H)
    assert dl.coverage(rp_d, 8, heads=3)[97] == set(range(8))
    # the virtual position is what is counted: rows 0 and 1 of three heads sit at positions 0, 1, 2 and 3, 4, 5
    assert dl.coverage(np.array([0, 5, 12]), 8, heads=3) == {5: {0, 1, 2}, 7: {3, 4, 5}}


def test_a_mapping_the_ladder_was_not_built_for_fails_the_coverage_assertion():
    g, (rp_d, _), _ = _views("plain")
    with pytest.raises(AssertionError, match="without every position"):
        dl.assert_coverage(rp_d, g.degrees, 32, "thirty-two rows per wave")
    with pytest.raises(AssertionError, match="not bracketed"):
        dl.assert_batches_bracketed([d for d in g.degrees if d != 48])


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("variant", dl.VARIANTS)
def test_linear_restatements_against_dense_products(variant):
    g, (rp, col), (t_rp, t_col) = _views(variant)
    N, D = g.N, 5
    A = dl.dense_counts(rp, col, N)
    assert torch.equal(dl.dense_counts(t_rp, t_col, N), A.t()), "the by-source view is the transpose"
    X, R = _rand((N, D), 1), _rand((N, D), 2)
    s, w = _rand((N,), 3).abs() + 0.1, _rand((N,), 4)
    Xd, Rd, sd, wd = X.double(), R.double(), s.double(), w.double()
    S, Ab = dl.walk(rp, col, X)
    _close(S, A @ Xd, "walk")
    _close(Ab, A @ Xd.abs(), "walk: absolute sums")
    deg = A.sum(1)
    inv = torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros_like(deg))
    _close(dl.sage_ref(rp, col, X, R)[0], inv[:, None] * (A @ Xd) + Rd, "sage mean + root")
    _close(dl.sage_ref(rp, col, X, None, mean=False)[0], A @ Xd, "sage plain sum")
    # sage backward: grad_tbl[j] = sum_i gy[i] / deg_i over the by-source view
    Sg = R * inv.float()[:, None]                                     # the backward's scratch g / deg, one fp32 tensor for both
    _close(dl.walk(t_rp, t_col, Sg)[0], A.t() @ Sg.double(), "sage backward")
    _close(dl.scaled_ref(rp, col, X, s, s)[0], sd[:, None] * (A @ (sd[:, None] * Xd)), "gcn")
    _close(dl.scaled_ref(t_rp, t_col, X, s, s)[0], sd[:, None] * (A.t() @ (sd[:, None] * Xd)), "gcn backward")
    _close(dl.scaled_ref(rp, col, X, s, s, own=X, w_own=w)[0], wd[:, None] * Xd + sd[:, None] * (A @ (sd[:, None] * Xd)), "jk")
    one = torch.ones(N)
    _close(dl.scaled_ref(rp, col, X, one, one, own=X, w_own=1.3, bias=R[0])[0], 1.3 * Xd + A @ Xd + Rd[0], "gin")
    Ah = sd[:, None] * A * sd[None, :]
    z = Xd
    for _ in range(3):
        z = 0.9 * (Ah @ z) + 0.1 * Xd
    _close(dl.appnp_ref(rp, col, X, s, 3, 0.1)[0], z, "appnp K = 3")
    _close(dl.appnp_ref(rp, col, X, s, 0, 0.1)[0], Xd, "appnp K = 0")
    M = _rand((D, D), 5)
    out, m, oa, ma = dl.gcn2_ref(rp, col, X, R, M, s, 0.2)
    m_d = 0.8 * (Ah @ Xd) + 0.2 * Rd
    _close(m, m_d, "gcn2 mix")
    _close(out, torch.relu(m_d @ M.double()), "gcn2")
    assert bool((ma >= m.abs() - 1e-12).all()) and bool((oa >= out.abs() - 1e-12).all()), "a scale bounds its value"


@pytest.mark.parametrize("variant", ["plain", "loops_rewritten"])
@pytest.mark.parametrize("t", [1.0, -0.7, 40.0])
def test_softmax_aggregation_restatement_against_a_dense_softmax(variant, t):
    g, (rp, col), _ = _views(variant)
    N, H = g.N, 3
    A = dl.dense_counts(rp, col, N)
    x, gz = _rand((N, H), 11), _rand((N, H), 12)
    xd = x.double().requires_grad_(True)
    td = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    v = torch.relu(xd) + 1e-7
    logit = td * v[None, :, :] + torch.log(A)[:, :, None]                    # [i, j, h]; log 0 = -inf removes a non-edge
    has = (A.sum(1) > 0)[:, None]
    lse_d = torch.where(has, torch.logsumexp(logit.detach()[:, :, :], dim=1), torch.zeros(N, H, dtype=torch.float64))
    al = torch.softmax(torch.where(has[:, :, None].expand_as(logit), logit, torch.zeros_like(logit)), dim=1) * has[:, :, None]
    o_d = (al * v[None, :, :]).sum(1)
    z_d = o_d + xd
    z, lse, o, za = dl.gen_ref(rp, col, x, t)
    _close(z, z_d.detach(), "z")
    _close(o, o_d.detach(), "o")
    _close(lse, lse_d, "lse", scale=max(1.0, lse_d.abs().max().item()))
    assert bool((za >= z.abs() - 1e-12).all())
    (z_d * gz.double()).sum().backward()
    gx, gt, gxa, gta = dl.gen_bwd_ref(rp, col, x, gz, t)
    assert gta.item() >= abs(gt.item())
    lsc = dl.gen_lse_scale(rp, col, x, t)
    assert bool((lsc >= lse.abs() - 1e-12).all()) and bool((lsc[A.sum(1) == 0] == 0).all()), "a row's own scale bounds its lse"
    _close(gx, xd.grad, "grad_x", scale=gxa.max().item())
    assert abs(gt.item() - td.grad.item()) <= 1e-9 * max(1.0, abs(td.grad.item())), (gt.item(), td.grad.item())
    assert bool((gxa >= gx.abs() - 1e-12).all())


@pytest.mark.parametrize("H,C", [(1, 3), (2, 3)])
def test_attention_restatements_against_dense_softmaxes(H, C):
    g, (rp, col), _ = _views("loops_rewritten")
    N, slope = g.N, 0.2
    A = dl.dense_counts(rp, col, N)
    logA = torch.log(A)[:, :, None]
    T, XR, gy = _rand((N, H * C), 21), _rand((N, H * C), 22), _rand((N, H * C), 23)
    a_s, a_d = _rand((H, C), 24) * 0.5, _rand((H, C), 25) * 0.5
    lk = torch.nn.functional.leaky_relu
    # GAT
    Td = T.double().requires_grad_(True)
    Tv = Td.reshape(N, H, C)
    ss, sd = (Tv * a_s.double()).sum(-1), (Tv * a_d.double()).sum(-1)
    al = torch.softmax(lk(ss[None, :, :] + sd[:, None, :], slope) + logA, dim=1)          # [i, j, h]
    out_d = torch.einsum("ijh,jhc->ihc", al, Tv.detach()).reshape(N, H * C)            # the gather part: T detached, as the op's
    r = dl.gat_ref(rp, col, T, a_s, a_d, H, C, slope, gy=gy)
    _close(r["out"], out_d.detach(), "gat out")
    _close(r["s_src"], ss.detach(), "s_src")
    gs, gd = torch.autograd.grad((out_d * gy.double()).sum(), (ss, sd), retain_graph=True)
    _close(r["ds_src"], gs, "gat ds_src", scale=r["ds_src_abs"].max().item())
    _close(r["ds_dst"], gd, "gat ds_dst", scale=r["ds_dst_abs"].max().item())
    _close(r["grad_tbl"], torch.einsum("ijh,ihc->jhc", al.detach(), gy.double().reshape(N, H, C)).reshape(N, H * C), "gat grad_tbl")
    for k in ("out", "grad_tbl", "ds_src", "ds_dst"):
        assert bool((r[k + "_abs"] >= r[k].abs() - 1e-12).all()), k
    # GATv2
    xl, xr = T.double().requires_grad_(True), XR.double().requires_grad_(True)
    att = a_s.double().clone().requires_grad_(True)
    u = xl.reshape(N, H, C)[None, :, :, :] + xr.reshape(N, H, C)[:, None, :, :]          # [i, j, h, c]
    e = (lk(u, slope) * att).sum(-1)
    al2 = torch.softmax(e + logA, dim=1)
    out2 = torch.einsum("ijh,jhc->ihc", al2, xl.reshape(N, H, C)).reshape(N, H * C)
    r2 = dl.gatv2_ref(rp, col, T, XR, a_s, H, C, slope, gy=gy)
    _close(r2["out"], out2.detach(), "gatv2 out")
    (out2 * gy.double()).sum().backward()
    _close(r2["dxl"], xl.grad, "gatv2 dxl", scale=r2["dxl_abs"].max().item())
    _close(r2["dxr"], xr.grad, "gatv2 dxr", scale=r2["dxr_abs"].max().item())
    _close(r2["datt"], att.grad.reshape(-1), "gatv2 datt", scale=r2["datt_abs"].max().item())
    for k in ("out", "dxl", "dxr"):
        assert bool((r2[k + "_abs"] >= r2[k].abs() - 1e-12).all()), k


def test_adaptedconv_restatement_against_a_dense_softmax():
    g, (rp, col), _ = _views("loops_rewritten")
    N, D, slope = g.N, 5, 0.1
    A = dl.dense_counts(rp, col, N)
    hS, hT, gout = _rand((N, D), 31), _rand((N, D), 32), _rand((N, D), 33)
    a1, a2 = _rand((D,), 34) * 0.3, _rand((D,), 35) * 0.3
    mask = np.random.default_rng(36).random(N) < 0.5
    m = torch.from_numpy(mask)
    tS, tT = hS.double().requires_grad_(True), hT.double().requires_grad_(True)
    b1, b2 = a1.double().requires_grad_(True), a2.double().requires_grad_(True)
    lk = torch.nn.functional.leaky_relu
    outs = []
    for t, b in ((tS, b1), (tT, b2)):
        e = (lk(t[None, :, :] + t[:, None, :], slope) * b).sum(-1)                     # [i, j]
        outs.append(torch.softmax(e + torch.log(A), dim=1) @ t)
    out_d = torch.where(m[:, None], outs[0], outs[1])
    r = dl.adapted_ref(rp, col, hS, hT, a1, a2, mask, D, slope, gout=gout)
    _close(r["out"], out_d.detach(), "adaptedconv out")
    (out_d * gout.double()).sum().backward()
    for got, want, what in zip(r["grads"], (tS.grad, tT.grad, b1.grad, b2.grad), ("dh_t2s", "dh_s2t", "da_t2s", "da_s2t")):
        _close(got, want, what, scale=max(want.abs().max().item(), 1.0))
    assert bool((r["out_abs"] >= r["out"].abs() - 1e-12).all())
    assert bool((r["grads_abs"] >= torch.maximum(r["grads"][0].abs(), r["grads"][1].abs()) - 1e-9).all())
    # both domains inside the rows: the mask the GPU test uses mixes them in every row of two or more edges
    dst, src = dl._edges(rp, col)
    assert len(set(m[src][dst == int(np.argmax(rp[1:] - rp[:-1]))].tolist())) == 2


def test_judge_takes_each_row_on_its_own_scale():
    ref = torch.tensor([[1000.0, 0.0], [1.0, 0.5], [0.0, 0.0]], dtype=torch.float64)
    sc = ref.abs()
    ok = ref.clone()
    ok[0, 0] += 5e-3
    share, deg = dl.judge(ok, ref, sc, 1e-5, [97, 3, 0], "within")
    assert deg == 97 and abs(share - 0.5) < 1e-6
    bad = ref.clone()
    bad[1, 1] += 5e-3                       # far inside 1e-5 of the tensor's maximum, far outside the row's own
    with pytest.raises(AssertionError, match=r"worst row 1 \(degree 3\)"):
        dl.judge(bad, ref, sc, 1e-5, [97, 3, 0], "short row")
    bad = ref.clone()
    bad[2, 0] = 1e-30                       # a row of scale 0 must be exact
    with pytest.raises(AssertionError, match="degree 0"):
        dl.judge(bad, ref, sc, 1e-5, [97, 3, 0], "empty row")
