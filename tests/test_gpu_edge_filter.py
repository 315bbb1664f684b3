"""GPU: csrc/bgnn_edge_filter.hip -- `ops.quantile_f32` against torch.quantile / torch.sort, and the fused edge-validity pass
(`fused=True`) against the torch filters of bridge.py (`fused=False`, the yardstick) on the office artefacts, on randomised
class-structured graphs and on a bridge of more than 2^24 edges.

Rule 5 (raw-feature cosine < threshold) is the one predicate that is not integer logic: both paths form the cosine in fp32 in
different summation orders, so an edge whose cosine lies within BAND(F) = 2 F 2^-24 + 8 2^-24 of the threshold (the fp32
dot-product bound for either order plus the two normalisations) may be decided differently.  Every test states how many such edges
its inputs have (measured on the torch path's own cosines) and caps their share at 0.1 %."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 1e-3


def band(feat):
    return (2 * feat + 8) * 2.0 ** -24


def bits(t):
    return t.detach().cpu().reshape(1).view(torch.int32).item()


# ---- quantile --------------------------------------------------------------------------------------------------------------------
def _values(n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "dups":                  # half-integer grid: heavy duplicates, negatives, zeros of both signs
        v = torch.round(torch.randn(n, generator=g) * 6) / 2
        z = v == 0
        v[z & (torch.rand(n, generator=g) < 0.5)] = -0.0
        return v
    return torch.sigmoid(torch.randn(n, generator=g) * 2)          # what the scorers emit


@pytest.mark.parametrize("n", [1, 2, 11820, 1_000_003])
def test_quantile_is_bit_identical_to_torch(n):
    from bridged_gnn_amd import ops
    for kind in ("dups", "probs"):
        v = _values(n, kind, seed=n).to(DEV)
        for q in (0.0, 0.1, 0.5, 0.9, 1.0):
            got, want = ops.quantile_f32(v, q), torch.quantile(v, q)
            assert got.shape == () and got.dtype == torch.float32
            print(f"quantile n={n} {kind} q={q}: got {got.item()!r} ({bits(got):#010x}) torch {want.item()!r} ({bits(want):#010x})")
            assert bits(got) == bits(want), (n, kind, q, got.item(), want.item())


def test_quantile_beyond_torchs_size_limit():
    from bridged_gnn_amd import ops
    n = (1 << 24) + 5
    v = torch.sigmoid(torch.randn(n, generator=torch.Generator().manual_seed(5)) * 2).to(DEV)
    with pytest.raises(RuntimeError, match="too large"):
        torch.quantile(v, 0.1)
    srt = torch.sort(v).values
    for q in (0.0, 0.1, 0.37, 0.5, 0.9, 1.0):
        p = q * (n - 1)
        lo, hi = int(np.floor(p)), int(np.ceil(p))
        t1, t2 = ops.quantile_f32(v, q), ops.quantile_f32(v, q)
        print(f"quantile n={n} q={q}: {srt[lo].item()!r} <= {t1.item()!r} <= {srt[hi].item()!r}")
        assert srt[lo].item() <= t1.item() <= srt[hi].item(), q
        assert bits(t1) == bits(t2), "two calls must agree bit for bit"


# ---- the torch rules, bit by bit (the predicates of bridge.check_added_edges_*_validity, fused=False) ----------------------------------
def torch_rule_bits(ei, e_sim, d_from, d_to, p_from, p_to, within, q, thres, thres_conf=None):
    e0, e1 = ei[0], ei[1]
    pf, pt = p_from.argmax(1), p_to.argmax(1)
    tm = d_to.train_mask[e1]
    t = e_sim.quantile(q) if thres_conf is None else thres_conf
    r1 = e_sim < t
    r2 = (pf[e0] != d_from.y[e0]) & tm if within else pf[e0] != d_from.y[e0]
    r3 = (pt[e1] != d_to.y[e1]) & tm
    r4 = pf[e0] != pt[e1]
    cos = F.cosine_similarity(d_from.x[e0], d_to.x[e1])
    return torch.stack([r1, r2, r3, r4, cos < thres]), cos


def cumulative(rules):
    return torch.cumsum(rules.long(), 0).clamp_(max=1).sum(1).tolist()


def flag_bits(flags):
    return torch.stack([(flags >> r) & 1 for r in range(5)]).bool()


def check_against_torch(flags, counts, rules, cos, thres, feat, what):
    """rules 1-4 bit for bit; rule 5 and the kept mask outside the band; the in-band share under the cap"""
    fb = flag_bits(flags)
    inband = (cos - thres).abs() <= band(feat)
    share = inband.float().mean().item()
    print(f"{what}: E={flags.numel()} in-band share {share:.2e} (cap {CAP:.0e}), rule-5 disagreements {(fb[4] != rules[4]).sum().item()}, "
          f"counts {counts}")
    assert share <= CAP, what
    for r in range(4):
        assert torch.equal(fb[r], rules[r]), f"{what}: rule {r + 1}"
    assert torch.equal(fb[4][~inband], rules[4][~inband]), f"{what}: rule 5 outside the band"
    assert torch.equal((flags == 0)[~inband], (~rules.any(0))[~inband]), f"{what}: kept mask outside the band"
    assert counts[:4] == cumulative(rules)[:4], what
    if not bool((fb[4] != rules[4]).any()):
        assert counts == cumulative(rules), what


# ---- office artefacts -----------------------------------------------------------------------------------------------------------
def test_office_fixtures_exact():
    """Exact equality: on these fixtures no edge's fp64 cosine is within BAND(256) = 3.1e-5 of 0.8 (the closest is 4.7e-5 away)."""
    from bridged_gnn_amd import bridge
    from bridged_gnn_amd.data import Data
    f, g, k = load_golden("filters_office_a2d.npz"), load_golden("office_a2d_graph.npz"), load_golden("knn_office_a2d.npz")
    ns = 2817
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    y = t(g["y"])
    ds = Data(x=t(g["x"][:ns]), y=y[:ns], train_mask=t(f["train_mask_src"]))
    dt = Data(x=t(g["x"][ns:]), y=y[ns:], train_mask=t(f["train_mask_tar"]))
    pcs, pct = t(f["probs_clf_src"]), t(f["probs_clf_tar"])
    ec, ew = t(f["cross_in"].astype(np.int64)), t(f["within_in"].astype(np.int64))
    # the reference's misaligned vectors -> the reference's own outputs
    out, c = bridge.check_added_edges_cross_domain_validity(ec, t(f["cross_e_sim_flat"]), ds, dt, pcs, pct, 0.1, 0.8, fused=True,
                                                            return_counts=True)
    assert np.array_equal(out.cpu().numpy(), f["cross_out"])
    _, c_ref = bridge.check_added_edges_cross_domain_validity(ec, t(f["cross_e_sim_flat"]), ds, dt, pcs, pct, 0.1, 0.8, return_counts=True)
    assert c == c_ref and c[4] == ec.shape[1] - out.shape[1]
    out_w, cw = bridge.check_added_edges_within_domain_validity(ew, t(f["within_e_sim_flat"]), ds, pcs, 0.1, 0.8, fused=True,
                                                                return_counts=True)
    assert np.array_equal(out_w.cpu().numpy(), f["within_out"])
    _, cw_ref = bridge.check_added_edges_within_domain_validity(ew, t(f["within_e_sim_flat"]), ds, pcs, 0.1, 0.8, return_counts=True)
    assert cw == cw_ref
    # aligned mode: the [Nq, k] tables instead of align_e_sim_to_edges
    sim_mat, idx_mat = t(k["cross_e_sim"]), t(k["cross_idx"].astype(np.int64))
    e_al = bridge.align_e_sim_to_edges(ec, sim_mat, idx_mat)
    want, c_want = bridge.check_added_edges_cross_domain_validity(ec, e_al, ds, dt, pcs, pct, 0.1, 0.8, return_counts=True)
    got, c_got = bridge.check_added_edges_cross_domain_validity(ec, (sim_mat, idx_mat), ds, dt, pcs, pct, 0.1, 0.8, fused=True,
                                                                return_counts=True)
    assert torch.equal(got, want) and c_got == c_want
    flags, _, sim = bridge.fused_edge_flags(ec, (sim_mat, idx_mat), ds, dt, pcs, pct, False, 0.1, 0.8)
    assert torch.equal(sim, e_al)
    rules, _ = torch_rule_bits(ec, e_al, ds, dt, pcs, pct, False, 0.1, 0.8)
    assert torch.equal(flag_bits(flags), rules) and c_got == cumulative(rules)
    # an edge that is not in the tables is reported
    bad = ec.clone()
    bad[0, 5] = (set(range(ns)) - set(k["cross_idx"][int(ec[1, 5])].tolist())).pop()
    with pytest.raises(RuntimeError, match="top-k tables"):
        bridge.check_added_edges_cross_domain_validity(bad, (sim_mat, idx_mat), ds, dt, pcs, pct, 0.1, 0.8, fused=True)
    bad[0, 5] = ns + 3
    with pytest.raises(RuntimeError, match="outside the tables"):
        bridge.check_added_edges_cross_domain_validity(bad, t(f["cross_e_sim_flat"]), ds, dt, pcs, pct, 0.1, 0.8, fused=True)


# ---- randomised parity -----------------------------------------------------------------------------------------------------------
def class_domain(n, feat, n_cls, seed, centres):
    """class-structured Gaussians (as synth.sync_rd_intra makes them) with a per-node noise level, so that cosines spread over
    (0, 1) instead of piling up at one value; class = node id % n_cls; some labels are -1, a few rows all-zero"""
    from bridged_gnn_amd.data import Data
    g = torch.Generator().manual_seed(seed)
    cls = torch.arange(n) % n_cls
    sigma = 0.1 + 1.4 * torch.rand(n, 1, generator=g)
    x = centres[cls] + sigma * torch.randn(n, feat, generator=g)
    x[torch.tensor([3, 77, 4000])] = 0.0
    y = cls.clone()
    y[torch.rand(n, generator=g) < 0.2] = -1
    probs = torch.softmax(torch.randn(n, n_cls, generator=g) + 2.5 * F.one_hot(cls, n_cls), dim=1)      # argmax = class for most nodes
    d = Data(x=x, y=y, train_mask=torch.rand(n, generator=g) < 0.5)
    return d.to(DEV), probs.to(DEV)


def topk_tables(n_from, n_to, k, n_cls, seed):
    """[n_to, k] candidate ids: half of each row from the query's own class, half anywhere; a similarity per entry"""
    g = torch.Generator().manual_seed(seed)
    q_cls = (torch.arange(n_to) % n_cls).unsqueeze(1)
    same = torch.randint(0, n_from // n_cls, (n_to, k // 2), generator=g) * n_cls + q_cls
    idx = torch.cat([same, torch.randint(0, n_from, (n_to, k - k // 2), generator=g)], dim=1)
    return idx.to(DEV), torch.sigmoid(torch.randn(n_to, k, generator=g) * 2).to(DEV)


@pytest.mark.parametrize("feat", [33, 256, 300])
@pytest.mark.parametrize("within", [False, True])
def test_randomised_parity_with_the_torch_path(feat, within):
    from bridged_gnn_amd import bridge, ops
    n, k, n_cls = 50_000, 20, 10
    centres = torch.randn(n_cls, feat, generator=torch.Generator().manual_seed(100 + feat))
    d_to, p_to = class_domain(n, feat, n_cls, 1 + feat, centres)
    d_from, p_from = (d_to, p_to) if within else class_domain(n + 123, feat, n_cls, 2 + feat, centres)
    idx_mat, sim_mat = topk_tables(d_from.x.shape[0], n, k, n_cls, 3 + feat)
    ei = ops.coalesce(ops.topk_edges(idx_mat))                     # sorted by `from`; duplicate candidates of a row collapse
    E = ei.shape[1]
    # bgnn_edge_filter.hip grid_for: at most MAX_BLOCKS = 4096 blocks; edge_validity_kernel walks 256 // 16 edges per block and trip,
    # edge_rule1_counts_kernel 256 (its grid is sized for 8 trips), select_pass_kernel is sized the same way
    assert E > 4096 * (256 // 16)
    e_al = bridge.align_e_sim_to_edges(ei, sim_mat, idx_mat)
    e_quirk = torch.sigmoid(torch.randn(E, generator=torch.Generator().manual_seed(9)) * 2).to(DEV)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(11)).to(DEV)
    for thres in (0.0, 0.8):
        for mode, e_sim_torch, e_sim_fused in (("aligned", e_al, (sim_mat, idx_mat)), ("quirk", e_quirk, e_quirk)):
            what = f"F={feat} within={within} thres={thres} {mode}"
            rules, cos = torch_rule_bits(ei, e_sim_torch, d_from, d_to, p_from, p_to, within, 0.1, thres)
            flags, counts, sim = bridge.fused_edge_flags(ei, e_sim_fused, d_from, d_to, p_from, p_to, within, 0.1, thres)
            assert torch.equal(sim, e_sim_torch), what
            check_against_torch(flags, counts, rules, cos, thres, feat, what)
            # the public filters agree with each other outside the band
            fn = bridge.check_added_edges_within_domain_validity if within else bridge.check_added_edges_cross_domain_validity
            a = (ei, e_sim_torch, d_to, p_to) if within else (ei, e_sim_torch, d_from, d_to, p_from, p_to)
            b = (ei, e_sim_fused) + a[2:]
            want, got = fn(*a, 0.1, thres), fn(*b, 0.1, thres, fused=True)
            assert torch.equal(want, ei[:, ~rules.any(0)]) and torch.equal(got, ei[:, flags == 0]), what
        # the same edges in scrambled order: no sortedness is assumed (the per-edge vector moves with its edges)
        what = f"F={feat} within={within} thres={thres} scrambled"
        rules_p, cos_p = torch_rule_bits(ei[:, perm], e_al[perm], d_from, d_to, p_from, p_to, within, 0.1, thres)
        flags_p, counts_p, _ = bridge.fused_edge_flags(ei[:, perm].contiguous(), (sim_mat, idx_mat), d_from, d_to, p_from, p_to, within, 0.1, thres)
        check_against_torch(flags_p, counts_p, rules_p, cos_p, thres, feat, what)
        flags_q, _, _ = bridge.fused_edge_flags(ei[:, perm].contiguous(), e_al[perm], d_from, d_to, p_from, p_to, within, 0.1, thres)
        assert torch.equal(flags_q, flags_p), what


# ---- scale and memory ----------------------------------------------------------------------------------------------------------------
def test_scale_beyond_2_pow_24_edges_and_memory():
    """200k sources x 1M targets, k = 20, F = 64: E >= 2^24, where `e_sim.quantile` raises and the torch path would gather
    2 * 4 * 64 = 512 bytes per edge.  Peak growth of the fused call: flag byte 1 + similarity 4 + select scratch (constant) + kept
    mask 1 + kept index list 8 + kept [2, E'] list 16 = 30 bytes per edge; the bar is 40."""
    from bridged_gnn_amd import bridge, ops
    from bridged_gnn_amd.data import Data
    ns, nt, k, feat, n_cls = 200_000, 1_000_000, 20, 64, 10
    centres = torch.randn(n_cls, feat, generator=torch.Generator().manual_seed(64))

    def domain(n, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        cls = torch.arange(n, device=DEV) % n_cls
        x = centres.to(DEV)[cls] + (0.1 + 1.4 * torch.rand(n, 1, device=DEV, generator=g)) * torch.randn(n, feat, device=DEV, generator=g)
        y = cls.clone()
        y[torch.rand(n, device=DEV, generator=g) < 0.2] = -1
        probs = torch.softmax(torch.randn(n, n_cls, device=DEV, generator=g) + 2.5 * F.one_hot(cls, n_cls), dim=1)
        return Data(x=x, y=y, train_mask=torch.rand(n, device=DEV, generator=g) < 0.5), probs
    ds, ps = domain(ns, 1)
    dt, pt = domain(nt, 2)
    g = torch.Generator(device=DEV).manual_seed(3)
    q_cls = (torch.arange(nt, device=DEV) % n_cls).unsqueeze(1)
    idx_mat = torch.cat([torch.randint(0, ns // n_cls, (nt, k // 2), device=DEV, generator=g) * n_cls + q_cls,
                         torch.randint(0, ns, (nt, k - k // 2), device=DEV, generator=g)], dim=1)
    # distinct similarities: consecutive fp32 bit patterns from 0.5 upwards, shuffled over the table
    sim_mat = (torch.randperm(nt * k, device=DEV, generator=g).to(torch.int32) + 0x3F000000).view(torch.float32).reshape(nt, k)
    ei = ops.coalesce(ops.topk_edges(idx_mat))
    E = ei.shape[1]
    assert E >= 1 << 24
    # bgnn_edge_filter.hip grid_for past MAX_BLOCKS = 4096 in every launch: 2048 values per block (select_pass, rule1_counts),
    # 16 rows per block (row_inv_norms, both domains), 16 edges per block (edge_validity)
    assert E > 4096 * 256 * 8 and min(ns, nt) > 4096 * (256 // 16)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, counts = bridge.check_added_edges_cross_domain_validity(ei, (sim_mat, idx_mat), ds, dt, ps, pt, 0.1, 0.0, fused=True,
                                                                 return_counts=True)
    torch.cuda.synchronize()
    growth = (torch.cuda.max_memory_allocated() - base) / E
    print(f"scale: E={E} kept={out.shape[1]} counts={counts} peak growth {growth:.1f} bytes/edge")
    assert growth <= 40.0
    assert out.shape[1] == E - counts[4]
    p = 0.1 * (E - 1)
    assert counts[0] in (int(np.floor(p)), int(np.floor(p)) + 1)
    # a random sample of 1M edges against the torch rules, gathered in chunks
    flags, counts2, sim = bridge.fused_edge_flags(ei, (sim_mat, idx_mat), ds, dt, ps, pt, False, 0.1, 0.0)
    assert counts2 == counts and torch.equal(out, ei[:, flags == 0])
    srt = torch.sort(sim).values
    s_lo, s_hi = srt[int(np.floor(p))], srt[int(np.ceil(p))]
    del srt
    sample = torch.randint(0, E, (1_000_000,), device=DEV, generator=g)
    n_band = n_diff = 0
    for chunk in sample.split(250_000):
        es = ei[:, chunk]
        sim_c = bridge.align_e_sim_to_edges(es, sim_mat, idx_mat)
        assert torch.equal(sim_c, sim[chunk])
        rules, cos = torch_rule_bits(es, sim_c, ds, dt, ps, pt, False, 0.1, 0.0, thres_conf=s_hi)
        fb = flag_bits(flags[chunk])
        sure = (sim_c < s_lo) | (sim_c >= s_hi)                    # the threshold lies in [sorted[lo], sorted[hi]]
        assert torch.equal(fb[0][sure], rules[0][sure])
        for r in (1, 2, 3):
            assert torch.equal(fb[r], rules[r]), f"rule {r + 1}"
        inband = cos.abs() <= band(feat)
        n_band += int(inband.sum())
        n_diff += int((fb[4] != rules[4]).sum())
        assert torch.equal(fb[4][~inband], rules[4][~inband])
    print(f"scale: sample in-band {n_band} of 1000000, rule-5 disagreements {n_diff}")
    assert n_band <= CAP * 1_000_000
