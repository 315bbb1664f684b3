"""GPU: half A parity -- scorers + top-k through the C ABI.  Index results must be BIT-EXACT vs the
oracle's declared rule (canonical fp64 score desc, index asc); probabilities within 1e-5."""
import numpy as np
import pytest
import torch

from conftest import assert_close, sub
from oracle import oracle_c as OC
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
TIE_ROWS = {591: 11, 888: 15}   # rows (of Nt) whose top-k SET differs from the reference's torch.topk on the office fixtures: k-boundary ties under
                                # the declared rule (canonical fp64 score desc, index asc); measured, pinned so that the count cannot drift
# edges of the office top-k lists that this package and the reference do not share (each way), measured on the GPU run and pinned:
# all of them lie in the tie rows above (tests assert that), cf. DESIGN.md section 2
CROSS_EDGE_DIFF = {591: 12, 888: 15}
WITHIN_EDGE_DIFF = {("a2d", "src"): (56, 56), ("a2d", "tar"): (48, 48), ("a2w", "src"): (53, 48), ("a2w", "tar"): (31, 31)}   # (edges, tie rows), k = 3
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_l2_normalize_bit_exact():
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(0)
    q = rng.standard_normal((3000, 128)).astype(np.float32)
    q[5] = 0.0                                      # eps clamp
    q[6] *= 1e-20
    got = ops.l2_normalize_rows(_t(q)).cpu().numpy()
    assert np.array_equal(got, OC.l2_normalize_rows(q))


@pytest.mark.parametrize("nq,nc,d,k", [(2000, 20000, 128, 20), (300, 5000, 64, 3), (129, 40000, 128, 20),
                                        (64, 10, 32, 3), (500, 3000, 128, 50), (77, 9000, 100, 24), (40, 6000, 256, 8)])
def test_cosine_topk_bit_exact(nq, nc, d, k):
    from bridged_gnn_amd import ops, synth
    q = OC.l2_normalize_rows(synth.gaussian_embeddings(nq, d, seed=nq))
    c = OC.l2_normalize_rows(synth.gaussian_embeddings(nc, d, seed=nc + 1))
    idx, val, nfb = ops.cosine_topk(_t(q), _t(c), k, apply_sigmoid=False)
    rv, ri = OC.cosine_topk(q, c, k)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert_close(val.cpu().numpy(), rv, rtol=1e-6, atol_scale=1e-7, what="scores")
    assert int(nfb[0].item()) <= max(2, nq // 100)


@pytest.mark.parametrize("seed", range(24))
def test_cosine_topk_fuzz_bit_exact(seed):
    """seeded random (Nq, Nc, d, k), clustered embeddings with near-duplicates: indices bit-exact vs the C oracle through
    the bf16-piece pass 1 + canonical re-score (+ exhaustive fallback when the proof margin is too small)."""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(500 + seed)
    d = int(rng.choice([32, 64, 128, 128, 256]))
    k = int(rng.choice([1, 3, 8, 20, 24])) if d == 256 else int(rng.choice([1, 3, 8, 20, 24, 30, 50]))
    nq, nc = int(rng.integers(1, 700)), int(rng.integers(max(k, 33), 12000))
    centers = rng.standard_normal((8, d))
    def emb(n):
        z = centers[rng.integers(0, 8, n)] + rng.standard_normal((n, d)) * rng.choice([0.05, 0.3, 1.0])
        return z.astype(np.float32)
    qe, ce = emb(nq), emb(nc)
    ce[rng.integers(0, nc, 5)] = ce[rng.integers(0, nc, 5)]              # exact duplicates
    ce[rng.integers(0, nc, 5)] *= np.float32(1.0 + 1e-6)                  # near duplicates (same direction up to rounding)
    q, c = OC.l2_normalize_rows(qe), OC.l2_normalize_rows(ce)
    idx, val, nfb = ops.cosine_topk(_t(q), _t(c), k, apply_sigmoid=False)
    rv, ri = OC.cosine_topk(q, c, k)
    assert np.array_equal(idx.cpu().numpy(), ri), f"seed={seed} d={d} k={k} nq={nq} nc={nc} fallback={int(nfb[0].item())}"
    assert_close(val.cpu().numpy(), rv, rtol=1e-6, atol_scale=1e-7, what="scores")


def test_cosine_topk_exact_ties_and_duplicates():
    """duplicated candidates give exactly equal scores: the lower index must win, everywhere."""
    from bridged_gnn_amd import ops, synth
    q = OC.l2_normalize_rows(synth.gaussian_embeddings(200, 128, seed=5))
    base = OC.l2_normalize_rows(synth.gaussian_embeddings(700, 128, seed=6))
    c = np.concatenate([base, base[:300], base[100:200], base])       # up to 4 copies
    idx, val, nfb = ops.cosine_topk(_t(q), _t(c), 20, apply_sigmoid=True)
    rv, ri = OC.cosine_topk(q, c, 20)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert_close(val.cpu().numpy(), O.sigmoid_f32(rv), rtol=1e-5, atol_scale=1e-6, what="probs")
    # all-identical candidates: every score ties -> indices 0..k-1; the margin proof must fail -> fallback
    c2 = np.repeat(base[:1], 500, axis=0)
    idx2, _, nfb2 = ops.cosine_topk(_t(q), _t(c2), 20)
    assert np.array_equal(idx2.cpu().numpy(), np.tile(np.arange(20), (200, 1)))
    assert int(nfb2[0].item()) == 200


def test_cosine_topk_gauss_golden_vs_reference(golden):
    """reference-produced index sets (Similar_noTrans + torch.topk) on tie-free Gaussian data."""
    from bridged_gnn_amd import ops, synth
    f = golden("knn_gauss.npz")
    ns, nt, d, k = int(f["ns"]), int(f["nt"]), int(f["d"]), int(f["k"])
    qs = ops.l2_normalize_rows(_t(synth.gaussian_embeddings(ns, d, seed=int(f["seed_src"]))))
    qt = ops.l2_normalize_rows(_t(synth.gaussian_embeddings(nt, d, seed=int(f["seed_tar"]))))
    idx, val, _ = ops.cosine_topk(qt, qs, k)
    mine = np.sort(idx.cpu().numpy(), axis=1)
    ref = np.sort(f["idx"].astype(np.int64), axis=1)
    assert (mine != ref).any(axis=1).sum() == 0          # (tie-free data: every row's index SET equals the reference's)
    assert_close(val.cpu().numpy(), -np.sort(-f["e_sim"], axis=1), rtol=1e-5, atol_scale=1e-6, what="e_sim")


@pytest.mark.parametrize("tag,kc", [("a2d", 20), ("a2w", 8)])
def test_office_bridge_from_shipped_ckpt(golden, tag, kc):
    """BASELINE config 1 through the reference-named entry points, from the shipped checkpoint."""
    from bridged_gnn_amd.bridge import BridgeScorer, add_topk_sim_cross_domain_edges, add_topk_sim_within_domain_edges
    from bridged_gnn_amd.data import Data
    f = golden(f"knn_office_{tag}.npz")
    sd = {"source_learner.sim_net." + k: torch.from_numpy(np.asarray(v)) for k, v in sub(f, "sim.").items()}
    model = BridgeScorer(sd, DEV)
    assert model.sim_mode == "mlp"
    ns = int(f["n_src"])
    y = torch.from_numpy(f["y"].astype(np.int64))
    ds, dt = Data(x=_t(f["z_src"]), y=y[:ns]), Data(x=_t(f["z_tar"]), y=y[ns:])
    ei, esim, idx, pcs, pct = add_topk_sim_cross_domain_edges(ds, dt, model, k=kc, z_src=_t(f["z_src"]), z_tar=_t(f["z_tar"]),
                                                              verbose=False)
    A, B, scale, shift, w2, b2 = O.mlp_pair_terms(f["z_src"], f["z_tar"], sub(f, "sim."))
    # (1) per-node terms within 1e-5, then indices bit-exact vs the oracle ON THE SAME A/B
    gA, gB, gs, gh, gw, gb = model.mlp_terms(_t(f["z_src"]), _t(f["z_tar"]))
    assert_close(gA.cpu().numpy(), A, what="A") ; assert_close(gB.cpu().numpy(), B, what="B")
    rv, ri = OC.mlp_topk(gA.cpu().numpy(), gB.cpu().numpy(), gs.cpu().numpy(), gh.cpu().numpy(), gw.cpu().numpy(), gb, kc)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert np.array_equal(ei.cpu().numpy(), O.topk_edges(ri))
    # (2) vs the reference's own output: probabilities, and index sets up to boundary ties
    assert_close(esim.cpu().numpy(), f["cross_e_sim"], rtol=1e-5, atol_scale=1e-6, what="e_sim")
    s = O.mlp_scores_canonical(A, B, scale, shift, w2, b2)
    srt = np.sort(s, axis=1)
    same = np.array([set(a) == set(b) for a, b in zip(idx.cpu().numpy(), f["cross_idx"])])
    assert ((srt[:, -kc] - srt[:, -kc - 1])[~same] < 2e-6).all()
    n_tie_rows = int((~same).sum())
    print(f"rows whose top-k SET differs from the reference's torch.topk (k-boundary ties under the declared rule): {n_tie_rows} of {same.shape[0]}")
    assert n_tie_rows == TIE_ROWS[same.shape[0]], n_tie_rows
    assert ei.shape == f["cross_edge_index"].shape
    # (2b) edge-level accounting against the reference's own coalesced edge list: every edge the two lists do not share belongs
    # to one of the tie rows above, as many edges are swapped in as out, and a swapped-in candidate's probability equals the
    # swapped-out one's (the reference's fp32 value) within 4 fp32 ulp of [0.5, 1): the reference's own rounding decided the row
    tie = set(np.nonzero(~same)[0].tolist())
    es = lambda e: set(map(tuple, np.asarray(e).T.tolist()))
    ours, ref = es(ei.cpu().numpy()), es(f["cross_edge_index"])
    only_o, only_r = ours - ref, ref - ours
    assert {t for _, t in only_o | only_r} <= tie and len(only_o) == len(only_r)
    print(f"cross edges not shared with the reference's list: {len(only_o)} of {len(ours)} (each way), all in the {n_tie_rows} tie rows")
    assert len(only_o) == CROSS_EDGE_DIFF[same.shape[0]], len(only_o)
    idx_h, esim_h = idx.cpu().numpy(), esim.cpu().numpy()
    for r in tie:
        mine = [j for j, c in enumerate(idx_h[r]) if c not in set(f["cross_idx"][r])]
        theirs = [j for j, c in enumerate(f["cross_idx"][r]) if c not in set(idx_h[r])]
        assert len(mine) == len(theirs) >= 1
        for a in mine:
            for b in theirs:
                assert abs(float(esim_h[r, a]) - float(f["cross_e_sim"][r, b])) <= 4 * 5.96e-8, (r, esim_h[r, a], f["cross_e_sim"][r, b])
    assert np.array_equal(pcs.argmax(1).cpu().numpy(), f["pred_clf_src"]) and np.array_equal(pct.argmax(1).cpu().numpy(), f["pred_clf_tar"])
    assert_close(pcs.cpu().numpy()[::16], f["probs_clf_src_rows"], what="probs_clf_src")
    # (3) within-domain k=3 (self matches kept, Appendix B-3)
    for dom, z in (("src", f["z_src"]), ("tar", f["z_tar"])):
        e2, es2, i2 = add_topk_sim_within_domain_edges(Data(x=_t(z)), model, k=3, z=_t(z), verbose=False)
        gA, gB, *_ = model.mlp_terms(_t(z), _t(z))
        _, ri = OC.mlp_topk(gA.cpu().numpy(), gB.cpu().numpy(), gs.cpu().numpy(), gh.cpu().numpy(), gw.cpu().numpy(), gb, 3)
        assert np.array_equal(i2.cpu().numpy(), ri)
        assert_close(es2.cpu().numpy(), f[f"within_{dom}_e_sim"], rtol=1e-5, atol_scale=1e-6, what=f"within {dom}")
        # edge-level accounting vs the reference's within-domain list: differences confined to rows whose index SET differs,
        # balanced, and the swapped candidates' probabilities equal within 4 ulp
        i2h, e2h = i2.cpu().numpy(), es2.cpu().numpy()
        wsame = np.array([set(a) == set(b) for a, b in zip(i2h, f[f"within_{dom}_idx"])])
        wtie = set(np.nonzero(~wsame)[0].tolist())
        o2, r2 = es(e2.cpu().numpy()), es(f[f"within_{dom}_edge_index"])
        assert {t for _, t in (o2 - r2) | (r2 - o2)} <= wtie and len(o2 - r2) == len(r2 - o2)
        print(f"within-{dom} edges not shared with the reference's list: {len(o2 - r2)} of {len(o2)}, in {len(wtie)} tie rows")
        assert (len(o2 - r2), len(wtie)) == WITHIN_EDGE_DIFF[(tag, dom)], (len(o2 - r2), len(wtie))
        for r in wtie:
            mine = [j for j, c in enumerate(i2h[r]) if c not in set(f[f"within_{dom}_idx"][r])]
            theirs = [j for j, c in enumerate(f[f"within_{dom}_idx"][r]) if c not in set(i2h[r])]
            for a in mine:
                for b in theirs:
                    assert abs(float(e2h[r, a]) - float(f[f"within_{dom}_e_sim"][r, b])) <= 4 * 5.96e-8


def test_cosine_v1_scorer_from_twitter_ckpt(golden):
    from bridged_gnn_amd.bridge import BridgeScorer
    f = golden("knn_cosine_v1.npz")
    sd = {"source_learner.sim_net." + k: torch.from_numpy(np.asarray(v)) for k, v in sub(f, "sim.").items()}
    model = BridgeScorer(sd, DEV)
    assert model.sim_mode == "cosine" and model.version == "v1"
    q_src, q_tar = model.cosine_q(_t(f["z_src"])), model.cosine_q(_t(f["z_tar"]))
    assert_close(q_src.cpu().numpy(), f["q_src"], what="q_src")
    assert_close(q_tar.cpu().numpy(), f["q_tar"], what="q_tar")
    idx, probs, _ = model.topk(_t(f["z_src"]), _t(f["z_tar"]), 20)
    # bit-exact vs the oracle on the GPU's own q (collapsed embeddings: cos in [0.95, 1])
    from bridged_gnn_amd import ops
    qs, qt = ops.l2_normalize_rows(q_src).cpu().numpy(), ops.l2_normalize_rows(q_tar).cpu().numpy()
    rv, ri = OC.cosine_topk(qt, qs, 20)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert_close(probs.cpu().numpy(), f["cross_e_sim"], rtol=1e-5, atol_scale=1e-6, what="e_sim vs reference")


def test_pair_probs_reference_shaped_api(golden):
    from bridged_gnn_amd.bridge import BridgeScorer, pair_enumeration
    f = golden("knn_office_a2d.npz")
    sd = {"source_learner.sim_net." + k: torch.from_numpy(np.asarray(v)) for k, v in sub(f, "sim.").items()}
    model = BridgeScorer(sd, DEV)
    ns = 2817
    pairs = pair_enumeration(torch.arange(ns, device=DEV).unsqueeze(-1), torch.arange(3, device=DEV).unsqueeze(-1)).t()
    p = model.pair_probs(_t(f["z_src"]), _t(f["z_tar"]), pairs[0], pairs[1]).view(-1, ns)
    tk = p.topk(20, dim=1)
    assert_close(tk.values.cpu().numpy(), f["cross_e_sim"][:3], rtol=1e-5, atol_scale=1e-6, what="pair probs")


def test_c5_scale_sampled_rows_bit_exact():
    """BASELINE config 5 at full size (100k x 100k, d=128, k=20): 96 sampled query rows re-done by the
    CPU oracle must match bit-exactly; all rows must be sorted and in range."""
    from bridged_gnn_amd import ops, synth
    q = synth.gaussian_embeddings(100_000, 128, seed=0)
    c = synth.gaussian_embeddings(100_000, 128, seed=1)
    qn, cn = ops.l2_normalize_rows(_t(q)), ops.l2_normalize_rows(_t(c))
    idx, val, nfb = ops.cosine_topk(qn, cn, 20)
    idx_h, val_h = idx.cpu().numpy(), val.cpu().numpy()
    assert idx_h.min() >= 0 and idx_h.max() < 100_000
    assert (np.diff(val_h, axis=1) <= 0).all()
    assert all(len(set(r)) == 20 for r in idx_h[::997])
    rows = np.arange(0, 100_000, 1043)[:96]
    # bgnn_knn.hip launch_refine (refine_kernel): at most 2048 blocks of 4 queries, so queries from 8192 on are re-scored in a block's
    # later trips; the sample below is taken from every trip
    assert q.shape[0] > 2048 * 4 and (rows >= 12 * 2048 * 4).any() and (rows < 2048 * 4).any()
    qh, ch = qn.cpu().numpy(), cn.cpu().numpy()
    assert np.array_equal(qh[rows], OC.l2_normalize_rows(q[rows]))
    _, ri = OC.cosine_topk(qh[rows], ch, 20)
    assert np.array_equal(idx_h[rows], ri)
    assert int(nfb[0].item()) < 100


def test_v1_sage_encoders_from_twitter_ckpt(golden):
    """GraphEncoder (2 x SAGEConv mean aggregation) through the fused CSR kernel vs the reference."""
    from bridged_gnn_amd.bridge import BridgeScorer
    from bridged_gnn_amd.data import Data
    f = golden("sage_encoder_v1.npz")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sub(f, "sd.").items()}
    model = BridgeScorer(sd, DEV)
    assert model.version == "v1"
    zs = model.encode_source(Data(x=_t(f["x_src"]), edge_index=_t(f["ei_src"].astype(np.int64))))
    zt = model.encode_target(Data(x=_t(f["x_tar"]), edge_index=_t(f["ei_tar"].astype(np.int64))))
    assert_close(zs.cpu().numpy(), f["z_src"], what="z_src")
    assert_close(zt.cpu().numpy(), f["z_tar"], what="z_tar")


def test_cosine_topk_cascade_stages_are_exercised():
    """The filter cascade stage by stage.  (a) collapsed embeddings (every candidate within ~1e-3 of every other one, like the
    reference's trained twitter embeddings, SURVEY 7 hard part 1): hundreds of candidates lie inside the fast pass's 2-eps margin,
    its 48-entry window overflows, the proof fails and the PRECISE pass (three products, eps ~ 6e-5, 56-entry window) resolves
    most of the rows, the exhaustive stage the rest; (b) well separated data: no row leaves the fast stage; (c) duplicated
    candidates tie exactly at the k boundary INSIDE the shortlist: resolved by the canonical rank (lower index), no further stage
    (a whole candidate set of identical vectors does reach the exhaustive stage: test_cosine_topk_exact_ties_and_duplicates).
    Indices bit-exact against the oracle in all three."""
    from bridged_gnn_amd import ops, synth
    rng = np.random.default_rng(42)
    d, k = 128, 20
    centre = rng.standard_normal(d)
    ce = (centre + 2e-2 * rng.standard_normal((6000, d))).astype(np.float32)        # cosines all in [0.97, 1]
    qe = (centre + 2e-2 * rng.standard_normal((300, d))).astype(np.float32)
    q, c = OC.l2_normalize_rows(qe), OC.l2_normalize_rows(ce)
    idx, val, nfb = ops.cosine_topk(_t(q), _t(c), k, apply_sigmoid=False)
    rv, ri = OC.cosine_topk(q, c, k)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert int(nfb[1].item()) > 0, "the collapsed embeddings were expected to overflow the fast pass's margin window"
    assert int(nfb[0].item()) < int(nfb[1].item()), "the precise pass should resolve part of the rows it is given"
    # (b)
    q2 = OC.l2_normalize_rows(synth.gaussian_embeddings(300, d, seed=8))
    c2 = OC.l2_normalize_rows(synth.gaussian_embeddings(6000, d, seed=9))
    idx2, _, nfb2 = ops.cosine_topk(_t(q2), _t(c2), k, apply_sigmoid=False)
    assert np.array_equal(idx2.cpu().numpy(), OC.cosine_topk(q2, c2, k)[1])
    assert int(nfb2[0].item()) == 0 and int(nfb2[1].item()) <= 1
    # (c) the k-th and (k+1)-th candidates of every query are the same vector
    c3 = np.concatenate([c2, c2[:3000]])
    idx3, _, nfb3 = ops.cosine_topk(_t(q2), _t(c3), k, apply_sigmoid=False)
    assert np.array_equal(idx3.cpu().numpy(), OC.cosine_topk(q2, c3, k)[1])
    assert int(nfb3[0].item()) == 0
