"""GPU: the cosine top-k cascade (bgnn_cosine_topk_f32) on every width, shortlist geometry and product set, and the row
normalisation off its one tested shape.  Indices bit-exact against oracle.oracle_c.cosine_topk everywhere.

The pass-1 kernel has 24 instantiations: d in {32, 64, 128, 256} x {narrow (k <= 20), wide (k > 20)} x NPROD in {1, 2, 3}.
  part 1  NPROD = 1, all eight (d, geometry) pairs at the edges of their tiling (second tile of one candidate, full last tile,
          head pass, ragged last query block, a block whose tile range straddles query blocks) and at k = 1, 20, 21, 56;
  part 2  NPROD = 3 as the precise pass, all eight pairs: collapsed embeddings for which a CPU model of the margins PROVES that
          the fast proof fails in every row (nfb[1] == Nq exactly), and names rows the precise pass must prove;
  part 3  NPROD = 2 and NPROD = 3 as the fast pass (BGNN_KNN_FAST_PRODUCTS, read once per process): one child process per value,
          one after another; an invalid value must behave as the default;
  part 4  bgnn_l2_normalize_rows_f32: partial LDS tiles, widths that are no multiple of 4, the thread-per-row kernel (d >= 3072).

The CPU model (`_margins`): the kernel's own bound knn_eps from the bf16 residual norms, the exact fp64 scores s and the fp64
value a of the fast pass's products.  If every score of a row lies so close together that
    (max_j s_j - min_j s_j) + max_j |a_j - s_j| + d nprod 1.3e-7  <  0.99 eps          (d nprod 1.3e-7: the MFMAs' fp32 sums)
then no compaction can cut by its margin (2 eps), a shortlist that has seen more than KP candidates has raised its threshold to
the approximate score of one of them, and the refine stage's proof  kth_exact > T + eps  cannot hold: the row goes on."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (32, 64, 128, 256)
SWITCH = "BGNN_KNN_FAST_PRODUCTS"
CHILD_TIMEOUT = 120          # seconds per child; a child takes a few seconds (start of torch + 32 calls on at most 8129 candidates)
MAX_SLOTS = 8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the geometry of csrc/bgnn_knn.hip, restated -------------------------------------------------------------------------------
def _ct(k):                  # candidates per staged step of a fast pass of one or two products; three products stage 32 for every k,
    return 64 if k <= 20 else 32    # as the precise pass and as the fast pass under BGNN_KNN_FAST_PRODUCTS=3


def _kp(k, nprod):           # shortlist entries a slot hands on: by the product set (three products: the precise geometry, in either role)
    return (48 if k <= 20 else 112) if nprod < 3 else (56 if k <= 20 else 120)


def _qb(d, k, nprod):        # queries per block = pass1_waves x 32
    narrow = k <= 20
    if nprod == 3:
        return (256 if narrow else 128) if d <= 64 else (128 if narrow else 64)
    return (256 if narrow else 128) if d <= 128 else (128 if narrow else 64)


def _fewest_candidates_of_a_query_blocks_largest_slot(nq, nc, qb, ct, blocks):
    """plan_pass1 without a head pass: the blocks take contiguous runs of `tpb` (query block, tile) pairs; a slot is the part of
    one run inside one query block.  -> over the query blocks, the least of (candidates of its largest slot)."""
    ntiles, nqb = -(-nc // ct), -(-nq // qb)
    total = ntiles * nqb
    nb = max(1, min(total, blocks))
    tpb = max(-(-total // nb), (ntiles + MAX_SLOTS - 2) // (MAX_SLOTS - 1))
    least = nc
    for b in range(nqb):
        lo, hi = b * ntiles, (b + 1) * ntiles
        cuts = [lo] + [t for t in range(lo + 1, hi) if t % tpb == 0] + [hi]
        least = min(least, max(min((t1 - lo) * ct, nc) - (t0 - lo) * ct for t0, t1 in zip(cuts, cuts[1:])))
    return least


# ---- the CPU model of the margins ----------------------------------------------------------------------------------------------
def _bf16(x):                # round to nearest even, as the (__bf16) conversions of split_rows_kernel
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).to(torch.float32).numpy()


def _split(x):
    hi = _bf16(x)
    r1 = x - hi                                         # exact in fp32
    mid = _bf16(r1)
    r2 = r1 - mid
    norm = lambda r: float(np.sqrt((r.astype(np.float64) ** 2).sum(1)).max())
    return hi.astype(np.float64), mid.astype(np.float64), norm(r1), norm(r2)


def _knn_eps(Ra, Raa, Rb, Rbb, d, nprod):
    """knn_eps of csrc/bgnn_knn.hip (a = candidates, b = queries), in fp64"""
    g, infl = 1e-6, 1.002
    Ra, Raa, Rb, Rbb = Ra * infl, Raa * infl, Rb * infl, Rbb * infl
    if nprod == 1:
        eps = Ra * (1 + g) + (1 + g + Ra) * Rb
    elif nprod == 2:
        eps = Ra * (1 + g) + (1 + g + Ra) * Rbb
    else:
        eps = Ra * Rb * 1.02 + Raa * (1 + g) + (1 + g + Raa) * Rbb
    return (eps + d * nprod * 1.2e-7 * 1.01) * 1.001


def _margins(q, c):
    """-> eps[1..3], lhs[1..2] = per row (spread + worst error of the fast products + accumulation), s = exact scores [Nq, Nc]"""
    d = q.shape[1]
    ch, _, Ra, Raa = _split(c)
    qh, qm, Rb, Rbb = _split(q)
    eps = {n: _knn_eps(Ra, Raa, Rb, Rbb, d, n) for n in (1, 2, 3)}
    s = q.astype(np.float64) @ c.astype(np.float64).T
    spread = s.max(1) - s.min(1)
    lhs = {1: spread + np.abs(qh @ ch.T - s).max(1) + d * 1.3e-7,
           2: spread + np.abs((qh + qm) @ ch.T - s).max(1) + 2 * d * 1.3e-7}
    return eps, lhs, s


def _collapsed(d, sigma, nq, nc, seed=1):
    """the recipe of test_cosine_topk_cascade_stages_are_exercised: every embedding within sigma of one centre"""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(d)
    ce = (centre + sigma * rng.standard_normal((nc, d))).astype(np.float32)
    qe = (centre + sigma * rng.standard_normal((nq, d))).astype(np.float32)
    return OC.l2_normalize_rows(qe), OC.l2_normalize_rows(ce)


def _assert_fast_proof_must_fail(q, c, k, nprod, eps, lhs, blocks, what):
    """the precondition of `nfb[1] == Nq`, see the module docstring"""
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    assert -(-nc // _ct(k)) < 128, f"{what}: the model covers the fast pass without a head pass"
    seen = _fewest_candidates_of_a_query_blocks_largest_slot(nq, nc, _qb(d, k, nprod), _ct(k), blocks)
    assert seen > _kp(k, nprod), f"{what}: a query block whose slots all see <= KP candidates ({seen}) never overflows"
    worst = float(lhs[nprod].max())
    print(f"{what}: spread + error {worst:.3e} against 0.99 eps{nprod} = {0.99 * eps[nprod]:.3e}; slots see >= {seen} candidates")
    assert worst < 0.99 * eps[nprod], f"{what}: {worst:.3e} >= {0.99 * eps[nprod]:.3e}: the fast proof may succeed in some row"


# ---- shared assertions ---------------------------------------------------------------------------------------------------------
def _assert_rows_strictly_sorted(q, c, idx, val, what):
    """(score desc, index asc), strictly: on the fp64 scores of the returned candidates (two distinct fp64 scores may round to one
    fp32 value); the fp32 values the kernel returns must not increase"""
    s = np.einsum("qkd,qd->qk", c.astype(np.float64)[idx], q.astype(np.float64))
    a, b, ia, ib = s[:, :-1], s[:, 1:], idx[:, :-1], idx[:, 1:]
    assert ((a > b) | ((a == b) & (ia < ib))).all(), f"{what}: a row is not sorted by (score desc, index asc)"
    assert (val[:, :-1] >= val[:, 1:]).all(), f"{what}: returned scores increase inside a row"


def _assert_matches_oracle(q, c, k, got, ref, what, fallback_cap=True):
    idx, val, nfb = got
    rv, ri = ref
    print(f"{what}: nfb = {nfb.tolist()}")
    assert idx.shape == ri.shape and idx.min() >= 0 and idx.max() < c.shape[0], what
    assert np.array_equal(idx, ri), f"{what}: {int((idx != ri).any(1).sum())} rows differ from the oracle, nfb = {nfb.tolist()}"
    assert_close(val, rv, rtol=1e-6, atol_scale=1e-7, what=f"{what}: scores")
    _assert_rows_strictly_sorted(q, c, idx, val, what)
    if fallback_cap:
        assert int(nfb[0]) <= max(2, q.shape[0] // 100), f"{what}: {int(nfb[0])} rows re-done exhaustively"


def _run(q, c, k):
    from bridged_gnn_amd import ops
    idx, val, nfb = ops.cosine_topk(_t(q), _t(c), k, apply_sigmoid=False)
    return idx.cpu().numpy(), val.cpu().numpy(), nfb.cpu().numpy()


def _gauss(n, d, seed):
    from bridged_gnn_amd import synth
    return OC.l2_normalize_rows(synth.gaussian_embeddings(n, d, seed=seed))


# ---- part 1: every default instantiation at its edges --------------------------------------------------------------------------
def _edge_pairs(d, k):
    ct = _ct(k)
    pairs = [(1, k),                      # every candidate is returned
             (33, ct + 1),                # the second tile holds one candidate
             (257, 127 * ct),             # no head pass, a full last tile, > 1 query block in every instantiation, ragged last block
             (70, 127 * ct + 1)]          # a head pass of 8 tiles; the main pass's last tile holds one candidate
    if _qb(d, k, 1) == 256:               # three query blocks: more (block, tile) pairs than resident blocks, so tpb > 1 and a
        pairs.append((600, 127 * ct + 1))  # block's tile range straddles query blocks
    return [(nq, nc) for nq, nc in pairs if nc >= k]


@pytest.mark.parametrize("k", [1, 20, 21, 56])
@pytest.mark.parametrize("d", WIDTHS)
def test_default_fast_pass_at_the_edges_of_its_tiling(d, k):
    for i, (nq, nc) in enumerate(_edge_pairs(d, k)):
        seed = 100_000 + 1000 * d + 10 * k + i
        q, c = _gauss(nq, d, seed), _gauss(nc, d, seed + 5)
        _assert_matches_oracle(q, c, k, _run(q, c, k), OC.cosine_topk(q, c, k), f"d={d} k={k} nq={nq} nc={nc}")


@pytest.mark.parametrize("d", [1, 33, 255])
def test_widths_that_are_zero_padded(d):
    """ops.cosine_topk pads to 32 / 64 / 256 columns; the oracle sees the unpadded rows.  d = 1: every score is +1 or -1, every
    row ties: the lowest indices of the +1 group, and rows re-done exhaustively are what the contract expects there."""
    nq, nc, k = 70, 300, 8
    q, c = _gauss(nq, d, 7000 + d), _gauss(nc, d, 7500 + d)
    got = _run(q, c, k)
    _assert_matches_oracle(q, c, k, got, OC.cosine_topk(q, c, k), f"d={d}", fallback_cap=d != 1)
    if d == 1:
        want = np.stack([np.nonzero(c[:, 0] == q[r, 0])[0][:k] for r in range(nq)])
        assert want.shape == (nq, k) and np.array_equal(got[0], want)


# ---- part 2: the precise pass, reached and checked, in all eight (d, geometry) pairs -------------------------------------------
NQ_PRECISE = 300             # more than one query block of every precise instantiation (QB <= 256)
# (d, k) -> (sigma, Nc, Nq).  A row is provable for the precise pass when s_(k) - s_(KP3 + 1) > 2 eps3; the gap grows with sigma^2
# and so does the spread that the precondition of nfb[1] == Nq caps, so what decides is the ratio (median gap) / (largest spread)
# of the data against 2 eps3 / (0.99 eps1 - worst error of the fast products).  Fewer candidates widen the gap, and 2 eps3 grows
# with d (d x 3 x 1.2e-7 alone is 9.3e-5 at d = 256), so the wider the rows the fewer the candidates; the floor is a fast slot that
# still sees more than KP of them.  Figures from the CPU model, seed 1: spread + error as a part of 0.99 eps1; provable rows.
PRECISE = {
    (32, 20): (0.025, 1000, NQ_PRECISE),      # 0.93; 165 of 300
    (32, 56): (0.025, 1000, NQ_PRECISE),      # 0.93; 139
    (64, 20): (0.032, 1000, NQ_PRECISE),      # 0.84; 237
    (64, 56): (0.032, 1000, NQ_PRECISE),      # 0.84; 212
    (128, 20): (0.044, 600, NQ_PRECISE),      # 0.85; 150
    (128, 56): (0.046, 800, NQ_PRECISE),      # 0.86; 114 (Nc = 600 would leave the wide slots 96 <= KP candidates: no overflow)
    (256, 20): (0.062, 250, NQ_PRECISE),      # 0.86; 157.  4 fast tiles of 64 > KP = 48; the precise slots hold 64 > KP3 = 56
    # wide at d = 256: the gap asks for Nc ~ 300 = 10 tiles of 32, and a slot of more than KP = 112 candidates for 4 tiles per
    # block, which ceil(10 / 7) = 2 does not give: it takes more (query block, tile) pairs than 3 x 256 resident blocks,
    # 10 x ceil(Nq / 64) > 768, Nq >= 4865 (asserted from the device's CU count like every other plan here)
    (256, 56): (0.062, 300, 5000),            # 0.94; 2930 of 5000.  Slots of 128 candidates in both passes
}


@pytest.mark.parametrize("d,k", list(PRECISE))
def test_precise_pass_is_reached_by_every_row_and_proves_the_rows_it_must(d, k):
    sigma, nc, nq = PRECISE[(d, k)]
    q, c = _collapsed(d, sigma, nq, nc)
    eps, lhs, s = _margins(q, c)
    blocks = torch.cuda.get_device_properties(0).multi_processor_count
    what = f"d={d} k={k} sigma={sigma} nc={nc} nq={nq}"
    _assert_fast_proof_must_fail(q, c, k, 1, eps, lhs, blocks, what)
    srt = -np.sort(-s, axis=1)
    rows = int((srt[:, k - 1] - srt[:, _kp(k, 3)] > 2 * eps[3]).sum())       # KP3 + 1 in 1-based counting
    print(f"{what}: 2 eps3 = {2 * eps[3]:.3e}, rows the precise pass must prove: {rows} of {nq}")
    assert rows >= nq // 4, f"{what}: only {rows} rows are provable for the precise pass"
    idx, val, nfb = _run(q, c, k)
    print(f"{what}: nfb = {nfb.tolist()}")
    assert np.array_equal(idx, OC.cosine_topk(q, c, k)[1]), f"{what}: indices differ from the oracle, nfb = {nfb.tolist()}"
    assert int(nfb[1]) == nq, f"{what}: {int(nfb[1])} of {nq} rows reached the precise pass"
    assert int(nfb[0]) <= nq - rows, f"{what}: {int(nfb[0])} rows left the precise pass unproven, at most {nq - rows} may"


# ---- part 3: the product sets 2 and 3 (and an invalid value), each in a child process ------------------------------------------
SIGMA_SWITCH = 0.01          # collapsed cases of part 3: tight enough for eps2 as well (eps2 ~ eps1 / 2, the error of two products
NC_SWITCH = 2000             # is 2.1e-3 of 0.99 eps2 = 2.8e-3 at d = 32, which leaves the spread 6e-4: sigma <= 0.015)


def _switch_cases():
    """name -> (q, c, k, kind); the same arrays in every process"""
    cases = {}
    for d in WIDTHS:
        base = _gauss(700, d, 6)
        qd = _gauss(200, d, 5)
        for k in (20, 56):
            ct = _ct(k)                                   # part 1's pairs; under =3 narrow stages 32, so both of them have a head pass there
            for nq, nc in ((257, 127 * ct), (70, 127 * ct + 1)):
                cases[f"gauss-d{d}-k{k}-{nq}x{nc}"] = (_gauss(nq, d, 31 * d + k + nq), _gauss(nc, d, 37 * d + k + nc), k, "gauss")
            cases[f"collapsed-d{d}-k{k}"] = (*_collapsed(d, SIGMA_SWITCH, NQ_PRECISE, NC_SWITCH, seed=2), k, "collapsed")
        cases[f"duplicates-d{d}"] = (qd, np.concatenate([base, base[:300], base[100:200], base]), 20, "duplicates")
        cases[f"identical-d{d}"] = (qd, np.repeat(base[:1], 500, axis=0), 20, "identical")
    return cases


def _run_cases(cases):
    out = {}
    for name, (q, c, k, _) in cases.items():
        out[name + "/idx"], out[name + "/val"], out[name + "/nfb"] = _run(q, c, k)
    return out


@pytest.fixture(scope="module")
def switch_runs(tmp_path_factory):
    """-> (cases, oracle results, {"default" | "2" | "3" | "7": arrays}); the children run one after another"""
    cases = _switch_cases()
    blocks = torch.cuda.get_device_properties(0).multi_processor_count
    for name, (q, c, k, kind) in cases.items():          # the preconditions of the exact counts, before any GPU call
        if kind == "collapsed":
            eps, lhs, _ = _margins(q, c)
            for nprod in (1, 2):
                _assert_fast_proof_must_fail(q, c, k, nprod, eps, lhs, blocks, f"{name}, {nprod} product(s)")
    ref = {name: OC.cosine_topk(q, c, k) for name, (q, c, k, _) in cases.items()}
    runs = {"default": _run_cases(cases)}
    outdir = tmp_path_factory.mktemp("knn_products")
    base = {k: v for k, v in os.environ.items() if k != SWITCH}
    for value in ("2", "3", "7"):
        path = str(outdir / f"products{value}.npz")
        try:
            r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--child", path], env=dict(base, **{SWITCH: value}), cwd=ROOT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:           # (subprocess.run has killed and reaped the child)
            log = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
            pytest.fail(f"{SWITCH}={value}: no result after {CHILD_TIMEOUT} s\n{log[-4000:]}")
        assert r.returncode == 0, f"{SWITCH}={value}: exit code {r.returncode}\n{r.stdout[-4000:]}"
        runs[value] = dict(np.load(path))
    return cases, ref, runs


def _got(run, name):
    return run[name + "/idx"], run[name + "/val"], run[name + "/nfb"]


@pytest.mark.parametrize("value", ["default", "2", "3", "7"])
def test_every_product_set_returns_the_oracles_neighbours(value, switch_runs):
    cases, ref, runs = switch_runs
    for name, (q, c, k, kind) in cases.items():
        _assert_matches_oracle(q, c, k, _got(runs[value], name), ref[name], f"{SWITCH}={value} {name}", fallback_cap=False)


@pytest.mark.parametrize("value", ["default", "2"])
def test_two_products_send_every_collapsed_row_to_the_precise_pass(value, switch_runs):
    """the eps1 / eps2 preconditions were asserted by the fixture; on Gaussian data (almost) no row leaves the fast stage"""
    cases, _, runs = switch_runs
    for name, (q, c, k, kind) in cases.items():
        nfb = runs[value][name + "/nfb"]
        if kind == "collapsed":
            assert int(nfb[1]) == q.shape[0], f"{SWITCH}={value} {name}: nfb = {nfb.tolist()}"
        if kind == "gauss":
            assert int(nfb[0]) <= max(2, q.shape[0] // 100), f"{SWITCH}={value} {name}: nfb = {nfb.tolist()}"


def test_three_fast_products_have_no_precise_stage(switch_runs):
    """nfb[1] stays 0; nfb[0] counts the rows the three-product pass could not prove"""
    cases, _, runs = switch_runs
    for name, (q, c, k, kind) in cases.items():
        nfb = runs["3"][name + "/nfb"]
        assert int(nfb[1]) == 0, f"{name}: nfb = {nfb.tolist()}"
        if kind == "gauss":
            assert int(nfb[0]) <= max(2, q.shape[0] // 100), f"{name}: nfb = {nfb.tolist()}"
        if kind == "identical":
            assert int(nfb[0]) == q.shape[0], f"{name}: nfb = {nfb.tolist()}"


def test_an_invalid_switch_value_is_the_default(switch_runs):
    cases, _, runs = switch_runs
    for name in cases:
        for part in ("/idx", "/val", "/nfb"):
            assert np.array_equal(runs["7"][name + part], runs["default"][name + part]), f"{name}{part}: {SWITCH}=7 differs from the default"


# ---- part 4: row normalisation off its one tested shape ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 100, 256, 3071, 3072, 4000])
def test_l2_normalize_rows_bit_exact_at_partial_tiles_and_wide_rows(d):
    """LDS tiles of min(64, 49152 // (4 (d + 1))) rows: 64 up to d = 191, 47 at d = 256, 4 at d = 3071 (the last tiled width); from
    d = 3072 on a thread per row.  n = 1, 63, 65, 130: one partial tile, one row short of 64, one row past it, 2 tiles + 2 rows."""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(9000 + d)
    for n in (1, 63, 65, 130):
        x = rng.standard_normal((n, d)).astype(np.float32)
        variants = [x]
        if n >= 3:
            x[n // 2] = 0.0                                 # the eps clamp
            x[n - 1] *= np.float32(1e-20)
        else:                                               # a single row: each kind on its own
            variants += [np.zeros_like(x), x * np.float32(1e-20)]
        for v in variants:
            got = ops.l2_normalize_rows(_t(v)).cpu().numpy()
            assert np.array_equal(got, OC.l2_normalize_rows(v)), f"n={n} d={d}"


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    np.savez(sys.argv[2], **_run_cases(_switch_cases()))
