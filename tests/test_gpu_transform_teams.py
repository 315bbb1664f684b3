"""GPU: team mode of the hidden transform (transform_stream_kernel, GemmParams::team_*; `ops.transform_team_runs` is the plan).
Every case runs `ops.adaptedconv_transform` in this process, team mode on, and once more in ONE fresh child process for all
cases with BGNN_TS_TEAMS=0 (the library reads the switch once): the rows of every tile the need bits (or the tail groups) say
are written must be equal bit for bit, and the rows behind row N stay untouched.  The plan is part of the check: a case that is
about team mode must have a run, a case about its limits must have none.

Team-mode situations covered:
  one run            a, b72, b100 (run to the partial last tile), c (run from tile 0: the block re-arms back), f (one tail group)
  no run             d (interleaved domains), e (3 tiles per block)
  two runs           h (table 1 then table 0, tiles that need both in between), i (directly adjacent: both teams switch at the same
                     loop head, the second run ends in the partial last tile), j (table 0 from tile 0, then tiles that need NEITHER
                     table, then table 1), l (h with Din = 100), m (two tail groups around a tile that holds rows of both; the
                     launch without the fused iteration), n (two tail groups on tile boundaries: adjacent runs)
  admission boundary k (a run of exactly 4 tiles per block is taken, one of 4 per block less one tile is not)
  run starts         at a multiple of the grid size (every block starts the run at the same local tile) and off one (the blocks'
                     local starts differ by one, so some round the start up to the DEPTH-unrolled loop head and some do not)
  fp64               the needed rows of every case against the float64 restatement of tests/test_gpu_classifier_stage.py
  admission          every clause of the launcher's `team_runs_admit`, one bad run at a time; three runs are refused
  stale plan         a need mask edited in place between two launches is planned anew"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gpu_classifier_stage import DEV, GUARD, SENTINEL, close, dev_head, domain_sums64, make_head, ref_transform, sentinel, untouched

pytestmark = pytest.mark.gpu

N_SRC, N_TAR = 40003, 50001          # case (a): boundary tile 1250 holds both domains, the last tile is partial
D = 128


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _st_graph(src_ids, tar_ids, seed):
    """2 within-domain in-edges per node + 2 source -> target bridge edges per target (from = neighbour, to = node)"""
    rng = np.random.default_rng(seed)
    ns, nt = len(src_ids), len(tar_ids)
    pick = lambda ids, k: ids[rng.integers(0, len(ids), k)]
    frm = np.concatenate([pick(src_ids, 2 * ns), pick(tar_ids, 2 * nt), pick(src_ids, 2 * nt)])
    to = np.concatenate([np.repeat(src_ids, 2), np.repeat(tar_ids, 2), np.repeat(tar_ids, 2)])
    return np.stack([frm, to]).astype(np.int64)


def _need_segments(case):
    """hand-made need masks as (value, tiles) segments (bit 0 = h_s2t, bit 1 = h_t2s), G = blocks of the launch"""
    G = _n_cu()
    if case in ("h", "l", "h64"):                       # table 1, five tiles that need both, table 0; the first run starts off a multiple of G
        return [(3, 37), (2, 4 * G + 3), (3, 5), (1, 4 * G + G // 2), (3, 2)]
    if case == "i":                                     # directly adjacent; the second run ends in the partial last tile
        return [(3, 37), (2, 4 * G + 3), (1, 4 * G + G // 2)]
    if case == "j":                                     # table 0 from tile 0, three tiles nobody needs, table 1
        return [(1, 4 * G), (0, 3), (2, 5 * G + 1), (3, 1)]
    if case == "k":                                     # 4 tiles per block less one tile | exactly 4 tiles per block
        return [(3, 1), (1, 4 * G - 1), (3, 1), (2, 4 * G), (3, 1)]
    return None


def _tail_groups(case):
    """-> (own rows, n_t2s, n_s2t) of the tail-form cases"""
    G = _n_cu()
    if case == "f":                                     # 4 tiles and a few per block need h_t2s only, a short group h_s2t only
        return 5003, 32 * (4 * G + 7) + 5, 1000
    if case == "m":                                     # both groups qualify; neither boundary on a tile boundary
        return 5003, 32 * (4 * G + 7) + 5, 32 * (4 * G + 2) + 9
    if case == "n":                                     # both boundaries on tile boundaries: the runs are directly adjacent
        return 32 * 156, 32 * (4 * G + 3), 32 * (4 * G + 1) + 11
    return None


def _domains(case):
    """-> (domain flags [n] bool, True = source; graph or None; tail_single; hand-made need mask or None)"""
    cu = _n_cu()
    segs, tail = _need_segments(case), _tail_groups(case)
    if segs is not None:                                # the mask decides which rows are compared, the flags stay random per row
        need = torch.cat([torch.full((k,), v, dtype=torch.int32) for v, k in segs])
        n = 32 * need.numel() - 7
        g = torch.Generator().manual_seed(17 + n)
        return (torch.rand(n, generator=g) < 0.45).numpy(), None, (0, 0), need
    if tail is not None:
        n = sum(tail)
        g = torch.Generator().manual_seed(11)
        return (torch.rand(n, generator=g) < 0.5).numpy(), None, tail[1:], None
    if case in ("a", "b72", "b100"):
        m = np.arange(N_SRC + N_TAR) < N_SRC
    elif case == "c":                                   # [T ; S]: the run comes first
        m = np.arange(N_SRC + N_TAR) >= N_TAR
    elif case == "d":                                   # domains interleaved every 64 rows
        m = (np.arange(20011) // 64) % 2 == 0
    elif case == "e":                                   # the target run gives every block 3 tiles (and some a 4th)
        m = np.arange(4099 + 32 * (3 * cu + cu // 2)) < 4099
    ids = np.arange(len(m))
    return m, _st_graph(ids[m], ids[~m], seed=len(m)), (0, 0), None


def _inputs(case):
    """host tensors of a case, the same in both processes"""
    din = {"b72": 72, "b100": 100, "l": 100}.get(case, 128)
    m, ei, tail, need = _domains(case)
    n = len(m)
    g = torch.Generator().manual_seed(1000 + n + din)
    m = torch.from_numpy(m)
    x = torch.randn(n, din, generator=g)
    x[m] += torch.randn(din, generator=g) * 0.5
    return x, m, make_head(g, 64 if case == "h64" else D, din, True), ei, tail, need


def _launch(c, **over):
    """one call on the device tensors of `_setup` (keywords replace entries of c) -> (h_t2s, h_s2t), sentinel-filled, n + GUARD rows"""
    from bridged_gnn_amd import ops
    c = dict(c, **over)
    out = (sentinel(c["n"] + GUARD, c["packed"][4]), sentinel(c["n"] + GUARD, c["packed"][4]))
    ops.adaptedconv_transform(c["x"], c["m8"], None, c["packed"], out=[out], sums=c["sums"], tail_single=c["tail"], tile_need=c["need"])
    torch.cuda.synchronize()
    return out


def _needed_rows(n, need, tail):
    """-> (rows of h_t2s that must be written [n] bool, rows of h_s2t)"""
    rows = torch.arange(n, device=DEV)
    if need is not None:
        return (need[rows // 32] & 2).bool(), (need[rows // 32] & 1).bool()
    t2s_begin, s2t_begin = n - tail[0] - tail[1], n - tail[1]
    return rows < s2t_begin, (rows < t2s_begin) | (rows >= s2t_begin)


def _setup(case):
    """the device tensors of a case: what `_launch` passes on, and what the checks need"""
    from bridged_gnn_amd import ops
    x, m, head, ei, tail, need = _inputs(case)
    n = x.shape[0]
    m8 = m.to(DEV, torch.uint8)
    if ei is not None:
        need = ops.build_dst_csr(torch.from_numpy(ei).to(DEV), n, rewrite_self_loops=True).tile_need(m8)
        assert need is not None, "s -> t bridges only: some tile needs one table"
    elif need is not None:
        need = need.to(DEV)
    return {"x": x.to(DEV), "m": m, "m8": m8, "head": head, "packed": ops.pack_transform_heads([dev_head(head)], x.shape[1]),
            "sums": domain_sums64(x, m).to(DEV), "need": need, "tail": tail, "n": n}


@functools.lru_cache(maxsize=None)
def _run(case):
    """-> (h_t2s [n + GUARD], h_s2t [n + GUARD], needed rows of h_t2s [n] bool, of h_s2t, plan, the case's device tensors);
    one launch per case and process, shared by the tests"""
    from bridged_gnn_amd import ops
    c = _setup(case)
    w_t2s, w_s2t = _needed_rows(c["n"], c["need"], c["tail"])
    plan = ops.transform_team_runs(c["n"], torch.device(DEV), c["need"], c["tail"])
    out = _launch(c)
    return out[0], out[1], w_t2s, w_s2t, plan, c


CASES = ("a", "b72", "b100", "c", "d", "e", "f", "h", "i", "j", "k", "l", "m", "n")
TWO_RUNS = ("h", "i", "j", "l", "m", "n")


def _off_child(outdir):
    assert os.environ.get("BGNN_TS_TEAMS") == "0"
    for case in CASES:
        h_t2s, h_s2t, w_t2s, w_s2t, _, _ = _run(case)
        assert untouched(h_t2s[-GUARD:]) and untouched(h_s2t[-GUARD:])
        torch.save((h_t2s[:-GUARD][w_t2s].cpu(), h_s2t[:-GUARD][w_s2t].cpu()), os.path.join(outdir, case + ".pt"))
        _run.cache_clear()


@pytest.fixture(scope="module")
def off_rows(tmp_path_factory):
    """needed rows of every case as the library writes them with BGNN_TS_TEAMS=0: one child process for all cases"""
    outdir = str(tmp_path_factory.mktemp("teams_off"))
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--off-child", outdir], env=dict(os.environ, BGNN_TS_TEAMS="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return lambda case: torch.load(os.path.join(outdir, case + ".pt"))


def _expected_plan(case):
    G = _n_cu()
    if case in ("a", "b72", "b100"):                    # tiles behind the boundary tile, to the partial last one: h_s2t only
        return [((N_SRC + 31) // 32, (N_SRC + N_TAR + 31) // 32, 0)]
    if case == "c":                                     # tiles in front of the boundary tile
        return [(0, N_TAR // 32, 0)]
    if case in ("h", "l", "h64"):
        return [(37, 4 * G + 40, 1), (4 * G + 45, 8 * G + G // 2 + 45, 0)]
    if case == "i":                                     # the second run begins where the first ends and reaches the last tile
        return [(37, 4 * G + 40, 1), (4 * G + 40, 8 * G + G // 2 + 40, 0)]
    if case == "j":
        return [(0, 4 * G, 0), (4 * G + 3, 9 * G + 4, 1)]
    if case == "k":                                     # the run of 4G tiles, not the one of 4G - 1
        return [(4 * G + 1, 8 * G + 1, 1)]
    if case in ("f", "m", "n"):                         # whole tiles inside each tail group; f: the h_s2t group is too short
        own, n_t2s, n_s2t = _tail_groups(case)
        s2t_begin = own + n_t2s
        runs = [((own + 31) // 32, s2t_begin // 32, 1), ((s2t_begin + 31) // 32, (s2t_begin + n_s2t + 31) // 32, 0)]
        return runs[:1] if case == "f" else runs
    return []                                           # d: runs of two tiles; e: 3 tiles per block


@pytest.mark.parametrize("case", CASES)
def test_team_mode_equals_the_switched_off_library(case, off_rows):
    """(a) [S ; T], s -> t bridges; (b) the same with Din = 72 / 100; (c) [T ; S]: the block re-arms back; (d) interleaved domains and
    (e) a run of 3 tiles per block: the plan is empty and the launch is the one without team mode; (f) tail groups, one long enough.
    Two runs in one launch, from hand-made need masks: (h) table 1, tiles that need both, table 0; (i) the runs directly adjacent, the
    second to the partial last tile; (j) table 0 from tile 0, tiles that need neither table, table 1; (k) one run of exactly 4 tiles
    per block and one a tile shorter; (l) = (h) with Din = 100; and from two tail groups: (m) around a tile with rows of both groups,
    (n) both boundaries on tile boundaries."""
    h_t2s, h_s2t, w_t2s, w_s2t, plan, c = _run(case)
    assert c["n"] % 32 != 0
    assert plan == _expected_plan(case), f"case {case}: plan {plan}"
    if plan:
        n_blocks = min((h_t2s.shape[0] - GUARD + 31) // 32, _n_cu())
        assert all((e - b) // n_blocks >= 4 for b, e, _ in plan)
    if case in TWO_RUNS:
        assert len(plan) == 2 and plan[0][2] != plan[1][2] and plan[0][1] <= plan[1][0]
    if case in ("i", "n"):
        assert plan[0][1] == plan[1][0], f"case {case}: the runs are directly adjacent"
    if case == "m":
        assert plan[0][1] + 1 == plan[1][0] and (c["n"] - c["tail"][1]) % 32 != 0, "one tile between the runs needs both tables"
    if case == "k":
        G = _n_cu()
        assert [e - b for b, e, _ in plan] == [4 * G] and int(c["need"][1: 4 * G].min()) == int(c["need"][1: 4 * G].max()) == 1
    off_t2s, off_s2t = off_rows(case)
    got_t2s, got_s2t = h_t2s[:-GUARD][w_t2s], h_s2t[:-GUARD][w_s2t]
    assert int(w_t2s.sum()) > 0 and int(w_s2t.sum()) > 0
    assert torch.equal(got_t2s.view(torch.int32).cpu(), off_t2s.view(torch.int32)), f"case {case}: needed h_t2s rows differ"
    assert torch.equal(got_s2t.view(torch.int32).cpu(), off_s2t.view(torch.int32)), f"case {case}: needed h_s2t rows differ"
    assert not bool((got_t2s.view(torch.int32) == 0x7FA5C3E1).all(dim=1).any()), f"case {case}: a needed h_t2s row was not written"
    assert not bool((got_s2t.view(torch.int32) == 0x7FA5C3E1).all(dim=1).any()), f"case {case}: a needed h_s2t row was not written"
    assert untouched(h_t2s[-GUARD:]) and untouched(h_s2t[-GUARD:]), f"case {case}: rows behind row N written"


def test_run_starts_on_and_off_a_multiple_of_the_grid():
    """A run that begins at a tile b with b % G == 0 starts at the same local tile in every block; with b % G != 0 the blocks below
    b % G start one local tile later than the others, so under the DEPTH = 2 unrolled loop some blocks round their start up and
    some do not.  The two-run cases have both kinds (their plans are asserted above)."""
    G = _n_cu()
    begins = [b for case in TWO_RUNS for b, _, _ in _expected_plan(case)]
    assert any(b % G == 0 for b in begins) and any(b % G != 0 for b in begins), begins


@pytest.mark.parametrize("case", CASES)
def test_team_mode_vs_fp64(case):
    """the needed rows of the same launches against the float64 restatement, at the project's default bar (which the library meets
    without team mode in tests/test_gpu_transform_need.py); `close` refuses a row that was never written"""
    h_t2s, h_s2t, w_t2s, w_s2t, _, c = _run(case)
    r_s2t, r_t2s = ref_transform(c["x"].double(), c["m"].to(DEV), c["sums"], c["head"])
    close(h_t2s[:-GUARD, :D][w_t2s].cpu().numpy(), r_t2s[w_t2s].cpu().numpy(), f"case {case}: needed h_t2s rows vs fp64")
    close(h_s2t[:-GUARD, :D][w_s2t].cpu().numpy(), r_s2t[w_s2t].cpu().numpy(), f"case {case}: needed h_s2t rows vs fp64")


# ---------------------------------------------------------------------------------------------------- admission and plan hygiene
def _inject(c, plan, monkeypatch):
    """the next launches on c get `plan` whatever the planner would say (the wrapper asks the planner when the mask has no plan)"""
    from bridged_gnn_amd import ops
    if c["need"] is not None:
        c["need"]._team_plan = None
    monkeypatch.setattr(ops, "transform_team_runs", lambda *a, **k: list(plan))


def _bad_plan(kind):
    """-> (case, plan with ONE run that `team_runs_admit` must empty).  A run admitted by mistake would skip a table in tiles that
    need it (or, for the clauses whose run cannot be given a meaning, change nothing): rows unwritten or unequal, never an access
    outside the tables -- tile indices are bounded by the block's tile count and the stores are range checked."""
    G = _n_cu()
    if kind == "D64":                                   # 128 packed columns: the 4-wave-per-table teams do not exist
        return "h64", _expected_plan("h64")
    if kind in ("tail1", "tail0"):
        own, n_t2s, _ = _tail_groups("m")
        good, sb = _expected_plan("m"), (own + n_t2s) // 32           # tile sb holds the last h_t2s-only and the first h_s2t-only rows
        return "m", ([(good[0][0], sb + 1, 1), good[1]] if kind == "tail1" else [good[0], (sb, good[1][1], 0)])
    good = _expected_plan("h")
    ntiles = good[1][1] + 2
    return "h", {"overlap": [good[0], (good[0][1] - 4, good[1][1], 0)],       # ... and over the five tiles that need both tables
                 "table2": [(good[0][0], good[0][1], 2), good[1]],
                 "end": [good[0], (good[1][0], ntiles + G, 0)],
                 "begin": [(-3, good[0][1], 1), good[1]],
                 "short": [(good[0][0], good[0][0] + 4 * G - 1, 1), good[1]]}[kind]


@pytest.mark.parametrize("kind", ["overlap", "table2", "end", "begin", "short", "tail1", "tail0", "D64"])
def test_a_run_the_launcher_must_not_take_changes_nothing(kind, monkeypatch):
    """one bad run per launch: the needed rows are bit for bit those of the same launch with the plan [], and written"""
    case, plan = _bad_plan(kind)
    _, _, w_t2s, w_s2t, real_plan, c = _run(case)
    assert real_plan, "the planner itself has runs for these inputs"
    _inject(c, plan, monkeypatch)
    bad = _launch(c)
    _inject(c, [], monkeypatch)
    ref = _launch(c)
    for name, t, w in (("h_t2s", 0, w_t2s), ("h_s2t", 1, w_s2t)):
        got, want = bad[t][:-GUARD][w].view(torch.int32), ref[t][:-GUARD][w].view(torch.int32)
        assert not bool((want == SENTINEL).all(dim=1).any()), f"{kind} {name}: a needed row was not written with the plan []"
        assert torch.equal(got, want), f"{kind} {name}: {int((got != want).any(dim=1).sum())} needed rows differ from the launch with the plan []"
        assert untouched(bad[t][-GUARD:]) and untouched(ref[t][-GUARD:]), f"{kind} {name}: rows behind row N written"


def test_three_runs_are_refused(monkeypatch):
    _, _, _, _, plan, c = _run("h")
    _inject(c, plan + [(0, 1, 0)], monkeypatch)
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE"):
        _launch(c)


def test_need_mask_edited_in_place_between_launches():
    """launch, make one tile inside the first run need both tables, launch again: the plan kept on the mask is stale, and a launch
    that used it would leave that tile's h_s2t rows unwritten.  Every needed row equals the unmasked call bit for bit
    (tests/test_gpu_transform_need.py holds the need-mask launch to that)."""
    from bridged_gnn_amd import ops
    c = dict(_run("h")[5])
    c["need"] = c["need"].clone()
    good = _expected_plan("h")
    _launch(c)
    assert c["need"]._team_plan[1] == good, "the first launch ran with both runs"
    tile = 40
    assert good[0][0] < tile < good[0][1] - 1
    c["need"][tile] = 3
    got = _launch(c)
    assert ops.transform_team_runs(c["n"], torch.device(DEV), c["need"]) == [good[1]]
    full = _launch(c, need=None)
    w_t2s, w_s2t = _needed_rows(c["n"], c["need"], c["tail"])
    rows = slice(32 * tile, 32 * tile + 32)
    assert bool(w_t2s[rows].all()) and bool(w_s2t[rows].all())
    for name, t, w in (("h_t2s", 0, w_t2s), ("h_s2t", 1, w_s2t)):
        gi, fi = got[t][:-GUARD].view(torch.int32), full[t][:-GUARD].view(torch.int32)
        assert not bool((gi[rows] == SENTINEL).all(dim=1).any()), f"{name}: rows of the edited tile were not written"
        assert torch.equal(gi[rows], fi[rows]), f"{name}: rows of the edited tile differ from the unmasked call"
        assert torch.equal(gi[w], fi[w]), f"{name}: needed rows differ from the unmasked call"
        assert untouched(got[t][-GUARD:])


def test_eval_forward_on_the_team_graph_vs_c_oracle():
    """(g) case (a)'s graph through the model's eval forward (the hidden conv's transform runs in team mode) against the C oracle's
    full forward at the default bar"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    from oracle import oracle_c as OC
    from oracle import oracle_np as O
    x, m, _, ei, _, _ = _inputs("a")
    n = x.shape[0]
    need = ops.build_dst_csr(torch.from_numpy(ei).to(DEV), n, rewrite_self_loops=True).tile_need(m.to(DEV, torch.uint8))
    assert ops.transform_team_runs(n, torch.device(DEV), need) == _expected_plan("a")
    torch.manual_seed(5)
    model = KTGNN_no_complement(128, 2, 2, 128, root_weight=False, use_bn=True, dim_share=128, need_complement=False)
    g = torch.Generator().manual_seed(3)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    model = model.to(DEV).eval()
    data = Data(x=x.to(DEV), edge_index=torch.from_numpy(ei).to(DEV), central_mask=m.to(DEV))
    with torch.no_grad():
        out = [t.cpu().numpy() for t in model(data)[:3]]
        emb = model.get_emb(data).cpu().numpy()[:, :128]
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    rowptr, col, _ = O.dst_csr(ei, m.numpy())
    rb, rt, rth, remb = OC.ktgnn_forward_eval(x.numpy(), rowptr, col, m.numpy(), sd, return_emb=True)
    for name, got, ref in (("hidden conv (BN+ReLU)", emb, remb), ("logp_base", out[0], rb), ("logp_target", out[1], rt), ("logp_target_hat", out[2], rth)):
        assert_close(got, ref, what=f"{name}, team graph")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--off-child":
        _off_child(sys.argv[2])
