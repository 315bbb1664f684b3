"""GPU: agg_wide_fast_kernel's single-tile claims from striped sub-queues (bgnn_adaptedconv_aggregate_queued_f32).

The library reads its scheduling switches once per process, so every schedule runs in a child process of its own, all cases in
one child, all children side by side (one module fixture):

  tile      BGNN_AGG_CLAIM=tile            single-tile claims, NQ = 4, the claim two tiles ahead
  chunk     BGNN_AGG_CLAIM=chunk           chunks of four tiles from one counter per XCD (the schedule before this one)
  general   BGNN_AGG_FAST=0                agg_wide_kernel
  nq1/2/8   BGNN_AGG_SUBQUEUES=1 / 2 / 8
  sync      BGNN_AGG_CLAIM_AHEAD=0         the claim waited for where it is issued

The children run with one resident block per CU (BGNN_AGG_BLOCKS_PER_CU=1), so that a block claims many tiles and its ring of four
claims wraps (case `clustered48k`: 6000 tiles on 256 blocks); this process runs the library's default at full occupancy.
Per case and schedule: the output rows and, in the ALPHA variant, the attention coefficients must equal the chunk child's and the
general kernel's bit for bit (compared as SHA-256 of the whole buffers, rows outside the range included); the column sums, fp32
partials in claim order, within the bar tests/test_gpu_round3.py uses (rtol 2e-6, atol 1e-3).  Written exactly once: `out` starts
as NaN, every row of the range ends finite and every other row NaN, and the node counts of the column sums, which count a row
each time it is finished, equal the range's (the ALPHA launch has no column sums: there a row finished twice would show only
in bits that differ, its rows and coefficients being checked as written / untouched and bit for bit).  Every case also runs
twice on ONE queue buffer (the entry zeroes it in between) and once with tile_queue = NULL (static stride)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (rows, D, graph, (row_begin, row_end) or None).  Tiles are 8 rows at D > 64 (LF = 32), 16 rows at D = 64 (LF = 16).
CASES = {
    "rows40": (40, 128, "near", None),                  # 5 tiles, a grid of 8 blocks: blocks without a tile; per_x = 1 pads every XCD to 8 positions
    "rows1003": (1003, 128, "near", None),              # a partial last tile
    "tiles1001": (8008, 128, "near", None),             # 1001 tiles: no multiple of NQ; per_x = 126 is no multiple of 8 (padded XCD segments)
    "tiles1004": (8032, 128, "near", None),             # a multiple of NQ = 4 but not of 8 * NQ: the sub-queues run dry at different times
    "clustered20k": (20000, 128, "near", None),
    "clustered48k": (48000, 128, "near", None),         # 6000 tiles: two dozen claims per block at one block per CU
    "range": (8008, 128, "near", (1003, 7001)),         # a partitioned launch's shape
    "empty": (6000, 128, "empty", None),                # rows without an edge, whole tiles of them among the rest (a tile without a step)
    "skew": (4096, 128, "skew", None),                  # 1, 4, 5 and 130 in-edges inside every tile: the waves of a block finish far apart
    "d72": (3001, 72, "near", None),                    # LF = 32 with invalid tail lanes
    "d64": (5003, 64, "near", None),                    # LF = 16
}
CONFIGS = {
    "tile": {"BGNN_AGG_CLAIM": "tile"},
    "chunk": {"BGNN_AGG_CLAIM": "chunk"},
    "general": {"BGNN_AGG_FAST": "0"},
    "nq1": {"BGNN_AGG_CLAIM": "tile", "BGNN_AGG_SUBQUEUES": "1"},
    "nq2": {"BGNN_AGG_CLAIM": "tile", "BGNN_AGG_SUBQUEUES": "2"},
    "nq8": {"BGNN_AGG_CLAIM": "tile", "BGNN_AGG_SUBQUEUES": "8"},
    "sync": {"BGNN_AGG_CLAIM": "tile", "BGNN_AGG_CLAIM_AHEAD": "0"},
}
CHILD_TIMEOUT = 120                                       # seconds; the seven children run side by side and take a few seconds each
KNOBS = ("BGNN_AGG_CLAIM", "BGNN_AGG_FAST", "BGNN_AGG_SUBQUEUES", "BGNN_AGG_CLAIM_AHEAD", "BGNN_AGG_CHUNK",
         "BGNN_AGG_INTERLEAVE", "BGNN_XCD_SEGMENTS", "BGNN_AGG_BLOCKS_PER_CU")


def _graph(kind, n, rng):
    """-> (rowptr, col) int32, by destination.  near: 9 in-edges on average, 90 % of them within 512 rows of the destination."""
    if kind == "skew":
        deg = np.tile(np.array([1, 4, 5, 130, 1, 4, 5, 130]), (n + 7) // 8)[:n]
    else:
        deg = rng.integers(1, 18, n)
        if kind == "empty":
            deg[rng.random(n) < 0.3] = 0
            deg[64:192] = 0                              # 16 tiles without any edge
            deg[-5:] = 0
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    dst = np.repeat(np.arange(n), deg)
    near = np.clip(dst + rng.integers(-512, 513, dst.size), 0, n - 1)
    col = np.where(rng.random(dst.size) < 0.9, near, rng.integers(0, n, dst.size))
    return rowptr.astype(np.int32), col.astype(np.int32)


def _inputs(case):
    n, D, kind, rng_rows = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))     # (the same inputs in every process)
    rowptr, col = _graph(kind, n, rng)
    ld = (D + 3) // 4 * 4
    both = torch.zeros(2, n, ld, device=DEV)             # one allocation: the two tables share a window
    both[:, :, :D] = torch.from_numpy(rng.standard_normal((2, n, D)).astype(np.float32)).to(DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    mask = rng.random(n) < 0.45
    return dict(n=n, D=D, ld=ld, tS=both[0], tT=both[1], rowptr=t(rowptr), col=t(col), m8=t(mask.astype(np.uint8)), mask=mask,
                a1=t((rng.standard_normal(D) * 0.3).astype(np.float32)), a2=t((rng.standard_normal(D) * 0.3).astype(np.float32)),
                sc=t(rng.uniform(0.5, 1.5, D).astype(np.float32)), sh=t(rng.standard_normal(D).astype(np.float32)),
                rows=rng_rows if rng_rows is not None else (0, n), n_edges=int(rowptr[-1]))


def _launch(c, out, alpha=None, sums=None, queue="fresh", words=None):
    """one call of bgnn_adaptedconv_aggregate_queued_f32; with `sums` also the BN-affine + ReLU epilogue"""
    from bridged_gnn_amd import _lib as L, ops
    q = ops._tile_queue(torch.device(DEV)) if isinstance(queue, str) else queue
    ep = sums is not None
    rb, re = c["rows"]
    rc = L.lib().bgnn_adaptedconv_aggregate_queued_f32(
        L.ptr_rows(c["tS"]), L.ptr_rows(c["tT"]), c["ld"], L.ptr(c["a1"]), L.ptr(c["a2"]), L.ptr(c["rowptr"]), L.ptr(c["col"]), L.ptr(c["m8"]),
        rb, re, c["D"], 0.1, L.ptr_rows(out), out.stride(0), L.ptr(alpha), L.ptr(c["sc"]) if ep else None, L.ptr(c["sh"]) if ep else None,
        1 if ep else 0, None, 0, rb, 1, L.ptr(sums), L.ptr(q), (0 if q is None else q.numel()) if words is None else words, c["n"], 1, L.stream())
    return rc, q


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _once(c, out, sums=None):
    """every row of the range written, no other row touched; with column sums: every row of the range finished exactly once"""
    rb, re = c["rows"]
    ok = bool(torch.isfinite(out[rb:re]).all()) and bool(torch.isnan(out[:rb]).all()) and bool(torch.isnan(out[re:]).all())
    if sums is not None:
        ld, m = c["ld"], c["mask"][rb:re]
        ok = ok and sums[2 * ld].item() == int(m.sum()) and sums[2 * ld + 1].item() == int((~m).sum())
    return ok


def _run_case(case):
    """-> {"out", "alpha_out", "alpha": digests; "sums": column sums; "once": bool; "again", "static": digests of the reruns}"""
    from bridged_gnn_amd import _lib as L
    c = _inputs(case)
    n, ld = c["n"], c["ld"]
    nan = lambda: torch.full((n, ld), float("nan"), device=DEV)
    res = {}
    out, sums = nan(), torch.zeros(2 * ld + 2, dtype=torch.float64, device=DEV)
    rc, q = _launch(c, out, sums=sums)
    L.check(rc, case)
    again, sums2 = nan(), torch.zeros_like(sums)
    L.check(_launch(c, again, sums=sums2, queue=q)[0], case)          # the same queue buffer, straight behind the first launch
    static, sums3 = nan(), torch.zeros_like(sums)
    L.check(_launch(c, static, sums=sums3, queue=None)[0], case)
    aout, alpha = nan(), torch.full((c["n_edges"],), float("nan"), device=DEV)
    L.check(_launch(c, aout, alpha=alpha)[0], case)
    torch.cuda.synchronize()
    e0, e1 = int(c["rowptr"][c["rows"][0]]), int(c["rowptr"][c["rows"][1]])      # the range's edges: written, no other
    res["once"] = (_once(c, out, sums) and _once(c, again, sums2) and _once(c, static, sums3) and _once(c, aout)
                   and bool(torch.isfinite(alpha[e0:e1]).all()) and bool(torch.isnan(alpha[:e0]).all()) and bool(torch.isnan(alpha[e1:]).all()))
    res["out"], res["again"], res["static"] = _digest(out), _digest(again), _digest(static)
    res["alpha_out"], res["alpha"] = _digest(aout), _digest(alpha)
    res["sums"] = [s.cpu().tolist() for s in (sums, sums2, sums3)]
    return res


def _child(path):
    with open(path, "w") as f:
        json.dump({case: _run_case(case) for case in CASES}, f)


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    """results of every case under every schedule of CONFIGS: one child process per schedule, started together"""
    outdir = tmp_path_factory.mktemp("agg_claim")
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    procs = {}
    for name, env in CONFIGS.items():
        procs[name] = subprocess.Popen([sys.executable, "-s", os.path.abspath(__file__), "--child", str(outdir / (name + ".json"))],
                                       env=dict(base, BGNN_AGG_BLOCKS_PER_CU="1", **env), cwd=ROOT, stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    res = {}
    try:
        for name, p in procs.items():
            # a child takes a few seconds (start of torch + 44 launches on graphs of at most 48 k rows); a ring that stops polls for ever
            log, _ = p.communicate(timeout=CHILD_TIMEOUT)
            assert p.returncode == 0, f"schedule {name}: exit code {p.returncode}\n{log[-4000:]}"
            with open(outdir / (name + ".json")) as f:
                res[name] = json.load(f)
    finally:                                              # the first failure or hang ends the other children too
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return res


def _same(got, ref, what):
    for key in ("out", "again", "static", "alpha_out", "alpha"):
        assert got[key] == ref["out" if key in ("again", "static") else key], f"{what}: {key} differs from the reference schedule's bits"
    assert got["once"], f"{what}: a row of the range unwritten or finished twice, or a row outside it touched"
    for s in got["sums"]:
        torch.testing.assert_close(torch.tensor(s, dtype=torch.float64), torch.tensor(ref["sums"][0], dtype=torch.float64), rtol=2e-6, atol=1e-3)


@pytest.mark.parametrize("case", list(CASES))
def test_single_tile_claims_equal_chunk_claims_and_the_general_kernel(case, schedules):
    """tile (NQ = 4, claim ahead), NQ = 1 / 2 / 8 and the synchronous claim against BGNN_AGG_CLAIM=chunk and BGNN_AGG_FAST=0"""
    chunk, general = schedules["chunk"][case], schedules["general"][case]
    _same(chunk, general, f"{case}: chunk vs general")
    for name in ("tile", "nq1", "nq2", "nq8", "sync"):
        _same(schedules[name][case], chunk, f"{case}: {name} vs chunk")
        _same(schedules[name][case], general, f"{case}: {name} vs general")


@pytest.mark.parametrize("case", list(CASES))
def test_the_default_schedule_at_full_occupancy(case, schedules):
    """this process: the library's default claim mode with every block resident that fits"""
    got = _run_case(case)
    _same(got, schedules["chunk"][case], f"{case}: default vs chunk")
    _same(got, schedules["general"][case], f"{case}: default vs general")


def test_a_queue_of_the_old_size_gets_chunk_claims_and_is_never_overrun(schedules):
    """8 words inside a buffer of sentinels: the same bits, the sentinels intact; fewer than 8 words are refused"""
    from bridged_gnn_amd import _lib as L
    case = "tiles1001"
    c = _inputs(case)
    buf = torch.full((4096,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = torch.full((c["n"], c["ld"]), float("nan"), device=DEV)
    sums = torch.zeros(2 * c["ld"] + 2, dtype=torch.float64, device=DEV)
    rc, _ = _launch(c, out, sums=sums, queue=buf[64:72])
    L.check(rc, "a queue of 8 words")
    torch.cuda.synchronize()
    assert _digest(out) == schedules["chunk"][case]["out"] and _once(c, out, sums)
    assert bool((buf[:64] == 0x5A5A5A5A).all()) and bool((buf[72:] == 0x5A5A5A5A).all())
    rc, _ = _launch(c, out, queue=buf[64:72], words=7)
    assert rc == -3                                       # BGNN_E_WORKSPACE
    assert int(L.lib().bgnn_aggregate_tile_queue_words()) >= 8


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2])
