"""GPU: agg_heads_fast_kernel, the narrow multi-head walk's plain launch (bgnn_adaptedconv_aggregate_queued_f32).

The library reads BGNN_HEADS_FAST once per process, so the two walks run in a child process each, every case in each child, the
children side by side (one module fixture):

  fast      (default)            agg_heads_fast_kernel where heads_fast_plan admits the launch
  general   BGNN_HEADS_FAST=0    agg_heads_lanes_kernel

Per case the whole `out` buffers must be equal bit for bit (compared as SHA-256, rows outside the range included).  `out` starts
as NaN: every row of the range ends finite and every other row NaN.  Two cases of the default child are also checked against an
fp64 numpy restatement of the walk at the suite's default bar, so that the two kernels cannot be wrong together.

Shapes: a row group is EP * heads = 6 (4) lanes, a wave holds 10 (16) of them and a block 40 (64) rows at heads = 3 (2); a step
covers EP * U = 8 edges of a row."""
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


def _case(n, heads=3, D=2, ep=2, graph="mixed", rows=None, place="one", slope=0.1):
    return dict(n=n, heads=heads, D=D, ep=ep, graph=graph, rows=rows, place=place, slope=slope)


CASES = {
    # tile edges: fewer rows than one wave's groups (most blocks of the minimum grid of 8 stay empty), one block + 1 row, many blocks
    "h3_rows7": _case(7), "h3_rows41": _case(41), "h3_rows3001": _case(3001),
    "h2_rows7": _case(7, heads=2), "h2_rows65": _case(65, heads=2), "h2_rows3001": _case(3001, heads=2),
    # 1, 8, 9 and 130 in-edges inside every wave: rows that end many steps before their wave does
    "h3_skew": _case(1200, graph="skew"), "h2_skew": _case(1200, heads=2, graph="skew"),
    # a row range off the tile boundaries inside a larger table (table_rows > row_end)
    "h3_range": _case(3001, rows=(1003, 2702)), "h2_range": _case(3001, heads=2, rows=(1003, 2702)),
    # column counts, with the fused log-softmax (ep_relu = 2) and without an epilogue
    "h3_d1_ls": _case(1003, D=1), "h3_d3_ls": _case(1003, D=3), "h3_d4_ls": _case(1003, D=4),
    "h3_d1": _case(1003, D=1, ep=0), "h3_d2": _case(1003, D=2, ep=0), "h3_d3": _case(1003, D=3, ep=0), "h3_d4": _case(1003, D=4, ep=0),
    "h2_d2": _case(1003, heads=2, ep=0),
    # table placement: one allocation with the t2s table on top, two allocations, a window of more than 2^31 bytes
    "h3_swapped": _case(1003, place="swapped"), "h3_separate": _case(1003, place="separate"), "h2_separate": _case(1003, heads=2, place="separate"),
    "h3_far": _case(1003, place="far"),
    # slopes: the ends of the plan's interval, and one outside it (both children then run the general kernel)
    "h3_slope0": _case(1003, slope=0.0), "h3_slope1": _case(1003, slope=1.0), "h2_slope0": _case(1003, heads=2, slope=0.0),
    "h3_slope1p5": _case(1003, slope=1.5),
}
ACCURACY = ("h3_rows3001", "h2_rows3001")                # D = 2 with both head counts: the default child keeps their `out`
CONFIGS = {"fast": {}, "general": {"BGNN_HEADS_FAST": "0"}}
CHILD_TIMEOUT = 120                                      # seconds; a child takes a few seconds (start of torch + 26 small launches)
KNOBS = ("BGNN_HEADS_FAST",)


def _graph(kind, n, rng):
    """-> (rowptr, col) int32 by destination, the degrees.  mixed: 0, 1, 7, 8, 9, 16 and 17 in-edges (an empty row, the multiples of
    a step's 8 slots and +-1), with whole waves of empty rows"""
    if kind == "skew":
        deg = np.tile(np.array([1, 8, 9, 130, 1, 8, 9, 130, 8, 1]), (n + 9) // 10)[:n]
    else:
        deg = rng.choice(np.array([0, 1, 7, 8, 9, 16, 17]), n)
        if n > 400:
            deg[64:192] = 0                              # 128 rows: whole waves (10 / 16 rows) and blocks (40 / 64 rows) without an edge
            deg[-3:] = 0
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    dst = np.repeat(np.arange(n), deg)
    near = np.clip(dst + rng.integers(-64, 65, dst.size), 0, n - 1)
    col = np.where(rng.random(dst.size) < 0.8, near, rng.integers(0, n, dst.size))
    return rowptr.astype(np.int32), col.astype(np.int32), deg


def _host_inputs(case):
    """the case's arrays on the host (the same in every process)"""
    c = CASES[case]
    n, heads = c["n"], c["heads"]
    rng = np.random.default_rng(sum(map(ord, case)))
    rows = c["rows"] if c["rows"] is not None else (0, n)
    last = rows[1] - 1
    rowptr, col, deg = _graph(c["graph"], n, rng)
    if deg[last] < 2:                                    # the last row of the range walks node 0 and the table's last node
        deg[last] = 9
        rowptr = np.zeros(n + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(deg)
        rowptr = rowptr.astype(np.int32)
        dst = np.repeat(np.arange(n), deg)
        col = np.clip(dst + rng.integers(-64, 65, dst.size), 0, n - 1).astype(np.int32)
    col[rowptr[last]], col[rowptr[last] + 1] = 0, n - 1
    tabs = rng.standard_normal((2, n, heads * 4)).astype(np.float32)       # (the padded columns carry values too: a_* ignores them)
    return dict(c, rows=rows, rowptr=rowptr, col=col, tabs=tabs, mask=rng.random(n) < 0.45,
                a=(rng.standard_normal((2, heads, c["D"])) * 0.5).astype(np.float32))


def _place(tabs, how):
    """-> (tS, tT, keep) on the device, or raises torch.OutOfMemoryError (far: 2.5 GB between the tables)"""
    n, ld = tabs.shape[1:]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if how == "separate":
        spacer = torch.empty(3 << 20, dtype=torch.uint8, device=DEV)
        return t(tabs[0]), t(tabs[1]), spacer
    if how == "far":
        gap = (5 << 29) // 4                             # 2.5 GB in floats
        big = torch.empty(gap + n * ld, dtype=torch.float32, device=DEV)
        tS, tT = big[:n * ld].view(n, ld), big[gap:].view(n, ld)
        tS.copy_(t(tabs[0])); tT.copy_(t(tabs[1]))
        assert (1 << 31) < tT.data_ptr() - tS.data_ptr() + n * ld * 4 < (1 << 32)
        return tS, tT, big
    both = t(tabs if how == "one" else tabs[::-1])
    return (both[0], both[1], both) if how == "one" else (both[1], both[0], both)


def _run_case(case, keep_out=None):
    """-> {"out": digest, "once": bool} or {"skipped": reason}"""
    from bridged_gnn_amd import _lib as L
    c = _host_inputs(case)
    n, heads = c["n"], c["heads"]
    try:
        tS, tT, keep = _place(c["tabs"], c["place"])
    except torch.OutOfMemoryError as e:
        return {"skipped": f"no room for the tables of {case}: {str(e)[:120]}"}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rowptr, col, m8, a = t(c["rowptr"]), t(c["col"]), t(c["mask"].astype(np.uint8)), t(c["a"])
    out = torch.full((n, heads * 4), float("nan"), device=DEV)
    rb, re = c["rows"]
    rc = L.lib().bgnn_adaptedconv_aggregate_queued_f32(
        L.ptr_rows(tS), L.ptr_rows(tT), 4, L.ptr(a[0]), L.ptr(a[1]), L.ptr(rowptr), L.ptr(col), L.ptr(m8),
        rb, re, c["D"], c["slope"], L.ptr_rows(out), 4, None, None, None, c["ep"], None, 0, rb, heads, None, None, 0, n, 0, L.stream())
    L.check(rc, case)
    torch.cuda.synchronize()
    once = bool(torch.isfinite(out[rb:re]).all()) and bool(torch.isnan(out[:rb]).all()) and bool(torch.isnan(out[re:]).all())
    if keep_out is not None:
        np.save(keep_out, out.cpu().numpy())
    del keep
    return {"out": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), "once": once}


def _child(outdir, name):
    res = {case: _run_case(case, os.path.join(outdir, case + ".npy") if name == "fast" and case in ACCURACY else None) for case in CASES}
    with open(os.path.join(outdir, name + ".json"), "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    """{"fast": {case: result}, "general": {...}, "dir": where the default child left the accuracy cases' outputs}"""
    outdir = tmp_path_factory.mktemp("heads_fast")
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    procs = {name: subprocess.Popen([sys.executable, "-s", os.path.abspath(__file__), "--child", str(outdir), name], env=dict(base, **env),
                                    cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for name, env in CONFIGS.items()}
    res = {"dir": str(outdir)}
    try:
        for name, p in procs.items():
            log, _ = p.communicate(timeout=CHILD_TIMEOUT)
            assert p.returncode == 0, f"{name} walk: exit code {p.returncode}\n{log[-4000:]}"
            with open(outdir / (name + ".json")) as f:
                res[name] = json.load(f)
    finally:                                             # the first failure ends the other child too
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_fast_walk_equals_the_general_walk_bit_for_bit(case, walks):
    fast, general = walks["fast"][case], walks["general"][case]
    for r in (fast, general):
        if "skipped" in r:
            pytest.skip(r["skipped"])
    assert fast["once"], f"{case}: fast walk left a row of the range unwritten or touched a row outside it"
    assert general["once"], f"{case}: general walk left a row of the range unwritten or touched a row outside it"
    assert fast["out"] == general["out"], f"{case}: the two walks differ in some bit of `out`"


def _walk_fp64(c):
    """the walk restated in fp64 numpy: per (row, head) a softmax over the in-edges of a . leaky_relu(h_j + h_i) on the first D
    columns, the weighted sum of the neighbours' four columns over (sum + 1e-16), then log_softmax over the D columns (ep = 2)"""
    n, heads, D, slope = c["n"], c["heads"], c["D"], c["slope"]
    rowptr, col, mask = c["rowptr"].astype(np.int64), c["col"].astype(np.int64), c["mask"]
    tabs = c["tabs"].astype(np.float64).reshape(2, n, heads, 4)
    a = np.zeros((2, heads, 4))
    a[:, :, :D] = c["a"]
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    dom = np.where(mask, 0, 1)                           # a source-domain row reads the t2s table (the first) and a_t2s
    hj, hi = tabs[dom[dst], col], tabs[dom[dst], dst]    # [E, heads, 4]
    z = hj + hi
    z = np.where(z > 0, z, z * slope)
    logit = (a[dom[dst]] * z).sum(-1)                    # [E, heads]
    mx = np.full((n, heads), -np.inf)
    np.maximum.at(mx, dst, logit)
    w = np.exp(logit - mx[dst])
    s = np.zeros((n, heads))
    np.add.at(s, dst, w)
    acc = np.zeros((n, heads, 4))
    np.add.at(acc, dst, w[:, :, None] * hj)
    r = acc / (s + 1e-16)[:, :, None]
    if c["ep"] == 2:
        x = r[:, :, :D]
        xm = x.max(-1, keepdims=True)
        r[:, :, :D] = x - xm - np.log(np.exp(x - xm).sum(-1, keepdims=True))
        r[:, :, D:] = 0.0
    return r.reshape(n, heads * 4)


@pytest.mark.parametrize("case", ACCURACY)
def test_default_walk_against_the_fp64_restatement(case, walks):
    from conftest import assert_close
    c = _host_inputs(case)
    got = np.load(os.path.join(walks["dir"], case + ".npy"))
    rb, re = c["rows"]
    assert_close(got[rb:re], _walk_fp64(c)[rb:re], what=case)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2], sys.argv[3])
