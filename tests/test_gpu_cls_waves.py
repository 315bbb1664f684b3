"""GPU: the two instantiations of `cls_stage_kernel` side by side -- four waves per block (one per SIMD) and eight (two per SIMD),
forced with BGNN_CLS_WAVES=4 | 8.  A wave owns whole 32-row tiles in both, and the operands, the order of the MFMAs per accumulator
and every conversion are the same, so `raw` and every skinny table must agree in every bit; only the column sums, which go through
floating-point atomics, may differ in their last bits, and those are held to the bar of tests/test_gpu_classifier_stage.py against
its fp64 restatement.

The switch is read by the library, so each value runs in a fresh child process: one child per value for all cases (inputs from the
builders of tests/test_gpu_classifier_stage.py), which leaves the SHA-256 of `raw` and of every table buffer (guard rows included)
and the column sums behind.  A third child runs under a value the switch does not know."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_classifier_stage as S

gpu = pytest.mark.gpu
EXTRA = 37                        # rows behind the kernel's rows that only the domain sums see: both domains exist even where the kernel's rows have one

# (Din, N, heads, D, relu, mask): N "W" = 32 * 8 * n_cu + 5 rows = 8 * n_cu + 1 tiles -- one wave of the eight-wave grid takes a second
# trip through the tile loop (the four-wave grid: every wave two, one a third), the last tile is ragged.  Din 128 runs the instantiation
# compiled for full rows, 68 and 100 the general one.  Masks: every kernel row source, every kernel row target, alternating.
CASES = (
    (128, 1, 2, 2, 1, "source"), (100, 1, 1, 9, 1, "alt"), (68, 31, 1, 4, 0, "target"), (100, 32, 2, 2, 0, "alt"), (128, 32, 1, 7, 0, "source"),
    (128, 33, 1, 9, 1, "target"), (68, 33, 2, 1, 1, "target"), (68, 4099, 2, 2, 1, "alt"), (100, 4099, 1, 12, 1, "source"),
    (128, 4099, 2, 2, 0, "alt"), (128, "W", 2, 2, 1, "alt"), (100, "W", 1, 9, 0, "target"), (68, "W", 2, 2, 0, "source"),
    (128, "W", 1, 4, 1, "source"),
)
UNKNOWN_CASES = (0, 3, 9)         # what the child under an unknown value runs
IDS = [f"din{c[0]}-n{c[1]}-h{c[2]}xD{c[3]}-relu{c[4]}-{c[5]}" for c in CASES]


def _resolve_n(ntok):
    return 32 * 8 * S._n_cu() + 5 if ntok == "W" else int(ntok)


def _case(i):
    din, ntok, heads, D, relu, mk = CASES[i]
    n = _resolve_n(ntok)
    case = S.make_case(din, n, heads, D, relu, ("tight", "inter")[i % 2], "one_source", bool(i % 3 == 0), 1 + i % 4, extra=EXTRA, seed=300 + i)
    m = case["m"]
    m[:n] = {"source": torch.ones(n, dtype=torch.bool), "target": torch.zeros(n, dtype=torch.bool), "alt": torch.arange(n) % 2 == 0}[mk]
    assert bool(m[n:].any()) and not bool(m[n:].all())
    case["sums_x"] = S.domain_sums64(case["x"], m)
    return case


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _zero_heads_rc():
    """the C entry with sk_heads = 0 (it admits 1 or 2): return code, and whether `raw` was left alone"""
    from bridged_gnn_amd import _lib, ops
    case = _case(0)
    n, din = case["n"], case["din"]
    x, m8 = case["x"][:n].to(S.DEV).contiguous(), case["m"][:n].to(S.DEV, torch.uint8)
    pair = ops.pack_transform_heads([S.dev_head(h) for h in case["heads"]], din)
    pack_t = ops.pack_transform_heads([S.dev_head(case["head2"])], 128)
    outs, _ = S._tables(n, 2, pair[4], "tight")
    raw = S.sentinel(n, 12)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    Wp, bp, gates, D, ldh, gconst = pair
    rc = _lib.lib().bgnn_classifier_stage_f32(p(x), n, din, din, p(m8), p(case["sums_x"].to(S.DEV)), 0, D, p(Wp), p(bp), p(gates), p(gconst),
                                              p(outs[0][1]), p(outs[0][0]), p(outs[1][1]), p(outs[1][0]), ldh, ldh, p(case["W"].to(S.DEV)),
                                              p(case["bias"].to(S.DEV)), 128, 1, p(torch.zeros(258, dtype=torch.float64, device=S.DEV)),
                                              p(pack_t[0]), p(pack_t[2]), p(raw), p(torch.empty(64, device=S.DEV)), _lib.stream())
    torch.cuda.synchronize()
    return int(rc), bool(S.untouched(raw))


def _child(out, which):
    res = {}
    for i in which:
        case = _case(i)
        r = S.run_stage(case)
        res[str(i)] = {"raw": _sha(r["raw"]), "tables": [_sha(b) for b in r["bufs"]], "colsum": r["colsum"].cpu().tolist()}
        S.check_guards(case, r, f"case {i}")
    res["zero_heads"] = _zero_heads_rc()
    with open(out, "w") as f:
        json.dump(res, f)


def _run_child(tmp, value, which):
    out = os.path.join(tmp, f"waves_{value}.json")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--child", out, ",".join(map(str, which))],
                       env=dict(os.environ, BGNN_CLS_WAVES=value), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"BGNN_CLS_WAVES={value}:\n{r.stdout[-4000:]}"
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cls_waves"))
    return {v: _run_child(tmp, v, range(len(CASES))) for v in ("4", "8")}


@gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_four_and_eight_waves_agree(runs, i):
    """`raw` and every table buffer bit for bit (SHA-256); the column sums and node counts of both against fp64 at the bar
    `check_colsum` of tests/test_gpu_classifier_stage.py sets (1e-6 relative + 1e-6 of the largest sum; counts exact)."""
    a, b = runs["4"][str(i)], runs["8"][str(i)]
    assert a["raw"] == b["raw"], "raw differs between the four- and the eight-wave kernel"
    assert a["tables"] == b["tables"], "a skinny table differs between the four- and the eight-wave kernel"
    case = _case(i)
    ref = S.reference(case, S.DEV)
    for v, r in (("4", a), ("8", b)):
        S.check_colsum(case, {"colsum": torch.tensor(r["colsum"], dtype=torch.float64, device=S.DEV)}, ref, f"BGNN_CLS_WAVES={v} case {i}")


@gpu
def test_zero_heads_is_refused_alike(runs):
    """sk_heads = 0 is outside what the C entry admits: the same refusal under both values, and nothing is written"""
    assert runs["4"]["zero_heads"] == runs["8"]["zero_heads"]
    rc, clean = runs["4"]["zero_heads"]
    assert rc < 0 and clean


@gpu
def test_unknown_value_is_the_default(runs, tmp_path):
    """a value the switch does not know: no error, and (either kernel giving the same bits) the outputs of the known values"""
    got = _run_child(str(tmp_path), "6", UNKNOWN_CASES)
    for i in UNKNOWN_CASES:
        assert got[str(i)]["raw"] == runs["4"][str(i)]["raw"] and got[str(i)]["tables"] == runs["4"][str(i)]["tables"]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        _child(sys.argv[2], [int(v) for v in sys.argv[3].split(",")])
