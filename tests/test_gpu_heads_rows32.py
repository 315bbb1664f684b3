"""GPU: the eval classifier stage on 32-byte node rows (C <= 2): agg_heads_rows32_kernel, the producers' stores into such
rows and `KTGNN_no_complement`'s eval forward on them, against the padded 48-byte rows they replace.

The library reads its switches once per process, so every configuration is a fresh child process that runs every case and leaves
SHA-256 digests behind (one module fixture, the children side by side):

  rows32    BGNN_HEADS_ROWS32=1                     32-byte rows where `ops.heads_rows32_plan` takes them, else the padded path
  rows48    BGNN_HEADS_ROWS32=0                     padded rows end to end (agg_heads_fast_kernel where its plan admits the launch)
  general   BGNN_HEADS_FAST=0                       padded rows, agg_heads_lanes_kernel
  waves8    BGNN_HEADS_ROWS32=1 BGNN_CLS_WAVES=8    the producers only, on the eight-wave cls_stage_kernel

Walk: per case the whole `out` buffer ([n, 3, 4], NaN before the launch: rows outside the range stay NaN) must be equal bit for bit
between rows32 and rows48; a case the plan refuses must take the padded path in every child and equal the general kernel.  Two cases
of the rows32 child are also held against an fp64 numpy restatement at the suite's default bar.  Producers: inside one child the
stage fills 32-byte and padded tables from the same inputs; unpacked, the former must equal the latter bit for bit, padding +0
(head 2 on one stage-A result: see `_run_producers`).  Model: the three outputs of the eager and the graphed eval forward on a
2 000-node bridged graph, rows32 against rows48, bit for bit with the forward's domain sums pinned (`_pin_domain_sums` says why).

Shapes: a row is walked by 4 lanes (2 sub-groups x 2 lanes), a wave holds 16 rows, a block 64; a step covers 8 edges of a row."""
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
DEGREES = (0, 1, 7, 8, 9, 16, 17, 40)                   # dead slots, exact and ragged steps of 8


def _case(n, C=2, dom="inter", slope=0.1, graph="mixed", rows=None, place="one", rows32=True):
    return dict(n=n, C=C, dom=dom, slope=slope, graph=graph, rows=rows, place=place, rows32=rows32)


CASES = {f"n{n}_c{C}_{dom}": _case(n, C, dom) for n in (1, 15, 16, 17, 63, 64, 65, 257) for C in (1, 2) for dom in ("inter", "block")}
CASES.update({
    "slope0": _case(257, slope=0.0), "slope1": _case(257, slope=1.0), "slope0_c1": _case(65, C=1, slope=0.0),
    "range": _case(257, rows=(37, 201)), "range_c1": _case(257, C=1, rows=(16, 17)),
    # the last seven rows hold 840 of 1090 edges: the waves of the last 17 rows take their ids as clamped dwords
    "tail_heavy": _case(257, graph="tail"), "tail_heavy_c1": _case(65, C=1, graph="tail"),
    "no_edges": _case(65, graph="none"),
    # refused by the plan: the padded path, which must equal the general kernel
    "refuse_c3": _case(257, C=3, rows32=False), "refuse_c4": _case(257, C=4, rows32=False),
    "refuse_hub": _case(257, graph="hub", rows32=False), "refuse_slope1p5": _case(257, slope=1.5, rows32=False),
    "refuse_two_windows": _case(257, place="far", rows32=False),
})
ACCURACY = ("n257_c2_inter", "n257_c1_block")
CONFIGS = {"rows32": {"BGNN_HEADS_ROWS32": "1"}, "rows48": {"BGNN_HEADS_ROWS32": "0"}, "general": {"BGNN_HEADS_FAST": "0"},
           "waves8": {"BGNN_HEADS_ROWS32": "1", "BGNN_CLS_WAVES": "8"}}
KNOBS = ("BGNN_HEADS_ROWS32", "BGNN_HEADS_FAST", "BGNN_CLS_WAVES", "BGNN_HUB_ROWS")
CHILD_TIMEOUT = 180                                      # seconds; a child takes a few seconds (start of torch + ~60 small launches)
PRODUCERS = [(n, hidden, C) for n in (33, 95, 1025) for hidden in (128, 64) for C in (1, 2)]


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
def _host_inputs(name):
    """the case's arrays on the host (the same in every process): padded tables [2, n, 3, 4] with zeros past column C"""
    c = CASES[name]
    n, C = c["n"], c["C"]
    rng = np.random.default_rng(sum(map(ord, name)))
    if c["graph"] == "none":
        deg = np.zeros(n, dtype=np.int64)
    elif c["graph"] == "tail":
        deg = np.ones(n, dtype=np.int64)
        deg[-7:] = 120
    else:
        deg = rng.permutation(np.resize(np.array(DEGREES[::-1]), n))       # (n = 1: 40 self loops)
        if c["graph"] == "hub":
            deg[n // 2] = 300                            # >= ops.HUB_THRESHOLD: the launch walks it in segments
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    dst = np.repeat(np.arange(n), deg)
    near = np.clip(dst + rng.integers(-16, 17, dst.size), 0, n - 1)
    col = np.where(rng.random(dst.size) < 0.8, near, rng.integers(0, n, dst.size))
    if col.size >= 2:
        col[0], col[-1] = n - 1, 0                       # the table's last and first node are walked
    tabs = np.zeros((2, n, 3, 4), dtype=np.float32)
    tabs[..., :C] = rng.standard_normal((2, n, 3, C))
    mask = (np.arange(n) % 2 == 0) if c["dom"] == "inter" else (np.arange(n) < (n + 1) // 2)
    return dict(c, rows=c["rows"] if c["rows"] is not None else (0, n), rowptr=rowptr.astype(np.int32), col=col.astype(np.int32),
                tabs=tabs.reshape(2, n, 12), mask=mask, a=(rng.standard_normal((2, 3, C)) * 0.5).astype(np.float32))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _place(both, how):
    """[2, n, w] on the device -> (t2s, s2t, keep): one allocation, or more than 4 GB between the two tables"""
    if how == "one":
        return both[0], both[1], both
    n, w = both.shape[1:]
    gap = ((1 << 32) + (1 << 20)) // 4                   # floats
    big = torch.empty(gap + n * w, dtype=torch.float32, device=DEV)
    t2s, s2t = big[:n * w].view(n, w), big[gap:].view(n, w)
    t2s.copy_(both[0]); s2t.copy_(both[1])
    return t2s, s2t, big


def _run_walk(name, keep_out=None):
    """-> {"out": digest, "once": bool, "rows32": which path ran} or {"skipped": reason}"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.classifier_stage import ClassifierStage
    c = _host_inputs(name)
    n, C, (rb, re) = c["n"], c["C"], c["rows"]
    col = _t(c["col"]) if c["col"].size else torch.zeros(1, dtype=torch.int32, device=DEV)       # (no edge: one unread id, never NULL)
    csr = ops.DstCSR(_t(c["rowptr"]), col, None, c["col"].size, n)
    m8, a, tabs = _t(c["mask"].astype(np.uint8)), _t(c["a"]), _t(c["tabs"])
    out = torch.full((n, 12), float("nan"), device=DEV)
    took32 = False
    try:
        if C <= 2:
            t8 = torch.stack((ClassifierStage.rows32_pack(tabs[0]), ClassifierStage.rows32_pack(tabs[1])))
            t2s, s2t, keep = _place(t8, c["place"])
            took32 = ops.heads_rows32_plan(t2s, s2t, csr, C, c["slope"], row_end=re)
        if took32:
            ops.adaptedconv_aggregate_heads_rows32(t2s, s2t, a[0], a[1], csr, m8, C, c["slope"], log_softmax=True, row_begin=rb, row_end=re, out=out)
        else:
            t2s, s2t, keep = _place(tabs, c["place"])
            ops.adaptedconv_aggregate(t2s, s2t, a[0], a[1], csr, m8, C, c["slope"], heads=3, log_softmax=True, row_begin=rb, row_end=re, out=out)
    except torch.OutOfMemoryError as e:
        return {"skipped": f"no room for the tables of {name}: {str(e)[:120]}"}
    torch.cuda.synchronize()
    once = bool(torch.isfinite(out[rb:re]).all()) and bool(torch.isnan(out[:rb]).all()) and bool(torch.isnan(out[re:]).all())
    if keep_out is not None:
        np.save(keep_out, out.cpu().numpy())
    del keep
    return {"out": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), "once": once, "rows32": bool(took32)}


# ---- the producers ----------------------------------------------------------------------------------------------------------------------
def _model(hidden, C, seed):
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    torch.manual_seed(seed)
    model = KTGNN_no_complement(32, C, 2, hidden, use_bn=True, dim_share=32).to(DEV).eval()
    with torch.no_grad():                                # non-trivial BatchNorm statistics
        for bn in list(model.bns) + [model.clf_transformer[1]]:
            bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.normal_(1, 0.2); bn.bias.normal_(0, 0.2)
    return model


def _run_producers(n, hidden, C):
    """the stage's tables of one activation in both layouts -> {"took32", "equal", "pad_zero"}"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.classifier_stage import ClassifierStage
    stage = _model(hidden, C, 7 * n + hidden + C)._stage
    rng = np.random.default_rng(n + hidden)
    x, m8 = _t(rng.standard_normal((n, hidden)).astype(np.float32)), _t((rng.random(n) < 0.45).astype(np.uint8))
    loops = torch.arange(n, dtype=torch.int32, device=DEV)
    csr = ops.DstCSR(torch.arange(n + 1, dtype=torch.int32, device=DEV), loops, None, n, n)        # (the plan looks for hub rows)
    bits = lambda t: t.contiguous().view(torch.int32)
    with torch.no_grad():
        sums = ops.domain_sums(x, m8)
        t2s = torch.full((n, 12), float("nan"), device=DEV)
        s2t = torch.full((n, 12), float("nan"), device=DEV)
        views = stage.views(t2s, s2t)
        a = stage.one_pass(x, m8, sums, views, None)
        tabs = stage.eval_tables_rows32(x, m8, sums, csr, None)
        if a is None or tabs is None:
            torch.cuda.synchronize()
            return {"took32": tabs is not None, "one_pass": a is not None}
        stage.target_stage_b(a, m8, views[2])
        # Head 2 needs the domain sums of the transformer's activation, which every one-pass launch accumulates anew through
        # floating-point atomics (their last bits vary from launch to launch): its bits are compared on ONE stage-A result, finished
        # into both layouts; the stage's own second launch is held to the padded table at 1e-5
        again = [t.clone() for t in tabs]
        stage.target_stage_b(a, m8, ClassifierStage.rows32_views(*again)[2], rows32=True)
    torch.cuda.synchronize()
    pads = (t2s, s2t)
    heads01 = all(torch.equal(bits(ClassifierStage.rows32_unpack(t8))[:, :8], bits(t48)[:, :8]) for t8, t48 in zip(tabs, pads))
    head2 = all(torch.equal(bits(ClassifierStage.rows32_unpack(t8)), bits(t48)) for t8, t48 in zip(again, pads))
    own = all(torch.allclose(t8[:, 4:8], t48[:, 8:12], rtol=1e-5, atol=1e-6) for t8, t48 in zip(tabs, pads))
    pad_zero = all(bool((bits(t8[:, 6:8]) == 0).all()) and (C == 2 or bool((bits(t8[:, 1:6:2]) == 0).all())) for t8 in list(tabs) + again)
    return {"took32": True, "one_pass": True, "equal": heads01 and head2, "own_sums_close": own, "pad_zero": pad_zero}


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def _pin_domain_sums(model):
    """The forward forms three sets of domain sums through floating-point atomics (of the input, of the hidden activation, of the
    transformer's activation), and the order of those atomics moves their last bits from launch to launch: the padded forward does
    not repeat its own output bits either (measured: four forwards of one process, four digests per output, in either layout).
    Both children therefore overwrite each of the three with the atomic-free two-stage sums (`domain_sums(deterministic=True)`) of
    the same rows, so that the comparison sees the layouts and nothing else."""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.ktgnn import _as_u8
    stage, hidden, one_pass = model._stage, model._hidden, model._stage.one_pass
    exact = lambda x, m8: ops.domain_sums(x.contiguous(), m8, deterministic=True)
    model._input_domain_sums = lambda x, central_mask, arena: exact(x, _as_u8(central_mask).contiguous())

    def hidden_pinned(x, csr, central_mask, want_sums=False, arena=None):
        h, sums = hidden(x, csr, central_mask, want_sums=True, arena=arena)
        sums.copy_(exact(h, _as_u8(central_mask).contiguous()))
        return (h, sums) if want_sums else h

    def one_pass_pinned(x, mask_u8, *args, **kwargs):
        a = one_pass(x, mask_u8, *args, **kwargs)
        a[2].copy_(exact(stage.transformer_hidden_eval(x), mask_u8))
        return a
    model._hidden, stage.one_pass = hidden_pinned, one_pass_pinned


def _run_model():
    """-> digests of the three outputs, eager and graphed, and whether the forward built 32-byte rows"""
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.data import Data
    ei, mask = synth.bridged_graph(1000, 1000, k_within=4, k_cross=8, n_extra=1500, cluster=128, seed=11)
    model = _model(128, 2, 5)
    _pin_domain_sums(model)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2000, 32)).astype(np.float32)).to(DEV)
    data = Data(x=x, edge_index=_t(ei), central_mask=_t(mask))
    calls = []
    walk = ops.adaptedconv_aggregate_heads_rows32
    ops.adaptedconv_aggregate_heads_rows32 = lambda *a, **k: (calls.append(1), walk(*a, **k))[1]
    sha = lambda ts: [hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest() for t in ts[:3]]
    try:
        with torch.no_grad():
            eager = sha(model(data))
        n_eager = len(calls)
        graphed = sha(model.graphed(data)())
    finally:
        ops.adaptedconv_aggregate_heads_rows32 = walk
    torch.cuda.synchronize()
    return {"eager": eager, "graphed": graphed, "rows32": n_eager == 1}


def _child(outdir, name):
    res = {}
    if name != "waves8":
        res["walk"] = {case: _run_walk(case, os.path.join(outdir, case + ".npy") if name == "rows32" and case in ACCURACY else None)
                       for case in CASES}
        res["model"] = _run_model()
    if name in ("rows32", "waves8"):
        res["producers"] = {f"{n}-{h}-{C}": _run_producers(n, h, C) for n, h, C in PRODUCERS}
    with open(os.path.join(outdir, name + ".json"), "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{config: what its child left, "dir": where the rows32 child left the accuracy cases' outputs}"""
    outdir = tmp_path_factory.mktemp("heads_rows32")
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    procs = {name: subprocess.Popen([sys.executable, "-s", os.path.abspath(__file__), "--child", str(outdir), name], env=dict(base, **env),
                                    cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for name, env in CONFIGS.items()}
    res = {"dir": str(outdir)}
    try:
        for name, p in procs.items():
            log, _ = p.communicate(timeout=CHILD_TIMEOUT)
            assert p.returncode == 0, f"{name} child: exit code {p.returncode}\n{log[-4000:]}"
            with open(outdir / (name + ".json")) as f:
                res[name] = json.load(f)
    finally:                                             # the first failure ends the other children too
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_walk_on_32_byte_rows_equals_the_padded_walk_bit_for_bit(case, runs):
    got = {name: runs[name]["walk"][case] for name in ("rows32", "rows48", "general")}
    for r in got.values():
        if "skipped" in r:
            pytest.skip(r["skipped"])
    for name, r in got.items():
        assert r["once"], f"{case}: the {name} walk left a row of the range unwritten or touched a row outside it"
    assert got["rows32"]["rows32"] == CASES[case]["rows32"], f"{case}: the plan's answer"
    assert not got["rows48"]["rows32"] and not got["general"]["rows32"], f"{case}: a switched-off child walked 32-byte rows"
    assert got["rows32"]["out"] == got["rows48"]["out"], f"{case}: 32-byte and padded rows differ in some bit of `out`"
    assert got["rows32"]["out"] == got["general"]["out"], f"{case}: differs from the general kernel in some bit of `out`"


def _walk_fp64(c):
    """the walk restated in fp64 numpy: per (row, head) a softmax over the in-edges of a . leaky_relu(h_j + h_i) on the C real
    columns, the weighted sum of the neighbours' columns over (sum + 1e-16), then log_softmax over the C columns"""
    n, C, slope = c["n"], c["C"], c["slope"]
    rowptr, col, mask = c["rowptr"].astype(np.int64), c["col"].astype(np.int64), c["mask"]
    tabs = c["tabs"].astype(np.float64).reshape(2, n, 3, 4)
    a = np.zeros((2, 3, 4))
    a[:, :, :C] = c["a"]
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    dom = np.where(mask, 0, 1)                           # a source-domain row reads the t2s table (the first) and a_t2s
    hj, hi = tabs[dom[dst], col], tabs[dom[dst], dst]    # [E, 3, 4]
    z = hj + hi
    z = np.where(z > 0, z, z * slope)
    logit = (a[dom[dst]] * z).sum(-1)                    # [E, 3]
    mx = np.full((n, 3), -np.inf)
    np.maximum.at(mx, dst, logit)
    w = np.exp(logit - mx[dst])
    s = np.zeros((n, 3))
    np.add.at(s, dst, w)
    acc = np.zeros((n, 3, 4))
    np.add.at(acc, dst, w[:, :, None] * hj)
    r = acc / (s + 1e-16)[:, :, None]
    x = r[:, :, :C]
    xm = x.max(-1, keepdims=True)
    r[:, :, :C] = x - xm - np.log(np.exp(x - xm).sum(-1, keepdims=True))
    r[:, :, C:] = 0.0
    return r.reshape(n, 12)


@pytest.mark.parametrize("case", ACCURACY)
def test_walk_on_32_byte_rows_against_the_fp64_restatement(case, runs):
    from conftest import assert_close
    c = _host_inputs(case)
    got = np.load(os.path.join(runs["dir"], case + ".npy"))
    assert_close(got, _walk_fp64(c), what=case)


@pytest.mark.parametrize("waves", ("rows32", "waves8"))
@pytest.mark.parametrize("n,hidden,C", PRODUCERS)
def test_producers_write_the_padded_tables_values_into_32_byte_rows(n, hidden, C, waves, runs):
    """hidden 128: the one-pass producer's envelope, both layouts are built and compared.  hidden 64 lies outside it (the stage
    then transforms x with kernels that only know padded rows): the stage must decline 32-byte rows.  These row counts run the
    four-wave cls_stage_kernel by default and the eight-wave one in the waves8 child; the eight-wave instantiation for Din < 128
    shares the epilogue's source and cannot be reached through a stage (the transformer is hidden x hidden)"""
    r = runs[waves]["producers"][f"{n}-{hidden}-{C}"]
    assert r["took32"] == r["one_pass"] == (hidden == 128)
    if r["took32"]:
        assert r["equal"], "a 32-byte table, unpacked, differs from the padded table in some bit"
        assert r["own_sums_close"], "head 2 of the stage's own 32-byte tables is not the padded table's"
        assert r["pad_zero"], "padding of a 32-byte row is not +0"


@pytest.mark.parametrize("how", ("eager", "graphed"))
def test_model_forward_on_32_byte_rows_equals_the_padded_forward_bit_for_bit(how, runs):
    new, old = runs["rows32"]["model"], runs["rows48"]["model"]
    assert new["rows32"] and not old["rows32"], "which layout the forward built"
    assert new[how] == old[how], f"{how} forward: an output differs in some bit between 32-byte and padded rows"


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2], sys.argv[3])
