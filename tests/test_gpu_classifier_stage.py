"""GPU: `ops.classifier_stage` (bgnn_classifier_stage_f32, cls_stage_kernel) at its own interface against an fp64 restatement of
KTGNN.py:275-284 / :432-434 written here in plain torch float64 -- every input width, head count and padded head width that
`bgnn_tf_cls_supported` admits, ragged and uneven tile counts, both table layouts, guard regions, the `raw` rows, the column
sums and the hand-over to stage B.  The one test without the gpu mark checks that restatement against the C oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import oracle_c as OC

DEV = "cuda:0"
gpu = pytest.mark.gpu
SENTINEL = 0x7FA5C3E1            # a NaN with a payload: "untouched" is a statement about bits, never about float equality
GUARD = 32                       # sentinel rows behind row N of every table


# ---------------------------------------------------------------------------------------------------- fp64 reference
def ref_transform(x, m, sums, head):
    """(h_s2t, h_t2s) of one conv on the rows x [N, Din] (float64), domain flags m (bool, True = source), with the domain-mean
    difference taken from `sums` = (source column sums | target column sums | n_S | n_T), the vector the kernels get."""
    din = x.shape[1]
    f = lambda k: head[k].to(x.device, torch.float64)
    delta = sums[:din] / sums[2 * din] - sums[din: 2 * din] / sums[2 * din + 1]
    c0, c1 = (float(v) for v in head["gate_const"]) if head.get("gate_const") is not None else (0.0, 0.0)
    g1, g2 = f("g_s2t"), f("g_t2s")
    gate_s = torch.tanh(x @ g1[:din] + delta @ g1[din:] + c0)
    gate_t = torch.tanh(x @ g2[:din] + delta @ g2[din:] + c1)
    W_t, W_s = f("W_t"), f("W_s")
    md = m.to(torch.float64)
    h_s2t = x @ W_t.T + f("b_t") - (md * gate_s)[:, None] * (W_t @ delta)[None, :]
    h_t2s = x @ W_s.T + f("b_s") + ((1.0 - md) * gate_t)[:, None] * (W_s @ delta)[None, :]
    return h_s2t, h_t2s


def ref_stage_a(x, m, W, bias, relu, head2):
    """activation a and raw [N, 12] of the one-pass stage, float64"""
    a = x @ W.to(x.device, torch.float64).T + bias.to(x.device, torch.float64)
    if relu:
        a = torch.clamp_min(a, 0.0)
    dout = a.shape[1]
    f = lambda k: head2[k].to(x.device, torch.float64)
    D2 = head2["W_t"].shape[0]
    raw = torch.zeros(x.shape[0], 12, dtype=torch.float64, device=x.device)
    raw[:, 0:D2] = a @ f("W_t").T                       # Wp2[0:4] = W_t zero padded to 4 rows
    raw[:, 4:4 + D2] = a @ f("W_s").T                   # Wp2[4:8] = W_s
    raw[:, 8] = a @ f("g_s2t")[:dout]                   # gates2[0, :128]
    raw[:, 9] = a @ f("g_t2s")[:dout]                   # gates2[1, :128]
    return a, raw


def domain_sums64(x, m):
    x = x.to(torch.float64)
    return torch.cat((x[m].sum(0), x[~m].sum(0), torch.tensor([float(m.sum()), float((~m).sum())], dtype=torch.float64)))


# ---------------------------------------------------------------------------------------------------- cases
def make_head(g, D, din, gate_const):
    r = lambda *s: torch.randn(*s, generator=g)
    return {"W_s": r(D, din) / math.sqrt(din), "W_t": r(D, din) / math.sqrt(din), "b_s": r(D) * 0.5, "b_t": r(D) * 0.5,
            "g_s2t": r(2 * din) * (0.7 / math.sqrt(din)), "g_t2s": r(2 * din) * (0.7 / math.sqrt(din)),
            "gate_const": (0.3, -0.2) if gate_const else None}


def make_case(din, n, heads, D, relu, layout, maskkind, gconst, D2, extra=0, seed=0, magnitudes=False, dout=128):
    """Host tensors of one call.  The kernel sees rows [0, n); `extra` further rows exist only in the domain sums (a rank's share of
    a partition).  The two domains differ by a fixed offset so that the rank-1 domain shift is as large as the linear term."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * din + n % 9973 + 13 * D + heads)
    na = n + extra
    if maskkind == "rand":
        m = torch.rand(na, generator=g) < 0.45
    else:                                              # all rows but one in one domain
        m = torch.full((na,), maskkind == "one_target", dtype=torch.bool)
        m[int(torch.randint(0, n, (1,), generator=g))] = maskkind != "one_target"
        if extra:
            m[n:] = torch.rand(extra, generator=g) < 0.5
    if extra:
        m[na - 1], m[na - 2] = True, False
    elif bool(m.all()) or not bool(m.any()):           # (cannot happen for n >= 2 with the kinds above; random masks of tiny n)
        m[0], m[-1] = True, False
    x = torch.randn(na, din, generator=g)
    x[m] += torch.randn(din, generator=g) * 0.5
    group = None
    if magnitudes:                                     # every tile mixes zero rows, 2^-12, 2^12 and unit rows
        group = torch.randint(0, 4, (na,), generator=g)
        x *= torch.tensor([0.0, 2.0 ** -12, 2.0 ** 12, 1.0])[group][:, None]
    W = torch.randn(dout, din, generator=g) / math.sqrt(din)
    if magnitudes:
        W[37] *= 2.0 ** 8                              # one row of the stationary operand far above the rest (ONE scale serves them all)
    bias = torch.randn(dout, generator=g) * 0.3
    return {"din": din, "n": n, "na": na, "heads": [make_head(g, D, din, gconst) for _ in range(heads)], "D": D, "relu": relu, "layout": layout,
            "x": x, "m": m, "W": W, "bias": bias, "head2": make_head(g, D2, dout, gconst), "D2": D2, "group": group, "sums_x": domain_sums64(x, m)}


def reference(case, dev):
    """everything the checks need, float64 on `dev`: per-head tables on the kernel's rows, stage A over ALL rows (kernel rows first)"""
    n = case["n"]
    x, m = case["x"].to(dev, torch.float64), case["m"].to(dev)
    sums = case["sums_x"].to(dev)
    tabs = [ref_transform(x[:n], m[:n], sums, h) for h in case["heads"]]
    a, raw = ref_stage_a(x, m, case["W"], case["bias"], case["relu"], case["head2"])
    colsum_all = torch.cat((a[m].sum(0), a[~m].sum(0), sums[-2:]))
    mk = m[:n]
    colsum = torch.cat((a[:n][mk].sum(0), a[:n][~mk].sum(0), torch.tensor([float(mk.sum()), float((~mk).sum())], dtype=torch.float64, device=dev)))
    return {"tables": tabs, "a": a[:n], "raw": raw[:n], "colsum": colsum, "colsum_all": colsum_all}


# ---------------------------------------------------------------------------------------------------- the yardstick itself (CPU)
def test_reference_matches_c_oracle_and_its_own_stage_b():
    """The fp64 restatement above against `oracle.oracle_c.adaptedconv_transform` (the reference's own order of operations in fp32)
    on one small case, and its `raw` layout against the consumer conv evaluated directly on the activation.
    Bar for the first: the project's default one, which every kernel is held to against this oracle -- it accumulates 20 fp32
    products per output in sequence, an expected rounding error of sqrt(20) * 2^-24 = 2.7e-7 of the terms' size (worst case
    1.2e-6), against 1e-5 relative + 1e-6 of the largest value.
    Bar for the second: both sides are fp64 evaluations of the same real-valued expression; 1e-12 leaves four digits over
    the 128-term sums' rounding."""
    case = make_case(20, 333, 1, 7, True, "tight", "rand", False, 3, seed=1)
    ref = reference(case, "cpu")
    h = case["heads"][0]
    prm = {"lin_s.weight": h["W_s"].numpy(), "lin_s.bias": h["b_s"].numpy(), "lin_t.weight": h["W_t"].numpy(), "lin_t.bias": h["b_t"].numpy(),
           "a_g_s2t.weight": h["g_s2t"].numpy()[None, :], "a_g_t2s.weight": h["g_t2s"].numpy()[None, :]}
    o_s2t, o_t2s = OC.adaptedconv_transform(case["x"].numpy(), case["m"].numpy(), prm)
    assert_close(o_s2t, ref["tables"][0][0].numpy(), what="C oracle h_s2t vs the fp64 reference")
    assert_close(o_t2s, ref["tables"][0][1].numpy(), what="C oracle h_t2s vs the fp64 reference")
    # stage B from raw == the consumer conv on a
    case = make_case(72, 257, 2, 2, True, "tight", "rand", True, 3, seed=2)
    ref = reference(case, "cpu")
    want = ref_transform(ref["a"], case["m"], ref["colsum"], case["head2"])
    got = ref_stage_b(ref["raw"], case["m"], ref["colsum"], case["head2"])
    for k in range(2):
        assert_close(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol_scale=1e-12, what="raw -> stage B vs conv on a")
    assert float(ref["raw"][:, 10:].abs().max()) == 0.0 and float(ref["raw"][:, 3].abs().max()) == 0.0


def ref_stage_b(raw, m, sums2, head2):
    """bgnn_narrow_transform_finish_f32 restated: the consumer conv's (h_s2t, h_t2s) from the raw rows alone, float64"""
    dout = (sums2.numel() - 2) // 2
    D2 = head2["W_t"].shape[0]
    f = lambda k: head2[k].to(raw.device, torch.float64)
    delta = sums2[:dout] / sums2[2 * dout] - sums2[dout: 2 * dout] / sums2[2 * dout + 1]
    c0, c1 = head2["gate_const"] if head2.get("gate_const") is not None else (0.0, 0.0)
    gate_s = torch.tanh(raw[:, 8] + delta @ f("g_s2t")[dout:] + c0)
    gate_t = torch.tanh(raw[:, 9] + delta @ f("g_t2s")[dout:] + c1)
    md = m.to(torch.float64)
    h_s2t = raw[:, 0:D2] + f("b_t") - (md * gate_s)[:, None] * (f("W_t") @ delta)[None, :]
    h_t2s = raw[:, 4:4 + D2] + f("b_s") + ((1.0 - md) * gate_t)[:, None] * (f("W_s") @ delta)[None, :]
    return h_s2t, h_t2s


# ---------------------------------------------------------------------------------------------------- running the kernel
def sentinel(*shape, dtype=torch.float32):
    if dtype == torch.float64:
        return torch.full(shape, (SENTINEL << 32) | 0x1234, dtype=torch.int64, device=DEV).view(torch.float64)
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def untouched(t):
    if t.dtype == torch.float64:
        return bool((t.view(torch.int64) == ((SENTINEL << 32) | 0x1234)).all())
    return bool((t.view(torch.int32) == SENTINEL).all())


def dev_head(h):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in h.items()}


def _tables(n, H, ldh, layout, blocks=3):
    """-> (outs = [(h_t2s, h_s2t)] * H views, buffers): tight tables of their own, or column blocks of the model's interleaved
    [rows, 3 * ldh] pair; all sentinel filled, GUARD rows behind row n"""
    if layout == "tight":
        bufs = [sentinel(n + GUARD, ldh) for _ in range(2 * H)]
        return [(bufs[2 * h], bufs[2 * h + 1]) for h in range(H)], bufs
    t2s, s2t = sentinel(n + GUARD, blocks * ldh), sentinel(n + GUARD, blocks * ldh)
    return [(t2s[:, h * ldh: (h + 1) * ldh], s2t[:, h * ldh: (h + 1) * ldh]) for h in range(H)], [t2s, s2t]


def abi_stage(x, n, din, ldx, m8, sums, pair, outs, row_stride, W, bias, dout, relu, colsum, pack_t, raw, small):
    """bgnn_classifier_stage_f32 itself, every buffer the caller's -> return code"""
    from bridged_gnn_amd import _lib
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    Wp, bp, gates, D, ldh, gconst = pair
    H = gates.shape[0]
    o1 = outs[1] if H > 1 else (None, None)
    return _lib.lib().bgnn_classifier_stage_f32(p(x), n, din, ldx, p(m8), p(sums), H, D, p(Wp), p(bp), p(gates), p(gconst), p(outs[0][1]), p(outs[0][0]),
                                                p(o1[1]), p(o1[0]), ldh, row_stride, p(W), p(bias), dout, 1 if relu else 0, p(colsum), p(pack_t[0]),
                                                p(pack_t[2]), p(raw), p(small), _lib.stream())


def run_stage(case, prefill=None):
    """one call of ops.classifier_stage on the case -> dict of device results"""
    from bridged_gnn_amd import ops
    n, din = case["n"], case["din"]
    H = len(case["heads"])
    xb = torch.full((n, din + 4), float("nan"), device=DEV)     # the kernel must never let a pad column reach a product
    xb[:, :din] = case["x"][:n].to(DEV)
    x = xb[:, :din]
    m8 = case["m"][:n].to(DEV, torch.uint8)
    pair = ops.pack_transform_heads([dev_head(h) for h in case["heads"]], din)
    pack_t = ops.pack_transform_heads([dev_head(case["head2"])], 128)
    assert pack_t[0].shape == (8, 128)
    ldh = pair[4]
    outs, bufs = _tables(n, H, ldh, case["layout"])
    cbuf = sentinel(258 + 6, dtype=torch.float64)
    colsum = cbuf[:258]
    colsum.copy_(torch.zeros(258, dtype=torch.float64) if prefill is None else prefill)
    W, bias = case["W"].to(DEV), case["bias"].to(DEV)
    assert ops.classifier_stage_supported(x, pair, W, pack_t)
    sums_x = case["sums_x"].to(DEV)
    raw = ops.classifier_stage(x, m8, sums_x, pair, outs, W, bias, colsum, pack_t, relu=bool(case["relu"]))
    # The wrapper allocates raw itself (uninitialised: a row the kernel skips would hold whatever was there, an earlier call's correct
    # values included).  The same call through the C entry into a sentinel-filled raw: the kernel is bit-deterministic in raw, so the
    # two agree in every word only if every row was written (a sentinel word is a NaN, which `close` refuses).
    raw_s = sentinel(n, 12)
    outs_s, _ = _tables(n, H, ldh, case["layout"])
    rc = abi_stage(x, n, din, x.stride(0), m8, sums_x, pair, outs_s, outs_s[0][0].stride(0), W, bias, 128, bool(case["relu"]),
                   torch.zeros(258, dtype=torch.float64, device=DEV), pack_t, raw_s, torch.empty(H * (2 * ldh + 2) + 8, device=DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int32), raw_s.view(torch.int32)), "raw differs from the same call into a sentinel-filled raw: rows left unwritten"
    torch.cuda.synchronize()
    return {"x": x, "m8": m8, "pair": pair, "pack_t": pack_t, "outs": outs, "bufs": bufs, "colsum": colsum, "cbuf": cbuf, "raw": raw, "ldh": ldh,
            "W": W, "bias": bias}


def over_default_bar(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (1e-6 * max(float(np.abs(ref).max()), 1e-30) + 1e-5 * np.abs(ref))).max())


def close(got, ref, what, **bar):
    """`assert_close` after a finiteness check: its `err > bar` is False for a NaN, and every sentinel here is one -- an output
    row that was never written, or a NaN pad column of x that reached a product, must fail, not pass"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} values are not finite (never written, or a pad column leaked)"
    assert_close(got, ref, what=what, **bar)


def check_tables_and_raw(case, res, ref, tag, rows=None):
    """tables and raw of the rows `rows` (default: all) against fp64 at the default bar; exact zeros; guard regions"""
    n, D, ldh = case["n"], case["D"], res["ldh"]
    sel = slice(None) if rows is None else rows
    for h, (t2s, s2t) in enumerate(res["outs"]):
        r_s2t, r_t2s = ref["tables"][h]
        close(s2t[:n, :D][sel].cpu().numpy(), r_s2t[sel].cpu().numpy(), f"{tag} head {h} h_s2t")
        close(t2s[:n, :D][sel].cpu().numpy(), r_t2s[sel].cpu().numpy(), f"{tag} head {h} h_t2s")
        if ldh > D:                                                 # pad columns D .. ldh-1: exactly zero
            assert float(s2t[:n, D:].abs().max()) == 0.0 and float(t2s[:n, D:].abs().max()) == 0.0, f"{tag} head {h}: pad columns"
    raw = res["raw"]
    close(raw[:, 0:4][sel].cpu().numpy(), ref["raw"][:, 0:4][sel].cpu().numpy(), f"{tag} raw W_t.a")
    close(raw[:, 4:8][sel].cpu().numpy(), ref["raw"][:, 4:8][sel].cpu().numpy(), f"{tag} raw W_s.a")
    close(raw[:, 8:10][sel].cpu().numpy(), ref["raw"][:, 8:10][sel].cpu().numpy(), f"{tag} raw gate products")
    assert bool((raw[:, 10:12].view(torch.int32) == 0).all()), f"{tag}: raw[:, 10:12] is not +0.0 in every row"


def check_guards(case, res, tag):
    n, H, ldh = case["n"], len(case["heads"]), res["ldh"]
    for b in res["bufs"]:
        assert untouched(b[n:]), f"{tag}: guard rows behind row N written"
    if case["layout"] != "tight":
        for b in res["bufs"]:
            assert untouched(b[:, H * ldh:]), f"{tag}: neighbour columns of the interleaved table written"
    assert untouched(res["cbuf"][258:]), f"{tag}: behind colsum written"


def check_colsum(case, res, ref, tag, prefill=None):
    want = ref["colsum"] if prefill is None else ref["colsum"] + prefill.to(DEV)
    close(res["colsum"].cpu().numpy(), want.cpu().numpy(), f"{tag} colsum", rtol=1e-6, atol_scale=1e-6)
    assert torch.equal(res["colsum"][256:], want[256:]), f"{tag}: node counts"


def check_stage_b(case, res, ref, tag, superset):
    """the kernel's raw through ops.narrow_transform_finish against the consumer conv on the fp64 activation.  `sums` is what the
    model passes: the kernel's own colsum, or (a rank's share) sums over a superset of the rows -- the reference's delta comes from
    the very vector the finish kernel gets."""
    from bridged_gnn_amd import ops
    n, D2 = case["n"], case["D2"]
    sums2 = ref["colsum_all"].clone() if superset else res["colsum"].clone()
    if case["layout"] != "tight" and res["ldh"] == 4:              # the model's layout: head 2 is the third column block
        out = (res["bufs"][0][:, 8:12], res["bufs"][1][:, 8:12])
        assert untouched(out[0]) and untouched(out[1])
        keep = [b[:, :8].clone() for b in res["bufs"]]
    else:
        out, keep = (sentinel(n + GUARD, 4), sentinel(n + GUARD, 4)), None
    ops.narrow_transform_finish(res["raw"], res["m8"], sums2, res["pack_t"], out)
    torch.cuda.synchronize()
    want = ref_transform(ref["a"], case["m"][:n].to(DEV), sums2, case["head2"])
    close(out[1][:n, :D2].cpu().numpy(), want[0].cpu().numpy(), f"{tag} stage B h_s2t")
    close(out[0][:n, :D2].cpu().numpy(), want[1].cpu().numpy(), f"{tag} stage B h_t2s")
    if D2 < 4:
        assert float(out[0][:n, D2:].abs().max()) == 0.0 and float(out[1][:n, D2:].abs().max()) == 0.0
    assert untouched(out[0][n:]) and untouched(out[1][n:]), f"{tag}: stage B wrote guard rows"
    if keep is not None:
        for b, k in zip(res["bufs"], keep):
            assert torch.equal(b[:, :8].view(torch.int32), k.view(torch.int32)), f"{tag}: stage B wrote its neighbours' columns"


# ---------------------------------------------------------------------------------------------------- the case table
DINS = (68, 96, 100, 124, 128)
# "A" = 32 * 4 * n_cu + 33 and "B" = 2 * 32 * 4 * n_cu + 1 rows: some waves of the persistent grid take one tile more than others
NS = (1, 31, 32, 33, 129, 4099, "A", "B")
SKINNY = ((2, 1), (2, 2), (2, 3), (2, 4), (1, 4), (1, 7), (1, 9), (1, 12))     # (heads, D): ldh 4 | 4 | 8 | 12 | 12
MASKS = ("rand", "one_source", "one_target")


def _case_table():
    """40 cases: every (Din, N) pair once, every skinny configuration with five of the eight N and at least three of the five Din,
    every pair of values of any two of the small axes (relu, layout, mask kind, gate constants, consumer D) at least once."""
    out = []
    for i in range(40):
        din, ntok = DINS[i % 5], NS[i % 8]
        heads, D = SKINNY[(i + i // 8) % 8]
        relu = (i + i // 2) % 2
        layout = ("tight", "inter")[(i // 2 + i // 5) % 2]
        mk = MASKS[(i + i // 3) % 3]
        gconst = (i // 3 + i // 7) % 2
        D2 = 1 + (i + i // 4) % 4
        out.append(pytest.param(din, ntok, heads, D, relu, layout, mk, gconst, D2, i,
                                id=f"{i:02d}-din{din}-n{ntok}-h{heads}xD{D}-relu{relu}-{layout}-{mk}-gc{gconst}-D2_{D2}"))
    return out


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _resolve_n(ntok):
    if ntok == "A":
        return 32 * 4 * _n_cu() + 33
    if ntok == "B":
        return 2 * 32 * 4 * _n_cu() + 1
    return int(ntok)


def test_case_table_covers_its_axes():
    """the selection above, checked: the claims of `_case_table`'s docstring"""
    rows = [p.values for p in _case_table()]
    assert len({(r[0], r[1]) for r in rows}) == 40
    for sk in SKINNY:
        mine = [r for r in rows if (r[2], r[3]) == sk]
        assert len({r[1] for r in mine}) == 5 and len({r[0] for r in mine}) >= 3
    small = (4, 5, 6, 7, 8)
    for a in small:
        for b in small:
            if a < b:
                na, nb = len({r[a] for r in rows}), len({r[b] for r in rows})
                assert len({(r[a], r[b]) for r in rows}) == na * nb, (a, b)
    for ax in small:                                          # and each of their values meets every Din and every skinny configuration
        nv = len({r[ax] for r in rows})
        assert len({(r[0], r[ax]) for r in rows}) == 5 * nv, ax
    for ax in (4, 5):
        assert len({(r[2], r[3], r[ax]) for r in rows}) == 16, ax


@gpu
@pytest.mark.parametrize("din,ntok,heads,D,relu,layout,maskkind,gconst,D2,idx", _case_table())
def test_classifier_stage_vs_fp64(din, ntok, heads, D, relu, layout, maskkind, gconst, D2, idx):
    """tables, raw, colsum, guard regions and the stage-B hand-over of one call, against the fp64 reference.  N = 1 takes its domain
    sums from a superset of the rows (one row has one domain), as does every eighth case: a rank's share of a partition."""
    n = _resolve_n(ntok)
    superset = n == 1 or idx % 8 == 5
    case = make_case(din, n, heads, D, relu, layout, maskkind, gconst, D2, extra=37 if superset else 0, seed=idx)
    ref = reference(case, DEV)
    res = run_stage(case)
    tag = f"case {idx}"
    check_tables_and_raw(case, res, ref, tag)
    check_colsum(case, res, ref, tag)
    check_guards(case, res, tag)
    check_stage_b(case, res, ref, tag, superset)


@gpu
@pytest.mark.parametrize("din", [100, 128])
def test_classifier_stage_mixed_magnitudes(din):
    """Tiles that mix all-zero rows, rows scaled by 2^-12 and 2^+12 and unit rows (the row scale is per row), under a first Linear one
    of whose rows is 2^8 above the rest (ONE power of two scales the whole stationary operand).  Each magnitude group is compared
    on its own: the absolute term of the bar follows the group's largest reference value."""
    case = make_case(din, 2085, 2, 3, 1, "inter", "rand", True, 4, seed=din, magnitudes=True)
    ref = reference(case, DEV)
    res = run_stage(case)
    grp = case["group"][: case["n"]].to(DEV)
    for k, name in enumerate(("zero rows", "rows * 2^-12", "rows * 2^12", "unit rows")):
        rows = torch.nonzero(grp == k).reshape(-1)
        assert rows.numel() > 400
        check_tables_and_raw(case, res, ref, f"magnitudes din={din} {name}", rows=rows)
    check_colsum(case, res, ref, f"magnitudes din={din}")
    check_guards(case, res, f"magnitudes din={din}")


@gpu
@pytest.mark.parametrize("relu", [0, 1])
def test_classifier_stage_colsum_many_tiles_per_lane(relu):
    """8 * 32 * 4 * n_cu rows: every lane of the persistent grid adds eight tiles' worth of activation values in fp32 before the
    block's partial reaches the fp64 accumulator -- the column sums must still meet the bar the two-launch path is held to.  With a
    pre-filled accumulator the result is prefill + sums (the entry point accumulates)."""
    n = 8 * 32 * 4 * _n_cu()
    case = make_case(100, n, 2, 2, relu, "tight", "rand", False, 2, seed=40 + relu)
    ref = reference(case, DEV)
    prefill = (torch.arange(258, dtype=torch.float64) * 0.5 - 40.0) * (n / 64.0)       # comparable to the sums; exact in fp64
    prefill[256:] = torch.tensor([3.0, 5.0], dtype=torch.float64)
    res = run_stage(case, prefill=prefill)
    check_colsum(case, res, ref, f"large N relu={relu} prefilled", prefill=prefill)
    got = (res["colsum"] - prefill.to(DEV))[:256].cpu().numpy()
    close(got, ref["colsum"][:256].cpu().numpy(), f"large N relu={relu} sums alone", rtol=1e-6, atol_scale=1e-6)
    check_guards(case, res, f"large N relu={relu}")


@gpu
@pytest.mark.parametrize("din,ntok,heads,D,layout", [(128, "B", 2, 2, "inter"), (100, 4099, 1, 9, "tight"), (68, 33, 2, 4, "inter")])
def test_classifier_stage_is_deterministic(din, ntok, heads, D, layout):
    """two identical calls: bit-equal tables and raw (only the fp64 atomics of colsum may differ in order)"""
    case = make_case(din, _resolve_n(ntok), heads, D, 1, layout, "rand", True, 2, seed=77)
    a, b = run_stage(case), run_stage(case)
    for x, y in zip(a["bufs"], b["bufs"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(a["raw"].view(torch.int32), b["raw"].view(torch.int32))


@gpu
def test_classifier_stage_refuses_shapes_outside_its_envelope():
    """Din = 64 and 132, a first Linear that is not 128 wide and two heads at ldh 8 (32 packed columns): BGNN_E_SHAPE from the entry
    point (RuntimeError from the wrapper), and no output buffer is touched."""
    from bridged_gnn_amd import _lib, ops
    L = _lib.lib()
    n = 64
    for din, dout, heads, D, why in ((64, 128, 2, 2, "Din = 64"), (132, 128, 2, 2, "Din = 132"), (96, 64, 2, 2, "Dout = 64"),
                                     (96, 256, 1, 4, "Dout = 256"), (96, 128, 2, 7, "two heads at ldh 8")):
        case = make_case(din, n, heads, D, 1, "tight", "rand", False, 2, seed=5, dout=dout)
        x = case["x"].to(DEV)
        m8 = case["m"].to(DEV, torch.uint8)
        pair = ops.pack_transform_heads([dev_head(h) for h in case["heads"]], din)
        pack_t = ops.pack_transform_heads([dev_head(case["head2"])], dout)
        ldh = pair[4]
        outs, bufs = _tables(n, heads, ldh, "tight")
        colsum = sentinel(2 * dout + 2, dtype=torch.float64)
        raw, small = sentinel(n, 12), sentinel(heads * (2 * ldh + 2) + 8)
        W, bias, sums = case["W"].to(DEV), case["bias"].to(DEV), case["sums_x"].to(DEV)
        rc = abi_stage(x, n, din, din, m8, sums, pair, outs, ldh, W, bias, dout, True, colsum, pack_t, raw, small)
        assert rc == -2, f"{why}: return code {rc}"
        assert L.bgnn_error_string(rc).decode().startswith("BGNN_E_SHAPE")
        with pytest.raises(RuntimeError, match="BGNN_E_SHAPE"):
            ops.classifier_stage(x, m8, sums, pair, outs, W, bias, colsum, pack_t, relu=True)
        assert not ops.classifier_stage_supported(x, pair, W, pack_t), why
        torch.cuda.synchronize()
        for b in bufs + [colsum, raw, small]:
            assert untouched(b), f"{why}: an output buffer was written"


@gpu
@pytest.mark.parametrize("din,ntok,heads,D,relu,D2,gconst", [(128, 4099, 2, 2, 1, 2, 0), (100, "A", 2, 4, 1, 4, 1), (68, 129, 1, 9, 0, 3, 1),
                                                           (124, 33, 1, 7, 1, 1, 1)])
def test_one_pass_and_two_launch_paths_side_by_side(din, ntok, heads, D, relu, D2, gconst, capsys):
    """For context: the one-pass kernel and the two-launch pair (ops.adaptedconv_transform in sums form + ops.linear_narrow_transform)
    on the same inputs, each as a multiple of the default bar against fp64.  Printed; the one-pass kernel is held to the bar, and the two
    are NOT compared bit for bit (their split arithmetic differs)."""
    from bridged_gnn_amd import ops
    case = make_case(din, _resolve_n(ntok), heads, D, relu, "tight", "rand", gconst, D2, seed=91)
    n = case["n"]
    ref = reference(case, DEV)
    res = run_stage(case)
    outs2, _ = _tables(n, heads, res["ldh"], "tight")
    xc = res["x"].contiguous()                                  # (the transform's wrapper takes whole rows only)
    ops.adaptedconv_transform(xc, res["m8"], None, res["pair"], out=outs2, sums=case["sums_x"].to(DEV))
    colsum2 = torch.zeros(258, dtype=torch.float64, device=DEV)
    raw2 = ops.linear_narrow_transform(xc, res["W"], res["bias"], res["m8"], colsum2, res["pack_t"], relu=bool(relu))
    torch.cuda.synchronize()
    worst = {"one-pass": {}, "two-launch": {}}
    for name, outs, raw, cs in (("one-pass", res["outs"], res["raw"], res["colsum"]), ("two-launch", outs2, raw2, colsum2)):
        t = 0.0
        for h, (t2s, s2t) in enumerate(outs):
            t = max(t, over_default_bar(s2t[:n, :D].cpu().numpy(), ref["tables"][h][0].cpu().numpy()),
                    over_default_bar(t2s[:n, :D].cpu().numpy(), ref["tables"][h][1].cpu().numpy()))
        worst[name]["tables"] = t
        worst[name]["raw"] = max(over_default_bar(raw[:, a:b].cpu().numpy(), ref["raw"][:, a:b].cpu().numpy()) for a, b in ((0, 4), (4, 8), (8, 10)))
        worst[name]["colsum"] = over_default_bar(cs.cpu().numpy(), ref["colsum"].cpu().numpy())
    with capsys.disabled():
        print(f"\n[paths] din={din} n={n} heads={heads} D={D} relu={relu}: worst error over the default bar  " +
              "  ".join(f"{k}: " + ", ".join(f"{q} {v:.3f}" for q, v in w.items()) for k, w in worst.items()))
    w = worst["one-pass"]
    assert w["tables"] <= 1.0 and w["raw"] <= 1.0, f"one-pass: {w}"
