"""GPU: one training step of the HIP KTGNN_no_complement against the REFERENCE's own fp64 training step (tests/golden/grads_*.npz,
`oracle/gen_golden.py --only grads`): outputs, loss, every parameter gradient, dL/dx and the BatchNorm buffers.  The fixtures keep
large tensors as summaries (oracle/grad_cases.py), so every tensor is compared IN FULL with the fp64 torch oracle run on the CPU
(`grad_cases.oracle_step`, which tests/test_oracle_torch.py pins to the same fixtures at 1e-10), and its stored elements (all of a
small tensor, the strided grid of a large one) directly with the fixture at the same bar.  The cases are chosen so that every form
of the training backward is reached at least once; the test also records which forms each case took (wrapped `ops` entry points),
so a refactor that moves a case to another branch fails here instead of dropping coverage.

Bars: every parameter gradient max|g - g_ref| <= 2e-5 max|g_ref| per tensor (the fp32 reference itself
reaches 1e-7..6e-6 where no leaky-ReLU kink flips; gen_golden prints it); a tensor whose reference gradient is zero up to rounding
(clf_transformer.0.bias, the Linear in front of a train-mode BatchNorm) <= 1e-6 of the model's largest gradient; dL/dx 2e-5 of
its max."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import grad_cases as GC
from oracle import oracle_torch as OT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BAR = 2e-5
KINK_CAP = 2e-4          # widest deviation from the unflipped reference a shown kink flip may explain (`_kink_flips`)

# forms of the training backward each case must reach.  A conv's dense-transform backward (`_TransformFn`) is "streaming" (Gram
# kernel + W-stationary linear: transform_bwd_consts then transform_bwd_prep), "fused_prep" (transform_bwd_prep alone) or the plain
# torch form (no ops call at all); listed as (Din, D) per conv.  `x_grad`: the first conv's form when x needs a gradient.
# agg: D of every aggregation backward (ops: the pull form for D <= 128, the atomic form above); heads: fused three-head backwards.
FORMS = {
    # conv0 (Din 256): torch form; classifier convs (C = 31 > 4): per-conv, streaming
    "office64": dict(streaming=[(64, 31)] * 3, fused_prep=[], x_grad=None, agg=[31, 31, 31, 64], heads=0),
    "office128": dict(streaming=[(128, 31)] * 3, fused_prep=[], x_grad=None, agg=[31, 31, 31, 128], heads=0),
    # conv0 streaming (static x) / fused_prep (p = 132 > 128); clf_base + clf_target(h) as one _TransformPairFn, clf_target(T(h))
    "heads3": dict(streaming=[(48, 64)] + [(64, 3)] * 3, fused_prep=[], x_grad="fused_prep", agg=[64], heads=1, pair=True),
    # conv0 (Din 37, padded): torch form
    "odd4": dict(streaming=[(64, 4)] * 3, fused_prep=[], x_grad=None, agg=[64], heads=1),
    "c3": dict(streaming=[(128, 2)] * 3, fused_prep=[], x_grad=None, agg=[128], heads=1),
    # D = 256: conv0 torch form and the atomic aggregation backward; classifier convs (Din 256): torch form, per-conv (C = 5)
    "wide5": dict(streaming=[], fused_prep=[], x_grad=None, agg=[5, 5, 5, 256], heads=0),
    # conv1 (hidden -> hidden, its input needs a gradient): fused_prep
    "l3": dict(streaming=[(32, 64)] + [(64, 3)] * 3, fused_prep=[(64, 64)], x_grad="fused_prep", agg=[64, 64], heads=1),
    # root_weight: lin_r under autograd, per-conv classifier path
    "root": dict(streaming=[(48, 64)] + [(64, 3)] * 3, fused_prep=[], x_grad="fused_prep", agg=[3, 3, 3, 64], heads=0),
}
HUB_CASES = ("heads3", "odd4", "l3", "root")          # the hidden pull backward at D = 64 walks hub segments on these graphs


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _setup(case):
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    model = KTGNN_no_complement(GC.CASES[case][1], GC.CASES[case][3], GC.CASES[case][4], GC.CASES[case][2],
                                root_weight=GC.CASES[case][5], use_bn=True, dim_share=GC.CASES[case][1], dropout=0.0)
    c = GC.load(case, template=model.state_dict())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    model = model.to(DEV).train()
    data = Data(x=_t(c["x"]), edge_index=_t(c["edge_index"]), y=_t(c["y"]), train_mask=_t(c["train_mask"]),
                central_mask=_t(c["central_mask"]))
    return c, model, data


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return GC.oracle_step(GC.load(case))


def _stored(got, ref, tol, what, scale=None):
    """the elements the fixture keeps (a small tensor in full, the grid of a large one) within tol * scale (default: max|ref|)"""
    bad = [(part, v) for part, v in GC.compare(got, ref, tol, scale) if part in ("full", "grid") and not v <= 1.0]
    assert not bad, (what, bad)


def _record_forms(monkeypatch):
    """wrap the ops entry points of the training backward; -> the list the calls are appended to"""
    from bridged_gnn_amd import ops
    calls = []
    shapes = {"transform_bwd_consts": lambda a: (a[5],),                             # din
              "transform_bwd_prep": lambda a: (a[0].shape[1], a[3]),                 # (Din, D)
              "gram": lambda a: (a[0].shape[1], a[1].shape[1]),
              "linear": lambda a: (a[0].shape[1], tuple(a[1].shape)),
              "adaptedconv_aggregate_bwd": lambda a: (a[6],),                        # D
              "adaptedconv_aggregate_heads_bwd": lambda a: (a[6], a[7])}             # (D, heads)
    for name, shape in shapes.items():
        f = getattr(ops, name)

        def wrapped(*a, _f=f, _name=name, _shape=shape, **k):
            calls.append((_name, *_shape(a)))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def _forms(calls):
    streaming, fused, agg, heads, grams = [], [], [], 0, []
    for i, (name, *s) in enumerate(calls):
        if name == "transform_bwd_prep":
            (streaming if i > 0 and calls[i - 1][0] == "transform_bwd_consts" else fused).append(tuple(s))
        elif name == "adaptedconv_aggregate_bwd":
            agg.append(s[0])
        elif name == "adaptedconv_aggregate_heads_bwd":
            heads += 1
        elif name == "gram":
            grams.append(tuple(s))
    return sorted(streaming), sorted(fused), sorted(agg), heads, grams


def _ratios(c, got, ref, bar):
    """name -> max error / allowed error of every gradient (and "dx") against full fp64 gradients `ref`"""
    out = {}
    for k, r in ref.items():
        m = float(np.abs(r).max())
        zero = k != "dx" and m < 1e-9 * c["gmax"]
        out[k] = float(np.abs(got[k] - r).max()) / ((1e-6 * c["gmax"]) if zero else (bar * m))
    return out


def _kink_flips(c, o, got, bar):
    """Leaky-ReLU kink flips.  The HIP forward forms h_j + h_i in fp32, so an element within rounding of zero can take the other
    slope than in the fp64 reference; the gradients then move by ~1e-4 of a tensor's max although the backward is exact.  The
    explanation is shown, not assumed: the leaky-ReLU inputs of every conv within 1e-6 of their max of zero are the candidates
    (the 8 nearest), the fp64 oracle is re-run with each one's slope flipped, the subset of flips that best explains the HIP
    result is picked (the flips' effects superpose to first order), and the oracle re-run with exactly those flips must meet the
    ordinary bar on every tensor.  -> (flips, full gradients of that oracle run)"""
    import itertools
    rec = []
    GC.oracle_step(c, record=rec)
    cands = []
    for ci, zs in enumerate(rec):
        for part, z in enumerate(zs):
            a = z.abs().reshape(-1)
            m = float(a.max())
            for i in torch.nonzero(a <= 1e-6 * m).reshape(-1).tolist():
                cands.append((float(a[i]) / m, ci, part, i))
    cands = sorted(cands)[:8]

    def flips_for(sel):
        fl = {}
        for _, ci, part, i in sel:
            pair = fl.setdefault(ci, [torch.zeros(rec[ci][0].shape, dtype=torch.bool), torch.zeros(rec[ci][1].shape, dtype=torch.bool)])
            pair[part].view(-1)[i] = True
        return {k: tuple(v) for k, v in fl.items()}

    def full(r):
        return dict(r["grad"], dx=r["dx"]) if "dx" in got else dict(r["grad"])
    base = full(o)
    deltas = [{k: v - base[k] for k, v in full(GC.oracle_step(c, flips=flips_for([cd]))).items()} for cd in cands]
    best, best_err = (), np.inf
    for n in range(len(cands) + 1):
        for sel in itertools.combinations(range(len(cands)), n):
            pred = {k: base[k] + sum((deltas[j][k] for j in sel), 0.0) for k in base}
            err = max(_ratios(c, got, pred, bar).values())
            if err < best_err:
                best, best_err = sel, err
    chosen = [cands[j] for j in best]
    return chosen, full(GC.oracle_step(c, flips=flips_for(chosen)))


def _check_grads(c, o, named, what, dx=None, bar=GRAD_BAR):
    """per-tensor bars against the fp64 oracle's full gradients (o: `_oracle`) and the reference's stored ones (named: name ->
    gradient tensor; dx: dL/dx when the run has one)"""
    gmax = c["gmax"]
    assert sorted(named) == sorted(c["grad"]), "parameter set"
    got = {k: v.detach().cpu().double().numpy() for k, v in named.items()}
    ref = dict(o["grad"])
    if dx is not None:
        got["dx"], ref["dx"] = dx, o["dx"]
    fixture_bar = bar
    if max(_ratios(c, got, ref, bar).values()) > 1.0:
        # a kink flip: the unflipped comparison must stay within KINK_CAP, the oracle with the flips that explain it within `bar`
        worst = max(_ratios(c, got, ref, KINK_CAP).values())
        assert worst <= 1.0, f"{what}: {worst * KINK_CAP:.2e} of a tensor's max against the fp64 oracle, beyond any kink flip"
        flips, ref = _kink_flips(c, o, got, bar)
        assert flips, f"{what}: off the {bar} bar and no kink flip explains it"
        print(f"{what}: kink flips (|z|/max, conv call, side, element) {flips}")
        fixture_bar = KINK_CAP
    for k, r in ref.items():
        m = float(np.abs(r).max())
        if k == "dx":
            assert_close(got[k], r, rtol=0.0, atol_scale=bar, what=f"{what} dL/dx")
            _stored(got[k], c["dx"], fixture_bar, f"{what} dL/dx (fixture)")
        elif m < 1e-9 * gmax:                     # zero up to rounding: absolute, against the model's largest gradient
            assert_close(got[k], r, rtol=0.0, atol_scale=1e-6 * gmax / max(m, 1e-30), what=f"{what} {k} (zero gradient)")
            _stored(got[k], c["grad"][k], 1e-6, f"{what} {k} (zero gradient, fixture)", scale=gmax)
        else:
            assert_close(got[k], r, rtol=0.0, atol_scale=bar, what=f"{what} {k}")
            _stored(got[k], c["grad"][k], fixture_bar, f"{what} {k} (fixture)")


def _step(c, model, data, x_grad):
    x = data.x.clone().requires_grad_(True) if x_grad else data.x
    data.x = x
    model.zero_grad(set_to_none=True)
    lb, lt, lth, _ = model(data)
    loss = OT.train_loss(lb, lt, lth, data.y, data.train_mask, data.central_mask)
    return x, (lb, lt, lth), loss


@pytest.mark.parametrize("x_grad", [False, True], ids=["static_x", "x_grad"])
@pytest.mark.parametrize("case", GC.CASES)
def test_training_step_matches_reference_fp64_gradients(case, x_grad, monkeypatch):
    c, model, data = _setup(case)
    calls = _record_forms(monkeypatch)
    x, outs, loss = _step(c, model, data, x_grad)
    o = _oracle(case)
    for nm, out in zip(("logp_base", "logp_target", "logp_target_hat"), outs):
        got = out.detach().cpu().numpy()
        assert_close(got, o[nm], what=f"{case} {nm}")
        _stored(got, c[nm], 1e-5, f"{case} {nm} (fixture)")
    assert abs(loss.item() - c["loss"][0]) <= 1e-6 * abs(c["loss"][0]), (loss.item(), c["loss"][0])
    for k, v in model.named_buffers():                       # the forward moved the running statistics once
        if v.dtype.is_floating_point:
            assert_close(v.cpu().numpy(), c["bn"][k], rtol=1e-6, atol_scale=1e-6, what=f"{case} {k}")
        else:
            assert int(v.item()) == int(c["bn"][k]), k
    del calls[:]                                            # (ops.linear also runs in some forwards)
    loss.backward()
    _check_grads(c, o, {k: p.grad for k, p in model.named_parameters()}, case,
                 dx=x.grad.cpu().double().numpy() if x_grad else None)
    # ---- the forms this case must reach
    f = FORMS[case]
    streaming, fused, agg, heads, grams = _forms(calls)
    want_streaming, want_fused = list(f["streaming"]), list(f["fused_prep"])
    if x_grad and f["x_grad"] == "fused_prep":                  # the first conv moves from the streaming form to fused_prep
        first = (c["feat"], c["hidden"])
        want_streaming.remove(first)
        want_fused.append(first)
    assert streaming == sorted(want_streaming), ("streaming transform backward", calls)
    assert fused == sorted(want_fused), ("fused_prep transform backward", calls)
    assert agg == sorted(f["agg"]) and heads == f["heads"], ("aggregation backward", calls)
    p_pair = 2 * (((2 * c["C"] + 3) + 3) // 4 * 4)
    assert ((p_pair, c["hidden"]) in grams) == f.get("pair", False), ("_TransformPairFn", grams)
    if case in HUB_CASES:
        assert model._csr.hub_tables() is not None and model._csr.transposed_hub_tables() is not None


def test_heads3_per_conv_narrow_path_matches_reference(monkeypatch):
    """heads3 with the fused three-head training path switched off: the per-conv narrow path (D = 3) against the same fixture"""
    monkeypatch.setenv("BGNN_FUSED_TRAIN_HEADS", "0")
    c, model, data = _setup("heads3")
    calls = _record_forms(monkeypatch)
    x, outs, loss = _step(c, model, data, True)
    assert abs(loss.item() - c["loss"][0]) <= 1e-6 * abs(c["loss"][0])
    del calls[:]
    loss.backward()
    o = _oracle("heads3")
    _check_grads(c, o, {k: p.grad for k, p in model.named_parameters()}, "heads3 per-conv", dx=x.grad.cpu().double().numpy())
    streaming, fused, agg, heads, _ = _forms(calls)
    assert agg == [3, 3, 3, 64] and heads == 0 and streaming == [(64, 3)] * 3 and fused == [(48, 64)], calls


@pytest.mark.parametrize("case", ["office64", "heads3"])
def test_graphed_training_step_matches_reference_fp64_gradients(case):
    """graphed_train_step with a zero learning rate (the weights stay the fixture's): after one replay every p.grad meets the
    same per-tensor bars.  The loss is written with float masks (device-only, no boolean indexing).  The BatchNorm buffers are
    not checked here: the warm-up steps move them."""
    c, model, data = _setup(case)
    y = data.y[:, None]
    tm = data.train_mask.float()
    tmt = (data.train_mask & ~data.central_mask).float()
    n = float(data.x.shape[0])

    def nll(lp, w):
        return -(lp.gather(1, y)[:, 0] * w).sum() / w.sum()

    def loss_fn(out):
        lb, lt, lth, _ = out
        kl = (lt.exp() * (lt - lth)).sum() / n
        return (nll(lb, tm) * 2.0 + nll(lt, tmt) + nll(lth, tmt)) / 4.0 + kl
    opt = torch.optim.Adam(model.parameters(), lr=0.0, capturable=True)
    step = model.graphed_train_step(data, loss_fn, opt)
    loss = step()
    torch.cuda.synchronize()
    assert abs(loss.item() - c["loss"][0]) <= 1e-6 * abs(c["loss"][0]), (loss.item(), c["loss"][0])
    _check_grads(c, _oracle(case), {k: p.grad for k, p in model.named_parameters()}, f"{case} graphed")
    for k, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), torch.from_numpy(c["sd"][k])), f"{k} moved at lr = 0"
