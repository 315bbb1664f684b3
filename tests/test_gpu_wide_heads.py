"""GPU: the wide three-head classifier walk (4 < C <= 32; bgnn_adaptedconv_aggregate_heads_wide_f32 and its pull-form backward)
against an fp64 torch restatement of KTGNN.py:292-305 + :435 per head, and the single-GPU training step behind
BGNN_WIDE_TRAIN_HEADS=1 against the reference's own fp64 gradients (tests/golden/grads_*.npz) and the default per-conv route."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.2


def _graph(N, E, seed, hubs=False):
    """seeded multigraph: duplicate edges, self loops, rows without in-edges; `hubs`: one destination and one source with far more
    than HUB_THRESHOLD edges (both directions of the hub machinery of the narrow kernels)"""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(seed)
    src = rng.integers(0, N, E)
    dst = rng.integers(0, N // 2, E) * 2                     # odd rows get no random in-edges
    dup = rng.integers(0, E, E // 10)
    src, dst = np.concatenate((src, src[dup])), np.concatenate((dst, dst[dup]))
    loops = rng.integers(0, N, 40)
    src, dst = np.concatenate((src, loops)), np.concatenate((dst, loops))
    if hubs:
        k = 12 * ops.HUB_THRESHOLD
        src = np.concatenate((src, rng.integers(0, N, k), np.full(k, 3)))
        dst = np.concatenate((dst, np.full(k, 4), rng.integers(0, N, k)))
    ei = torch.from_numpy(np.stack((src, dst)).astype(np.int64)).to(DEV)
    csr = ops.build_dst_csr(ei, N, rewrite_self_loops=False)
    mask = torch.from_numpy(rng.random(N) < 0.45).to(DEV)
    return csr, mask


def _inputs(N, D, heads, seed):
    from bridged_gnn_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    ld = ops.pad4(D)

    def table():
        t = torch.randn(N, heads, ld, device=DEV, generator=g)
        t[:, :, D:] = float("nan")                           # pad columns are never read as data
        return t.reshape(N, heads * ld).contiguous()
    t2s, s2t = table(), table()
    a_t = (torch.randn(heads, D, device=DEV, generator=g) * 0.5).contiguous()
    a_s = (torch.randn(heads, D, device=DEV, generator=g) * 0.5).contiguous()
    return t2s, s2t, a_t, a_s


def _reference(t2s, s2t, a_t, a_s, csr, mask, D, heads, gout):
    """fp64: per head the GATv2 softmax aggregation over the CSR's edges (the kernel's +1e-16) and log_softmax over D classes;
    -> (logp [N, heads, D], m, s [N, heads], dT2S, dS2T [N, heads, D], da_t, da_s [heads, D])"""
    from bridged_gnn_amd import ops
    N, ld = csr.num_nodes, ops.pad4(D)
    E = csr.num_edges
    rp = csr.rowptr.long().cpu()
    col = csr.col[:E].long().cpu()
    dst = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    ms = mask.cpu().bool()
    T = t2s.double().cpu().view(N, heads, ld)[:, :, :D].clone().requires_grad_(True)
    S = s2t.double().cpu().view(N, heads, ld)[:, :, :D].clone().requires_grad_(True)
    at = a_t.double().cpu().clone().requires_grad_(True)
    as_ = a_s.double().cpu().clone().requires_grad_(True)
    dsel = ms[dst][:, None, None]
    H = torch.where(ms[:, None, None], T, S)                 # own-domain table of every row
    Hj = torch.where(dsel, T[col], S[col])                   # the destination's domain picks the table
    z = Hj + H[dst]
    a = torch.where(dsel, at[None], as_[None])
    lg = (a * torch.nn.functional.leaky_relu(z, SLOPE)).sum(-1)     # [E, heads]
    m = torch.full((N, heads), -np.inf, dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, heads), lg.detach(), "amax")
    p = torch.exp(lg - m[dst])
    s = torch.zeros(N, heads, dtype=torch.float64).index_add(0, dst, p)
    alpha = p / (s[dst] + 1e-16)
    o = torch.zeros(N, heads, D, dtype=torch.float64).index_add(0, dst, alpha[:, :, None] * Hj)
    logp = torch.log_softmax(o, dim=-1)
    (logp * gout.double().cpu().view(N, heads, ld)[:, :, :D]).sum().backward()
    return logp.detach(), m, s.detach(), T.grad, S.grad, at.grad, as_.grad


def _check(csr, mask, D, heads, seed, da_atol=1e-6):
    from bridged_gnn_amd import ops
    N, ld = csr.num_nodes, ops.pad4(D)
    t2s, s2t, a_t, a_s = _inputs(N, D, heads, seed)
    m_u8 = mask.to(torch.uint8).contiguous()
    out, ms = ops.adaptedconv_aggregate_heads_wide(t2s, s2t, a_t, a_s, csr, m_u8, D, heads, SLOPE)
    g = torch.randn(N, heads * ld, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 1))
    dt, ds, dat, das = ops.adaptedconv_aggregate_heads_wide_bwd(t2s, s2t, a_t, a_s, csr, m_u8, D, heads, out, ms, g, SLOPE)
    torch.cuda.synchronize()
    logp, m, s, rT, rS, rat, ras = _reference(t2s, s2t, a_t, a_s, csr, mask, D, heads, g)
    o3 = out.cpu().view(N, heads, ld)
    w = f"heads {heads} D {D}"
    assert_close(o3[:, :, :D].numpy(), logp.numpy(), what=f"{w} log-probs")
    assert torch.all(o3[:, :, D:] == 0), f"{w}: pad columns of out"
    msc = ms.cpu().double()
    live = torch.isfinite(m)
    assert torch.equal(torch.isfinite(msc[:, :, 0]), live) and bool((msc[:, :, 1][~live] == 0).all()), f"{w}: rows without in-edges"
    assert_close(msc[:, :, 0][live].numpy(), m[live].numpy(), what=f"{w} state max")
    assert_close(msc[:, :, 1].numpy(), s.numpy(), what=f"{w} state sum")
    for got, ref, nm in ((dt, rT, "dh_t2s"), (ds, rS, "dh_s2t")):
        g3 = got.cpu().view(N, heads, ld)
        assert_close(g3[:, :, :D].numpy(), ref.numpy(), what=f"{w} {nm}")
        assert torch.all(g3[:, :, D:] == 0), f"{w}: pad columns of {nm}"
    assert_close(dat.cpu().numpy(), rat.numpy(), atol_scale=da_atol, what=f"{w} da_t2s")
    assert_close(das.cpu().numpy(), ras.numpy(), atol_scale=da_atol, what=f"{w} da_s2t")
    return t2s, s2t, a_t, a_s, m_u8, out, ms, g, (dt, ds, dat, das)


@pytest.mark.parametrize("D", [5, 7, 9, 16, 17, 31, 32])
@pytest.mark.parametrize("heads", [2, 3])
def test_wide_heads_match_fp64_on_a_multigraph(heads, D):
    csr, mask = _graph(3000, 24000, seed=D * 10 + heads)
    assert int((csr.rowptr[1:] == csr.rowptr[:-1]).sum()) > 0        # rows without in-edges are covered
    _check(csr, mask, D, heads, seed=D + heads)


@pytest.mark.parametrize("D,heads", [(31, 3), (9, 2), (17, 3)])
def test_wide_heads_match_fp64_with_hub_rows(D, heads):
    csr, mask = _graph(2500, 15000, seed=7, hubs=True)
    assert csr.hub_tables() is not None and csr.transposed_hub_tables() is not None
    # da sums every edge in fp32, and one lane group walks the 1536-edge hub row in sequence: measured 1.6e-6 of max|da| at
    # (17, 3); every other tensor stays at the default bar
    _check(csr, mask, D, heads, seed=3, da_atol=4e-6)


def test_wide_heads_backward_is_deterministic():
    from bridged_gnn_amd import ops
    csr, mask = _graph(20000, 400000, seed=11, hubs=True)
    t2s, s2t, a_t, a_s, m_u8, out, ms, g, first = _check(csr, mask, 31, 3, seed=5)
    for _ in range(2):
        again = ops.adaptedconv_aggregate_heads_wide_bwd(t2s, s2t, a_t, a_s, csr, m_u8, 31, 3, out, ms, g, SLOPE)
        for a, b in zip(first, again):
            assert torch.equal(a, b)


@pytest.mark.parametrize("D", [4, 33])
def test_wide_heads_refuse_shapes_outside_the_envelope(D):
    from bridged_gnn_amd import ops
    csr, mask = _graph(500, 3000, seed=1)
    t2s, s2t, a_t, a_s = _inputs(500, D, 3, seed=2)
    m_u8 = mask.to(torch.uint8).contiguous()
    assert not ops.wide_heads_supported(3, D)
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE"):
        ops.adaptedconv_aggregate_heads_wide(t2s, s2t, a_t, a_s, csr, m_u8, D, 3, SLOPE)
    ld = ops.pad4(D)
    out = torch.zeros(500, 3 * ld, device=DEV)
    ms = torch.zeros(500, 3, 2, device=DEV)
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE"):
        ops.adaptedconv_aggregate_heads_wide_bwd(t2s, s2t, a_t, a_s, csr, m_u8, D, 3, out, ms, out.clone(), SLOPE)


def test_wide_heads_backward_without_rows_writes_zero_da():
    """N = 0: the backward still writes da (zeros); the entry is called directly, every pointer a valid 16-byte-aligned buffer"""
    from bridged_gnn_amd import _lib as L
    lib = L.lib()
    buf = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    ibuf = torch.zeros(4, dtype=torch.int32, device=DEV)
    mask = torch.zeros(4, dtype=torch.uint8, device=DEV)
    D, heads, ld = 31, 3, 32
    da_t = torch.full((heads, D), float("nan"), device=DEV)
    da_s = torch.full((heads, D), float("nan"), device=DEV)
    wsb = lib.bgnn_aggregate_heads_wide_bwd_workspace_bytes(0, heads, ld)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=DEV)
    t, a = buf(4 * heads * ld), buf(heads * D)
    rc = lib.bgnn_adaptedconv_aggregate_heads_wide_bwd_f32(
        L.ptr(t), L.ptr(t), ld, L.ptr(a), L.ptr(a), L.ptr(ibuf), L.ptr(ibuf), L.ptr(mask), L.ptr(ibuf), L.ptr(ibuf), 0, D, heads, SLOPE,
        L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(da_t), L.ptr(da_s), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_heads_wide_bwd_f32")
    torch.cuda.synchronize()
    assert torch.equal(da_t, torch.zeros_like(da_t)) and torch.equal(da_s, torch.zeros_like(da_s))


# ------------------------------------------------------------------------------------------------ single-GPU opt-in
WIDE_CASES = ("office64", "office128")


def _record_wide(monkeypatch):
    from bridged_gnn_amd import ops
    from test_gpu_grads_reference import _record_forms
    calls = _record_forms(monkeypatch)
    f = ops.adaptedconv_aggregate_heads_wide_bwd

    def wrapped(*a, **k):
        calls.append(("adaptedconv_aggregate_heads_wide_bwd", a[6], a[7]))
        return f(*a, **k)
    monkeypatch.setattr(ops, "adaptedconv_aggregate_heads_wide_bwd", wrapped)
    return calls


@pytest.mark.parametrize("case", WIDE_CASES)
def test_opt_in_wide_training_step_matches_reference_fp64_gradients(case, monkeypatch):
    from test_gpu_grads_reference import _check_grads, _forms, _oracle, _setup, _stored, _step
    monkeypatch.setenv("BGNN_WIDE_TRAIN_HEADS", "1")
    c, model, data = _setup(case)
    calls = _record_wide(monkeypatch)
    x, outs, loss = _step(c, model, data, False)
    o = _oracle(case)
    for nm, out in zip(("logp_base", "logp_target", "logp_target_hat"), outs):
        got = out.detach().cpu().numpy()
        assert_close(got, o[nm], what=f"{case} {nm}")
        _stored(got, c[nm], 1e-5, f"{case} {nm} (fixture)")
    assert abs(loss.item() - c["loss"][0]) <= 1e-6 * abs(c["loss"][0]), (loss.item(), c["loss"][0])
    del calls[:]
    loss.backward()
    _check_grads(c, o, {k: p.grad for k, p in model.named_parameters()}, f"{case} wide heads")
    _, _, agg, heads, _ = _forms(calls)
    wide = [s for name, *s in calls if name == "adaptedconv_aggregate_heads_wide_bwd"]
    assert agg == [c["hidden"]] and heads == 0 and wide == [[31, 3]], calls


@pytest.mark.parametrize("case", WIDE_CASES)
def test_opt_in_wide_training_step_matches_the_default_route(case, monkeypatch):
    from test_gpu_grads_reference import _setup, _step
    res = []
    for flag in ("0", "1"):
        monkeypatch.setenv("BGNN_WIDE_TRAIN_HEADS", flag)
        c, model, data = _setup(case)
        _, outs, loss = _step(c, model, data, False)
        loss.backward()
        res.append((float(loss), [o.detach() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    (l0, o0, g0), (l1, o1, g1) = res
    assert abs(l1 - l0) <= 2e-6 * abs(l0), (l0, l1)
    for a, b in zip(o1, o0):
        assert float((a - b).abs().max()) < 2e-5
    gmax = max(float(g.abs().max()) for g in g0.values())
    for k in g0:
        e = float((g1[k] - g0[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * gmax)
        assert e < 3e-3, (k, e)


def test_opt_in_wide_graphed_step_equals_the_eager_step(monkeypatch):
    from bridged_gnn_amd import ops
    from test_gpu_grads_reference import _setup
    monkeypatch.setenv("BGNN_WIDE_TRAIN_HEADS", "1")
    c, model, data = _setup("office64")
    captured = []                                   # (entry, called while the stream was being captured)
    for name in ("adaptedconv_aggregate_heads_wide", "adaptedconv_aggregate_heads_wide_bwd"):
        f = getattr(ops, name)

        def wrapped(*a, _f=f, _name=name, **k):
            captured.append((_name, torch.cuda.is_current_stream_capturing()))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
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
    # the captured step itself took the wide route, forward and backward
    assert ("adaptedconv_aggregate_heads_wide", True) in captured and ("adaptedconv_aggregate_heads_wide_bwd", True) in captured, captured
    loss_g = float(step())
    torch.cuda.synchronize()
    graphed = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    loss_e = loss_fn(model(data))
    loss_e.backward()
    assert abs(loss_g - float(loss_e)) <= 1e-6 * abs(float(loss_e)), (loss_g, float(loss_e))
    for k, p in model.named_parameters():
        assert_close(graphed[k].cpu().numpy(), p.grad.cpu().numpy(), what=f"graphed vs eager {k}")
