"""GPU: similarity-learner training (bridged_gnn_amd.simlearner) -- the HIP pair passes of csrc/bgnn_pair_mlp.hip against the fp64
restatement of tests/test_simlearner_host.py (which is pinned there to plain autograd), the reference's own fp64 office fixture
(tools/gen_golden_simlearner.py: step-1 gradients, three Adam steps, running statistics, eval scores), and an end-to-end run from
training to a bridged graph."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_simlearner_host import FIX, office, random_case, restate, seeded_model

pytestmark = pytest.mark.gpu
# KINK_CAP: a ReLU kink flip moves one pair's term; over a Cartesian list the gradients of W1 and z are small differences of
# per-pair terms, so one flip weighs more against their max than in the graph models' 2e-4
GRAD_BAR, KINK_CAP = 2e-5, 5e-3
# the office fixture's lin_self.1.weight (W1 of the pair scorer, summed over three Cartesian lists): 4.1e-5 of its max measured on
# an MI355X, the same as plain fp32 autograd of the reference's formulation; held to twice that
LIN1_BAR = 8.2e-5
# Adam check: entries that may miss their per-entry bar (2 measured on an MI355X, see the test)
ADAM_MISS_MAX = 6


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape
    return (got - ref).abs().max().item(), max(ref.abs().max().item(), 1e-30)


def _bar(got, ref, rel, what, scale=None):
    """max |got - ref| <= rel * max |ref| (or rel * scale for a tensor that is 0 in exact arithmetic) + 1e-7 -> err / bar scale"""
    e, m = _err(got, ref)
    m = m if scale is None else scale
    assert e <= rel * m + 1e-7, f"{what}: max err {e:.3e} > {rel * m + 1e-7:.3e}"
    return e / m


# BN1's bias and Linear(2H, 128)'s bias feed BN2, whose backward sums to 0 over the batch: both gradients are 0 in exact
# arithmetic, so they are held to the bar of dW1, the gradient of the same pairs' segment sums
ZERO_GRADS = ("dbe1", "db1")


def _grad_bars(g, r, rel, keys):
    worst = {}
    for k in keys:
        worst[k] = _bar(g[k], r[k], rel, k, scale=_err(r["dW1"], r["dW1"])[1] if k in ZERO_GRADS else None)
    return worst


def _run_kernels(z1, z2, idx1, idx2, y, prm, same):
    """train-mode Similar_v2 on fp32 copies -> (p, loss, counts, module, grads dict)"""
    from bridged_gnn_amd.simlearner import Similar_v2
    H = z1.shape[1]
    sim = Similar_v2(H, 3, train_dropout=False).to(z1.device)
    bn1, l1, bn2, _, l2 = sim.lin_self
    with torch.no_grad():
        for t, k in ((bn1.weight, "g1"), (bn1.bias, "be1"), (l1.weight, "W1"), (l1.bias, "b1"), (bn2.weight, "g2"), (bn2.bias, "be2"),
                     (l2.weight, "w2"), (l2.bias, "b2")):
            t.copy_(prm[k].float())
    a = z1.float().clone().requires_grad_(True)
    b = a if same else z2.float().clone().requires_grad_(True)
    p, loss, counts = sim.pair_bce(a, b, idx1, idx2, y)
    loss.backward()
    g = dict(dg1=bn1.weight.grad, dbe1=bn1.bias.grad, dW1=l1.weight.grad, db1=l1.bias.grad, dg2=bn2.weight.grad, dbe2=bn2.bias.grad,
             dw2=l2.weight.grad, db2=l2.bias.grad, dz=a.grad, dzb=None if same else b.grad)
    return p, loss, counts, sim, g


CASES = [  # (N1, N2, H, P, same, unused)
    (40, 30, 32, 2, False, False),
    (40, 30, 32, 3, False, False),
    (300, 200, 128, 4099, False, True),
    (700, 500, 64, 1000003, False, True),
    (300, 300, 128, 20011, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"P{c[3]}{'_same' if c[4] else ''}")
def test_pair_kernels_match_fp64_restatement(case):
    dev = _dev()
    N1, N2, H, P, same, unused = case
    z1, z2, idx1, idx2, y, prm = random_case(N1, N2, H, P, seed=P, same=same, unused=unused, dev=dev)
    r = restate(z1, z2, idx1, idx2, y, **prm)
    p, loss, counts, sim, g = _run_kernels(z1, z2, idx1, idx2, y, prm, same)
    _bar(p, r["p"], 1e-5, "p")
    _bar(loss, r["loss"], 1e-5, "loss")
    bn1, _, bn2, _, _ = sim.lin_self
    _bar(bn1.running_mean, 0.1 * r["bn1_mean"], 1e-5, "bn1 running_mean")
    _bar(bn1.running_var, 0.9 + 0.1 * r["bn1_var"] * P / (P - 1), 1e-5, "bn1 running_var")
    _bar(bn2.running_mean, 0.1 * r["bn2_mean"], 1e-5, "bn2 running_mean")
    _bar(bn2.running_var, 0.9 + 0.1 * r["bn2_var"] * P / (P - 1), 1e-5, "bn2 running_var")
    assert int(bn1.num_batches_tracked) == 1 and int(bn2.num_batches_tracked) == 1
    # counts: pairs whose fp64 probability sits within fp32 round-off of 0.5 may fall either way
    near = ((r["p"] - 0.5).abs() < 1e-5).sum().item()
    assert (counts.cpu() - r["counts"].cpu()).abs().max().item() <= near
    # batch statistics over 2 or 3 rows: the BN backwards subtract nearly equal terms (x_hat = +-1), so fp32 keeps fewer digits
    bar = GRAD_BAR if P > 3 else 1e-4
    worst = {}
    dz_ref = r["dz1"] + r["dz2"] if same else r["dz1"]
    worst["dz1"] = _bar(g["dz"], dz_ref, bar, "dz1")
    if not same:
        worst["dz2"] = _bar(g["dzb"], r["dz2"], bar, "dz2")
    worst.update(_grad_bars(g, r, bar, ("dg1", "dbe1", "dW1", "db1", "dg2", "dbe2", "dw2", "db2")))
    print(f"P={P}: worst gradient error / max {max(worst.values()):.2e}")


def test_pair_lists_cartesian_and_balanced():
    """the two list shapes the learner draws: a 200 x 200 Cartesian list (sampling) and a 99 262-pair balanced list"""
    from bridged_gnn_amd.simlearner import pair_enumeration
    dev = _dev()
    z1, z2, _, _, _, prm = random_case(500, 400, 128, 2, seed=11, dev=dev)
    gen = torch.Generator().manual_seed(5)
    s1, s2 = torch.randint(0, 500, (200,), generator=gen), torch.randint(0, 400, (200,), generator=gen)
    pe = pair_enumeration(s1[:, None], s2[:, None]).t()
    balanced = (torch.randint(0, 500, (99262,), generator=gen), torch.randint(0, 400, (99262,), generator=gen))
    for i1, i2 in ((pe[0].contiguous(), pe[1].contiguous()), balanced):
        i1, i2 = i1.to(dev), i2.to(dev)
        y = ((i1 % 7) == (i2 % 7)).to(torch.uint8)
        r = restate(z1, z2, i1, i2, y, **prm)
        p, loss, counts, sim, g = _run_kernels(z1, z2, i1, i2, y, prm, False)
        _bar(loss, r["loss"], 1e-5, "loss")
        ours = dict(dW1=g["dW1"], dg1=g["dg1"], dg2=g["dg2"], dw2=g["dw2"], dz1=g["dz"], dz2=g["dzb"])
        over = []
        for k in ours:
            e, m = _err(ours[k], r[k])
            print(f"P={i1.shape[0]} {k}: err {e:.2e} max {m:.2e}")
            if e > GRAD_BAR * m + 1e-9:
                assert e <= KINK_CAP * m, f"{k}: {e:.3e} beyond any ReLU kink flip"
                over.append(k)
        if over:
            # ReLU kink flips: an fp32 pre-activation of BN2's output within rounding of zero may take the other side.  The fp64
            # restatement with the kernels' ReLU pattern must then meet the ordinary bar on every tensor.
            mask = _kernel_relu_mask(z1, z2, i1, i2, prm)
            r2 = restate(z1, z2, i1, i2, y, relu_mask=mask, **prm)
            print(f"P={i1.shape[0]}: {int((mask != _fp64_mask(z1, z2, i1, i2, prm)).sum())} "
                  f"kink flips; re-checked {over}")
            for k in ours:
                _bar(ours[k], r2[k], GRAD_BAR, k + " (kernels' ReLU pattern)")


def _fp64_mask(z1, z2, i1, i2, prm):
    return _preact(z1, z2, i1, i2, prm, torch.float64) > 0


def _kernel_relu_mask(z1, z2, i1, i2, prm):
    return _preact(z1, z2, i1, i2, prm, torch.float32) > 0


def _preact(z1, z2, i1, i2, prm, dt):
    """BN2's output g2 x2 + be2 per pair as the pair passes form it (fp32: the same per-node products, the kernels' fp64 batch
    statistics, x2 = (A[idx1] + B[idx2] - mean) * rstd), or in fp64"""
    import torch.nn as nn
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.simlearner import _bn1_half
    H, P = z1.shape[1], i1.shape[0]
    f = {k: v.to(dt) for k, v in prm.items()}
    bn = nn.BatchNorm1d(2 * H).to(z1.device, dt)
    c1 = torch.bincount(i1, minlength=z1.shape[0]).double()
    c2 = torch.bincount(i2, minlength=z2.shape[0]).double()
    _, a_in, _ = _bn1_half(z1.to(dt), c1, P, f["g1"], f["be1"], bn, slice(0, H), 1e-5, 0.1)
    _, b_in, _ = _bn1_half(z2.to(dt), c2, P, f["g1"], f["be1"], bn, slice(H, 2 * H), 1e-5, 0.1)
    A = (a_in.to(dt) @ f["W1"][:, :H].t()).contiguous()
    B = torch.addmm(f["b1"], b_in.to(dt), f["W1"][:, H:].t()).contiguous()
    if dt == torch.float32:
        st = ops.pair_mlp_stats(A, B, i1, i2)
        mean, rstd = st[:128].float(), (1.0 / torch.sqrt(st[128:] + 1e-5)).float()
    else:
        u = A[i1] + B[i2]
        mean, rstd = u.mean(0), (u.var(0, unbiased=False) + 1e-5).rsqrt()
    return f["g2"] * ((A[i1] + B[i2] - mean) * rstd) + f["be2"]


EVAL_CASES = [  # (N1, N2, H, P, same)
    (40, 30, 32, 2, False),
    (300, 200, 128, 4099, False),
    (300, 300, 128, 20011, True),
    (500, 400, 128, 99262, False),
]


@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: f"P{c[3]}{'_same' if c[4] else ''}")
def test_eval_pass_matches_eval_mode_sequential(case):
    """pm_eval through Similar_v2.pair_scores in eval mode against a plain eval-mode nn.Sequential(BN, Linear, BN, ReLU, Linear) +
    sigmoid on the concatenated layout (fp64, the same fp32 values), with non-trivial running statistics"""
    import torch.nn as nn
    from bridged_gnn_amd.simlearner import Similar_v2
    dev = _dev()
    N1, N2, H, P, same = case
    z1, z2, idx1, idx2, y, prm = random_case(N1, N2, H, P, seed=P + 7, same=same, dev=dev)
    sim = Similar_v2(H, 3, train_dropout=False).to(dev)
    bn1, l1, bn2, _, l2 = sim.lin_self
    gen = torch.Generator().manual_seed(P)
    with torch.no_grad():
        for t, k in ((bn1.weight, "g1"), (bn1.bias, "be1"), (l1.weight, "W1"), (l1.bias, "b1"), (bn2.weight, "g2"), (bn2.bias, "be2"),
                     (l2.weight, "w2"), (l2.bias, "b2")):
            t.copy_(prm[k].float())
        bn1.running_mean.copy_(0.5 * torch.randn(2 * H, generator=gen))
        bn1.running_var.copy_(0.3 + 2 * torch.rand(2 * H, generator=gen))
        bn2.running_mean.copy_(0.3 * torch.randn(128, generator=gen))
        bn2.running_var.copy_(0.05 + 0.5 * torch.rand(128, generator=gen))
    sim.eval()
    a = z1.float()
    b = a if same else z2.float()
    p, counts = sim.pair_scores(a, b, idx1, idx2, y)
    p_nolabel, none = sim.pair_scores(a, b, idx1, idx2)
    assert none is None and torch.equal(p, p_nolabel)
    assert torch.equal(sim.similarity_cross_domain(a, b, idx1, idx2), p)                # the reference-shaped entry points
    seq = nn.Sequential(nn.BatchNorm1d(2 * H), nn.Linear(2 * H, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Linear(128, 1))
    seq.load_state_dict(sim.lin_self.state_dict())
    seq = seq.to(dev, torch.float64).eval()
    with torch.no_grad():
        pref = torch.sigmoid(seq(torch.cat((a.double()[idx1], b.double()[idx2]), 1)).squeeze(-1))
    e = (p.double() - pref).abs().max().item()
    print(f"eval P={P}: max |p - p_ref| {e:.2e}")
    assert e <= 2e-6
    yb = y.bool()
    pos = p > 0.5                                                    # the counts are exactly those of the pass's own p ...
    own = torch.stack(((pos & yb).sum(), (pos & ~yb).sum(), (~pos & yb).sum())).double()
    assert torch.equal(counts, own), (counts, own)
    rpos = pref > 0.5                                                # ... and the reference's except for pairs at p ~ 0.5
    ref = torch.stack(((rpos & yb).sum(), (rpos & ~yb).sum(), (~rpos & yb).sum())).double()
    near = int(((pref - 0.5).abs() < 1e-5).sum())
    assert (counts - ref).abs().max().item() <= near
    if P > 1000:
        assert bool((ref > 0).all()), "the case should exercise TP, FP and FN"


def test_backward_is_bitwise_repeatable_and_atomic_free():
    from bridged_gnn_amd import ops
    dev = _dev()
    z1, z2, idx1, idx2, y, prm = random_case(3000, 2000, 128, 300007, seed=9, dev=dev)
    outs = []
    for _ in range(2):
        p, loss, counts, sim, g = _run_kernels(z1, z2, idx1, idx2, y, prm, False)
        outs.append([p, loss, counts] + [g[k] for k in ("dz", "dzb", "dg1", "dbe1", "dW1", "db1", "dg2", "dbe2", "dw2", "db2")])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert ops.pair_csr(idx1, idx2, 3000, 2000)[0][-1].item() == 300007


def test_saturated_logits_give_torch_zero_gradient():
    """where p rounds to exactly 1.0f or 0.0f torch's chain (p - y) / max(p (1 - p), 1e-12) * p (1 - p) / P is exactly 0"""
    from bridged_gnn_amd import ops
    dev = _dev()
    z1, z2, idx1, idx2, y, prm = random_case(200, 150, 128, 5000, seed=21, dev=dev)
    f = {k: v.float().contiguous() for k, v in prm.items()}
    A = (torch.randn(200, 128, device=dev) * 3).contiguous()
    B = (torch.randn(150, 128, device=dev) * 3).contiguous()
    w2 = (f["w2"].reshape(-1) * 400).contiguous()                 # logits of several hundred: most pairs saturate
    stats = ops.pair_mlp_stats(A, B, idx1, idx2)
    p, dl, sums = ops.pair_mlp_loss(A, B, idx1, idx2, y, stats, f["g2"], f["be2"], w2, f["b2"])
    sat = (p == 1.0) | (p == 0.0)
    assert sat.sum().item() > 1000 and (~sat).sum().item() > 0
    assert torch.all(dl[sat] == 0)
    # elsewhere: torch's own fp32 chain on the kernel's p
    pt = p.clone().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy(pt, y.float()).backward()
    ref = pt.grad * (1 - p) * p
    assert torch.equal(ref == 0, dl == 0)
    assert (dl - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def test_p_le_1_raises():
    dev = _dev()
    z1, z2, idx1, idx2, y, prm = random_case(10, 10, 16, 1, seed=1, dev=dev)
    with pytest.raises(ValueError):
        _run_kernels(z1, z2, idx1, idx2, y, prm, False)


def _office_gpu(dropout):
    dev = _dev()
    ds, dt = office(dev)
    return ds, dt, seeded_model(ds, dt, dropout=dropout).to(dev)


def _office_eager_dw1(f, ds, dt):
    """d loss_sim / d lin_self.1.weight at step 1 by plain fp32 autograd (the reference's formulation) on the seeded model"""
    import torch.nn.functional as F
    _, _, model = _office_gpu(dropout=False)
    dev = ds.x.device
    seq = model.source_learner.sim_net.lin_self
    h_src = model.source_learner.backbone(ds.x).detach()
    h_tar = model.target_learner.encode(dt)[0].detach()
    loss = 0
    for name, (za, zb, ya, yb) in (("src", (h_src, h_src, ds.y, ds.y)), ("tar", (h_tar, h_tar, dt.y, dt.y)),
                                   ("cross", (h_src, h_tar, ds.y, dt.y))):
        i1, i2 = (torch.from_numpy(f[f"s1/idx/{name}"].astype(np.int64)).to(dev)).unbind(0)
        p = torch.sigmoid(seq(torch.cat((za[i1], zb[i2]), 1)))
        loss = loss + F.binary_cross_entropy(p, (ya[i1] == yb[i2]).float().unsqueeze(-1))
    loss.backward()
    return seq[1].weight.grad


def test_office_fixture_step1_gradients_and_three_adam_steps():
    from bridged_gnn_amd import simlearner as SL
    f = load_golden(FIX)
    ds, dt, model = _office_gpu(dropout=False)
    opt, opt_d = SL.make_optimizers(model)
    names = {id(p): k for k, p in model.named_parameters()}
    grads = {}
    for o, pre in ((opt, "s1/grad"), (opt_d, "s1/dgrad")):
        real = o.step

        def step(*a, _real=real, _pre=pre, _o=o, **k):
            if not grads.get(_pre + "done"):
                for grp in _o.param_groups:
                    for p in grp["params"]:
                        grads[(_pre, names[id(p)])] = p.grad.detach().clone()
                grads[_pre + "done"] = True
            return _real(*a, **k)
        o.step = step
    enu = (SL.Pair_Enumerator(ds, "train"), SL.Pair_Enumerator(dt, "train"), SL.Pair_Enumerator_cross(ds, dt, "train"))
    np.random.seed(0)
    tuples = []
    for step in range(1, 4):
        r = SL.train_adv_few_shot(step, ds, dt, model, opt, opt_d, pair_enumerator_src_train=enu[0], pair_enumerator_tar_train=enu[1],
                                  pair_enumerator_cross_train=enu[2], max_class_num=10, sample_size=40000, use_clf=True)
        tuples.append([r[0], *r[1], r[2], r[3], r[4], r[5]])
    # lin_self.1.weight is held to LIN1_BAR (fixed).  For information, the reference's own fp32 arithmetic (plain autograd on the
    # concatenated layout) on the same step-1 lists and representations reaches the same error: over Cartesian lists each node's
    # segment meets the same partners, so dW1 is a small difference of per-pair terms and carries fp32's forward error.
    eager_w1 = _office_eager_dw1(f, ds, dt)
    e32, m32 = _err(eager_w1, f["s1/grad/source_learner.sim_net.lin_self.1.weight"])
    print(f"lin_self.1.weight by fp32 autograd: err {e32:.3e} max {m32:.3e} -> {e32 / m32:.2e}")
    # step-1 gradients against the reference's fp64 gradients
    worst, off, gerr = 0.0, [], {}
    for (pre, key), g in ((k, v) for k, v in grads.items() if isinstance(k, tuple)):
        if f"{pre}/{key}" in f:
            e, m = _err(g, f[f"{pre}/{key}"])
        else:
            idx = torch.from_numpy(f[f"s1/grad_idx/{key}"])
            e, _ = _err(g.reshape(-1).cpu()[idx], f[f"{pre}/{key}/sub"])
            m = float(f[f"{pre}/{key}/max"])
        if key.endswith(("lin_self.0.bias", "lin_self.1.bias")):          # 0 in exact arithmetic (ZERO_GRADS)
            m = float(np.abs(f["s1/grad/source_learner.sim_net.lin_self.1.weight"]).max())
        print(f"{pre}/{key}: err {e:.3e} max {m:.3e} -> {e / m:.2e}")
        bar = (LIN1_BAR if key.endswith("lin_self.1.weight") else GRAD_BAR) * m
        gerr[key] = e
        if e > bar + 1e-9:
            off.append(f"{pre}/{key}: gradient err {e:.3e} > {GRAD_BAR * m:.3e}")
        worst = max(worst, e / m)
    print(f"step-1 gradients: worst error / max |g| = {worst:.2e} (bar {GRAD_BAR})")
    print("tuples", np.array(tuples), "reference", f["step/tuple"])
    assert not off, off
    # losses of the three steps
    t, ft = np.array(tuples), f["step/tuple"]
    for j in (0, 4, 5, 6, 7):
        assert np.abs(t[:, j] - ft[:, j]).max() <= 1e-5 * np.abs(ft[:, j]).max(), f"tuple column {j}: {t[:, j]} vs {ft[:, j]}"
    assert np.abs(t[:, 1:4] - ft[:, 1:4]).max() <= 2e-3, (t[:, 1:4], ft[:, 1:4])
    # parameters after three steps.  Adam's first steps are about lr * sign(g) and then follow ratios of gradients, so an entry's
    # step is as exact as its gradients: with rho = max(gradient bar, 3 x the measured step-1 error) / |g| (step-1 fp64 gradient,
    # weight decay included) it may be off by about 3 lr min(1, 8 rho).  Steps 2 and 3 carry ReLU kink flips of their own (the
    # fixture holds step-1 gradients only), so an entry may miss that bar: such entries must stay within 3 lr (a move the other
    # way) and be at most ADAM_MISS_MAX (2 of 55 329 measured); their count is printed.  This is looser than holding every entry
    # with a non-zero step-1 gradient to its bar, and DESIGN.md section 11 says so.
    allowed, checked = 0, 0
    for key, p in model.named_parameters():
        src = key.startswith("source_learner.")
        lr = 1e-2 if src else 1e-3
        pre = "s1/dgrad" if key.startswith("discriminator.") else "s1/grad"
        if f"s3/param/{key}" in f:
            got, ref = p.detach().double().cpu().reshape(-1), torch.from_numpy(f[f"s3/param/{key}"]).double().reshape(-1)
            g1 = torch.from_numpy(f[f"{pre}/{key}"]).double().reshape(-1)
            gmax = g1.abs().max().item()
        else:
            idx = torch.from_numpy(f[f"s1/grad_idx/{key}"])
            got, ref = p.detach().double().cpu().reshape(-1)[idx], torch.from_numpy(f[f"s3/param/{key}/sub"])
            g1 = torch.from_numpy(f[f"{pre}/{key}/sub"])
            gmax = float(f[f"{pre}/{key}/max"])
        if key.endswith(("lin_self.0.bias", "lin_self.1.bias")):                  # 0 in exact arithmetic
            gmax = float(np.abs(f["s1/grad/source_learner.sim_net.lin_self.1.weight"]).max())
        geff = (g1 + 5e-3 * ref) if src else g1
        rho = 8 * max(GRAD_BAR * gmax, 3 * gerr[key]) / (geff.abs() + 1e-30)
        scale = 2e-5 * max(ref.abs().max().item(), 1.0)
        tol = scale + 3 * lr * rho.clamp(max=1.0)
        err = (got - ref).abs()
        assert bool((err <= 3 * lr + scale).all()), f"{key}: an entry moved more than 3 lr ({err.max().item():.3e})"
        allowed += int((err > tol).sum())
        checked += err.numel()
    print(f"Adam: {allowed} of {checked} entries checked miss their per-entry bar (within 3 lr)")
    assert allowed <= ADAM_MISS_MAX
    for k, v in model.state_dict().items():
        if "num_batches" in k:
            assert int(v) == int(f[f"s3/bn/{k}"]), k
        elif k.endswith("lin_self.2.running_mean"):
            # BN2's batch means carry lin_self.1.bias, whose gradient is 0 in exact arithmetic: Adam turns its round-off into
            # steps of up to lr in either direction (in the fp64 reference too), so this buffer is held to those steps only
            assert np.abs(v.double().cpu().numpy() - f[f"s3/bn/{k}"]).max() <= 3 * 1e-2, k
        elif "running" in k:
            _bar(v, f[f"s3/bn/{k}"], 1e-4, k)
    enu_val = (SL.Pair_Enumerator(ds, "val"), SL.Pair_Enumerator(dt, "val"), SL.Pair_Enumerator_cross(ds, dt, "val"))
    enu_test = (SL.Pair_Enumerator(ds, "test"), SL.Pair_Enumerator(dt, "test"), SL.Pair_Enumerator_cross(ds, dt, "test"))
    ev = SL.eval_adv_v2(ds, dt, model, split="val", enu_list=enu_val) + SL.eval_adv_v2(ds, dt, model, split="test", enu_list=enu_test)
    print("eval after step 3:", np.array(ev), "reference:", f["s3/eval"])
    # same index lists (bit-identical samplers), but the model after three Adam steps is not bit-identical: Adam turns the round-off
    # of gradients that are 0 in exact arithmetic (the two biases before BN2) into full steps, in the fp64 reference as well.  A
    # pair at p ~ 0.5 or one classifier row may then fall the other way: 1e-2 is about one of ~120 test rows of a 31-class macro-f1
    assert np.abs(np.array(ev) - f["s3/eval"]).max() <= 1e-2


def test_end_to_end_train_to_bridged_graph(tmp_path):
    import types
    from bridged_gnn_amd import simlearner as SL
    from bridged_gnn_amd.bridge import BridgeScorer, gen_bridged_graph
    dev = _dev()
    ds, dt = office(dev)
    args = types.SimpleNamespace(dataset_name="office_amazon2dslr")
    state, best = SL.main_adv_v2(args, ds, dt, save=True, repeat=1, num_epoch=5, seed=0, hidden=128, norm_mode="None",
                                 start_eval_epoch=1, max_class_num=10, sample_size=40000, device=dev, ckpt_dir=str(tmp_path),
                                 verbose=False)
    assert state is not None and 1 <= best["epoch"] <= 5 and np.isfinite(best["loss"])
    ck = torch.load(tmp_path / "model_AdvLearner_office_amazon2dslr_best.ckpt", map_location="cpu")
    f = load_golden(FIX)
    assert list(ck.keys()) == list(f["keys"])
    assert all(torch.isfinite(v.float()).all() for v in ck.values())
    scorer = BridgeScorer(ck, dev)
    assert scorer.version == "v2" and scorer.sim_mode == "mlp"
    merged = gen_bridged_graph(ds, dt, scorer, k_cross=20, k_within=3, check_cross=True, check_within=True)
    n = ds.x.shape[0] + dt.x.shape[0]
    ei = merged.edge_index
    assert merged.x.shape[0] == n and ei.shape[0] == 2 and ei.shape[1] > 0
    assert int(ei.min()) >= 0 and int(ei.max()) < n
