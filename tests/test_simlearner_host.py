"""CPU: the similarity-learner training of bridged_gnn_amd.simlearner against the reference's own fixture
(tools/gen_golden_simlearner.py) where no GPU is needed -- split masks, samplers (bit-identical index lists), the seeded model's
keys / shapes / parameter sums -- plus an fp64 restatement of the per-node decomposition of the pair scorer
pinned to plain autograd on the concatenated layout, and f1 from confusion counts."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden

FIX = "simlearner_office_a2d.npz"


def office(dev="cpu"):
    from bridged_gnn_amd import bridge
    from bridged_gnn_amd.data import Data
    g = load_golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
             y=torch.from_numpy(g["y"]).to(dev), central_mask=torch.from_numpy(g["central_mask"]).to(dev))
    ds, dt, _, _ = bridge.dataset_conversion(d, seed=0)
    return ds, dt


def seeded_model(ds, dt, dropout=True):
    from bridged_gnn_amd import simlearner as SL
    from bridged_gnn_amd.utils import set_random_seed
    set_random_seed(0)
    return SL.Adversarial_Learner_v2(ds, dt, dim_hidden=128, num_layer=2, use_norm=True, source_clf=True, norm_mode="None",
                                     norm_scale=1., sim_mode="mlp", backbone="mlp", dropout=dropout)


def _digest(a, b):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(np.asarray(a, np.int64)).tobytes())
    h.update(np.ascontiguousarray(np.asarray(b, np.int64)).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def restate(z1, z2, idx1, idx2, y, g1, be1, W1, b1, g2, be2, w2, b2, eps=1e-5, relu_mask=None):
    """fp64 per-node form of Similar_v2(mode='mlp') + BCE in train mode: forward, BN batch statistics and every gradient from
    per-node segment sums S1 / S2.  Works on any device.  relu_mask [P, 128] (bool): the ReLU pattern to use
    instead of the fp64 one (a pre-activation within rounding of 0 may take the other side in fp32)."""
    P, H = int(idx1.shape[0]), int(z1.shape[1])
    N1, N2 = int(z1.shape[0]), int(z2.shape[0])
    c1 = torch.bincount(idx1, minlength=N1).double()
    c2 = torch.bincount(idx2, minlength=N2).double()

    def half(z, c, g, b):
        mu = (c @ z) / P
        var = (c @ (z - mu).square()) / P
        r = (var + eps).rsqrt()
        xh = (z - mu) * r
        return mu, var, r, xh, xh * g + b
    mu1, var1, r1, xh1, a_in = half(z1, c1, g1[:H], be1[:H])
    mu2, var2, r2, xh2, b_in = half(z2, c2, g1[H:], be1[H:])
    A, B = a_in @ W1[:, :H].t(), b_in @ W1[:, H:].t() + b1
    u = A[idx1] + B[idx2]
    mu_u, var_u = u.mean(0), u.var(0, unbiased=False)
    ru = (var_u + eps).rsqrt()
    x2 = (u - mu_u) * ru
    yb = g2 * x2 + be2
    mask = (yb > 0) if relu_mask is None else relu_mask
    h = yb * mask
    p = torch.sigmoid(h @ w2.reshape(-1) + b2.reshape(()))
    yd = y.double()
    loss = F.binary_cross_entropy(p, yd)
    dl = (p - yd) / torch.clamp((1 - p) * p, min=1e-12) / P * (1 - p) * p
    dy = dl[:, None] * w2.reshape(1, -1) * mask
    sdy, sdyx = dy.sum(0), (dy * x2).sum(0)
    du = g2 * ru * (dy - sdy / P - x2 * (sdyx / P))
    S1 = torch.zeros(N1, u.shape[1], dtype=u.dtype, device=u.device).index_add_(0, idx1, du)
    S2 = torch.zeros(N2, u.shape[1], dtype=u.dtype, device=u.device).index_add_(0, idx2, du)

    def half_bwd(S, Wh, xh, r, c, g):
        D = S @ Wh
        sd, sdx = D.sum(0), (xh * D).sum(0)
        return g * r * (D - c[:, None] * (sd / P + xh * (sdx / P))), sdx, sd
    dz1, dg1a, db1a = half_bwd(S1, W1[:, :H], xh1, r1, c1, g1[:H])
    dz2, dg1b, db1b = half_bwd(S2, W1[:, H:], xh2, r2, c2, g1[H:])
    return dict(p=p, loss=loss, dl=dl, counts=torch.stack((((p > 0.5) & (yd == 1)).sum(), ((p > 0.5) & (yd == 0)).sum(),
                                                           ((p <= 0.5) & (yd == 1)).sum())).double(),
                bn1_mean=torch.cat((mu1, mu2)), bn1_var=torch.cat((var1, var2)), bn2_mean=mu_u, bn2_var=var_u,
                dz1=dz1, dz2=dz2, dg1=torch.cat((dg1a, dg1b)), dbe1=torch.cat((db1a, db1b)), dW1=torch.cat((S1.t() @ a_in, S2.t() @ b_in), 1),
                db1=S1.sum(0), dg2=sdyx, dbe2=sdy, dw2=(dl[:, None] * h).sum(0).reshape(w2.shape), db2=dl.sum().reshape(b2.shape))


def random_case(N1, N2, H, P, seed, same=False, unused=True, dtype=torch.float64, dev="cpu"):
    gen = torch.Generator().manual_seed(seed)
    z1 = torch.randn(N1, H, generator=gen, dtype=torch.float64) * 1.5 + 0.3
    z2 = z1 if same else torch.randn(N2, H, generator=gen, dtype=torch.float64) - 0.2
    N2 = z2.shape[0]
    lim1, lim2 = (N1 * 2 // 3, N2 * 2 // 3) if unused else (N1, N2)        # the top third of the nodes is never referenced
    idx1 = torch.randint(0, lim1, (P,), generator=gen)
    idx2 = torch.randint(0, lim2, (P,), generator=gen)
    y = (torch.rand(P, generator=gen) < 0.3).to(torch.uint8)
    prm = dict(g1=1 + 0.2 * torch.randn(2 * H, generator=gen, dtype=torch.float64), be1=0.1 * torch.randn(2 * H, generator=gen, dtype=torch.float64),
               W1=torch.randn(128, 2 * H, generator=gen, dtype=torch.float64) / (2 * H) ** 0.5,
               b1=0.1 * torch.randn(128, generator=gen, dtype=torch.float64), g2=1 + 0.2 * torch.randn(128, generator=gen, dtype=torch.float64),
               be2=0.1 * torch.randn(128, generator=gen, dtype=torch.float64),
               w2=torch.randn(1, 128, generator=gen, dtype=torch.float64) / 128 ** 0.5, b2=0.1 * torch.randn(1, generator=gen, dtype=torch.float64))
    # values representable in fp32: the fp64 restatement and the fp32 kernels then start from the same numbers
    cast = lambda t: t.float().to(dev, dtype) if t.is_floating_point() else t.to(dev)   # noqa: E731
    return cast(z1), (cast(z1) if same else cast(z2)), idx1.to(dev), idx2.to(dev), y.to(dev), {k: cast(v) for k, v in prm.items()}


def autograd_reference(z1, z2, idx1, idx2, y, prm, eps=1e-5):
    """plain autograd on the concatenated layout, nn.BatchNorm1d in train mode (fp64)"""
    H = z1.shape[1]
    z1 = z1.clone().requires_grad_(True)
    z2 = z1 if z2 is None else z2.clone().requires_grad_(True)
    seq = nn.Sequential(nn.BatchNorm1d(2 * H), nn.Linear(2 * H, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Linear(128, 1)).to(z1.device, z1.dtype)
    with torch.no_grad():
        seq[0].weight.copy_(prm["g1"]); seq[0].bias.copy_(prm["be1"])
        seq[1].weight.copy_(prm["W1"]); seq[1].bias.copy_(prm["b1"])
        seq[2].weight.copy_(prm["g2"]); seq[2].bias.copy_(prm["be2"])
        seq[4].weight.copy_(prm["w2"]); seq[4].bias.copy_(prm["b2"])
    p = torch.sigmoid(seq(torch.cat((z1[idx1], z2[idx2]), 1)).squeeze(-1))
    loss = F.binary_cross_entropy(p, y.to(p.dtype))
    loss.backward()
    return z1, z2, seq, p, loss


@pytest.mark.parametrize("same", [False, True])
def test_decomposition_matches_autograd(same):
    z1, z2, idx1, idx2, y, prm = random_case(60, 45, 16, 700, seed=3 + same, same=same)
    r = restate(z1, z2, idx1, idx2, y, **prm)
    za, zb, seq, p, loss = autograd_reference(z1, None if same else z2, idx1, idx2, y, prm)
    P = idx1.shape[0]

    def close(a, b, what):
        a, b = a.detach(), b.detach()
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), what
    close(r["p"], p, "p")
    close(r["loss"], loss, "loss")
    close(0.1 * r["bn1_mean"], seq[0].running_mean, "bn1 running_mean")
    close(0.9 + 0.1 * r["bn1_var"] * P / (P - 1), seq[0].running_var, "bn1 running_var")
    close(0.1 * r["bn2_mean"], seq[2].running_mean, "bn2 running_mean")
    close(0.9 + 0.1 * r["bn2_var"] * P / (P - 1), seq[2].running_var, "bn2 running_var")
    if same:
        close(r["dz1"] + r["dz2"], za.grad, "dz (z1 is z2)")
    else:
        close(r["dz1"], za.grad, "dz1")
        close(r["dz2"], zb.grad, "dz2")
    for k, t in (("dg1", seq[0].weight), ("dbe1", seq[0].bias), ("dW1", seq[1].weight), ("db1", seq[1].bias), ("dg2", seq[2].weight),
                 ("dbe2", seq[2].bias), ("dw2", seq[4].weight), ("db2", seq[4].bias)):
        close(r[k], t.grad, k)


def test_f1_from_counts_matches_sklearn():
    from bridged_gnn_amd.simlearner import f1_from_counts, macro_f1
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    cases = [(rng.integers(0, 2, 200), rng.integers(0, 2, 200)), (np.zeros(50, int), np.zeros(50, int)),
             (np.zeros(50, int), np.ones(50, int)), (np.ones(50, int), np.zeros(50, int)), (np.ones(3, int), np.ones(3, int))]
    for yt, yp in cases:
        tp, fp, fn = int(((yp == 1) & (yt == 1)).sum()), int(((yp == 1) & (yt == 0)).sum()), int(((yp == 0) & (yt == 1)).sum())
        want = sk.f1_score(yt, yp, average="binary", zero_division=0)
        assert abs(f1_from_counts(tp, fp, fn) - want) < 1e-15
    for _ in range(5):
        yt, yp = rng.integers(0, 31, 120), rng.integers(0, 31, 120)
        yp[:40] = yt[:40]
        want = sk.f1_score(yt, yp, average="macro")
        assert abs(macro_f1(torch.from_numpy(yt), torch.from_numpy(yp)) - want) < 1e-12


def test_masks_and_samplers_reproduce_reference():
    from bridged_gnn_amd import simlearner as SL
    f = load_golden(FIX)
    ds, dt = office()
    for dn, d in (("src", ds), ("tar", dt)):
        for m in ("train", "val", "test"):
            assert np.array_equal(getattr(d, m + "_mask").numpy(), f[f"mask/{dn}_{m}"]), (dn, m)
    enu = (SL.Pair_Enumerator(ds, "train"), SL.Pair_Enumerator(dt, "train"), SL.Pair_Enumerator_cross(ds, dt, "train"))
    np.random.seed(0)
    for step in range(3):
        for name, e in zip(("src", "tar", "cross"), enu):
            i1, i2 = e.sampling(max_class_num=10, sample_size=40000, shuffle=False)
            assert i1.dtype == torch.int64 and i1.shape == (40000,)
            if step == 0:
                assert np.array_equal(np.stack((i1.numpy(), i2.numpy())), f[f"s1/idx/{name}"].astype(np.int64)), name
    got = []
    for mode in ("val", "test"):
        for e in (SL.Pair_Enumerator(ds, mode), SL.Pair_Enumerator(dt, mode), SL.Pair_Enumerator_cross(ds, dt, mode)):
            i1, i2 = e.balanced_sampling(max_class_num=31, sample_size=100000, shuffle=False)
            assert i1.shape == (99262,)
            got.append(_digest(i1.numpy(), i2.numpy()))
    assert np.array_equal(np.stack(got), f["eval/digest"])


def test_empty_bucket_raises_like_reference():
    from bridged_gnn_amd import simlearner as SL
    from bridged_gnn_amd.data import Data
    d = Data(x=torch.zeros(6, 2), y=torch.tensor([0, 0, 1, 1, 2, 2]), train_mask=torch.tensor([1, 1, 1, 1, 0, 0], dtype=torch.bool))
    e = SL.Pair_Enumerator(d, "train")
    with pytest.raises(ValueError):
        e.sampling(max_class_num=3, sample_size=100, shuffle=False)
    with pytest.raises(NotImplementedError):
        e.sampling(max_class_num=3, sample_size=100, shuffle=True)


def test_seeded_model_matches_reference_keys_and_init():
    f = load_golden(FIX)
    ds, dt = office()
    m = seeded_model(ds, dt)
    sd = m.state_dict()
    assert list(sd.keys()) == list(f["keys"])
    shapes = [[s for s in row if s >= 0] for row in f["shapes"].tolist()]
    assert [list(v.shape) for v in sd.values()] == shapes
    for k, p in m.named_parameters():
        pd = p.detach().double()
        want = f[f"init_sum/{k}"]
        assert pd.sum().item() == want[0] and pd.square().sum().item() == want[1], k


def test_unsupported_configurations_raise():
    from bridged_gnn_amd import simlearner as SL
    ds, dt = office()
    with pytest.raises(NotImplementedError):
        SL.Adversarial_Learner_v2(ds, dt, dim_hidden=16, sim_mode="cosine")
    with pytest.raises(NotImplementedError):
        SL.Adversarial_Learner_v2(ds, dt, dim_hidden=16, backbone="gnn")
    with pytest.raises(NotImplementedError):
        SL.Pair_Enumerator(ds, "all")


def test_bn1_per_node_halves_match_autograd():
    """simlearner's per-node BN1 (train mode) -- count-weighted statistics, running update and the per-node backward of one half
    of the concatenation -- against nn.BatchNorm1d on the gathered rows z[idx]"""
    from bridged_gnn_amd.simlearner import _bn1_half, _bn1_half_bwd
    gen = torch.Generator().manual_seed(4)
    N, H, P = 50, 12, 900
    z = torch.randn(N, H, generator=gen, dtype=torch.float64).float().double() * 2 + 0.5
    idx = torch.randint(0, N - 10, (P,), generator=gen)                    # repeated nodes and never-referenced ones
    G = torch.randn(P, H, generator=gen, dtype=torch.float64)               # upstream gradient of every pair row
    gamma = (1 + 0.3 * torch.randn(2 * H, generator=gen, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(2 * H, generator=gen, dtype=torch.float64)).float().double()
    ref = nn.BatchNorm1d(H).double()
    with torch.no_grad():
        ref.weight.copy_(gamma[H:]); ref.bias.copy_(beta[H:])
    zz = z.clone().requires_grad_(True)
    out = ref(zz[idx])
    (out * G).sum().backward()
    mod = nn.BatchNorm1d(2 * H)
    c = torch.bincount(idx, minlength=N).double()
    xh, y, rstd = _bn1_half(z, c, P, gamma, beta, mod, slice(H, 2 * H), 1e-5, 0.1)
    D = torch.zeros(N, H, dtype=torch.float64).index_add_(0, idx, G)
    dz, dgamma, dbeta = _bn1_half_bwd(D, xh, rstd, c, gamma[H:], P)

    def close(a, b, what, rel=2e-6):
        a, b = a.double(), b.double()
        assert (a - b).abs().max().item() <= rel * max(1.0, b.abs().max().item()), what
    close(y[idx], out.detach(), "forward")
    close(mod.running_mean[H:], ref.running_mean, "running_mean")
    close(mod.running_var[H:], ref.running_var, "running_var")
    assert torch.equal(mod.running_mean[:H], torch.zeros(H)) and torch.equal(mod.running_var[:H], torch.ones(H))
    close(dz, zz.grad, "dz")
    assert torch.equal(dz[N - 10:], torch.zeros(10, H))                      # nodes without pairs get no gradient
    close(dgamma, ref.weight.grad, "dgamma")
    close(dbeta, ref.bias.grad, "dbeta")
