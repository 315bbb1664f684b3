"""CPU: the v1 similarity learner of bridged_gnn_amd.simlearner_v1 against the reference's own fixture
(tools/gen_golden_simlearner_v1.py) where no GPU is needed -- the seeded model's keys / shapes / parameter sums, the step-1 pair
lists, the shipped v1 checkpoints' key layout -- plus an fp64 restatement of the per-node form of the cosine scorer
 pinned to plain autograd on the reference's gathered layout."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

FIX = "simlearner_v1_office_a2d.npz"


def _digest(a, b):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(np.asarray(a, np.int64)).tobytes())
    h.update(np.ascontiguousarray(np.asarray(b, np.int64)).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def office(dev="cpu", variant="a"):
    """the fixture's graphs: variant a as given, b twitter-style (source edges -> self loops, y % 2)"""
    from bridged_gnn_amd import bridge
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.simlearner_v1 import twitter_self_loops
    g = load_golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(g["x"]), edge_index=torch.from_numpy(g["edge_index"]).long(), y=torch.from_numpy(g["y"]),
             central_mask=torch.from_numpy(g["central_mask"]))
    ds, dt, _, _ = bridge.dataset_conversion(d, seed=0)
    if variant == "b":
        twitter_self_loops(ds)
        ds.y, dt.y = ds.y % 2, dt.y % 2
    for d in (ds, dt):
        for k, v in list(vars(d).items()):
            if torch.is_tensor(v):
                setattr(d, k, v.to(dev))
    return ds, dt


def seeded_model(ds, dt, dropout=True):
    from bridged_gnn_amd import simlearner_v1 as V1
    from bridged_gnn_amd.utils import set_random_seed
    set_random_seed(0)
    return V1.Adversarial_Learner(ds, dt, dim_hidden=64, num_layer=2, source_clf=True, norm_mode="None", norm_scale=1., dropout=dropout)


def restate(tables, plan, lists):
    """fp64 per-node form of the cosine pair losses on normalised tables: -> (losses [K], dl per list,
    G per table = sum_p dl_p q^other over every pair that references the node, counts [K, 3] = TP, FP, FN)."""
    losses, dls, counts = [], [], []
    G = [torch.zeros_like(t) for t in tables]
    for (a, b), (i1, i2, y) in zip(plan, lists):
        P = i1.shape[0]
        c = (tables[a][i1] * tables[b][i2]).sum(1)
        p = torch.sigmoid(c)
        yd = y.double()
        losses.append(F.binary_cross_entropy(p, yd))
        dl = (p - yd) / torch.clamp((1 - p) * p, min=1e-12) / P * (1 - p) * p
        dls.append(dl)
        G[a].index_add_(0, i1, dl[:, None] * tables[b][i2])
        G[b].index_add_(0, i2, dl[:, None] * tables[a][i1])
        pos, one = p > 0.5, yd == 1
        counts.append([int((pos & one).sum()), int((pos & ~one).sum()), int((~pos & one).sum())])
    return torch.stack(losses), dls, G, counts


def _small_sim(H, seed):
    from bridged_gnn_amd.simlearner_v1 import Similar
    torch.manual_seed(seed)
    sim = Similar(H, 3, train_dropout=False).double()
    with torch.no_grad():
        for bn in (sim.lin_self[0], sim.lin_self[2]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    return sim


def _reference_layout(sim, hs, ht, lists):
    """the reference's train step pair part (scripts.py:36-48, models.py:124-130, :143-148): lin_self four times (src, tar, src,
    tar), biasatt on gathered rows, CosineSimilarity, sigmoid, BCE"""
    (i1s, i2s, ys), (i1t, i2t, yt), (i1c, i2c, yc) = lists
    cs = torch.nn.CosineSimilarity(dim=1)
    z = sim.lin_self(hs)
    l_s = F.binary_cross_entropy(torch.sigmoid(cs(z[i1s] + sim.biasatt(z[i1s]), z[i2s] + sim.biasatt(z[i2s]))), ys.double())
    z = sim.lin_self(ht)
    l_t = F.binary_cross_entropy(torch.sigmoid(cs(z[i1t] + sim.biasatt(z[i1t]), z[i2t] + sim.biasatt(z[i2t]))), yt.double())
    zs, zt = sim.lin_self(hs), sim.lin_self(ht)
    l_c = F.binary_cross_entropy(torch.sigmoid(cs(zs[i1c] + sim.biasatt(zs[i1c]), zt[i2c] + sim.biasatt(zt[i2c]))), yc.double())
    return l_s, l_t, l_c


def _lists(Ns, Nt, P, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for a, b in ((Ns, Ns), (Nt, Nt), (Ns, Nt)):
        i1 = torch.randint(0, a * 2 // 3, (P,), generator=g)           # the top third of the nodes is never referenced
        i2 = torch.randint(0, b * 2 // 3, (P,), generator=g)
        out.append((i1, i2, (torch.rand(P, generator=g) < 0.4).to(torch.uint8)))
    return out


@pytest.mark.parametrize("zero_row", [False, True])
def test_per_node_form_matches_reference_layout_autograd(zero_row):
    """fp64: losses, every parameter / input gradient and the BN state of the per-node form (q^ once per domain, BN advanced
    four times, one G per domain) equal plain autograd of the reference's gathered layout to 1e-12"""
    from bridged_gnn_amd.simlearner_v1 import cosine_normalize
    H, Ns, Nt, P = 16, 40, 30, 500
    g = torch.Generator().manual_seed(3)
    hs0 = torch.randn(Ns, H, generator=g, dtype=torch.float64) * 1.3 + 0.2
    ht0 = torch.randn(Nt, H, generator=g, dtype=torch.float64) - 0.1
    lists = _lists(Ns, Nt, P, 5)
    ref, mine = _small_sim(H, 1), _small_sim(H, 1)
    if zero_row:
        with torch.no_grad():                          # q of every node is exactly 0: the clamp of the norm bites
            for s in (ref, mine):
                s.lin_self[4].weight.zero_()
                for m in (s.biasatt[0], s.biasatt[2]):
                    m.bias.zero_()
    hs_r, ht_r = hs0.clone().requires_grad_(), ht0.clone().requires_grad_()
    ls = _reference_layout(ref, hs_r, ht_r, lists)
    sum(ls).backward()

    hs_m, ht_m = hs0.clone().requires_grad_(), ht0.clone().requires_grad_()
    qs = cosine_normalize(mine.node_q(hs_m))
    qt = cosine_normalize(mine.node_q(ht_m))
    mine.advance_bn(hs_m, ht_m)
    qs_d, qt_d = qs.detach(), qt.detach()
    losses, _, G, _ = restate((qs_d, qt_d), ((0, 0), (1, 1), (0, 1)), lists)
    torch.autograd.backward((qs, qt), (G[0], G[1]))

    for a, b in zip(losses, ls):
        assert abs(a.item() - b.item()) <= 1e-12
    assert (hs_m.grad - hs_r.grad).abs().max() <= 1e-12 * max(hs_r.grad.abs().max().item(), 1.0)
    assert (ht_m.grad - ht_r.grad).abs().max() <= 1e-12 * max(ht_r.grad.abs().max().item(), 1.0)
    for (k, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
        if pr.grad is None:
            assert pm.grad is None or pm.grad.abs().max() == 0, k
            continue
        assert (pm.grad - pr.grad).abs().max() <= 1e-12 * max(pr.grad.abs().max().item(), 1.0), k
    for (k, br), (_, bm) in zip(ref.named_buffers(), mine.named_buffers()):
        assert torch.equal(br, bm), k
    assert int(mine.lin_self[0].num_batches_tracked) == int(mine.lin_self[2].num_batches_tracked) == 4


def test_within_list_on_one_table_is_z1_is_z2():
    """a within-domain list on one table: G sums both sides of every pair (z1 is z2), as autograd of q[idx1] . q[idx2] does"""
    g = torch.Generator().manual_seed(7)
    q = F.normalize(torch.randn(25, 128, generator=g, dtype=torch.float64), dim=1).requires_grad_()
    i1, i2 = torch.randint(0, 25, (300,), generator=g), torch.randint(0, 25, (300,), generator=g)
    i2[:20] = i1[:20]                                               # pairs of a node with itself
    y = (torch.rand(300, generator=g) < 0.5).to(torch.uint8)
    loss = F.binary_cross_entropy(torch.sigmoid((q[i1] * q[i2]).sum(1)), y.double())
    loss.backward()
    losses, _, G, _ = restate((q.detach(),), ((0, 0),), ((i1, i2, y),))
    assert abs(losses[0].item() - loss.item()) <= 1e-14
    assert (G[0] - q.grad).abs().max() <= 1e-15


def test_seeded_model_matches_reference_keys_and_init():
    fx = load_golden(FIX)
    for v in ("a", "b"):
        ds, dt = office(variant=v)
        m = seeded_model(ds, dt)
        sd = m.state_dict()
        if v == "a":
            assert list(sd.keys()) == [str(k) for k in fx["keys"]]
            shapes = [list(t.shape) + [-1] * (2 - t.dim()) for t in sd.values()]
            assert np.array_equal(np.array(shapes, np.int64), fx["shapes"])
        for k, p in m.named_parameters():
            pd = p.detach().double()
            ref = fx[f"{v}/init_sum/{k}"]
            assert pd.sum().item() == ref[0] and pd.square().sum().item() == ref[1], (v, k)


def test_step1_pair_lists_match_reference():
    from bridged_gnn_amd.simlearner import Pair_Enumerator, Pair_Enumerator_cross
    fx = load_golden(FIX)
    for v in ("a", "b"):
        ds, dt = office(variant=v)
        enu = (Pair_Enumerator(ds, mode="train"), Pair_Enumerator(dt, mode="train"), Pair_Enumerator_cross(ds, dt, mode="train"))
        np.random.seed(0)
        for name, e in zip(("src", "tar", "cross"), enu):
            i1, i2 = e.sampling(max_class_num=2, sample_size=40000, shuffle=False)
            if v == "a":
                ref = fx[f"{v}/s1/idx/{name}"].astype(np.int64)
                assert np.array_equal(i1.numpy(), ref[0]) and np.array_equal(i2.numpy(), ref[1]), (v, name)
            else:
                assert np.array_equal(_digest(i1.numpy(), i2.numpy()), fx[f"{v}/s1/digest/{name}"]), (v, name)


class _Shape:
    def __init__(self, n_feat, n_cls):
        self.num_features = n_feat
        self.y = torch.tensor([n_cls - 1])


@pytest.mark.parametrize("tag", ["twitter", "hamilton", "howard"])
def test_shipped_v1_checkpoints_load_strict(tag):
    """the shipped v1 checkpoints' key / shape lists load strict=True into a matching Adversarial_Learner, in its key order"""
    from bridged_gnn_amd.simlearner_v1 import Adversarial_Learner
    fx = load_golden(FIX)
    keys = [str(k) for k in fx[f"ckpt/{tag}/keys"]]
    shapes = fx[f"ckpt/{tag}/shapes"]
    sh = {k: tuple(int(d) for d in s if d >= 0) for k, s in zip(keys, shapes)}
    n_feat = sh["source_learner.backbone.convs.0.lin_l.weight"][1]
    n_cls = sh["source_learner.sim_net.lin_clf.weight"][0]
    hidden = sh["source_learner.backbone.convs.0.lin_l.weight"][0]
    m = Adversarial_Learner(_Shape(n_feat, n_cls), _Shape(n_feat, n_cls), dim_hidden=hidden, norm_mode="None")
    assert list(m.state_dict().keys()) == keys
    sd = {k: (torch.zeros(sh[k], dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.zeros(sh[k])) for k in keys}
    m.load_state_dict(sd, strict=True)
    # num_batches_tracked = 4 x the best epoch: each step advances both lin_self BatchNorms four times
    nbt = fx[f"ckpt/{tag}/nbt"]
    assert len(nbt) == 2 and nbt[0] == nbt[1] and nbt[0] % 4 == 0


def test_unsupported_options_raise():
    from bridged_gnn_amd import simlearner_v1 as V1
    ds, dt = office()
    m = seeded_model(ds, dt)
    with pytest.raises(NotImplementedError):
        V1.eval_within_domain(ds, m, mode="val", domain="source", conf_lower_bound=0.1)
    with pytest.raises(NotImplementedError):
        V1.eval_cross_domain(ds, dt, m, mode="val", conf_lower_bound=0.1)
    with pytest.raises(NotImplementedError):
        V1.train_adv_few_shot(1, ds, dt, m, None, None, metric="auc")


def test_twitter_self_loops():
    from bridged_gnn_amd.simlearner_v1 import twitter_self_loops
    ds, _ = office()
    ori = ds.edge_index
    got = twitter_self_loops(ds)
    assert got is ori
    n = ds.x.shape[0]
    assert torch.equal(ds.edge_index, torch.stack((torch.arange(n), torch.arange(n))))
