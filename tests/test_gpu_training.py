"""GPU: backward of the fused aggregation -- gradients through the HIP path vs the
CPU torch/autograd oracle (fp64), and an optimisation step of KTGNN_no_complement with the reference's loss."""
import numpy as np
import pytest
import torch

from oracle import oracle_torch as OT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("din,D,n", [(24, 16, 300), (20, 7, 257), (48, 64, 400), (32, 128, 500), (16, 2, 1000), (40, 100, 333), (12, 36, 900), (8, 4, 2049), (8, 3, 500), (8, 1, 300)])
def test_adaptedconv_gradients_vs_autograd_oracle(din, D, n):
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.ktgnn import AdaptedConv
    ei, mask = synth.random_multigraph(n, 8 * n, frac_src=0.45, n_isolated=3, seed=n + D)
    rng = np.random.default_rng(D)
    x = rng.standard_normal((n, din)).astype(np.float32)
    w = rng.standard_normal((n, D)).astype(np.float32)                    # dL/dout
    torch.manual_seed(D)
    conv = AdaptedConv(din, D, root_weight=False).to(DEV)
    xg = _t(x).requires_grad_(True)
    csr = ops.build_dst_csr(_t(ei), n)
    out = conv(xg, None, central_mask=_t(mask), csr=csr)
    (out * _t(w)).sum().backward()
    # oracle in fp64 on the CPU
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.state_dict().items()}
    xo = torch.from_numpy(x).double().requires_grad_(True)
    mo = torch.from_numpy(mask)
    e1, e2 = OT.graph_partition(torch.from_numpy(ei), mo)
    oo = OT.adaptedconv(xo, mo, e1, e2, p)
    (oo * torch.from_numpy(w).double()).sum().backward()
    # measured (tools/grad_error_table.py): every tensor <= 1.2e-6 on these shapes.  The bar leaves room for ONE leaky-relu
    # kink flip: h_j + h_i is formed from fp32 tables, the oracle's from fp64 ones, and an element within rounding of 0 takes
    # slope 1 on one side and 0.1 on the other -- the end-to-end error then jumps to 1e-4..1e-3 for that element although the
    # backward itself is exact to 1e-7 (test_aggregation_backward_exact_on_the_same_tables shows exactly that case)
    assert _rel(out.detach().cpu().double(), oo.detach()) < 2e-6
    assert _rel(xg.grad.cpu().double(), xo.grad) < 2e-5, "dL/dx"
    for name, prm in conv.named_parameters():
        assert _rel(prm.grad.cpu().double(), p[name].grad) < 2e-5, name


@pytest.mark.parametrize("D,n", [(128, 6000), (2, 6000), (16, 3000)])
def test_aggregation_backward_exact_on_the_same_tables(D, n):
    """The aggregation backward against fp64 autograd ON THE SAME fp32 TABLES (so no leaky-relu kink can flip between the two
    sides): <= 1e-6 for every table element and both attention vectors.  At (D, n) = (128, 6000) the end-to-end comparison
    with an fp64 forward (tools/grad_error_table.py) shows 8e-4 on the t2s side -- one kink flip from the tables' fp32
    rounding, not an error of the backward; this test pins that statement."""
    import torch.nn.functional as F
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.ktgnn import _AggregateFn
    ei, mask = synth.random_multigraph(n, 8 * n, frac_src=0.45, n_isolated=3, seed=n + D)
    rng = np.random.default_rng(D)
    ld = ops.pad4(D)
    tabs = []
    for _ in range(2):
        t = np.zeros((n, ld), np.float32)
        t[:, :D] = rng.standard_normal((n, D)).astype(np.float32)
        tabs.append(t)
    a = rng.standard_normal((2, D)).astype(np.float32) * 0.3
    w = rng.standard_normal((n, D)).astype(np.float32)
    csr = ops.build_dst_csr(_t(ei), n)
    m8 = _t(mask).to(torch.uint8)
    g1, g2 = _t(tabs[0]).requires_grad_(True), _t(tabs[1]).requires_grad_(True)
    ga1, ga2 = _t(a[0]).requires_grad_(True), _t(a[1]).requires_grad_(True)
    out = _AggregateFn.apply(g1, g2, ga1, ga2, csr, m8, D, 0.1)[:, :D]
    (out * _t(w)).sum().backward()
    mo = torch.from_numpy(mask)
    e1, e2 = OT.graph_partition(torch.from_numpy(ei), mo)
    t1 = torch.from_numpy(tabs[0][:, :D]).double().requires_grad_(True); t2 = torch.from_numpy(tabs[1][:, :D]).double().requires_grad_(True)
    b1 = torch.from_numpy(a[0]).double().requires_grad_(True); b2 = torch.from_numpy(a[1]).double().requires_grad_(True)
    al = OT.segment_softmax(torch.cat((F.leaky_relu(t1[e1[0]] + t1[e1[1]], 0.1) @ b1, F.leaky_relu(t2[e2[0]] + t2[e2[1]], 0.1) @ b2)),
                            torch.cat((e1[1], e2[1])), n)
    o = torch.zeros(n, D, dtype=torch.float64)
    o = o.index_add(0, e1[1], t1[e1[0]] * al[: e1.shape[1], None]).index_add(0, e2[1], t2[e2[0]] * al[e1.shape[1]:, None])
    (o * torch.from_numpy(w).double()).sum().backward()
    assert _rel(out.detach().cpu().double(), o.detach()) < 1e-6
    assert _rel(g1.grad[:, :D].cpu().double(), t1.grad) < 1e-6 and _rel(g2.grad[:, :D].cpu().double(), t2.grad) < 1e-6
    # (the attention vectors' gradients are sums over ALL edges, accumulated with fp32 atomics in an order that changes from run
    #  to run: 1e-6 typical, 4e-6 seen)
    assert _rel(ga1.grad.cpu().double(), b1.grad) < 1e-5 and _rel(ga2.grad.cpu().double(), b2.grad) < 1e-5


@pytest.mark.parametrize("p,q,n", [(260, 128, 5000), (8, 128, 3333), (36, 4, 1025), (288, 64, 700), (4, 4, 5)])
def test_gram_kernel_vs_fp64(p, q, n):
    """bgnn_gram_f32 (A^T B over the node dimension; weight gradients of the dense transform) vs fp64."""
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(p * q + n)
    A = rng.standard_normal((n, p)).astype(np.float32)
    B = rng.standard_normal((n, q)).astype(np.float32)
    got = ops.gram(_t(A), _t(B)).cpu().double()
    ref = torch.from_numpy(A).double().t() @ torch.from_numpy(B).double()
    assert _rel(got, ref) < 1e-5
    assert torch.equal(ops.gram(_t(A), _t(B)).cpu().double(), got), "deterministic"


@pytest.mark.parametrize("d,nv,n", [(128, 2, 4097), (256, 2, 1000), (36, 4, 777), (4, 1, 3)])
def test_rowdot_kernel_vs_fp64(d, nv, n):
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(d + nv + n)
    X = rng.standard_normal((n, d + 4)).astype(np.float32)
    V = rng.standard_normal((nv, d)).astype(np.float32)
    got = ops.rowdot(_t(X)[:, :d], _t(V)).cpu().double()               # a column-slice view (row stride d + 4)
    ref = torch.from_numpy(X[:, :d]).double() @ torch.from_numpy(V).double().t()
    assert _rel(got, ref) < 1e-5


@pytest.mark.parametrize("seed", range(20))
def test_pull_backward_equals_atomic_backward(seed):
    """the atomic-free pull form and the atomic scatter form of the aggregation backward are the same function: compare
    them against each other on seeded random shapes over the pull envelope (D <= 128: every lane-group width)."""
    from bridged_gnn_amd import _lib, ops, synth
    rng = np.random.default_rng(300 + seed)
    D = int([1, 2, 3, 4, 36, 40, 64, 100, 128, 5, 8, 12, 16, 17, 24, 31, 32, 33, 7, 96][seed])
    n = int(rng.integers(40, 2500))
    ei, mask = synth.random_multigraph(n, int(rng.integers(1, 10)) * n, frac_src=float(rng.uniform(0.2, 0.8)), n_isolated=2, seed=seed)
    csr = ops.build_dst_csr(_t(ei), n)
    ld = ops.pad4(D)
    hS = torch.zeros(n, ld, device=DEV); hT = torch.zeros(n, ld, device=DEV)
    hS[:, :D] = torch.randn(n, D, device=DEV); hT[:, :D] = torch.randn(n, D, device=DEV)
    a1, a2 = torch.randn(D, device=DEV) * 0.3, torch.randn(D, device=DEV) * 0.3
    m8 = _t(mask).to(torch.uint8)
    out, alpha = ops.adaptedconv_aggregate(hS, hT, a1, a2, csr, m8, D, 0.1, want_alpha=True)
    g = torch.zeros(n, ld, device=DEV); g[:, :D] = torch.randn(n, D, device=DEV)
    pull = ops.adaptedconv_aggregate_bwd(hS, hT, a1, a2, csr, m8, D, out, alpha, g, 0.1)
    # the atomic form, called directly
    L = _lib.lib()
    d1, d2 = torch.zeros_like(hS), torch.zeros_like(hT)
    da1, da2 = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    rc = L.bgnn_adaptedconv_aggregate_bwd_f32(_lib.ptr(hS), _lib.ptr(hT), ld, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(csr.rowptr), _lib.ptr(csr.col),
                                              _lib.ptr(m8), 0, n, D, 0.1, _lib.ptr(out), ld, _lib.ptr(alpha), _lib.ptr(g), ld,
                                              _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(da1), _lib.ptr(da2), _lib.stream())
    assert rc == 0
    for name, a, b in (("dh_t2s", pull[0], d1), ("dh_s2t", pull[1], d2), ("da_t2s", pull[2], da1), ("da_s2t", pull[3], da2)):
        assert _rel(a.double().cpu(), b.double().cpu()) < 2e-5, (name, D, n)


@pytest.mark.parametrize("n,feat,hidden,C,ne", [(600, 12, 16, 3, 5000), (5000, 32, 64, 2, 45000)])
def test_training_steps_follow_the_autograd_oracle(n, feat, hidden, C, ne):
    """3 Adam steps of the reference recipe (lr 1e-3, wd 5e-3, loss of main_graph_knowledge_transfer.py:44-54),
    dropout off, BN in train mode: loss trajectory and final weights vs the CPU torch oracle model.  The second size is
    inside the envelopes of the streaming kernels (W-stationary Linear, Gram weight gradients, the paired classifier
    transform), the first below them (library fallbacks); the fused BN and the three-head aggregation run in both."""
    from bridged_gnn_amd import synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    ei, mask = synth.random_multigraph(n, ne, frac_src=0.5, seed=77)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, feat)).astype(np.float32)
    y = rng.integers(0, C, size=n)
    train = rng.random(n) < 0.6
    torch.manual_seed(3)
    model = KTGNN_no_complement(feat, C, 2, hidden, use_bn=True, dim_share=feat, dropout=0.0)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    data = Data(x=_t(x), edge_index=_t(ei), y=_t(y), train_mask=_t(train), central_mask=_t(mask))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lb, lt, lth, _ = model(data)
        loss = OT.train_loss(lb, lt, lth, data.y, data.train_mask, data.central_mask)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    # ---- oracle: the whole-model train-mode step in plain CPU torch (OT.ktgnn_train, pinned to the reference's own fp64
    #      gradients by tests/test_oracle_torch.py); the module only holds the parameters and buffers for Adam
    class Ref(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = KTGNN_no_complement(feat, C, 2, hidden, use_bn=True, dim_share=feat, dropout=0.0)
            self.m.load_state_dict(sd0)
        def forward(self, xx, mo, e1, e2):
            return OT.ktgnn_train(xx, mo, e1, e2, dict(self.m.named_parameters()), dict(self.m.named_buffers()))
    ref = Ref().train()
    mo = torch.from_numpy(mask)
    e1, e2 = OT.graph_partition(torch.from_numpy(ei), mo)
    ropt = torch.optim.Adam(ref.m.parameters(), lr=1e-3, weight_decay=5e-3)
    rlosses = []
    for _ in range(3):
        ropt.zero_grad()
        lb, lt, lth = ref(torch.from_numpy(x), mo, e1, e2)
        l = OT.train_loss(lb, lt, lth, torch.from_numpy(y), torch.from_numpy(train), mo)
        l.backward()
        ropt.step()
        rlosses.append(l.item())
    assert np.allclose(losses, rlosses, rtol=2e-4), (losses, rlosses)
    assert losses[2] < losses[0]
    for (k, v), (_, r) in zip(model.state_dict().items(), ref.m.state_dict().items()):
        if v.dtype.is_floating_point:
            assert torch.allclose(v.cpu(), r, rtol=2e-3, atol=2e-4), k


@pytest.mark.parametrize("din,D,n", [(128, 128, 3000), (128, 2, 4099), (36, 7, 1234), (64, 31, 999), (256, 64, 500)])
def test_transform_bwd_prep_matches_torch_formula(din, D, n):
    """bgnn_transform_bwd_prep_f32 (one stream) == the element-wise torch chain it replaces in _TransformFn.backward."""
    from bridged_gnn_amd import ops
    g = torch.Generator(device=DEV).manual_seed(din + D)
    ld = ops.pad4(D)
    x = torch.randn(n, din, device=DEV, generator=g)
    G1 = torch.zeros(n, ld, device=DEV); G2 = torch.zeros(n, ld, device=DEV)
    G1[:, :D] = torch.randn(n, D, device=DEV, generator=g); G2[:, :D] = torch.randn(n, D, device=DEV, generator=g)
    m = torch.rand(n, device=DEV, generator=g) < 0.4
    gx = torch.randn(2, din, device=DEV, generator=g) * 0.2
    gconst = torch.randn(2, device=DEV, generator=g) * 0.3
    wd = torch.zeros(2, 2 * D, device=DEV)
    wd[0, :D] = torch.randn(D, device=DEV, generator=g); wd[1, D:] = torch.randn(D, device=DEV, generator=g)
    counts = torch.tensor([float(m.sum()), float((~m).sum())], dtype=torch.float64, device=DEV)
    Gall, side = ops.transform_bwd_prep(x, G1, G2, D, m.to(torch.uint8), gx, gconst, wd, counts)
    gam = torch.tanh(x.double() @ gx.double().t() + gconst.double())
    zero = gam.new_zeros(())
    want_side = torch.stack((torch.where(m, gam[:, 0], zero), torch.where(m, zero, gam[:, 1]),
                             torch.ones_like(gam[:, 0]), torch.zeros_like(gam[:, 0])), dim=1)
    cat = torch.cat((G1[:, :D], G2[:, :D]), dim=1).double()
    dc = cat @ wd.double().t()
    dpre = torch.where(torch.stack((m, ~m), dim=1), dc * (1 - gam * gam), zero)
    p = ops.pad4(2 * D + 3)
    want = torch.zeros(n, p, dtype=torch.float64, device=DEV)
    want[:, :2 * D], want[:, 2 * D:2 * D + 2] = cat, dpre
    want[:, 2 * D + 2] = torch.where(m, 1.0 / counts[0], -1.0 / counts[1])
    assert Gall.shape == (n, p)
    assert torch.equal(Gall[:, :2 * D].double(), cat)
    assert torch.allclose(Gall.double(), want, rtol=1e-5, atol=1e-5 * float(dc.abs().max()))
    assert torch.allclose(side.double(), want_side, rtol=1e-5, atol=2e-6)
    if D <= 128:
        # want_ex: the used entries of Gall^T side from the same pass (u1, u2, bias sums, sum dpre), deterministic
        Gall2, ex = ops.transform_bwd_prep(x, G1, G2, D, m.to(torch.uint8), gx, gconst, wd, counts, want_ex=True)
        assert torch.equal(Gall2, Gall)
        full = want.t() @ want_side                                              # [p, 4] in fp64
        ref = torch.zeros_like(full)
        ref[:D, 0], ref[D:2 * D, 1], ref[:2 * D + 2, 2] = full[:D, 0], full[D:2 * D, 1], full[:2 * D + 2, 2]
        assert torch.allclose(ex.double(), ref, rtol=1e-4, atol=2e-5 * float(full.abs().max())), float((ex.double() - ref).abs().max())
        assert torch.equal(ops.transform_bwd_prep(x, G1, G2, D, m.to(torch.uint8), gx, gconst, wd, counts, want_ex=True)[1], ex)


@pytest.mark.parametrize("n,d,relu,p", [(5000, 128, True, 0.0), (3001, 64, True, 0.5), (777, 100, False, 0.25), (4097, 8, True, 0.0)])
def test_fused_bn_relu_dropout_matches_torch_formula(n, d, relu, p):
    """bgnn_bn_relu_dropout_f32 / _bwd (KTGNN.py:420-430 in train mode) vs the fp64 torch formula with the SAME mask (read back
    from the kernel's output: y == 0 where dropped) -- forward, dL/dx, dL/dgamma, dL/dbeta and the running buffers."""
    from bridged_gnn_amd.ktgnn import bn_relu_dropout_train
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, d) + rng.uniform(-2, 2, d)).astype(np.float32)
    w = rng.standard_normal((n, d)).astype(np.float32)
    torch.manual_seed(n)
    bn = torch.nn.BatchNorm1d(d).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    bn.train()
    xg = _t(x).requires_grad_(True)
    y = bn_relu_dropout_train(xg, bn, relu, p)
    assert type(y.grad_fn).__name__ == "_BnReluDropFnBackward", "the fused path must be the one that runs"
    (y * _t(w)).sum().backward()
    # fp64 reference with the kernel's own mask
    xo = torch.from_numpy(x).double().requires_grad_(True)
    g = bn.weight.detach().cpu().double().requires_grad_(True)
    b = bn.bias.detach().cpu().double().requires_grad_(True)
    mean, var = xo.mean(0), xo.var(0, unbiased=False)
    z = (xo - mean) / torch.sqrt(var + bn.eps) * g + b
    z = torch.relu(z) if relu else z
    yc = y.detach().cpu().double()
    if p > 0:
        thr = round(p * 65536)
        live = z.detach().abs() > 1e-6
        keep = (yc != 0) | ~live                      # dropped <=> output zero although the activation is not
        frac = float(((yc != 0) & live).double().sum() / live.double().sum())
        assert abs(frac - (1 - thr / 65536)) < 0.02, frac
        z = torch.where(keep, z * (65536.0 / (65536 - thr)), torch.zeros_like(z))
    (z * torch.from_numpy(w).double()).sum().backward()
    assert _rel(yc, z.detach()) < 2e-6
    assert _rel(xg.grad.cpu().double(), xo.grad) < 2e-5
    assert _rel(bn.weight.grad.cpu().double(), g.grad) < 2e-5
    assert _rel(bn.bias.grad.cpu().double(), b.grad) < 2e-5
    rm = 0.1 * mean.detach()
    rv = 0.9 + 0.1 * xo.detach().var(0, unbiased=True)
    assert _rel(bn.running_mean.cpu().double(), rm) < 1e-6 and _rel(bn.running_var.cpu().double(), rv) < 1e-6
    assert int(bn.num_batches_tracked) == 1
    if p > 0:                                          # a second call draws a different mask
        y2 = bn_relu_dropout_train(xg, bn, relu, p)
        assert not torch.equal(y2 == 0, y == 0)


@pytest.mark.parametrize("D,n,seed", [(2, 3000, 0), (4, 1500, 1), (3, 700, 2), (1, 400, 3), (2, 20000, 4)])
def test_three_head_aggregation_backward_equals_three_single_heads(D, n, seed):
    """`_AggregateHeadsFn` (one CSR walk for the three classifier convs, log_softmax fused, alpha rebuilt from the rows'
    softmax state) vs three `_AggregateFn` + F.log_softmax: outputs and every gradient (tables, attention vectors)."""
    import torch.nn.functional as F
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.ktgnn import _AggregateFn, _AggregateHeadsFn
    ei, mask = synth.random_multigraph(n, 9 * n, frac_src=0.4, n_isolated=3, seed=seed)
    rng = np.random.default_rng(seed)
    csr = ops.build_dst_csr(_t(ei), n)
    mask_u8 = _t(mask).to(torch.uint8)

    def leaves():
        r = np.random.default_rng(100 + seed)
        tabs = []
        for _ in range(6):
            t = np.zeros((n, 4), np.float32)
            t[:, :D] = r.standard_normal((n, D)).astype(np.float32)
            tabs.append(_t(t).requires_grad_(True))
        a_t = _t(r.standard_normal((3, D)).astype(np.float32)).requires_grad_(True)
        a_s = _t(r.standard_normal((3, D)).astype(np.float32)).requires_grad_(True)
        return tabs, a_t, a_s
    w = _t(rng.standard_normal((n, 3, D)).astype(np.float32))
    tabs, a_t, a_s = leaves()
    logp = _AggregateHeadsFn.apply(csr, mask_u8, D, 0.1, a_t, a_s, *tabs)[:, :, :D]
    (logp * w).sum().backward()
    tabs2, a_t2, a_s2 = leaves()
    outs = [F.log_softmax(_AggregateFn.apply(tabs2[2 * h], tabs2[2 * h + 1], a_t2[h], a_s2[h], csr, mask_u8, D, 0.1)[:, :D], dim=1)
            for h in range(3)]
    ref = torch.stack(outs, dim=1)
    (ref * w).sum().backward()
    assert _rel(logp.detach().double(), ref.detach().double()) < 1e-5
    for h in range(6):
        assert _rel(tabs[h].grad.double(), tabs2[h].grad.double()) < 2e-5, f"table {h}"
        assert float(tabs[h].grad[:, D:].abs().max()) == 0.0 if D < 4 else True
    assert _rel(a_t.grad.double(), a_t2.grad.double()) < 1e-4 and _rel(a_s.grad.double(), a_s2.grad.double()) < 1e-4


@pytest.mark.parametrize("D,seed", [(128, 0), (64, 1), (36, 2), (16, 3)])
def test_pull_backward_with_hub_segments_equals_the_plain_pull(D, seed, monkeypatch):
    """Graphs with hub rows (in-degree and out-degree >= ops.HUB_THRESHOLD): the segmented pull backward
    (bgnn_adaptedconv_aggregate_bwd_pull_f32 with hub tables) equals the plain one to fp32 rounding in every output, and is deterministic."""
    from bridged_gnn_amd import ops, synth
    n = 3000
    ei, mask = synth.random_multigraph(n, 6 * n, frac_src=0.4, n_isolated=2, seed=seed)
    rng = np.random.default_rng(seed)
    hubs_in, hubs_out = rng.choice(n, size=5, replace=False), rng.choice(n, size=4, replace=False)
    extra_in = np.stack([rng.integers(0, n, size=5 * 700), np.repeat(hubs_in, 700)])          # 700 in-edges each
    extra_out = np.stack([np.repeat(hubs_out, 500), rng.integers(0, n, size=4 * 500)])         # 500 out-edges each
    ei = np.concatenate([ei, extra_in, extra_out], axis=1).astype(np.int64)
    csr = ops.build_dst_csr(_t(ei), n)
    assert csr.hub_tables() is not None and csr.transposed_hub_tables() is not None
    ld = ops.pad4(D)
    g = torch.Generator(device=DEV).manual_seed(seed)
    hS = torch.zeros(n, ld, device=DEV); hT = torch.zeros(n, ld, device=DEV)
    hS[:, :D] = torch.randn(n, D, device=DEV, generator=g); hT[:, :D] = torch.randn(n, D, device=DEV, generator=g)
    a1, a2 = torch.randn(D, device=DEV, generator=g) * 0.3, torch.randn(D, device=DEV, generator=g) * 0.3
    m8 = _t(mask).to(torch.uint8)
    monkeypatch.setenv("BGNN_HUB_ROWS", "0")
    out, alpha = ops.adaptedconv_aggregate(hS, hT, a1, a2, csr, m8, D, 0.1, want_alpha=True)
    gr = torch.zeros(n, ld, device=DEV); gr[:, :D] = torch.randn(n, D, device=DEV, generator=g)
    plain = ops.adaptedconv_aggregate_bwd(hS, hT, a1, a2, csr, m8, D, out, alpha, gr, 0.1)
    monkeypatch.delenv("BGNN_HUB_ROWS")
    hub = ops.adaptedconv_aggregate_bwd(hS, hT, a1, a2, csr, m8, D, out, alpha, gr, 0.1)
    hub2 = ops.adaptedconv_aggregate_bwd(hS, hT, a1, a2, csr, m8, D, out, alpha, gr, 0.1)
    for name, a, b, c in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), hub, plain, hub2):
        assert _rel(a.double().cpu(), b.double().cpu()) < (1e-5 if name.startswith("da") else 2e-6), name
        if name.startswith("dh"):
            assert torch.equal(a, c), name + " deterministic"


@pytest.mark.parametrize("D,heads,seed", [(2, 3, 0), (4, 2, 1), (3, 3, 2)])
def test_heads_backward_with_hub_segments_equals_the_plain_one(D, heads, seed, monkeypatch):
    """the interleaved-heads pull backward on a graph with in- and out-degree hubs: segments + fixed-order merges
    (bgnn_adaptedconv_aggregate_heads_bwd_f32 with hub tables) == the plain kernels (fp32 rounding), deterministic."""
    from bridged_gnn_amd import ops, synth
    n = 3000
    ei, mask = synth.random_multigraph(n, 6 * n, frac_src=0.4, n_isolated=2, seed=seed)
    rng = np.random.default_rng(seed)
    hubs_in, hubs_out = rng.choice(n, size=5, replace=False), rng.choice(n, size=4, replace=False)
    ei = np.concatenate([ei, np.stack([rng.integers(0, n, size=5 * 700), np.repeat(hubs_in, 700)]),
                         np.stack([np.repeat(hubs_out, 500), rng.integers(0, n, size=4 * 500)])], axis=1).astype(np.int64)
    csr = ops.build_dst_csr(_t(ei), n)
    assert csr.hub_tables() is not None and csr.transposed_hub_tables() is not None
    g = torch.Generator(device=DEV).manual_seed(seed)
    m8 = _t(mask).to(torch.uint8)
    t2s = torch.zeros(n, heads * 4, device=DEV); s2t = torch.zeros(n, heads * 4, device=DEV)
    for h in range(heads):
        t2s[:, 4 * h:4 * h + D] = torch.randn(n, D, device=DEV, generator=g)
        s2t[:, 4 * h:4 * h + D] = torch.randn(n, D, device=DEV, generator=g)
    a1 = torch.randn(heads, D, device=DEV, generator=g) * 0.3; a2 = torch.randn(heads, D, device=DEV, generator=g) * 0.3
    ms = torch.zeros(n, heads, 2, device=DEV)
    out = ops.adaptedconv_aggregate(t2s, s2t, a1, a2, csr, m8, D, 0.1, heads=heads, log_softmax=True, state_ms=ms, part=3)
    gr = torch.zeros(n, heads * 4, device=DEV)
    for h in range(heads):
        gr[:, 4 * h:4 * h + D] = torch.randn(n, D, device=DEV, generator=g)
    hub = ops.adaptedconv_aggregate_heads_bwd(t2s, s2t, a1, a2, csr, m8, D, heads, out, ms, gr, True, 0.1)
    hub2 = ops.adaptedconv_aggregate_heads_bwd(t2s, s2t, a1, a2, csr, m8, D, heads, out, ms, gr, True, 0.1)
    monkeypatch.setenv("BGNN_HUB_ROWS", "0")
    plain = ops.adaptedconv_aggregate_heads_bwd(t2s, s2t, a1, a2, csr, m8, D, heads, out, ms, gr, True, 0.1)
    for name, a, b, c in zip(("dh_t2s", "dh_s2t", "da_t2s", "da_s2t"), hub, plain, hub2):
        assert _rel(a.double().cpu(), b.double().cpu()) < (1e-5 if name.startswith("da") else 2e-6), name
        if name.startswith("dh"):
            assert torch.equal(a, c), name + " deterministic"
