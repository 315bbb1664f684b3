"""GPU: step 2's fused loss, metric counts and driver (ops.step2_*, bridged_gnn_amd.transfer) against the reference's own numbers in
tests/golden/transfer_office_a2d.npz (tools/gen_golden_transfer.py), against fp64 torch on the host, and against a loop composed
from the existing pieces (model forward, the torch-op loss of bench.py, optimizer.step(), separate eval forwards).
Past the grid cap of 1024 blocks: the three-table loss at (N, C) = (16389, 31), (16389, 40), (131077, 3), the
single-table loss at (524295, 2) and (16389, 31), the AUC count at N = 600 011 with and without ties against the integer rank
statistic on the host; and labels outside [0, C), which select nothing in the loss, the single-table loss and the counts."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FIX = "transfer_office_a2d.npz"
DEV = "cuda:0"
FWD_RTOL = 1e-6          # forward quantities (the bar of test_gpu_training.py)
GRAD_REL_OF_MAX = 2e-5   # gradients: of the table's largest (the bar used there for gradients)
TRAJ_RTOL = 2e-4         # loss trajectories of equal-seed loops (test_gpu_training.py:196)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ref_loss64(s, t, h, y, train, central, Lambda=1.0):
    """main_graph_knowledge_transfer.py:44-54 in fp64 on the host -> (terms [5], grads)"""
    s, t, h = (v.detach().double().cpu().requires_grad_(True) for v in (s, t, h))
    y, train, central = y.cpu(), train.cpu().bool(), central.cpu().bool()
    tt = train & ~central
    a = F.nll_loss(s[train], y[train])
    b = F.nll_loss(t[tt], y[tt])
    c = F.nll_loss(h[tt], y[tt])
    kl = F.kl_div(h, t, log_target=True, reduction="batchmean")
    loss = (a * 2. + b + c) / 4. + kl * Lambda
    grads = torch.autograd.grad(loss, (s, t, h), allow_unused=True)
    return np.array([loss.item(), a.item(), b.item(), c.item(), kl.item()]), [g if g is not None else torch.zeros_like(s) for g in grads]


def check_terms(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rel = np.abs(got - want) / np.abs(want)
    print(f"[{what}] loss terms rel err {rel}")
    assert (rel <= FWD_RTOL).all(), (what, got, want)


def check_grads(got, want, what):
    for name, g, w in zip("sth", got, want):
        w = w.double()
        err = float((g.double().cpu() - w).abs().max())
        bar = GRAD_REL_OF_MAX * float(w.abs().max())
        print(f"[{what}] grad_{name}: max err {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, name, err, bar)


def run_loss(s, t, h, y, train, central, Lambda=1.0):
    from bridged_gnn_amd import ops
    s, t, h = (v.detach().requires_grad_(True) for v in (s, t, h))
    loss, terms = ops.step2_loss(s, t, h, y, train, central, Lambda, return_terms=True)
    loss.backward()
    return loss, terms, (s.grad, t.grad, h.grad)


def test_loss_and_gradients_match_the_reference_fixture(golden):
    g = golden(FIX)
    s, t, h = (_dev(g[f"office/lp_{k}"]) for k in "sth")
    y, train, central = _dev(g["office/sub_y"]), _dev(g["office/sub_train"]), _dev(g["office/sub_central"])
    loss, terms, grads = run_loss(s, t, h, y, train, central)
    check_terms(terms[:5].cpu().numpy(), g["office/loss"], "fixture")
    assert abs(float(loss.detach()) - g["office/loss"][0]) <= 2e-7 * abs(g["office/loss"][0])          # the fp32 rounding of the fp64 total
    assert terms[5:7].tolist() == [float(g["office/sub_train"].sum()), float((g["office/sub_train"] & ~g["office/sub_central"]).sum())]
    check_grads(grads, [torch.from_numpy(g[f"office/grad_{k}"]) for k in "sth"], "fixture")


def random_case(N, C, seed, strided):
    gen = torch.Generator().manual_seed(seed)
    ld = C + 5 if strided else C
    tabs = []
    for _ in range(3):
        buf = torch.full((N, ld), float("nan"))
        buf[:, :C] = F.log_softmax(torch.randn(N, C, generator=gen) * 2, dim=1)
        tabs.append(buf.to(DEV)[:, :C])
    y = torch.randint(0, C, (N,), generator=gen)
    train = torch.rand(N, generator=gen) < 0.6
    central = torch.rand(N, generator=gen) < 0.7
    return tabs, y.to(DEV), train.to(DEV), central.to(DEV)


@pytest.mark.parametrize("C", [1, 2, 3, 31, 40])
@pytest.mark.parametrize("strided", [False, True])
def test_loss_over_class_counts_and_strides(C, strided):
    N = 1003                                   # not a multiple of any block's rows
    (s, t, h), y, train, central = random_case(N, C, 100 + C, strided)
    assert s.stride(0) == (C + 5 if strided else C)
    want, wgrads = ref_loss64(s, t, h, y, train, central, Lambda=0.7)
    loss, terms, grads = run_loss(s, t, h, y, train, central, Lambda=0.7)
    if C == 1:                                 # log-probs of one class are all 0: every term is exactly 0 (no relative error to take)
        assert terms[:5].abs().max().item() == 0.0 and np.abs(want).max() == 0.0
    else:
        check_terms(terms[:5].cpu().numpy(), want, f"C={C} strided={strided}")
    check_grads(grads, wgrads, f"C={C} strided={strided}")
    loss2, terms2, grads2 = run_loss(s, t, h, y, train, central, Lambda=0.7)
    assert torch.equal(terms, terms2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))      # bitwise


def test_loss_with_an_empty_target_selection():
    (s, t, h), y, train, central = random_case(777, 5, 3, False)
    central = central | train                  # no train row in the target domain
    want, wgrads = ref_loss64(s, t, h, y, train, central)
    loss, terms, grads = run_loss(s, t, h, y, train, central)
    v = terms.cpu().numpy()
    assert np.isnan(v[0]) and np.isnan(v[2]) and np.isnan(v[3]) and np.isnan(want[2]) and v[6] == 0
    check_terms(v[[1, 4]], want[[1, 4]], "empty target")
    # the reference's gradients: NaN where the NaN mean reaches (nowhere: an empty selection has no rows), finite elsewhere
    assert all(torch.isfinite(g).all() for g in grads)
    check_grads(grads, [torch.nan_to_num(w) for w in wgrads], "empty target")


@pytest.mark.parametrize("C", [2, 31])
def test_single_table_loss(C):
    from bridged_gnn_amd import ops
    (s, _, _), y, train, _ = random_case(1003, C, 7, True)
    s = s.detach().requires_grad_(True)
    loss, terms = ops.step2_nll(s, y, train, return_terms=True)
    (loss * 3).backward()
    s64 = s.detach().double().cpu().requires_grad_(True)
    ref = F.nll_loss(s64[train.cpu()], y.cpu()[train.cpu()])
    (ref * 3).backward()
    assert abs(terms[0].item() - ref.item()) <= FWD_RTOL * abs(ref.item()) and terms[1].item() == int(train.sum())
    err, bar = float((s.grad.double().cpu() - s64.grad).abs().max()), GRAD_REL_OF_MAX * float(s64.grad.abs().max())
    assert err <= bar


# ---- past the grid cap: every block takes a second trip of its grid-stride loop ------------------------------------------------
S2_MAX_BLOCKS = 1024                           # bgnn_step2.hip: `constexpr int S2_MAX_BLOCKS = 1024`


def s2_blocks_wanted(N, C):
    """the blocks `s2_blocks` (bgnn_step2.hip) would launch without its cap: 256 / GL rows per block, GL = s2_group(C) lanes per row"""
    gl = 1
    while gl < C and gl < 32:
        gl *= 2
    return -(-N // (256 // gl))


@pytest.mark.parametrize("N,C", [(16389, 31), (16389, 40), (131077, 3)])
@pytest.mark.parametrize("strided", [False, True])
def test_loss_past_the_grid_cap(N, C, strided):
    """forward, backward and the finishing block's sum over all 1024 partial rows"""
    assert s2_blocks_wanted(N, C) > S2_MAX_BLOCKS
    (s, t, h), y, train, central = random_case(N, C, 200 + C, strided)
    assert s.stride(0) == (C + 5 if strided else C)
    want, wgrads = ref_loss64(s, t, h, y, train, central, Lambda=0.7)
    loss, terms, grads = run_loss(s, t, h, y, train, central, Lambda=0.7)
    check_terms(terms[:5].cpu().numpy(), want, f"N={N} C={C} strided={strided}")
    assert terms[5:7].tolist() == [float(train.sum()), float((train & ~central).sum())]
    check_grads(grads, wgrads, f"N={N} C={C} strided={strided}")
    loss2, terms2, grads2 = run_loss(s, t, h, y, train, central, Lambda=0.7)
    assert torch.equal(terms, terms2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))      # bitwise


@pytest.mark.parametrize("N,C", [(524295, 2), (16389, 31)])
def test_single_table_loss_past_the_grid_cap(N, C):
    from bridged_gnn_amd import ops
    # forward: one row per lane (s2_nll_fwd_kernel: s2_blocks(N, 1)), backward: 256 / GL rows per block (s2_nll_bwd_kernel)
    assert s2_blocks_wanted(N, C) > S2_MAX_BLOCKS and (C != 2 or s2_blocks_wanted(N, 1) > S2_MAX_BLOCKS)
    (s, _, _), y, train, _ = random_case(N, C, 17, True)
    s = s.detach().requires_grad_(True)
    loss, terms = ops.step2_nll(s, y, train, return_terms=True)
    (loss * 3).backward()
    s64 = s.detach().double().cpu().requires_grad_(True)
    ref = F.nll_loss(s64[train.cpu()], y.cpu()[train.cpu()])
    (ref * 3).backward()
    assert abs(terms[0].item() - ref.item()) <= FWD_RTOL * abs(ref.item()) and terms[1].item() == int(train.sum())
    err, bar = float((s.grad.double().cpu() - s64.grad).abs().max()), GRAD_REL_OF_MAX * float(s64.grad.abs().max())
    print(f"[N={N} C={C}] nll rel err {abs(terms[0].item() - ref.item()) / abs(ref.item()):.3e}, grad max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def test_labels_outside_the_classes_select_nothing():
    """the kernels' contract for y < 0 and y >= C: such a row is in no selection.  Loss terms, row counts and all three gradients,
    the single-table loss and its gradient and the confusion counts equal, bit for bit, the same calls with those rows cleared
    from the masks and relabelled 0 -- and the cleared calls meet the fp64 reference."""
    from bridged_gnn_amd import ops, transfer
    N, C = 1003, 31
    (s, t, h), y, train, central = random_case(N, C, 300, True)
    gen = torch.Generator().manual_seed(301)
    u = torch.rand(N, generator=gen).to(DEV)
    bad = train & (u < 0.05)
    low = bad & (torch.rand(N, generator=gen).to(DEV) < 0.5)
    assert 10 <= int(bad.sum()) and 0 < int(low.sum()) < int(bad.sum()) and bool((bad & ~central).any()) and bool((bad & central).any())
    y_bad = torch.where(low, torch.full_like(y, -1), torch.where(bad, torch.full_like(y, C), y))
    y_clr, train_clr = torch.where(bad, torch.zeros_like(y), y), train & ~bad
    # the three-table loss
    loss, terms, grads = run_loss(s, t, h, y_bad, train, central, Lambda=0.7)
    loss_c, terms_c, grads_c = run_loss(s, t, h, y_clr, train_clr, central, Lambda=0.7)
    assert torch.equal(terms, terms_c) and torch.equal(loss.detach(), loss_c.detach())
    assert all(torch.equal(a, b) for a, b in zip(grads, grads_c))
    want, wgrads = ref_loss64(s, t, h, y_clr, train_clr, central, Lambda=0.7)
    check_terms(terms_c[:5].cpu().numpy(), want, "cleared labels")
    check_grads(grads_c, wgrads, "cleared labels")
    assert terms_c[5:7].tolist() == [float(train_clr.sum()), float((train_clr & ~central).sum())]
    # the single-table loss
    outs = []
    for yy, mm in ((y_bad, train), (y_clr, train_clr)):
        sv = s.detach().requires_grad_(True)
        l1, t1 = ops.step2_nll(sv, yy, mm, return_terms=True)
        (l1 * 3).backward()
        outs.append((t1, sv.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    s64 = s.detach().double().cpu().requires_grad_(True)
    ref = F.nll_loss(s64[train_clr.cpu()], y_clr.cpu()[train_clr.cpu()])
    (ref * 3).backward()
    assert abs(outs[1][0][0].item() - ref.item()) <= FWD_RTOL * abs(ref.item()) and outs[1][0][1].item() == int(train_clr.sum())
    assert float((outs[1][1].double().cpu() - s64.grad).abs().max()) <= GRAD_REL_OF_MAX * float(s64.grad.abs().max())
    # the confusion counts: the bad rows sit in selection 0 (train) and, some of them, in the two others
    bits = [train, (u < 0.3) & ~central, ((u > 0.5) | bad) & ~central]
    assert all(bool((b & bad).any()) for b in bits)
    bits_clr = [b & ~bad for b in bits]

    def pack(bs):
        return (bs[0].to(torch.uint8) | (bs[1].to(torch.uint8) << 1) | (bs[2].to(torch.uint8) << 2)).contiguous()
    combos = transfer._DTC_COMBOS
    got = ops.step2_counts((s, t, h), y_bad, pack(bits), combos)
    got_c = ops.step2_counts((s, t, h), y_clr, pack(bits_clr), combos)
    assert torch.equal(got, got_c) and torch.equal(got_c, bincount_counts((s, t, h), y_clr, bits_clr, combos, C))


def auc_by_ranks(score, y, sel):
    """roc_auc_score(y[sel], score[sel]) as its integer rank statistic on the host: over (positive, negative) pairs, 2 per negative
    below the positive and 1 per negative level with it, in int64, then one fp64 quotient"""
    score, y, sel = (v.cpu().numpy() for v in (score, y, sel))
    neg = np.sort(score[sel & (y == 0)])
    pos = score[sel & (y == 1)]
    below = np.searchsorted(neg, pos, side="left").astype(np.int64)
    upto = np.searchsorted(neg, pos, side="right").astype(np.int64)
    u2 = int((2 * below + (upto - below)).sum())
    return u2 / (2.0 * pos.shape[0] * neg.shape[0]), pos.shape[0], neg.shape[0]


@pytest.mark.parametrize("ties", [False, True])
def test_auc_past_one_trip_of_the_grid(ties):
    from bridged_gnn_amd import ops
    N = 600_011
    assert N > S2_MAX_BLOCKS * 256                 # s2_auc_kernel: one row per lane, s2_blocks(N, 1) blocks
    gen = torch.Generator().manual_seed(400)
    y = torch.randint(0, 2, (N,), generator=gen)
    score = torch.rand(N, generator=gen) + 0.1 * y  # positives score a little higher: an AUC away from 1/2
    if ties:
        score = torch.round(score * 64) / 64       # 72 distinct scores at the most: every positive has thousands of level negatives
    sel = torch.rand(N, generator=gen) < 0.5
    ref, n_pos, n_neg = auc_by_ranks(score, y, sel)
    assert min(n_pos, n_neg) > 100_000 and 0.55 < ref < 0.75
    assert score.dtype == torch.float32 and (np.unique(score.numpy()).shape[0] <= 72) == ties
    got = float(ops.step2_auc(score.to(DEV), y.to(DEV), sel.to(DEV)))
    print(f"ties={ties}: auc {got!r}, rank statistic {ref!r}")
    assert abs(got - ref) <= 1e-12


def bincount_counts(tabs, y, sel_bits, combos, C):
    out = []
    for tb, bit in combos:
        m = sel_bits[bit]
        out.append(torch.bincount(y[m] * C + tabs[tb].argmax(1)[m], minlength=C * C).view(C, C))
    return torch.stack(out)


@pytest.mark.parametrize("N,C", [(1003, 2), (1003, 31), (5000, 49), (5000, 50), (5000, 60), (1_000_000, 2), (1_000_000, 31)])
def test_counts_equal_bincount(N, C):
    from bridged_gnn_amd import ops, transfer
    (s, t, h), y, train, central = random_case(N, C, 11, N < 10000)
    gen = torch.Generator().manual_seed(5)
    u = torch.rand(N, generator=gen).to(DEV)
    bits = [train, (u < 0.3) & ~central, (u > 0.5) & ~central]
    sel = (bits[0].to(torch.uint8) | (bits[1].to(torch.uint8) << 1) | (bits[2].to(torch.uint8) << 2)).contiguous()
    # 5 C^2 cells: C = 49 -> 12005, the largest LDS histogram (12288 cells, 48 KiB dynamic LDS); C = 50 -> 12500 and C = 60 -> global atomics
    combos = transfer._DTC_COMBOS
    got = ops.step2_counts((s, t, h), y, sel, combos)
    want = bincount_counts((s, t, h), y, bits, combos, C)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(ops.step2_counts((s, t, h), y, sel, combos), got)


def test_counts_on_the_fixture_tables(golden):
    from bridged_gnn_amd import ops
    g = golden(FIX)
    tabs = [_dev(g[f"office/lp_{k}"]) for k in "sth"]
    for tb in tabs:                                     # tie-free by assertion
        top = tb.topk(2, dim=1).values
        assert bool((top[:, 0] > top[:, 1]).all())
    y, train, central = _dev(g["office/sub_y"]), _dev(g["office/sub_train"]), _dev(g["office/sub_central"])
    lab = y >= 0
    bits = [train & lab, ~central & lab, lab]
    sel = (bits[0].to(torch.uint8) | (bits[1].to(torch.uint8) << 1) | (bits[2].to(torch.uint8) << 2)).contiguous()
    combos = ((0, 0), (1, 1), (2, 1), (0, 2), (2, 2))
    got = ops.step2_counts(tabs, y, sel, combos)
    assert torch.equal(got, bincount_counts(tabs, y.clamp_min(0), bits, combos, 31))


@pytest.mark.parametrize("pre", ["bin/", "bin/tie/"])
def test_auc_matches_the_reference(golden, pre):
    from bridged_gnn_amd import ops, transfer
    from bridged_gnn_amd.data import Data
    g = golden(FIX)
    y = _dev(g["bin/y"])
    tgt = ~g["bin/central_mask"]
    sels = [_dev(m) for m in (g["bin/train_mask"], g["bin/val_mask"] & tgt, g["bin/test_mask"] & tgt)]
    for i, (k, m) in enumerate(zip("shh", sels)):
        auc = float(ops.step2_auc(_dev(g[f"{pre}score_{k}"]), y, m))
        assert abs(auc - g[pre + "test_auc"][i]) <= 1e-12, (k, auc, g[pre + "test_auc"][i])
    for i, k in enumerate("sth"):
        assert abs(float(ops.step2_auc(_dev(g[f"{pre}score_{k}"]), y, sels[2])) - g[pre + "each_auc"][i]) <= 1e-12
    # through the driver, on a stand-in model that returns the fixture's tables (the scores are exp'ed on the device)
    data = Data(x=_dev(g["bin/x"]), edge_index=_dev(g["bin/edge_index"]), y=y,
                **{k: _dev(g["bin/" + k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    tabs = tuple(_dev(g[f"{pre}lp_{k}"]) for k in "sth")

    class Tables(torch.nn.Module):
        def forward(self, d):
            return (*tabs, None)
    m = Tables()
    assert np.abs(np.array(transfer.test(data, m, "bin", gnn="KTGNN", metric="auc")) - g[pre + "test_auc"]).max() <= 1e-12
    assert np.abs(np.array(transfer.get_each_clf_res(data, m, metric="auc")) - g[pre + "each_auc"]).max() <= 1e-12
    for metric, key in (("f1", "test_f1"), ("acc", "test_acc")):
        assert np.abs(np.array(transfer.test(data, m, "bin", gnn="KTGNN", metric=metric)) - g[pre + key]).max() <= 1e-12
    assert np.abs(np.array(transfer.test(data, m, "bin", gnn="KTGNN", f1_average="micro")) - g[pre + "test_f1_micro"]).max() <= 1e-12
    assert np.abs(np.array(transfer.get_each_clf_res(data, m)) - g[pre + "each_f1"]).max() <= 1e-12
    with pytest.raises(ValueError, match="Only one class"):
        ops_auc = ops.step2_auc(_dev(g[f"{pre}score_s"]), torch.ones_like(y), sels[0])
        transfer._check_auc(float(ops_auc))


def office_data(golden):
    from bridged_gnn_amd.data import Data
    og = golden("office_a2d_graph.npz")
    d = Data(x=_dev(og["x"]), edge_index=_dev(og["edge_index"]).long(), y=_dev(og["y"]).long(),
             **{k: _dev(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False                    # main_graph_knowledge_transfer.py:404
    d.to_undirected_()                                 # :411
    return d


def build_ktgnn(data, C, hidden, dropout):
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    return KTGNN_no_complement(data.x.shape[1], C, 2, hidden, root_weight=False, use_dist_loss=False, dropout=dropout, use_bn=True, step=1,
                               dim_share=data.x.shape[1], need_complement=False).to(DEV)


def test_scores_of_the_fixture_model_reproduce_the_reference(golden):
    from bridged_gnn_amd import transfer
    g = golden(FIX)
    data = office_data(golden)
    model = build_ktgnn(data, 31, 64, 0.5)
    model.load_state_dict({k[len("office/param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("office/param/")})
    model.eval()
    with torch.no_grad():
        lps = [t.clone() for t in model(data)[:3]]
    # no argmax may flip: the top-two margin of every scored row exceeds twice the forward bar (cap: zero excluded rows)
    tgt = ~data.central_mask
    scored = ((lps[0], data.train_mask | (data.test_mask & tgt)), (lps[1], data.test_mask & tgt), (lps[2], (data.val_mask | data.test_mask) & tgt))
    for lp, rows in scored:
        top = lp[rows].double().topk(2, dim=1).values
        bar = 2 * (1e-5 * top.abs().max(1).values + 1e-6 * lp.abs().max().double())
        assert bool(((top[:, 0] - top[:, 1]) > bar).all())
    rows = torch.from_numpy(g["office/rows"])
    for k, lp in zip("sth", lps):                      # the HIP forward against the stored rows; its predictions against the reference's
        ref = g[f"office/lp_{k}"]
        print(f"lp_{k}: max |HIP - reference fp32| on the stored rows {np.abs(lp[rows].cpu().numpy() - ref).max():.3e} (max |lp| {np.abs(ref).max():.3f})")
        assert torch.equal(lp.argmax(1).cpu(), torch.from_numpy(g[f"office/pred_{k}"].astype(np.int64)))
    for got, key in ((transfer.test(data, model, "office", gnn="KTGNN"), "office/test_f1"),
                     (transfer.test(data, model, "office", gnn="KTGNN", f1_average="micro"), "office/test_f1_micro"),
                     (transfer.test(data, model, "office", gnn="KTGNN", metric="acc"), "office/test_acc"),
                     (transfer.get_each_clf_res(data, model), "office/each_f1")):
        print(key, got, g[key])
        assert np.abs(np.array(got) - g[key]).max() <= 1e-12, key


def test_train_gnn_follows_the_references_recorded_run(golden):
    """train_gnn(dropout=0, verbose=False) for the fixture's 20 epochs against the reference's fp64 run.  Bars: the yardstick of a
    quantity is the largest deviation, over the 20 epochs, of the reference's own fp32 run from its fp64 run; the HIP run (fp32 with
    other summation orders) is allowed 4x that, per quantity: each of the four loss series and each of the six F1 series (test's
    train / val / test, get_each_clf_res's lp_s / lp_t / lp_t^) has its own yardstick.  Three F1 series did not move between the
    reference's two runs: their bar is 0, i.e. the HIP run's predictions on those rows must give the fp64 run's F1 exactly.
    Yardstick / measured on an MI355X / bar (profiles/transfer/README.md): loss_train 8.91e-06 / 2.54e-07 / 3.56e-05; loss_target
    1.91e-05 / 2.73e-07 / 7.66e-05; loss_target_only 8.05e-05 / 2.38e-07 / 3.22e-04; loss_kl 4.46e-06 / 1.99e-08 / 1.78e-05; F1 train
    2.93e-04 / 0 / 1.17e-03; val 0 / 0 / 0; test 2.31e-03 / 0 / 9.24e-03; each lp_s 0 / 0 / 0; lp_t 0 / 0 / 0; lp_t^ 2.31e-03 / 0 /
    9.24e-03; best epoch 19 = 19 (the recorded loss_target falls monotonically: the selection RULE is pinned by
    tests/test_transfer_host.py and by the dropout run below, not here)."""
    from bridged_gnn_amd import transfer
    g = golden(FIX)
    data = office_data(golden)
    hist = {}
    lb, each = transfer.train_gnn(types.SimpleNamespace(dataset_name="office_amazon2dslr"), transfer.pyg_dataset(data), data, save=False,
                                  repeat=1, num_epoch=20, step_size=100, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, lr=1e-3,
                                  wd=5e-3, use_shceduler=True, step=1, Lambda=1., metric="f1", f1_average="macro", dropout=0.0,
                                  verbose=False, history=hist)
    got = np.array([lb["source&target"], lb["target_hat"], lb["target"], lb["kl"]]).T
    r64, r32 = g["run64/loss"], g["run32/loss"]
    yard = np.abs(r32 - r64).max(0)
    dev = np.abs(got - r64).max(0)
    print("loss yardstick", yard, "measured", dev, "bar", 4 * yard)
    f_got = np.concatenate([np.array(hist["eval_res"]), np.array([each["source&target"], each["target"], each["target_hat"]]).T], axis=1)
    f64 = np.concatenate([g["run64/eval_res"], g["run64/eval_res_each"]], axis=1)
    f32 = np.concatenate([g["run32/eval_res"], g["run32/eval_res_each"]], axis=1)
    f_yard = np.abs(f32 - f64).max(0)
    f_dev = np.abs(f_got - f64).max(0)
    print("f1 yardstick", f_yard, "measured", f_dev, "bar", 4 * f_yard)
    print("best epoch", hist["best_epoch"], int(g["run64/best_epoch"]))
    assert (dev <= 4 * yard).all()
    assert (f_dev <= 4 * f_yard).all()
    assert hist["best_epoch"] == int(g["run64/best_epoch"])


def torch_op_loss(lb, lt, lth, y, tm, cm):
    """the torch-op form of bench.py:706-715"""
    tmt = tm & ~cm
    w_b, w_t = tm.float() / tm.sum(), tmt.float() / tmt.sum()
    yi = y.clamp_min(0)[:, None]
    nll = lambda logp, w: -(logp.gather(1, yi).squeeze(1) * w).sum()
    kl = F.kl_div(lth, lt, log_target=True, reduction="batchmean")
    return (2 * nll(lb, w_b) + nll(lt, w_t) + nll(lth, w_t)) / 4 + kl, nll(lth, w_t), nll(lt, w_t), kl


def test_train_gnn_with_dropout_equals_the_composed_loop(golden):
    from torch.optim.lr_scheduler import StepLR
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.utils import set_random_seed
    data = office_data(golden)
    E = 8
    hist = {}
    lb, _ = transfer.train_gnn(types.SimpleNamespace(dataset_name="office"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=E,
                               step_size=3, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False,
                               history=hist)
    set_random_seed(0)
    model = build_ktgnn(data, 31, 64, 0.5)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
    sched = StepLR(opt, step_size=3, gamma=0.1)
    want = []
    for _ in range(E):
        model.train()
        opt.zero_grad()
        lp_s, lp_t, lp_h, _ = model(data)
        terms = torch_op_loss(lp_s, lp_t, lp_h, data.y, data.train_mask, data.central_mask)
        terms[0].backward()
        opt.step()
        want.append([float(v) for v in terms])
        model.eval()
        with torch.no_grad():
            model(data)
            model(data)                                 # test() and get_each_clf_res(): two eval forwards
        sched.step()
    got = np.array([lb["source&target"], lb["target_hat"], lb["target"], lb["kl"]]).T
    print("dropout loop max rel dev", (np.abs(got - np.array(want)) / np.abs(np.array(want))).max(0))
    assert np.allclose(got, np.array(want), rtol=TRAJ_RTOL), (got, want)
    # the best epoch is the first strict minimum of loss_target (nll of lp_t^) of THIS run, whatever its shape
    lt = lb["target_hat"]
    assert hist["best_epoch"] == transfer.select_best(lt)[-1] == int(np.argmin(lt))
    assert hist["best_acc"]["loss"] == min(lt) and [hist["best_acc"][k] for k in ("train", "val", "test")] == hist["eval_res"][hist["best_epoch"]]


def test_deferred_epochs_do_not_wait_for_the_device(golden, monkeypatch):
    from bridged_gnn_amd import transfer
    data = office_data(golden)
    calls = {"sync": 0, "epochs": 0}
    step0, drain0 = transfer._train_step, transfer._History.drain
    names = ("item", "tolist", "cpu", "numpy", "__bool__", "__int__", "__float__", "nonzero")
    orig = {n: getattr(torch.Tensor, n) for n in names}

    def counted(n):
        def f(self, *a, **k):
            if calls["epochs"] and self.is_cuda:
                calls["sync"] += 1
            return orig[n](self, *a, **k)
        return f

    def step(*a, **k):
        if calls["epochs"] == 0:
            torch.cuda.set_sync_debug_mode("error")     # from the first epoch on a synchronising torch call raises
            for n in names:
                monkeypatch.setattr(torch.Tensor, n, counted(n))
            monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.__setitem__("sync", calls["sync"] + 1))
        calls["epochs"] += 1
        return step0(*a, **k)

    def drain(self):
        torch.cuda.set_sync_debug_mode("default")       # the loop is over: the history is read once
        calls["epochs"] = 0
        return drain0(self)
    monkeypatch.setattr(transfer, "_train_step", step)
    monkeypatch.setattr(transfer._History, "drain", drain)
    seen = []
    try:
        hist = {}
        transfer.train_gnn(types.SimpleNamespace(dataset_name="office"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=6, step_size=2,
                           gnn="KTGNN", seed=0, num_layer=2, hidden=64, verbose=False, history=hist)
        seen.append(calls["sync"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert seen == [0] and len(hist["eval_res"]) == 6 and hist["best_epoch"] is not None


def test_train_gnn_noDTC_equals_the_composed_graphsage_loop(golden):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.sage import GraphSAGE
    from bridged_gnn_amd.utils import set_random_seed
    data = office_data(golden)
    ds = transfer.pyg_dataset(data)
    hist = {}
    assert transfer.train_gnn_noDTC(types.SimpleNamespace(dataset_name="office"), ds, data, repeat=1, num_epoch=5, gnn="GraphSAGE", seed=0,
                                    num_layer=2, hidden=64, use_scheduler=False, dropout=0.5, verbose=False, history=hist) is None
    set_random_seed(0)
    model = GraphSAGE(ds, 2, 64, root_weight=True, dropout=0.5).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
    want, scores = [], []
    tm = data.train_mask
    w = tm.float() / tm.sum()
    for _ in range(5):
        model.train()
        opt.zero_grad()
        lp = model(data)
        loss = -(lp.gather(1, data.y.clamp_min(0)[:, None]).squeeze(1) * w).sum()
        loss.backward()
        opt.step()
        want.append(float(loss))
        model.eval()
        with torch.no_grad():
            pred = model(data).argmax(1)
        scores.append([transfer.f1_from_counts(torch.bincount(data.y[m] * 31 + pred[m], minlength=961).view(31, 31).cpu().numpy())
                       for m in (data.train_mask, data.val_mask, data.test_mask)])
    assert np.allclose(hist["loss_train"], want, rtol=TRAJ_RTOL), (hist["loss_train"], want)
    f_dev = np.abs(np.array(hist["eval_res"]) - np.array(scores)).max()
    print("noDTC f1 dev", f_dev)
    # both loops are eager fp32 with equal seeds and differ in the loss's summation order only; an F1 is a function of integer counts,
    # so any deviation is a flipped prediction: the bar is equality (up to the 1e-12 of the host formula)
    assert f_dev <= 1e-12
    lt = hist["loss_train"]
    assert hist["best_epoch"] == transfer.select_best(lt)[-1] == int(np.argmin(lt))


@pytest.mark.parametrize("extra", [["--to_undirected"], ["--to_undirected", "--no_dtc"]])
def test_main_runs_from_a_saved_bridged_graph(golden, tmp_path, extra, capsys):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.data import Data, save_bridged_graph
    og = golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.from_numpy(og["edge_index"]).long(), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    path = str(tmp_path / "office_amazon2dslr_bridged_graph.dat")
    save_bridged_graph(d, path)
    res = transfer.main(["--num_layer", "2", "--hidden_dim", "64", "--num_epoch", "3", "--dataset_name", "office_amazon2dslr",
                         "--path_data", path] + extra)
    out = capsys.readouterr().out
    assert out.count("Epoch: 00") == 3 and "[Best Score]" in out and "[Run-1 score]" in out
    if "--no_dtc" in extra:
        assert res is None
    else:
        lb, each = res
        assert len(lb["source&target"]) == 3 and all(np.isfinite(lb[k]).all() for k in lb) and len(each["target_hat"]) == 3
        assert out.count("Loss_clf:") == 3


def test_setup_refuses_what_sklearn_would_choke_on(golden):
    from bridged_gnn_amd import transfer
    data = office_data(golden)
    model = build_ktgnn(data, 31, 64, 0.5)
    src = int(torch.nonzero(data.central_mask)[0])
    data.val_mask = data.val_mask.clone()
    data.val_mask[src] = True
    with pytest.raises(ValueError, match="source"):
        transfer.test(data, model, "office", gnn="KTGNN")
    data = office_data(golden)
    data.y = data.y.clone()
    data.y[int(torch.nonzero(data.test_mask)[0])] = -1
    with pytest.raises(ValueError, match="labels"):
        transfer.test(data, model, "office", gnn="KTGNN")


def test_public_single_step_and_scoring_entry_points(golden):
    """train, train_noDTC, test_noDTC, test(gnn != 'KTGNN') and get_each_clf_res(metric='acc') against the same quantities formed with
    torch ops on twin models (same seed, dropout off)."""
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.sage import GraphSAGE
    from bridged_gnn_amd.utils import set_random_seed
    data = office_data(golden)
    y = data.y
    tgt = ~data.central_mask

    def twins(make):
        out = []
        for _ in range(2):
            set_random_seed(3)
            m = make()
            out.append((m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)))
        return out
    (m1, o1), (m2, o2) = twins(lambda: build_ktgnn(data, 31, 64, 0.0))
    before = [p.detach().clone() for p in m1.parameters()]
    got = transfer.train(data, m1, o1, gnn="KTGNN", Lambda=0.5, verbose=False)
    m2.train()
    o2.zero_grad()
    lp_s, lp_t, lp_h, _ = m2(data)
    total, nll_h, nll_t, kl = torch_op_loss(lp_s, lp_t, lp_h, y, data.train_mask, data.central_mask)
    want = [float(total - 0.5 * kl), float(nll_h), float(nll_t), float(kl)]            # (loss, loss_clf_t2 [lp_t^], loss_clf_t1 [lp_t], loss_kl)
    assert len(got) == 4 and all(isinstance(v, float) for v in got) and np.allclose(got, want, rtol=1e-5), (got, want)
    assert abs(want[1] - want[2]) > 1e-3 * abs(want[1])                                # the two target terms differ: their order is checked
    (total - 0.5 * kl).backward()
    o2.step()
    moved = [float((a.detach() - b).abs().max()) for a, b in zip(m1.parameters(), before)]
    assert max(moved) > 5e-4 and max(moved) <= 1.1e-3                                  # the optimizer step was taken (Adam's first step: ~lr)
    # get_each_clf_res(metric='acc'): the three heads' accuracy on test & ~central
    m2.eval()
    with torch.no_grad():
        lps = m2(data)[:3]
    sel = data.test_mask & tgt
    want = [float((lp.argmax(1)[sel] == y[sel]).double().mean()) for lp in lps]
    assert np.abs(np.array(transfer.get_each_clf_res(data, m2, metric="acc")) - np.array(want)).max() <= 1e-12
    # the plain backbone
    ds = transfer.pyg_dataset(data)
    assert (ds.num_classes, ds.num_nodes, ds.num_features, ds.num_edges, ds[0]) == (31, 3408, 256, data.edge_index.shape[1], data)
    (g1, p1), (g2, p2) = twins(lambda: GraphSAGE(ds, 2, 64, root_weight=True, dropout=0.0).to(DEV))
    got = transfer.train_noDTC(data, g1, p1, gnn="GraphSAGE")
    g2.train()
    p2.zero_grad()
    tm = data.train_mask
    ref = F.nll_loss(g2(data)[tm], y[tm])
    assert isinstance(got, float) and abs(got - float(ref)) <= 1e-5 * abs(float(ref))
    ref.backward()
    p2.step()
    g2.eval()
    with torch.no_grad():
        pred = g2(data).argmax(1)
    cms = [torch.bincount(y[m] * 31 + pred[m], minlength=961).view(31, 31).cpu().numpy() for m in (tm, data.val_mask, data.test_mask)]
    for kw, fn in ((dict(metric="f1"), transfer.f1_from_counts), (dict(metric="f1", f1_average="micro"), lambda c: transfer.f1_from_counts(c, "micro")),
                   (dict(metric="acc"), transfer.accuracy_from_counts)):
        assert np.abs(np.array(transfer.test_noDTC(data, g2, gnn="GraphSAGE", **kw)) - np.array([fn(c) for c in cms])).max() <= 1e-12
    assert transfer.test(data, g2, "office", gnn="GraphSAGE") == transfer.test_noDTC(data, g2, gnn="GraphSAGE")


def test_step2_loss_inside_a_captured_graph():
    """forward + backward of ops.step2_loss captured into a HIP graph and replayed on new table contents, with eager work (a large
    torch reduction, a count pass) between the replays: every replay equals the eager pass on the same contents bit for bit."""
    from bridged_gnn_amd import ops
    N, C = 200_000, 31
    (s, t, h), y, train, central = random_case(N, C, 21, False)
    train_u8, central_u8 = ops.as_u8(train), ops.as_u8(central)
    st = [v.clone().requires_grad_(True) for v in (s, t, h)]

    def fwd_bwd():
        loss, terms = ops.step2_loss(*st, y, train_u8, central_u8, 0.7, return_terms=True)
        loss.backward()
        return loss, terms
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for v in st:
                v.grad = None
            fwd_bwd()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in st:
        v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, terms = fwd_bwd()
    gen = torch.Generator().manual_seed(9)
    for rep in range(3):
        new = [F.log_softmax(torch.randn(N, C, generator=gen) * (1 + rep), dim=1).to(DEV) for _ in range(3)]
        with torch.no_grad():
            for v, n in zip(st, new):
                v.copy_(n)
        junk = torch.randn(4_000_000, device=DEV).sum()                # eager work between replays, multi-block reduction included
        ops.step2_counts(new, y, ops.as_u8(train), ((0, 0),))
        graph.replay()
        torch.cuda.synchronize()
        e_loss, e_terms, e_grads = run_loss(*new, y, train, central, Lambda=0.7)
        assert torch.equal(terms, e_terms) and torch.equal(loss.detach(), e_loss.detach()), rep
        assert all(torch.equal(v.grad, g) for v, g in zip(st, e_grads)), rep
        assert bool(torch.isfinite(junk))
