"""GPU: `optim.FusedAdam` (one HIP launch per step, bgnn_adam_step_f32) against `torch.optim.Adam`."""
import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import StepLR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD, STEPS, STEP_SIZE, GAMMA = 1e-3, 5e-3, 50, 3, 0.5
ODD = (1, 31, 33, 4097)


def office_shapes(golden):
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    F = golden("office_a2d_graph.npz")["x"].shape[1]
    m = KTGNN_no_complement(F, 31, 2, 64, root_weight=False, use_dist_loss=False, dropout=0.5, use_bn=True, step=1, dim_share=F, need_complement=False)
    return [tuple(p.shape) for p in m.parameters()]


def make_case(golden, seed=0):
    """-> (initial values, per-step gradients | None) as fp32 CPU tensors: the office model's parameter shapes, the odd sizes, a tensor
    that will live 4 bytes off a 16-byte boundary, and (last) a tensor that never receives a gradient"""
    g = torch.Generator().manual_seed(seed)
    shapes = office_shapes(golden) + [(n,) for n in ODD] + [(37,), (19,)]
    init = [torch.randn(s, generator=g) * 0.3 for s in shapes]
    grads = [[torch.randn(s, generator=g) * (0.05 + 0.02 * k) for s in shapes[:-1]] + [None] for k in range(STEPS)]
    return init, grads


def device_params(init):
    """leaf tensors on the GPU; the one before last is a view that starts one float into its buffer"""
    out = []
    for i, t in enumerate(init):
        if i == len(init) - 2:
            buf = torch.zeros(t.numel() + 1, device=DEV)
            buf[1:] = t.to(DEV)
            p = buf[1:].detach().requires_grad_()
            assert p.data_ptr() % 16 == 4
        else:
            p = t.to(DEV).clone().requires_grad_()
        out.append(p)
    return out


def set_grads(params, grads):
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif p.grad is None:
            p.grad = g.to(p.device, p.dtype).clone()
        else:
            p.grad.copy_(g)


def test_fused_adam_follows_torch_adam_in_fp64(golden):
    """50 steps, wd = 5e-3, StepLR(3, 0.5), on the same gradients: the yardstick of a tensor is the deviation of torch's own fp32 GPU
    Adam from torch's fp64 CPU Adam at step 50; the kernel (fp32, its own operation order) is allowed 4x that, per tensor."""
    from bridged_gnn_amd.optim import FusedAdam, lr_table
    init, grads = make_case(golden)
    p64 = [t.double().clone().requires_grad_() for t in init]
    o64 = torch.optim.Adam(p64, lr=LR, weight_decay=WD)
    s64 = StepLR(o64, step_size=STEP_SIZE, gamma=GAMMA)
    p32 = device_params(init)
    o32 = torch.optim.Adam(p32, lr=LR, weight_decay=WD)
    s32 = StepLR(o32, step_size=STEP_SIZE, gamma=GAMMA)
    pk = device_params(init)
    ok = FusedAdam(pk, lr=LR, weight_decay=WD, lr_table=lr_table(LR, STEPS, STEP_SIZE, GAMMA))
    for k in range(STEPS):
        set_grads(p64, grads[k])
        set_grads(p32, grads[k])
        set_grads(pk, grads[k])
        o64.step(), s64.step()
        o32.step(), s32.step()
        ok.step()
    assert int(ok.step_word.item()) == STEPS
    worst = 0.0
    for i, (a64, a32, ak) in enumerate(zip(p64, p32, pk)):
        yard = float((a32.detach().cpu().double() - a64.detach()).abs().max())
        dev = float((ak.detach().cpu().double() - a64.detach()).abs().max())
        print(f"tensor {i} {tuple(a64.shape)}: yardstick {yard:.3e} measured {dev:.3e} bar {4 * yard:.3e}")
        worst = max(worst, dev / yard if yard > 0 else (0.0 if dev == 0 else float("inf")))
    print(f"worst measured / yardstick over the tensors: {worst:.3f} (bar 4)")
    for i, (a64, a32, ak) in enumerate(zip(p64, p32, pk)):
        yard = float((a32.detach().cpu().double() - a64.detach()).abs().max())
        dev = float((ak.detach().cpu().double() - a64.detach()).abs().max())
        assert dev <= 4 * yard, (i, tuple(a64.shape), dev, yard)
    assert torch.equal(pk[-1].detach().cpu(), init[-1])                  # no gradient: untouched, like torch
    assert float((pk[0].detach().cpu() - init[0]).abs().max()) > 1e-3     # (and the others really moved)


def test_eager_and_replayed_steps_are_bit_equal(golden):
    from bridged_gnn_amd.optim import FusedAdam, lr_table
    init, grads = make_case(golden, seed=1)
    n = 7
    tab = lr_table(LR, n, 2, 0.1)
    pe = device_params(init)
    oe = FusedAdam(pe, lr=LR, weight_decay=WD, lr_table=tab)
    for k in range(n):
        set_grads(pe, grads[k])
        oe.step()
    pg = device_params(init)
    og = FusedAdam(pg, lr=LR, weight_decay=WD, lr_table=tab)
    set_grads(pg, grads[0])
    before = [p.detach().clone() for p in pg]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    og.flush()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, pg)) and int(og.step_word.item()) == 0      # a capture runs nothing
    for k in range(n):
        set_grads(pg, grads[k])                                          # in place: the addresses the graph holds
        graph.replay()
    torch.cuda.synchronize()
    assert int(og.step_word.item()) == n
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(oe.exp_avg + oe.exp_avg_sq, og.exp_avg + og.exp_avg_sq):
        assert torch.equal(a, b)
    og.zero_state()
    assert int(og.step_word.item()) == 0 and all(float(t.abs().max()) == 0 for t in og.exp_avg + og.exp_avg_sq)


def test_state_dict_round_trips_with_torch_adam(golden):
    """5 fused steps, hand the state to `torch.optim.Adam`, one more step with each: both are fp32 with torch's operation order but their
    own rounding of the step size, so the parameters agree to a few ulp -- 4 ulp of the value (rtol 2.4e-7) plus 4 ulp of an update of at
    most ~10 lr (atol 4 * 6e-8 * 1e-2).  And back: a torch state loaded into FusedAdam."""
    from bridged_gnn_amd.optim import FusedAdam
    init, grads = make_case(golden, seed=2)
    init, grads = init[:-1], [g[:-1] for g in grads]                      # (every tensor has a gradient: torch keeps no state otherwise)
    pk = device_params(init + [init[-1]])[:-1]
    ok = FusedAdam(pk, lr=LR, weight_decay=WD)
    for k in range(5):
        set_grads(pk, grads[k])
        ok.step()
    sd = ok.state_dict()
    assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == list(range(len(pk)))
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} and float(v["step"]) == 5.0 for v in sd["state"].values())
    pt = [p.detach().clone().requires_grad_() for p in pk]
    ot = torch.optim.Adam(pt, lr=LR, weight_decay=WD)
    ot.load_state_dict(sd)
    for i, p in enumerate(pt):
        assert torch.equal(ot.state[p]["exp_avg"], ok.exp_avg[i]) and torch.equal(ot.state[p]["exp_avg_sq"], ok.exp_avg_sq[i])
    set_grads(pk, grads[5])
    set_grads(pt, grads[5])
    ok.step()
    ot.step()
    for a, b in zip(pk, pt):
        assert torch.allclose(a.detach(), b.detach(), rtol=2.4e-7, atol=2.4e-9), float((a - b).abs().max())
    assert float(ot.state[pt[0]]["step"]) == 6.0
    # and back
    pb = [p.detach().clone().requires_grad_() for p in pt]
    ob = FusedAdam(pb, lr=LR, weight_decay=WD)
    ob.load_state_dict(ot.state_dict())
    assert int(ob.step_word.item()) == 6
    set_grads(pb, grads[6])
    set_grads(pt, grads[6])
    ob.step()
    ot.step()
    for a, b in zip(pb, pt):
        assert torch.allclose(a.detach(), b.detach(), rtol=2.4e-7, atol=2.4e-9), float((a - b).abs().max())
