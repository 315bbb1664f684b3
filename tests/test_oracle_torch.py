"""CPU: pins the torch/autograd oracle (oracle/oracle_torch.py, the gradient checker) -- its forward must equal
the golden vectors produced by the reference's own AdaptedConv, and its whole-model training step (outputs, loss, gradients,
BatchNorm buffers) must equal the reference's own fp64 training step."""
import numpy as np
import pytest
import torch

from conftest import assert_close, sub
from oracle import grad_cases as GC
from oracle import oracle_torch as OT


@pytest.mark.parametrize("D", [2, 31, 64])
def test_torch_oracle_forward_matches_reference_golden(golden, D):
    c = golden(f"conv_small_D{D}.npz")
    mask = torch.from_numpy(c["central_mask"])
    e1, e2 = OT.graph_partition(torch.from_numpy(c["edge_index"].astype(np.int64)), mask)
    p = {k: torch.from_numpy(v) for k, v in sub(c, "p.").items()}
    out = OT.adaptedconv(torch.from_numpy(c["x"]), mask, e1, e2, p)
    assert_close(out.numpy(), c["out"], what=f"torch oracle D={D}")


def test_train_loss_formula():
    torch.manual_seed(0)
    lp = [torch.log_softmax(torch.randn(6, 3), 1) for _ in range(3)]
    y = torch.tensor([0, 1, 2, 0, 1, 2])
    tm = torch.tensor([1, 1, 0, 1, 1, 0], dtype=torch.bool)
    cm = torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.bool)
    loss = OT.train_loss(lp[0], lp[1], lp[2], y, tm, cm)
    kl = (lp[1].exp() * (lp[1] - lp[2])).sum() / 6
    ref = (2 * (-lp[0][tm, y[tm]]).mean() + (-lp[1][[3, 4], y[[3, 4]]]).mean() + (-lp[2][[3, 4], y[[3, 4]]]).mean()) / 4 + kl
    assert torch.allclose(loss, ref, atol=1e-6)


@pytest.mark.parametrize("case", GC.CASES)
def test_torch_oracle_training_step_matches_reference_gradients(case):
    """The whole-model train-mode oracle (OT.ktgnn_train + OT.train_loss, fp64) against the reference's own fp64 training step
    (tests/golden/grads_*.npz): outputs, loss terms, every parameter gradient, dL/dx and the BatchNorm buffers after the forward
    agree to 1e-10 relative -- the same maths in a different op order.  Pins the checker of every gradient test on the GPU.
    (Large tensors are stored as summaries, oracle/grad_cases.py: strided grid, row (block) and column sums, amax, sum of squares.)"""
    c = GC.load(case)
    r = GC.oracle_step(c)
    assert np.abs(r["loss"] - c["loss"]).max() <= 1e-12 * abs(c["loss"][0]), (r["loss"], c["loss"])
    for nm in ("logp_base", "logp_target", "logp_target_hat", "dx"):
        bad = [(part, v) for part, v in GC.compare(r[nm], c[nm], 1e-10) if not v <= 1.0]
        assert not bad, (nm, bad)
    assert sorted(r["grad"]) == sorted(c["grad"]), "parameter set"
    for k, g in r["grad"].items():
        ref = c["grad"][k]
        amax = float(np.abs(ref["full"]).max()) if "full" in ref else float(ref["amax"])
        if amax < 1e-9 * c["gmax"]:        # mathematically zero (clf_transformer.0.bias: a Linear in front of a train-mode BN)
            bad = [(part, v) for part, v in GC.compare(g, ref, 1e-12, scale=c["gmax"]) if not v <= 1.0]
        else:
            bad = [(part, v) for part, v in GC.compare(g, ref, 1e-10) if not v <= 1.0]
        assert not bad, (k, bad)
    for k, v in c["bn"].items():
        if v.dtype.kind == "f":
            assert np.abs(r["bn"][k] - v).max() <= 1e-12 * np.abs(v).max(), k
        else:
            assert np.array_equal(r["bn"][k], v), k
