"""`FusedAdam`: `torch.optim.Adam(params, lr, weight_decay)` (main_graph_knowledge_transfer.py:205, :353) as ONE HIP launch per step
for every parameter tensor of a model (`bgnn_adam_step_f32`, csrc/bgnn_optim.hip), with the step number and the learning-rate
schedule on the device.  Nothing but addresses is baked into a captured graph, so a replayed training step follows the schedule a
host-side `StepLR` would have produced (`lr_table`) without the host touching the optimizer.

Also here, because the captured epoch of `transfer.train_gnn(graphed=True)` needs them next to the optimizer:
`lr_table` (the schedule as the host scheduler's own numbers) and `draw_dropout_seeds` (the seeds an eager run would draw)."""
import ctypes as C

import torch

from . import _lib as L

__all__ = ["FusedAdam", "lr_table", "draw_dropout_seeds"]


def lr_table(lr, num_steps, step_size=None, gamma=0.1):
    """-> fp64 CPU tensor [max(num_steps, 1)]: entry k is the learning rate of optimizer step k + 1 when a `StepLR(step_size, gamma)`
    is stepped once after every optimizer step (main_graph_knowledge_transfer.py:206, :247).  The values are read off a real
    `StepLR` driving a throw-away optimizer: the reference's own numbers, whatever way torch forms them (it multiplies the running
    value by gamma; `lr * gamma ** k` differs from that in the last bit).  `step_size=None`: no scheduler, a constant table."""
    n = max(int(num_steps), 1)
    if step_size is None:
        return torch.full((n,), float(lr), dtype=torch.float64)
    from torch.optim.lr_scheduler import StepLR
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    sched = StepLR(opt, step_size=step_size, gamma=gamma)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return torch.tensor(out, dtype=torch.float64)


def draw_dropout_seeds(num_steps, layers):
    """-> int64 CPU tensor [num_steps, layers]: the dropout seeds an eager run of `num_steps` training steps draws from the HOST
    generator, one per dropout layer per step in forward order (`ktgnn._BnReluDropFn`, `sage.SAGEConv.run`: one scalar
    `random_()` each), drawn here the same way, so the generator is left exactly where that run would leave it."""
    out = torch.empty(int(num_steps), int(layers), dtype=torch.int64)
    for s in range(int(num_steps)):
        for l in range(int(layers)):
            out[s, l] = int(torch.empty((), dtype=torch.int64).random_().item())
    return out


class FusedAdam:
    """Adam over `params` (fp32 CUDA tensors, contiguous) in one launch per step.

    FusedAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, lr_table=None)
      lr_table: fp64 sequence, the rate of step s (1-based) is lr_table[min(s, len) - 1] (see `lr_table()`); None: constant `lr`.
    step(advance=True): `step_word` (device int64 [1]) += 1, then the update launch.  With `advance=False` the caller has advanced
      the word itself (a captured epoch shares one word between the optimizer, its dropout seeds and its history row) and step()
      is exactly one launch.
    zero_state(): moments and step word back to zero, on the device.
    state_dict() / load_state_dict(): torch Adam's layout (per parameter `step`, `exp_avg`, `exp_avg_sq`), so a run can be continued
      with either optimizer.  ONE step number serves all tensors: a parameter that only sometimes receives a gradient is bias-
      corrected with the global step, where torch counts that parameter's own steps.

    Gradients.  The kernel reads a device table of addresses.  step() compares the addresses of `p.grad` with the ones it uploaded
    last and uploads again when they moved (a parameter whose grad is None gets 0 and is skipped, as in torch).  Inside a stream
    capture nothing can be uploaded: step() then records the addresses the captured backward produced and `flush()`, called after
    the capture has ended, uploads them -- the table is read when the graph is REPLAYED, and the captured backward writes its
    gradients to those same addresses on every replay.  So: grads are read at capture time only; do not free or move them (no
    `zero_grad(set_to_none=True)` outside the graph) while the graph is in use."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lr_table=None):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("FusedAdam got an empty parameter list")
        dev = self.params[0].device
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == dev):
                raise RuntimeError("FusedAdam updates contiguous fp32 CUDA(HIP) tensors of one device; there is no CPU path")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0 and weight_decay >= 0.0 and lr >= 0.0):
            raise ValueError("FusedAdam: lr, eps, weight_decay >= 0 and betas in [0, 1) expected")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.device = dev
        with torch.cuda.device(dev):
            self.chunk = int(L.lib().bgnn_adam_chunk_elems())
            # both moments of every tensor in ONE buffer (tensor starts 16-byte aligned): zero_state() is one fill
            offs, total = [], 0
            for p in self.params:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4
            self._moments = torch.zeros(2, max(total, 4), dtype=torch.float32, device=dev)
            self.exp_avg = [self._moments[0, o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]
            self.exp_avg_sq = [self._moments[1, o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]
            self.step_word = torch.zeros(1, dtype=torch.int64, device=dev)
            cmap = [(t, c) for t, p in enumerate(self.params) for c in range((p.numel() + self.chunk - 1) // self.chunk)]
            self.n_chunks = len(cmap)
            self._chunk_map = torch.tensor(cmap if cmap else [(0, 0)], dtype=torch.int32).to(dev)
            self._records = torch.zeros(len(self.params), 5, dtype=torch.int64, device=dev)
            self._host_records = torch.zeros(len(self.params), 5, dtype=torch.int64)
            self._uploaded = None                  # the (param, grad) addresses the device table holds
            self._pending = False                  # addresses recorded during a capture, not uploaded yet
            self.set_lr_table(lr_table)

    # ---- schedule ------------------------------------------------------------------------------------------------------
    def set_lr_table(self, table=None):
        t = torch.as_tensor([self.lr] if table is None else table, dtype=torch.float64).reshape(-1)
        if t.numel() < 1:
            raise ValueError("FusedAdam: an empty lr_table")
        self._lr_host = t.clone()
        with torch.cuda.device(self.device):
            self._lr_table = t.to(self.device)

    # ---- the gradient table -----------------------------------------------------------------------------------------------
    def _addresses(self):
        out = []
        for p in self.params:
            g = p.grad
            if g is not None and not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == p.numel()
                                      and g.device == p.device):
                raise RuntimeError("FusedAdam needs dense contiguous fp32 gradients on the parameter's device")
            out.append((p.data_ptr(), g.data_ptr() if g is not None else 0))
        return tuple(out)

    def _fill_host(self, addr):
        h = self._host_records
        for i, ((pp, gp), p) in enumerate(zip(addr, self.params)):
            h[i, 0], h[i, 1], h[i, 2], h[i, 3], h[i, 4] = pp, gp, self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), p.numel()

    def flush(self):
        """upload the addresses recorded by a step() that ran inside a stream capture (call after the capture, before a replay)"""
        if self._pending:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam.flush() inside a stream capture: call it after the capture has ended")
            self._records.copy_(self._host_records)
            self._pending = False

    def step(self, advance=True):
        addr = self._addresses()
        capturing = torch.cuda.is_current_stream_capturing()
        if addr != self._uploaded:
            self._fill_host(addr)
            self._uploaded = addr
            self._pending = True
        if not capturing:
            self.flush()
        with torch.cuda.device(self.device):
            if advance:
                self.step_word.add_(1)
            rc = L.lib().bgnn_adam_step_f32(L.ptr(self._records), len(self.params), L.ptr(self._chunk_map), self.n_chunks,
                                            L.ptr(self.step_word), L.ptr(self._lr_table), int(self._lr_table.numel()),
                                            C.c_double(self.betas[0]), C.c_double(self.betas[1]), C.c_double(self.eps),
                                            C.c_double(self.weight_decay), L.stream())
        L.check(rc, "bgnn_adam_step_f32")

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.zero_()

    def zero_state(self):
        self._moments.zero_()
        self.step_word.zero_()

    # ---- torch Adam's state layout --------------------------------------------------------------------------------------------
    def _param_group(self, step):
        ref = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        grp = dict(ref.state_dict()["param_groups"][0])
        n = int(self._lr_host.numel())
        grp["lr"] = float(self._lr_host[min(step + 1, n) - 1])           # the rate of the NEXT step
        grp["params"] = list(range(len(self.params)))
        return grp

    def state_dict(self):
        step = int(self.step_word.item())
        state = {}
        if step > 0:
            for i in range(len(self.params)):
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": self.exp_avg[i].clone(), "exp_avg_sq": self.exp_avg_sq[i].clone()}
        return {"state": state, "param_groups": [self._param_group(step)]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if len(order) != len(self.params):
            raise ValueError("loaded state dict holds a different number of parameters")
        self.zero_state()
        step = 0
        for k, idx in enumerate(order):
            st = sd["state"].get(idx)
            if st is None:
                continue
            self.exp_avg[k].copy_(st["exp_avg"])
            self.exp_avg_sq[k].copy_(st["exp_avg_sq"])
            step = max(step, int(float(st["step"])))
        self.step_word.fill_(step)
        g = groups[0]
        self.betas, self.eps, self.weight_decay = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"]), float(g["weight_decay"])
