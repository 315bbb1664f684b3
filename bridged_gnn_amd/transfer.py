"""Step 2 of Bridged-GNN: knowledge transfer on the bridged graph -- the reference's `main_graph_knowledge_transfer.py`.

Same names, arguments, defaults and return values as the reference: `pyg_dataset` (:16-24), `train` (:39-68), `test` (:73-118),
`get_each_clf_res` (:119-142), `train_gnn` (:143-262), `train_noDTC` / `test_noDTC` / `train_gnn_noDTC` (:265-396), `main`
(:399-421) and its command line (:423-439) behind `python -m bridged_gnn_amd.transfer`.

What runs differently underneath:
  * the loss (:44-54, :269) is one HIP pass forward and one backward (`ops.step2_loss` / `ops.step2_nll`): no boolean-mask indexing,
    fixed-order fp64 sums, no memset node;
  * the scores come from integer confusion counts taken on the device (`ops.step2_counts`, AUC: `ops.step2_auc`) and turned into
    sklearn's numbers on the host (`f1_from_counts`, `accuracy_from_counts`): no prediction array crosses to the host;
  * inside the training loops `test` and `get_each_clf_res` share ONE eval forward and ONE count launch per epoch;
  * with `verbose=False` and `save=False` an epoch never waits for the device: losses and counts go to device history buffers
    that are read once after the last epoch, and the best epoch is then chosen from that history with the reference's own
    comparison (`loss_target < best`, on fp32 values).

Additive keyword arguments (defaults keep the reference's behaviour): `dropout=0.5` (the reference fixes it at :179),
`verbose=True`, `ckpt_dir='../ckpt'`, `history=None` (a dict that receives the per-epoch scores and the best epoch), `graphed=False`
(`--graphed`: every epoch is one replay of a captured HIP graph, see `_GraphedEpoch`; the run is the eager run), and `--gpu` now
selects the device (the reference parses it and then hard-codes cuda:1, :36).

Deviations from the reference, all on paths the reference cannot complete:
  * `train` / `train_gnn` with `gnn != 'KTGNN'` raise NotImplementedError (in the reference those branches die on an undefined
    `loss_kl`, :65); `train_gnn_noDTC` builds `gnn='GraphSAGE'` only (what `main` passes);
  * `get_each_clf_res(metric='acc')` applies `.exp()` to the integer predictions in the reference (:137-139) and is never called
    that way; here it returns the accuracy of the three heads;
  * a val / test mask that holds a source node makes the reference hand sklearn arrays of different lengths (:96-100); that
    ValueError is raised here at set-up, once per graph; so is a label outside [0, C) on a scored row (sklearn would score -1 as
    a class of its own; `main` clears such rows from the train mask only, :404);
  * StepLR is built without `verbose=` (removed from torch).
"""
import argparse
import os
import time

import numpy as np
import torch
from torch.optim.lr_scheduler import StepLR

from . import ops
from .data import load_bridged_graph
from .utils import set_random_seed

__all__ = ["pyg_dataset", "train", "test", "get_each_clf_res", "train_gnn", "train_noDTC", "test_noDTC", "train_gnn_noDTC", "main",
           "f1_from_counts", "accuracy_from_counts", "auc_from_rank_counts", "score_from_counts", "select_best", "build_parser"]

_HISTORY_BYTES = 64 << 20          # device history of a deferred run is flushed to the host (one wait) whenever it reaches this size


class pyg_dataset:
    """The dataset stand-in the reference hands its model constructors (main_graph_knowledge_transfer.py:16-24): the four sizes of one
    graph, and the graph itself as item 0."""

    def __init__(self, data):
        n, f = data.x.shape
        self.num_nodes, self.num_features = n, f
        self.num_edges = data.edge_index.shape[1]
        self.num_classes = int(data.y.max().item()) + 1
        self.data = (data,)

    def __getitem__(self, idx):
        return self.data[idx]


def select_best(losses, start=666):
    """The reference's best-epoch rule (:238 on loss_target, :374 on loss_train): walk the epochs in order and take an epoch when
    its loss is strictly below the best so far, which starts at 666 -> list of the 0-based epochs at which the best moved (the last
    entry is the best epoch; empty when no loss ever got below `start`).  A tie keeps the earlier epoch; NaN never wins."""
    best, taken = start, []
    for i, v in enumerate(losses):
        if v < best:
            best = v
            taken.append(i)
    return taken


# ---- sklearn's numbers from integer counts (host side) ----------------------------------------------------------------------------
def f1_from_counts(cm, average="macro"):
    """sklearn.metrics.f1_score(y_true, y_pred, average=...) from a confusion matrix cm[true, predicted] of integer counts.
    'macro': unweighted mean of the per-label F1 = 2 tp / (2 tp + fp + fn) over the labels present in y_true or y_pred;
    'micro': 2 sum tp / (2 sum tp + sum fp + sum fn)."""
    cm = np.asarray(cm, dtype=np.int64)
    tp = np.diag(cm).astype(np.float64)
    true_n, pred_n = cm.sum(1).astype(np.float64), cm.sum(0).astype(np.float64)
    if average == "micro":
        den = true_n.sum() + pred_n.sum()
        return float(2.0 * tp.sum() / den) if den > 0 else 0.0
    if average != "macro":
        raise NotImplementedError(f"f1 average {average!r}")
    present = (true_n + pred_n) > 0
    if not present.any():
        return float("nan")
    return float(np.mean(2.0 * tp[present] / (true_n[present] + pred_n[present])))


def accuracy_from_counts(cm):
    """sklearn.metrics.accuracy_score from a confusion matrix of integer counts"""
    cm = np.asarray(cm, dtype=np.int64)
    n = int(cm.sum())
    return float(np.trace(cm) / n) if n else float("nan")


def auc_from_rank_counts(u2, n_pos, n_neg):
    """sklearn.metrics.roc_auc_score (binary) from the tie-aware rank statistic: u2 = sum over positives of
    2 #{negatives scored lower} + #{negatives scored equal}.  One class only -> ValueError, as sklearn raises."""
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return float(u2) / (2.0 * float(n_pos) * float(n_neg))


def score_from_counts(cm, metric, f1_average="macro"):
    if metric == "f1":
        return f1_from_counts(cm, f1_average)
    if metric == "acc":
        return accuracy_from_counts(cm)
    raise NotImplementedError("NotImplemented Metric:{}".format(metric))


def _check_auc(v):
    if v != v:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return v


# ---- per-graph set-up ----------------------------------------------------------------------------------------------------------
class _Plan:
    """what the passes need from a graph, built once: labels, uint8 masks, the selection bits of the scored rows.
    dtc: bit 0 = train, bit 1 = val & ~central, bit 2 = test & ~central (what :82-105 and :124-131 score);
    plain (noDTC): bit 0 / 1 / 2 = train / val / test (:284-295)."""

    def __init__(self, data, dtc):
        masks = [getattr(data, k) for k in ("train_mask", "val_mask", "test_mask")]
        self.key = self._key(data, dtc)
        self._keep = [getattr(data, k) for k in ("y", "train_mask", "val_mask", "test_mask")]      # the key holds ids: keep them alive
        self.dtc = dtc
        self.y = data.y.long().contiguous()
        self.train_u8 = ops.as_u8(masks[0].bool())
        bits = [m.bool() for m in masks]
        bad = torch.zeros((), dtype=torch.bool, device=self.y.device)
        if dtc:
            central = data.central_mask.bool()
            self._keep.append(data.central_mask)
            self.central_u8 = ops.as_u8(central)
            bad = (bits[1] & central).any() | (bits[2] & central).any()
            bits = [bits[0], bits[1] & ~central, bits[2] & ~central]
        self.bits = bits
        self.sel = (bits[0].to(torch.uint8) | (bits[1].to(torch.uint8) << 1) | (bits[2].to(torch.uint8) << 2)).contiguous()
        lab = self.y[self.sel != 0]
        lo, hi = (int(lab.min()), int(lab.max())) if lab.numel() else (0, 0)        # set-up: the one place that waits for the device
        if bool(bad):
            raise ValueError("a val / test mask holds a source (central) node: the reference scores lp[mask] against "
                             "y[mask & ~central] and sklearn raises on the two lengths (main_graph_knowledge_transfer.py:96-100)")
        self.label_range = (lo, hi)

    @staticmethod
    def _key(data, dtc):
        names = ("y", "train_mask", "val_mask", "test_mask") + (("central_mask",) if dtc else ())
        return (dtc,) + tuple((id(getattr(data, k)), getattr(data, k)._version, getattr(data, k).device) for k in names)

    def check_classes(self, C):
        lo, hi = self.label_range
        if lo < 0 or hi >= C:
            raise ValueError(f"labels of scored rows span [{lo}, {hi}] but the model has {C} classes: every row of the train mask and of "
                             "the (target) val / test masks needs a label in [0, C)")


def _plan(data, dtc):
    p = data.__dict__.get("_bgnn_step2_plan" + ("" if dtc else "_plain"))
    if p is None or p.key != _Plan._key(data, dtc):
        p = _Plan(data, dtc)
        data.__dict__["_bgnn_step2_plan" + ("" if dtc else "_plain")] = p
    return p


_DTC_COMBOS = ((0, 0), (2, 1), (2, 2), (0, 2), (1, 2))        # test(): lp_s | train, lp_t^ | val, lp_t^ | test; each: lp_s, lp_t (, lp_t^) | test
_PLAIN_COMBOS = ((0, 0), (0, 1), (0, 2))


def _eval_dtc(data, model, plan, counts_out=None, auc_out=None):
    """ONE eval forward and ONE count launch for both `test` and `get_each_clf_res` -> counts int64 [5, C, C] on the device
    (`_DTC_COMBOS`); with `auc_out` (fp64 [3] device) also the three AUCs of `test(metric='auc')`."""
    with torch.no_grad():
        model.eval()
        lp_s, lp_t, lp_h, _ = model(data)
        plan.check_classes(lp_s.shape[1])
        counts = ops.step2_counts((lp_s, lp_t, lp_h), plan.y, plan.sel, _DTC_COMBOS, out=counts_out)
        if auc_out is not None:
            _need_binary(lp_s.shape[1])
            for j, (lp, b) in enumerate(((lp_s, 0), (lp_h, 1), (lp_h, 2))):
                auc_out[j] = ops.step2_auc(lp[:, 1].exp(), plan.y, plan.bits[b])
    return counts, (lp_s, lp_t, lp_h)


def _eval_plain(data, model, plan, counts_out=None, auc_out=None):
    with torch.no_grad():
        model.eval()
        lp = model(data)
        lp = lp[0] if isinstance(lp, (tuple, list)) else lp
        plan.check_classes(lp.shape[1])
        counts = ops.step2_counts((lp,), plan.y, plan.sel, _PLAIN_COMBOS, out=counts_out)
        if auc_out is not None:
            _need_binary(lp.shape[1])
            for j in range(3):
                auc_out[j] = ops.step2_auc(lp[:, 1].exp(), plan.y, plan.bits[j])
    return counts, lp


def _need_binary(C):
    if C != 2:
        raise ValueError(f"metric='auc' needs binary labels (the reference scores exp(log_probs[:, 1])); the model has {C} classes")


# ---- the reference's functions --------------------------------------------------------------------------------------------------
def _prime(model, data, loss_of):
    """Build what the model caches per graph on first use (hub tables, the transposed CSR, packed weights: each build waits for the
    device once) BEFORE the epoch loop: one train-mode forward + backward and one eval forward, after which the parameters, the
    BatchNorm buffers and both generators (host: the dropout seeds come from it; device) are put back, so the run that follows is unchanged."""
    rng, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(data.x.device)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    loss_of(model(data)).backward()
    model.eval()
    with torch.no_grad():
        model(data)
    model.zero_grad(set_to_none=True)
    model.load_state_dict(state)
    torch.set_rng_state(rng)
    torch.cuda.set_rng_state(rng_dev, data.x.device)


def _train_step(data, model, optimizer, plan, Lambda):
    """:40-67 without the prints -> the loss pass's fp64 [8] device vector (ops.STEP2_TERMS)"""
    model.train()
    optimizer.zero_grad()
    lp_s, lp_t, lp_h, loss_dist = model(data)
    loss, terms = ops.step2_loss(lp_s, lp_t, lp_h, plan.y, plan.train_u8, plan.central_u8, Lambda, return_terms=True)
    if loss_dist is not None:
        loss = loss + loss_dist
    loss.backward()
    optimizer.step()
    return terms


def train(data, model, optimizer, clip_grad=False, gnn=None, Lambda=1., verbose=True):
    """main_graph_knowledge_transfer.py:39-68 -> (loss, loss_clf_t2 [lp_t^], loss_clf_t1 [lp_t], loss_kl) as Python floats (fp32 values).
    Only `gnn='KTGNN'`: the reference's other branch fails on an undefined `loss_kl` (:65)."""
    if gnn != "KTGNN":
        raise NotImplementedError("train() supports gnn='KTGNN' only (the reference's other branch raises NameError on loss_kl); "
                                  "use train_noDTC for a plain backbone")
    t = _train_step(data, model, optimizer, _plan(data, True), Lambda).float().tolist()
    if verbose:
        print(t[1], t[2], t[3])
        print('Loss_clf:{:.3f} | Loss_kl:{:.3f}'.format(t[0], t[4]))
    return t[0], t[3], t[2], t[4]


def test(data, model, dataset_name=None, gnn=None, metric='f1', f1_average='macro'):
    """main_graph_knowledge_transfer.py:73-118 -> [train, val, test] scores.  For `gnn='KTGNN'` the train mask is scored with lp_s
    over ALL train rows, val / test with lp_t^[mask] against y[mask & ~central] (:82-105): a val / test mask holding a source node
    raises ValueError, as sklearn does on the two lengths.  Any other `gnn`: macro-F1 (f1_average) of `model(data)` on the three masks."""
    if gnn != 'KTGNN':
        counts, _ = _eval_plain(data, model, _plan(data, False))
        return [f1_from_counts(c, f1_average) for c in counts.cpu().numpy()]
    plan = _plan(data, True)
    if metric == 'auc':
        auc = torch.empty(3, dtype=torch.float64, device=plan.y.device)
        _eval_dtc(data, model, plan, auc_out=auc)
        return [_check_auc(v) for v in auc.tolist()]
    if metric not in ('f1', 'acc'):
        raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
    counts, _ = _eval_dtc(data, model, plan)
    return [score_from_counts(c, metric, f1_average) for c in counts[:3].cpu().numpy()]


def get_each_clf_res(data, model, metric='f1', f1_average='macro'):
    """main_graph_knowledge_transfer.py:119-142 -> [lp_s, lp_t, lp_t^] scores on test & ~central.  `metric='acc'` is broken in the
    reference (`.exp()` on the predictions, :137-139); here it is the three heads' accuracy."""
    plan = _plan(data, True)
    if metric == 'auc':
        with torch.no_grad():
            model.eval()
            lps = model(data)[:3]
            _need_binary(lps[0].shape[1])
            return [_check_auc(float(ops.step2_auc(lp[:, 1].exp(), plan.y, plan.bits[2]))) for lp in lps]
    if metric not in ('f1', 'acc'):
        raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
    counts, _ = _eval_dtc(data, model, plan)
    c = counts.cpu().numpy()
    return [score_from_counts(c[k], metric, f1_average) for k in (3, 4, 2)]


def _device_of(args):
    gpu = getattr(args, "gpu", None)
    return torch.device("cuda", torch.cuda.current_device() if gpu is None else int(gpu))


class _History:
    """Per-epoch loss terms, confusion counts and AUCs on the device.  `every=1` (verbose / save): each epoch is read as soon as it
    is written.  Otherwise the buffers are read when they are full (by default never before the last epoch) -- one wait."""

    def __init__(self, dev, num_epoch, n_terms, K, C, auc, every):
        per = 8 * (n_terms + K * C * C + 3)
        self.cap = max(1, min(num_epoch, every if every else max(1, _HISTORY_BYTES // per)))
        self.terms = torch.zeros(self.cap, n_terms, dtype=torch.float64, device=dev)
        self.counts = torch.zeros(self.cap, K, C, C, dtype=torch.int64, device=dev)
        self.auc = torch.zeros(self.cap, 3, dtype=torch.float64, device=dev) if auc else None
        self.n = 0

    def slot(self):
        i = self.n
        self.n += 1
        return self.terms[i], self.counts[i], (self.auc[i] if self.auc is not None else None)

    @property
    def full(self):
        return self.n == self.cap

    def drain(self):
        """-> list of (terms fp32-rounded list, counts ndarray, auc list | None), oldest first"""
        n, self.n = self.n, 0
        if n == 0:
            return []
        terms = self.terms[:n].float().cpu().tolist()
        counts = self.counts[:n].cpu().numpy()
        auc = self.auc[:n].cpu().tolist() if self.auc is not None else [None] * n
        return [(terms[i], counts[i], auc[i]) for i in range(n)]


_AUC_GRAPHED_MAX_ROWS = 1 << 15


class _GraphedEpoch:
    """One epoch of `train_gnn` / `train_gnn_noDTC` -- zero-grad, train forward, loss, backward, Adam, eval forward, counts (and AUCs),
    the epoch's `_History` row -- captured into ONE HIP graph on one stream; `replay()` is one submission and waits for nothing.
    What makes the replayed run the eager run:
      * warm-up and capture leave no trace: parameters, BatchNorm buffers (`num_batches_tracked` included), optimizer state and both
        generators are put back afterwards, so epoch 1 starts from the state the eager run's epoch 1 starts from;
      * the optimizer is `optim.FusedAdam`: its step number is a device word advanced inside the graph, its learning rate comes
        from a device table that a real StepLR filled (`optim.lr_table`);
      * the dropout seeds are the ones the eager run would draw from the host generator (`optim.draw_dropout_seeds`, drawn before
        the loop, the generator left where the eager run leaves it) in a device table; the graph loads row `step - 1` into the
        words of a `ktgnn.DropoutSeedFeed` and the kernels add them to a baked seed of 0;
      * the packed / folded weight copies are dropped before the capture and again between the update and the eval forward, so their
        rebuild is part of the graph and runs on every replay;
      * terms, counts and AUCs are copied to row `(step - 1) % cap` of the history by device-indexed copies inside the graph.
    `loss_of(model_output) -> (loss, terms)`; `evaluate(counts_out, auc_out)` is the eval forward + count launch."""

    def __init__(self, data, model, optimizer, hist, num_epoch, layers, loss_of, evaluate):
        from .ktgnn import _DROPOUT_STEP, DropoutSeedFeed
        from .optim import draw_dropout_seeds
        dev = data.x.device
        self.model, self.opt, self.hist = model, optimizer, hist
        drop_caches = getattr(model, "_drop_param_caches", lambda: None)
        self._drop_caches = drop_caches
        step = optimizer.step_word
        rows = max(int(num_epoch), 1)
        seeds_dev = torch.empty(rows, max(layers, 1), dtype=torch.int64, device=dev)       # filled after the capture: read at replay
        words = torch.empty(max(layers, 1), dtype=torch.int64, device=dev)
        feed = DropoutSeedFeed(words)
        counts_stage = torch.empty_like(hist.counts[0])
        auc_stage = torch.empty_like(hist.auc[0]) if hist.auc is not None else None
        if auc_stage is not None and data.x.shape[0] > _AUC_GRAPHED_MAX_ROWS:
            raise NotImplementedError(f"graphed=True with metric='auc' covers graphs of up to {_AUC_GRAPHED_MAX_ROWS} nodes: beyond that "
                                      "`ops.step2_auc` reduces with a multi-block torch sum, whose memset node must not be captured")
        cap = hist.cap

        def epoch():
            step.add_(1)
            row = step - 1
            if layers:
                words.copy_(seeds_dev.index_select(0, row.clamp(0, rows - 1)).view(-1))
            feed.rewind()
            model.train()
            model.zero_grad(set_to_none=True)
            loss, terms = loss_of(model(data))
            loss.backward()
            optimizer.step(advance=False)
            drop_caches()                                  # the weights moved, their host-side version counters did not
            evaluate(counts_stage, auc_stage)
            slot = row.remainder(cap)
            hist.terms.index_copy_(0, slot, terms.view(1, -1))
            hist.counts.index_copy_(0, slot, counts_stage.unsqueeze(0))
            if auc_stage is not None:
                hist.auc.index_copy_(0, slot, auc_stage.view(1, -1))
            if feed.taken != layers:
                raise RuntimeError(f"graphed=True: the training forward took {feed.taken} dropout seeds, {layers} were prepared "
                                   "(a dropout layer outside the HIP kernels' envelope draws from the device generator)")

        rng, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        seeds_dev.zero_()
        _DROPOUT_STEP[0] = feed
        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):                  # kernel attributes, workspaces, library handles: settled before the capture
                drop_caches()
                epoch()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            model.zero_grad(set_to_none=True)              # the captured backward allocates the gradients the replays write
            drop_caches()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                epoch()
        finally:
            _DROPOUT_STEP[0] = None
        optimizer.flush()                                  # the gradients' addresses, known now
        model.load_state_dict(state)
        optimizer.zero_state()
        torch.set_rng_state(rng)
        torch.cuda.set_rng_state(rng_dev, dev)
        drop_caches()
        if layers and num_epoch:
            seeds_dev.copy_(draw_dropout_seeds(num_epoch, layers))      # the host generator moves as in the eager loop
        self._keep = (seeds_dev, words, counts_stage, auc_stage)

    def replay(self):
        self.graph.replay()

    def finish(self):
        """after the last epoch: the trained parameters are in the model; forget the graph's copies of them"""
        self._drop_caches()
        self.model.zero_grad(set_to_none=True)


def _graphed_optimizer(model, lr, wd, num_epoch, step_size, gamma):
    from .optim import FusedAdam, lr_table
    return FusedAdam(model.parameters(), lr=lr, weight_decay=wd, lr_table=lr_table(lr, num_epoch, step_size, gamma))


def _say(verbose, *a):
    if verbose:
        print(*a)


def _summary(final_acc, best_acc, verbose):
    """:251-261"""
    best_test_run = np.argmax(final_acc['test'])
    final_acc_avg, final_acc_std = {}, {}
    for key in final_acc:
        best_acc[key] = max(final_acc[key])
        final_acc_avg[key] = np.mean(final_acc[key])
        final_acc_std[key] = np.std(final_acc[key])
    _say(verbose, '[Average Score] {} '.format(final_acc_avg))
    _say(verbose, '[std Score] {} '.format(final_acc_std))
    _say(verbose, '[Best Score] {}'.format(best_acc))
    _say(verbose, '[Best test run] {}'.format(best_test_run))


def train_gnn(args, dataset, data, save=False, repeat=3, num_epoch=200, gnn='GCN', seed=None, step_size=100, gamma=0.1,
              num_layer=2, hidden=64, lr=1e-3, wd=5e-3, use_shceduler=True, step=1, Lambda=1., f1_average='macro', metric='f1', noDTC=False,
              dropout=0.5, verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:143-262 -> (loss_bucket, res_bucket_each).  `gnn='KTGNN'` only (the other backbones cannot
    get past `train` in the reference).  The model is `KTGNN_no_complement` built as at :179, Adam(lr, wd), StepLR(step_size, gamma);
    the best epoch is the one with the lowest `loss_target` (nll of lp_t^, :238); `save=True` writes
    {ckpt_dir}/model_{gnn}_{args.dataset_name}_best.ckpt at every improvement.  One eval forward per epoch serves both `test` and
    `get_each_clf_res`.  With `verbose=False, save=False` no epoch waits for the device.  `history` (a dict) receives 'eval_res'
    (per epoch [train, val, test]), 'best_epoch' (0-based, of the last repeat), 'best_acc' and 'final_acc'.  `graphed=True`: every
    epoch is one replay of a HIP graph captured per repeat (`_GraphedEpoch`): the same run, launch cost paid once."""
    if gnn != 'KTGNN':
        if gnn in ('MLP', 'GCN', 'GraphSAGE', 'GAT', 'GATv2'):
            raise NotImplementedError(f"train_gnn(gnn={gnn!r}): the reference's train() fails on an undefined loss_kl for every backbone "
                                      "but KTGNN; GraphSAGE runs through train_gnn_noDTC")
        raise NotImplementedError('Not Implemented Model:{}'.format(gnn))
    from .ktgnn import KTGNN_no_complement
    dev = _device_of(args)
    with torch.cuda.device(dev):
        data = data.to(dev)
        plan = _plan(data, True)
        C = data.y.max().item() + 1
        plan.check_classes(C)
        if metric == 'auc':
            _need_binary(C)
        elif metric not in ('f1', 'acc'):
            raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
        final_acc = {'train': [], 'val': [], 'test': []}
        loss_bucket = {'source&target': [], 'target_hat': [], 'target': [], 'kl': []}
        if save:
            os.makedirs(ckpt_dir, exist_ok=True)
        for train_id in range(1, 1 + repeat):
            _say(verbose, 'repeat {}/{}'.format(train_id, repeat))
            data_split_seed = 0
            model_init_seed = train_id - 1 if seed is None else seed
            set_random_seed(model_init_seed)
            model = KTGNN_no_complement(dataset.num_features, C, num_layer, hidden, root_weight=False, use_dist_loss=False, dropout=dropout,
                                        use_bn=True, step=step, dim_share=data.x.shape[1], need_complement=False)
            model = model.to(dev)
            _prime(model, data, lambda o: ops.step2_loss(o[0], o[1], o[2], plan.y, plan.train_u8, plan.central_u8, Lambda))
            _say(verbose, data)
            _say(verbose, model)
            _say(verbose, 'auto fixed data split seed to {}, model init seed to {}'.format(data_split_seed, model_init_seed))
            if verbose:
                print(data)
                print('[Dataset-{}] train_num:{}, val_num:{}, test_num:{}, class_num:{}'.format(
                    args.dataset_name, data.train_mask.sum().item(), data.val_mask.sum().item(), data.test_mask.sum().item(), C))
            if graphed:
                if dropout > 0 and not (hidden % 4 == 0 and 4 <= hidden <= 1024 and num_layer > 1):
                    raise NotImplementedError("graphed=True with dropout needs hidden % 4 == 0 and 4 <= hidden <= 1024 (the fused "
                                              "BatchNorm / ReLU / dropout kernel, whose masks come from the host generator's seeds)")
                optimizer = _graphed_optimizer(model, lr, wd, num_epoch, step_size if use_shceduler else None, gamma)
                scheduler = None
            else:
                optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
                scheduler = StepLR(optimizer, step_size=step_size, gamma=gamma) if use_shceduler else None
            best_acc = {'train': 0, 'val': 0, 'test': 0, 'loss': 666}
            res_bucket_each = {'source&target': [], 'target': [], 'target_hat': []}
            eval_hist, best_epoch = [], [None]
            hist = _History(dev, num_epoch, 8, len(_DTC_COMBOS), C, metric == 'auc', 1 if (verbose or save) else 0)
            t0 = [time.time()]

            def consume():
                for terms, counts, auc in hist.drain():
                    epoch = len(eval_hist) + 1
                    loss_train, loss_target, loss_target_only, loss_kl = terms[0], terms[3], terms[2], terms[4]
                    if verbose:
                        print(terms[1], terms[2], terms[3])
                        print('Loss_clf:{:.3f} | Loss_kl:{:.3f}'.format(loss_train, loss_kl))
                    loss_bucket['source&target'].append(loss_train)
                    loss_bucket['target_hat'].append(loss_target)
                    loss_bucket['target'].append(loss_target_only)
                    loss_bucket['kl'].append(loss_kl)
                    if metric == 'auc':
                        eval_res = [_check_auc(v) for v in auc]
                    else:
                        eval_res = [score_from_counts(counts[k], metric, f1_average) for k in range(3)]
                    each = [f1_from_counts(counts[k], 'macro') for k in (3, 4, 2)]       # get_each_clf_res(data, model, metric='f1'), :227
                    eval_hist.append(eval_res)
                    res_bucket_each['source&target'].append(each[0])
                    res_bucket_each['target'].append(each[1])
                    res_bucket_each['target_hat'].append(each[2])
                    _say(verbose, 'Epoch: {:03d}, Loss:{:.4f} Train: {:.4f}, Val:{:.4f}, Test: {:.4f}, Time(s/epoch):{:.4f}'.format(
                        epoch, loss_train, *eval_res, time.time() - t0[0]))
                    if select_best([loss_target], best_acc['loss']):                    # :238
                        best_acc['train'], best_acc['val'], best_acc['test'] = eval_res
                        best_acc['loss'] = loss_target
                        best_epoch[0] = epoch - 1
                        if save:                                                        # every=1: the model is still this epoch's
                            torch.save(model.state_dict(), os.path.join(ckpt_dir, f'model_{gnn}_{args.dataset_name}_best.ckpt'))

            ge = None
            if graphed:
                ge = _GraphedEpoch(data, model, optimizer, hist, num_epoch, len(model.convs) if dropout > 0 else 0,
                                   lambda o: ops.step2_loss(o[0], o[1], o[2], plan.y, plan.train_u8, plan.central_u8, Lambda, return_terms=True),
                                   lambda counts, auc: _eval_dtc(data, model, plan, counts_out=counts, auc_out=auc))
            for epoch in range(1, 1 + num_epoch):
                t0[0] = time.time()
                terms_slot, counts_slot, auc_slot = hist.slot()
                if ge is not None:
                    ge.replay()                          # the graph writes this epoch's row itself
                else:
                    terms_slot.copy_(_train_step(data, model, optimizer, plan, Lambda))
                    _eval_dtc(data, model, plan, counts_out=counts_slot, auc_out=auc_slot)
                if scheduler is not None:
                    scheduler.step()
                if hist.full:
                    consume()
            consume()
            if ge is not None:
                ge.finish()
            _say(verbose, '[Run-{} score] {}'.format(train_id, best_acc))
            for k in final_acc:
                final_acc[k].append(best_acc[k])
            if history is not None:
                history.update(eval_res=eval_hist, best_epoch=best_epoch[0], best_acc=dict(best_acc), final_acc=final_acc)
        _summary(final_acc, best_acc, verbose)
    return loss_bucket, res_bucket_each


def _train_step_noDTC(data, model, optimizer, plan, gnn):
    model.train()
    optimizer.zero_grad()
    out = model(data)
    log_probs, loss_dist = out if gnn == 'KTGNN' else (out, None)
    loss, terms = ops.step2_nll(log_probs, plan.y, plan.train_u8, return_terms=True)
    if loss_dist is not None:
        loss = loss + loss_dist
    loss.backward()
    optimizer.step()
    return loss.detach(), terms


def train_noDTC(data, model, optimizer, gnn=None):
    """main_graph_knowledge_transfer.py:265-275 -> the loss as a Python float"""
    return _train_step_noDTC(data, model, optimizer, _plan(data, False), gnn)[0].item()


def test_noDTC(data, model, gnn=None, metric='f1', f1_average='macro'):
    """main_graph_knowledge_transfer.py:279-300 -> [train, val, test] scores of `model(data)` over the three masks (all rows)."""
    plan = _plan(data, False)
    if metric == 'auc':
        auc = torch.empty(3, dtype=torch.float64, device=plan.y.device)
        _eval_plain(data, model, plan, auc_out=auc)
        return [_check_auc(v) for v in auc.tolist()]
    if metric not in ('f1', 'acc'):
        raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
    counts, _ = _eval_plain(data, model, plan)
    return [score_from_counts(c, metric, f1_average) for c in counts.cpu().numpy()]


def train_gnn_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, gnn='GCN', seed=None, num_layer=2, hidden=64,
                    lr=1e-3, wd=5e-3, use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro',
                    dropout=0.5, verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 for `gnn='GraphSAGE'` (what `main` passes under --no_dtc: `sage.GraphSAGE`) and
    `gnn='GCN'` (the function's own default: `gcn.GCNNet`), Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` (:374); `save=True` writes
    {ckpt_dir}/model_{gnn}_{args.dataset_name}_share_best.ckpt.  Returns None like the reference; `history` (a dict) receives
    'loss_train', 'eval_res', 'best_epoch', 'best_acc', 'final_acc'.  `graphed=True`: as in `train_gnn`."""
    if gnn not in ('GraphSAGE', 'GCN'):
        if gnn in ('MLP', 'GAT', 'GATv2', 'KTGNN'):
            raise NotImplementedError(f"train_gnn_noDTC(gnn={gnn!r}): the baselines implemented here are GraphSAGE (the one `main` "
                                      "uses) and GCN; GAT and GATv2 run through gat.train_gat_noDTC and gatv2.train_gatv2_noDTC; "
                                      "MLP and KTGNN without DTC are not built")
        raise NotImplementedError('Not Implemented Model:{}'.format(gnn))
    from .gcn import GCNNet
    from .sage import GraphSAGE

    def make_model():
        if gnn == 'GCN':
            return GCNNet(dataset, num_layer, hidden=hidden, dropout=dropout)
        return GraphSAGE(dataset, num_layer, hidden, root_weight=True, dropout=dropout)

    return _train_plain_backbone(args, dataset, data, make_model, gnn, lambda model: len(model.convs) - 1 if dropout > 0 else 0,
                                 save, repeat, num_epoch, seed, lr, wd, use_scheduler, step_size, gamma, metric, f1_average, verbose,
                                 ckpt_dir, history, graphed)


def _train_plain_backbone(args, dataset, data, make_model, tag, dropout_words, save, repeat, num_epoch, seed, lr, wd, use_scheduler,
                          step_size, gamma, metric, f1_average, verbose, ckpt_dir, history, graphed):
    """The run of `train_gnn_noDTC` (:302-396) for any backbone whose forward returns log-probabilities: `make_model()` builds it (on
    the host, after the seed is set), `tag` names it in the checkpoint file, `dropout_words(model)` is the number of dropout seeds
    one training forward takes (the words a captured epoch prepares)."""
    dev = _device_of(args)
    with torch.cuda.device(dev):
        data = data.to(dev)
        plan = _plan(data, False)
        C = dataset.num_classes
        plan.check_classes(C)
        if metric == 'auc':
            _need_binary(C)
        elif metric not in ('f1', 'acc'):
            raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
        final_acc = {'train': [], 'val': [], 'test': []}
        if save:
            os.makedirs(ckpt_dir, exist_ok=True)
        for train_id in range(1, 1 + repeat):
            _say(verbose, 'repeat {}/{}'.format(train_id, repeat))
            data_split_seed = 0
            model_init_seed = train_id - 1 if seed is None else seed
            set_random_seed(model_init_seed)
            model = make_model().to(dev)
            _prime(model, data, lambda lp: ops.step2_nll(lp, plan.y, plan.train_u8))
            _say(verbose, data)
            _say(verbose, model)
            _say(verbose, 'auto fixed data split seed to {}, model init seed to {}'.format(data_split_seed, model_init_seed))
            if verbose:
                print(data)
                print('[Dataset-{}] train_num:{}, val_num:{}, test_num:{}, class_num:{}'.format(
                    dataset, data.train_mask.sum().item(), data.val_mask.sum().item(), data.test_mask.sum().item(), dataset.num_classes))
            if graphed:
                optimizer = _graphed_optimizer(model, lr, wd, num_epoch, step_size if use_scheduler else None, gamma)
                scheduler = None
            else:
                optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
                scheduler = StepLR(optimizer, step_size=step_size, gamma=gamma) if use_scheduler else None
            best_acc = {'train': 0, 'val': 0, 'test': 0, 'loss': 666}
            eval_hist, loss_hist, best_epoch = [], [], [None]
            hist = _History(dev, num_epoch, 2, len(_PLAIN_COMBOS), C, metric == 'auc', 1 if (verbose or save) else 0)
            t0 = [time.time()]

            def consume():
                for terms, counts, auc in hist.drain():
                    epoch = len(eval_hist) + 1
                    loss_train = terms[0]
                    if metric == 'auc':
                        eval_res = [_check_auc(v) for v in auc]
                    else:
                        eval_res = [score_from_counts(counts[k], metric, f1_average) for k in range(3)]
                    eval_hist.append(eval_res)
                    loss_hist.append(loss_train)
                    _say(verbose, 'Epoch: {:03d}, Loss:{:.4f} Train: {:.4f}, Val:{:.4f}, Test: {:.4f}, Time(s/epoch):{:.4f}'.format(
                        epoch, loss_train, *eval_res, time.time() - t0[0]))
                    if select_best([loss_train], best_acc['loss']):                     # :374
                        best_acc['train'], best_acc['val'], best_acc['test'] = eval_res
                        best_acc['loss'] = loss_train
                        best_epoch[0] = epoch - 1
                        if save:
                            torch.save(model.state_dict(), os.path.join(ckpt_dir, f'model_{tag}_{args.dataset_name}_share_best.ckpt'))

            ge = None
            if graphed:
                ge = _GraphedEpoch(data, model, optimizer, hist, num_epoch, dropout_words(model),
                                   lambda lp: ops.step2_nll(lp, plan.y, plan.train_u8, return_terms=True),
                                   lambda counts, auc: _eval_plain(data, model, plan, counts_out=counts, auc_out=auc))
            for epoch in range(1, 1 + num_epoch):
                t0[0] = time.time()
                terms_slot, counts_slot, auc_slot = hist.slot()
                if ge is not None:
                    ge.replay()
                else:
                    terms_slot.copy_(_train_step_noDTC(data, model, optimizer, plan, None)[1])    # gnn=None: the forward returns log-probabilities alone
                    _eval_plain(data, model, plan, counts_out=counts_slot, auc_out=auc_slot)
                if scheduler is not None:
                    scheduler.step()
                if hist.full:
                    consume()
            consume()
            if ge is not None:
                ge.finish()
            _say(verbose, '[Run-{} score] {}'.format(train_id, best_acc))
            for k in final_acc:
                final_acc[k].append(best_acc[k])
            if history is not None:
                history.update(loss_train=loss_hist, eval_res=eval_hist, best_epoch=best_epoch[0], best_acc=dict(best_acc),
                               final_acc=final_acc)
        _summary(final_acc, best_acc, verbose)


# the reference's command line (:424-435) as a table: flag -> (type | None for a switch, default, choices, help)
_FLAGS = {
    "gpu": (int, 0, None, "index of the GPU to run on"),
    "dataset_name": (str, "twitter_unrelational", None, "name used in log lines and checkpoint files"),
    "model_name": (str, "KTGNN", ("MLP", "GCN", "GAT", "GATv2", "GraphSAGE", "KTGNN"), "backbone (only KTGNN trains here; the baselines run under --no_dtc --baseline)"),
    "eval_metric": (str, "f1", ("f1", "auc"), "score reported per epoch"),
    "save": (None, False, None, "write the best epoch's parameters"),
    "to_undirected": (None, False, None, "add every edge's reverse before training"),
    "no_dtc": (None, False, None, "train a plain backbone (see --baseline) on the bridged graph instead of KTGNN"),
    "baseline": (str, "GraphSAGE", ("GraphSAGE", "GCN"), "the backbone --no_dtc trains (this package's own flag: the reference always "
                 "trains GraphSAGE there and ignores --model_name)"),
    "graphed": (None, False, None, "run every epoch as one replay of a captured HIP graph (the same run, launch cost paid once)"),
    "num_layer": (int, 2, None, None),
    "num_epoch": (int, 300, None, None),
    "hidden_dim": (int, 64, None, None),
    "path_data": (str, "../data_bridged_graph/twitter_unrelational_bridged_graph.dat", None, "bridged graph written by step 1"),
}


def build_parser():
    """the reference's flags and defaults (`--gpu` is honoured here)"""
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.transfer", description="Step 2 of Bridged-GNN: knowledge transfer on a bridged graph")
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=default, choices=choices, help=text)
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421.  `args`: the parsed namespace, or a list of command-line words (None: sys.argv).
    -> what the routed trainer returns ((loss_bucket, res_bucket_each), or None under --no_dtc)."""
    from .bridge import eval_bridged_Graph
    if args is None or isinstance(args, (list, tuple)):
        args = build_parser().parse_args(args)
    set_random_seed(0)
    dev = _device_of(args)
    with torch.cuda.device(dev):
        data = load_bridged_graph(args.path_data).to(dev)
        _say(verbose, data)
        eval_bridged_Graph(data)
        data.train_mask[data.y == -1] = False
        dataset = pyg_dataset(data)
        step_size, gamma = 100, 0.1
        if args.to_undirected:
            data.to_undirected_()
        if args.no_dtc:
            return train_gnn_noDTC(args, dataset, data, save=False, repeat=1, num_epoch=args.num_epoch, gnn=getattr(args, "baseline", "GraphSAGE"), seed=0,
                                   num_layer=args.num_layer, hidden=args.hidden_dim, lr=1e-3, wd=5e-3, use_scheduler=False, step=1,
                                   step_size=step_size, gamma=gamma, metric=args.eval_metric, f1_average='macro', verbose=verbose,
                                   graphed=getattr(args, "graphed", False))
        return train_gnn(args, dataset, data, save=False, repeat=1, num_epoch=args.num_epoch, step_size=step_size, gamma=gamma,
                         gnn=args.model_name, seed=0, num_layer=args.num_layer, hidden=args.hidden_dim, lr=1e-3, wd=5e-3,
                         use_shceduler=True, step=1, Lambda=1., metric=args.eval_metric, f1_average='macro', verbose=verbose,
                         graphed=getattr(args, "graphed", False))


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(args=_args)
