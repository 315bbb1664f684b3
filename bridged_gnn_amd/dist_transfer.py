"""Step 2's KT-GNN training (`transfer.train_gnn`, the reference's main_graph_knowledge_transfer.py:143-262) on a destination-node
partition: one process per GPU, every rank training and scoring the rows it owns; new -- the reference is single-device.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m bridged_gnn_amd.dist_transfer <transfer's flags>

The run is the single-GPU eager run.  Every rank seeds and builds the same `KTGNN_no_complement` the way `train_gnn` does, so the
host generator stands where `train_gnn` leaves it before epoch 1 (its `_prime` puts both generators back) and the dropout layers
(`dist_train._SyncBnReluDrop`) draw the single-GPU run's seeds; a rank's masks are its rows of the whole-graph masks.  Per epoch:
  1. `PartitionedTrainer.forward` on the owned rows (train mode);
  2. `reference_loss_terms`: the rank's share of the loss and of the eight terms of `ops.STEP2_TERMS`; ONE all-reduce of the terms;
  3. backward, `sync_grads` (one bucketed all-reduce), Adam, StepLR -- on every rank alike, so the replicas stay equal;
  4. the eval forward of `dist.PartitionedKTGNN` over the same model (its input halo stays resident: `x` is handed over as the same
     tensor every epoch; the eval affine of every BatchNorm is rebuilt because the train forward moved the running buffers);
  5. `ops.step2_counts` on the owned rows with `transfer`'s combos and selection bits; ONE all-reduce of the int64 counts;
  6. scores from the counts on the host (`transfer.score_from_counts`), best epoch by the lowest `loss_target` (:238).
With `verbose=False, save=False` the terms and counts stay on the device until the last epoch.  Rank 0 alone prints and saves.
Not here: `metric='auc'` (its rank statistic needs every negative's score on one rank) and graphed epochs."""
import os
import time

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import StepLR

from . import ops, transfer
from .dist import PartitionedKTGNN
from .dist_train import PartitionedTrainer
from .utils import set_random_seed

__all__ = ["train_gnn_partitioned", "ranks_from_env", "build_parser", "main"]

build_parser = transfer.build_parser            # the command line is `transfer`'s, flag for flag


def train_gnn_partitioned(args, dataset, data, rank, world, device, group=None, owner=None, save=False, repeat=3, num_epoch=200,
                          gnn='GCN', seed=None, step_size=100, gamma=0.1, num_layer=2, hidden=64, lr=1e-3, wd=5e-3, use_shceduler=True,
                          step=1, Lambda=1., f1_average='macro', metric='f1', noDTC=False, dropout=0.5, verbose=True,
                          ckpt_dir='../ckpt', history=None):
    """`transfer.train_gnn` (eager) on rank `rank` of `world` -> (loss_bucket, res_bucket_each), identical on every rank.  `data` is
    the whole graph (replicated: the partition is planned from it, `owner` as in `dist.PartitionPlan`); `group`: the process group
    (None: the default one; world 1 needs none).  `history` receives what `train_gnn` puts there and 'counts': per epoch the
    int64 [5, C, C] confusion counts over all ranks (`transfer._DTC_COMBOS`).  Rank 0 alone prints and, with `save=True`, writes
    {ckpt_dir}/model_KTGNN_{args.dataset_name}_best.ckpt."""
    if gnn != 'KTGNN':
        raise NotImplementedError(f"train_gnn_partitioned(gnn={gnn!r}): KTGNN only; GraphSAGE and GCN train on a partition through "
                                  "dist_sage / dist_gcn")
    if metric == 'auc':
        raise NotImplementedError("train_gnn_partitioned(metric='auc'): the rank statistic needs every negative's score on one rank")
    if metric not in ('f1', 'acc'):
        raise NotImplementedError('NotImplemented Metric:{}'.format(metric))
    from .ktgnn import KTGNN_no_complement
    dev = torch.device(device)
    chatty = verbose and rank == 0
    say = lambda *a: transfer._say(chatty, *a)
    with torch.cuda.device(dev):
        data = data.to(dev)
        plan = transfer._plan(data, True)
        C = data.y.max().item() + 1
        plan.check_classes(C)
        final_acc = {'train': [], 'val': [], 'test': []}
        loss_bucket = {'source&target': [], 'target_hat': [], 'target': [], 'kl': []}
        ckpt = os.path.join(ckpt_dir, f'model_{gnn}_{args.dataset_name}_best.ckpt')
        if save and rank == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
        ei, cm = data.edge_index.cpu().numpy(), data.central_mask.cpu().numpy()
        for train_id in range(1, 1 + repeat):
            say('repeat {}/{}'.format(train_id, repeat))
            model_init_seed = train_id - 1 if seed is None else seed
            set_random_seed(model_init_seed)
            model = KTGNN_no_complement(dataset.num_features, C, num_layer, hidden, root_weight=False, use_dist_loss=False, dropout=dropout,
                                        use_bn=True, step=step, dim_share=data.x.shape[1], need_complement=False)
            model = model.to(dev)
            tr = PartitionedTrainer(model, ei, cm, rank, world, dev, owner=owner, group=group)
            pk = PartitionedKTGNN(model, ei, cm, rank, world, dev, owner=owner, group=group)
            own = tr.owned_global
            x_own, y_own = data.x[own].contiguous(), plan.y[own].contiguous()
            tm_own, sel_own = data.train_mask[own].bool(), plan.sel[own].contiguous()
            say(model)
            say('auto fixed data split seed to {}, model init seed to {}'.format(0, model_init_seed))
            say('[Dataset-{}] rank {}/{}: {} of {} rows, {} halo rows, class_num:{}'.format(
                args.dataset_name, rank, world, tr.n_local, tr.n_global, tr.n_halo, C))
            optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
            scheduler = StepLR(optimizer, step_size=step_size, gamma=gamma) if use_shceduler else None
            best_acc = {'train': 0, 'val': 0, 'test': 0, 'loss': 666}
            res_bucket_each = {'source&target': [], 'target': [], 'target_hat': []}
            eval_hist, counts_hist, best_epoch, pending = [], [], [None], []
            t0 = [time.time()]

            def consume():
                for terms_dev, counts_dev in pending:
                    terms, counts = terms_dev.float().cpu().tolist(), counts_dev.cpu().numpy()
                    epoch = len(eval_hist) + 1
                    loss_train, loss_target, loss_target_only, loss_kl = terms[0], terms[3], terms[2], terms[4]
                    if chatty:
                        print(terms[1], terms[2], terms[3])
                        print('Loss_clf:{:.3f} | Loss_kl:{:.3f}'.format(loss_train, loss_kl))
                    loss_bucket['source&target'].append(loss_train)
                    loss_bucket['target_hat'].append(loss_target)
                    loss_bucket['target'].append(loss_target_only)
                    loss_bucket['kl'].append(loss_kl)
                    eval_res = [transfer.score_from_counts(counts[k], metric, f1_average) for k in range(3)]
                    each = [transfer.f1_from_counts(counts[k], 'macro') for k in (3, 4, 2)]        # get_each_clf_res(metric='f1'), :227
                    eval_hist.append(eval_res)
                    counts_hist.append(counts)
                    for key, v in zip(('source&target', 'target', 'target_hat'), each):
                        res_bucket_each[key].append(v)
                    say('Epoch: {:03d}, Loss:{:.4f} Train: {:.4f}, Val:{:.4f}, Test: {:.4f}, Time(s/epoch):{:.4f}'.format(
                        epoch, loss_train, *eval_res, time.time() - t0[0]))
                    if transfer.select_best([loss_target], best_acc['loss']):                       # :238
                        best_acc['train'], best_acc['val'], best_acc['test'] = eval_res
                        best_acc['loss'] = loss_target
                        best_epoch[0] = epoch - 1
                        if save and rank == 0:                                                      # read every epoch: still this epoch's model
                            torch.save(model.state_dict(), ckpt)
                pending.clear()

            for epoch in range(1, 1 + num_epoch):
                t0[0] = time.time()
                model.train()
                optimizer.zero_grad()
                loss, terms = tr.reference_loss_terms(tr.forward(x_own), y_own, tm_own, Lambda)
                terms = tr.comm.all_reduce(terms)
                loss.backward()
                tr.sync_grads()
                optimizer.step()
                model.eval()
                lps = pk.forward(x_own)
                counts = torch.zeros(len(transfer._DTC_COMBOS), C, C, dtype=torch.int64, device=dev)
                if tr.n_local:
                    ops.step2_counts(lps, y_own, sel_own, transfer._DTC_COMBOS, out=counts)
                pending.append((terms, tr.comm.all_reduce(counts)))
                if scheduler is not None:
                    scheduler.step()
                if verbose or save:
                    consume()
            consume()
            say('[Run-{} score] {}'.format(train_id, best_acc))
            for k in final_acc:
                final_acc[k].append(best_acc[k])
            if history is not None:
                history.update(eval_res=eval_hist, counts=counts_hist, best_epoch=best_epoch[0], best_acc=dict(best_acc), final_acc=final_acc)
        transfer._summary(final_acc, best_acc, chatty)
    return loss_bucket, res_bucket_each


def ranks_from_env(env=None, n_devices=None):
    """-> (rank, world, device, backend) of this process from RANK / WORLD_SIZE / LOCAL_RANK (LOCAL_WORLD_SIZE) as
    `torch.distributed.run` sets them.  One GPU per local rank and RCCL ("nccl"); when the node has fewer GPUs than local ranks
    they share devices (a rehearsal) and the group is gloo, because RCCL refuses two ranks on one device."""
    env = os.environ if env is None else env
    rank, world = int(env.get("RANK", 0)), int(env.get("WORLD_SIZE", 1))
    local = int(env.get("LOCAL_RANK", rank))
    local_world = int(env.get("LOCAL_WORLD_SIZE", world))
    if not (0 <= rank < world):
        raise ValueError(f"RANK={rank} outside WORLD_SIZE={world}")
    n = torch.cuda.device_count() if n_devices is None else int(n_devices)
    if n < 1:
        raise RuntimeError("bridged_gnn_amd.dist_transfer needs a GPU; there is no CPU path")
    return rank, world, torch.device("cuda", local % n), ("nccl" if n >= local_world else "gloo")


def main(args=None, verbose=True, env=None):
    """`transfer.main` (main_graph_knowledge_transfer.py:399-421) for one rank of a `torch.distributed.run` launch."""
    from .bridge import eval_bridged_Graph
    from .data import load_bridged_graph
    if args is None or isinstance(args, (list, tuple)):
        args = build_parser().parse_args(args)
    if args.no_dtc:
        raise NotImplementedError("--no_dtc: the plain backbones train on a partition through bridged_gnn_amd.dist_sage / dist_gcn "
                                  "(`PartitionedSAGE`, `PartitionedGCN`); this driver trains KTGNN")
    if getattr(args, "graphed", False):
        raise NotImplementedError("--graphed: a partitioned epoch is not captured into a HIP graph; run without it")
    if args.eval_metric == 'auc':
        raise NotImplementedError("--eval_metric auc: not available on a partition; use f1")
    rank, world, dev, backend = ranks_from_env(env)
    torch.cuda.set_device(dev)
    started = False
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend, rank=rank, world_size=world, **({"device_id": dev} if backend == "nccl" else {}))
        started = True
    try:
        set_random_seed(0)
        data = load_bridged_graph(args.path_data).to(dev)
        transfer._say(verbose and rank == 0, data)
        eval_bridged_Graph(data)
        data.train_mask[data.y == -1] = False
        dataset = transfer.pyg_dataset(data)
        if args.to_undirected:
            data.to_undirected_()
        return train_gnn_partitioned(args, dataset, data, rank, world, dev, save=False, repeat=1, num_epoch=args.num_epoch,
                                     step_size=100, gamma=0.1, gnn=args.model_name, seed=0, num_layer=args.num_layer,
                                     hidden=args.hidden_dim, lr=1e-3, wd=5e-3, use_shceduler=True, step=1, Lambda=1.,
                                     metric=args.eval_metric, f1_average='macro', verbose=verbose)
    finally:
        if started:
            dist.destroy_process_group()


if __name__ == '__main__':
    _args = build_parser().parse_args()
    if int(os.environ.get("RANK", 0)) == 0:
        print(_args)
    main(args=_args)
