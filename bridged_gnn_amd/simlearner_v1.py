"""Step 1 of the bridged-graph recipe with the v1 similarity learner, the reference's default (`Adversarial_Learner` with
GraphSAGE encoders and the cosine pair scorer `Similar`, models/models.py:67-169, :220-263, :576-622, :704-750, :815-844;
`train_adv_few_shot` / `eval_adv` / `main_adv`, scripts.py:28-94, :98-309).  Recipes #1, #4 and #5 of run.sh train it.

Modules keep the reference's class names, constructor arguments and state_dict keys, so a checkpoint written here loads into the
reference with strict=True and into `bridge.BridgeScorer` (version v1, sim_mode cosine) without conversion.

The cosine scorer is exact in per-node form: biasatt is row-wise, so q = u + biasatt(u), u = lin_self(z)
and its row normalisation are computed once per node; what is left per pair is one 128-wide dot.  Training runs the pair lists
through the HIP loss pass and the backward through one atomic-free segment sum per domain (csrc/bgnn_pair_cos.hip,
`_CosPairsFn`); evaluation counts TP / FP / FN / TN over the reference's full Cartesian products without materialising a pair.

Supported: norm_mode 'None' (ReLU + dropout fused into the SAGE epilogue) and the three PairNorm modes (unfused), metric 'f1'.
`conf_lower_bound` and metric 'auc' raise NotImplementedError (no recipe passes them).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ktgnn import Linear
from .sage import SAGEConv, SageGraph
from .simlearner import (Decoder, Discriminator, PairNorm, Pair_Enumerator, Pair_Enumerator_cross, _dev_idx, _to, f1_from_counts,
                         macro_f1, make_optimizers)

__all__ = ["GraphEncoder", "Similar", "Source_Learner", "Target_Learner_AE", "Adversarial_Learner", "cosine_normalize",
           "train_adv_few_shot", "eval_within_domain", "eval_cross_domain", "eval_adv", "main_adv", "twitter_self_loops"]

Q = ops.PAIR_COS_WIDTH


def _unsupported(what):
    raise NotImplementedError(f"{what} is not supported by bridged_gnn_amd.simlearner_v1")


class GraphEncoder(nn.Module):
    """models/models.py:220-263: SAGEConv -> PairNorm -> ReLU -> dropout(0.5) -> SAGEConv.  With norm_mode 'None' the ReLU and the
    dropout run fused in the first conv's aggregation epilogue; the other PairNorm modes run conv, PairNorm, ReLU, dropout in
    turn.  `dropout=False` switches the dropout off (tests)."""

    def __init__(self, dim_in, dim_out, dim_hidden=64, layer_num=2, root_weight=True, norm_mode="PN-SCS", norm_scale=1,
                 log_softmax=False, dropout=True):
        super().__init__()
        self.convs = nn.ModuleList()
        if layer_num == 1:
            self.convs.append(SAGEConv(dim_in, dim_out, root_weight=root_weight))
        else:
            for num in range(layer_num):
                a = dim_in if num == 0 else dim_hidden
                b = dim_out if num == layer_num - 1 else dim_hidden
                self.convs.append(SAGEConv(a, b, root_weight=root_weight))
        self.norm = PairNorm(mode=norm_mode, scale=norm_scale)
        self.log_softmax, self.dropout = log_softmax, dropout
        self._graph_key = self._graph = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """SageGraph of edge_index, cached against the tensor (identity, in-place version, shape)."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = SageGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, x, edge_index):
        g = edge_index if isinstance(edge_index, SageGraph) else self.graph(edge_index, x.shape[0])
        p = 0.5 if (self.dropout and self.training) else 0.0
        last = len(self.convs) - 1
        for ind, conv in enumerate(self.convs):
            if ind == last:
                x = conv.run(x, g)
            elif self.norm.mode == "None":
                x = conv.run(x, g, epilogue="relu", p_drop=p)
            else:
                x = F.relu(self.norm(conv.run(x, g)))
                if p > 0:
                    x = F.dropout(x, p=p, training=True)
        return F.log_softmax(x, dim=1) if self.log_softmax else x


def cosine_normalize(q, eps=1e-8):
    """q / max(|q|_2, eps) per row, formed as torch 2.x's cosine_similarity forms it (the norm cloned, then clamped in place under
    no_grad), so autograd through it is the reference's own gradient, zero rows included."""
    n = torch.linalg.vector_norm(q, 2, dim=1, keepdim=True).clone()
    with torch.no_grad():
        n.clamp_min_(eps)
    return q / n


class _CosPairsFn(torch.autograd.Function):
    """Mean BCE of sigmoid(q^a[idx1] . q^b[idx2]) for K pair lists over normalised per-node tables.  plan[k] = (a, b) names the two
    tables of list k (a == b for a within-domain list).  -> (loss_1, ..., loss_K, counts [K, 3] = TP, FP, FN at p > 0.5).
    The backward forms, per table, one segment sum over every pair that references it (all lists, both sides):
    G_t[n] = sum_p dl_p q^other(p), atomic-free, each row written once."""

    @staticmethod
    def forward(ctx, plan, n_tab, *args):
        tables, lists = args[:n_tab], args[n_tab:]
        losses, counts, dls = [], [], []
        for k, (a, b) in enumerate(plan):
            i1, i2, y = lists[3 * k:3 * k + 3]
            _, dl, sums = ops.pair_cos_loss(tables[a], tables[b], i1, i2, y)
            losses.append((sums[0] / int(i1.shape[0])).to(torch.float32))
            counts.append(sums[1:4])
            dls.append(dl)
        ctx.plan, ctx.n_tab = plan, n_tab
        ctx.save_for_backward(*tables, *[t for k in range(len(plan)) for t in lists[3 * k:3 * k + 2]], *dls)
        counts = torch.stack(counts)
        ctx.mark_non_differentiable(counts)
        return (*losses, counts)

    @staticmethod
    def backward(ctx, *grads):
        plan, n_tab, K = ctx.plan, ctx.n_tab, len(ctx.plan)
        saved = ctx.saved_tensors
        tables, idx, dls = saved[:n_tab], saved[n_tab:n_tab + 2 * K], saved[n_tab + 2 * K:]
        sizes = [int(t.shape[0]) for t in tables]
        off = np.concatenate(([0], np.cumsum(sizes)))
        allq = tables[0] if n_tab == 1 else torch.cat(tables).contiguous()
        n_all = int(off[-1])
        out = []
        for t in range(n_tab):
            if not ctx.needs_input_grad[2 + t]:
                out.append(None)
                continue
            own, other, dl = [], [], []
            for k, (a, b) in enumerate(plan):
                i1, i2 = idx[2 * k], idx[2 * k + 1]
                d = dls[k] * grads[k].to(torch.float32)
                if a == t:
                    own.append(i1), other.append(i2 + int(off[b])), dl.append(d)
                if b == t:
                    own.append(i2), other.append(i1 + int(off[a])), dl.append(d)
            if not own:
                out.append(torch.zeros_like(tables[t]))
                continue
            own, other, dl = torch.cat(own), torch.cat(other).contiguous(), torch.cat(dl).contiguous()
            rp, pm = ops.pair_csr(own, other, sizes[t], n_all)
            out.append(ops.pair_cos_segsum(allq, rp, pm, other, dl))
        return (None, None, *out, *([None] * (3 * K)))


def cos_pair_losses(tables, plan, lists):
    """tables: normalised [N_t, 128] fp32 tables; plan: [(a, b)] per list; lists: [(idx1, idx2, y_pair)] on the tables' device.
    -> ([mean BCE per list], counts [K, 3] fp64)."""
    flat = []
    for i1, i2, y in lists:
        flat += [i1.contiguous(), i2.contiguous(), y.to(torch.uint8).reshape(-1).contiguous()]
    tabs = [t.contiguous() for t in tables]
    r = _CosPairsFn.apply(tuple(plan), len(tabs), *tabs, *flat)
    return list(r[:-1]), r[-1]


class Similar(nn.Module):
    """models/models.py:67-169, the cosine pair scorer.  Keys biasatt.{0,2}.*, lin_clf.*, lin_self.{0,1,2,4}.* as in the reference;
    `train_dropout=False` switches off the 0.6 dropout before lin_clf (tests)."""

    def __init__(self, in_channels, num_clf_classes, dropout=0.6, use_clf=True, train_dropout=True):
        super().__init__()
        self.biasatt = nn.Sequential(
            Linear(Q, 64, bias=True, weight_initializer="glorot"),
            nn.Tanh(),
            Linear(64, Q, bias=True, weight_initializer="glorot"),
        )
        for m in self.biasatt:
            if isinstance(m, nn.Linear):          # the reference's test: its PyG Linear layers are not nn.Linear, so none is re-drawn
                nn.init.kaiming_normal_(m.weight)
                nn.init.constant_(m.bias, 0)
        self.use_clf = use_clf
        if use_clf:
            self.lin_clf = Linear(in_channels, num_clf_classes, bias=True, weight_initializer="glorot")
        self.lin_self = nn.Sequential(
            nn.BatchNorm1d(in_channels),
            Linear(in_channels, 64, bias=False, weight_initializer="glorot"),
            nn.BatchNorm1d(64),
            nn.Tanh(),
            Linear(64, Q, bias=False, weight_initializer="glorot"),
        )
        self.dropout, self.train_dropout = dropout, train_dropout
        self.reset_parameters()

    def reset_parameters(self):
        if self.use_clf:
            self.lin_clf.reset_parameters()
        for m in self.lin_self:
            if isinstance(m, nn.Linear):
                m.reset_parameters()

    def classify(self, z):
        """log_softmax(lin_clf(dropout(relu(z)))) (:133-137)"""
        h = F.relu(z)
        if self.train_dropout:
            h = F.dropout(h, p=self.dropout, training=self.training)
        return F.log_softmax(self.lin_clf(h), dim=-1)

    def node_q(self, z):
        """q = u + biasatt(u), u = lin_self(z): one lin_self call (in train mode: batch statistics, one running update)."""
        u = self.lin_self(z)
        return u + self.biasatt(u)

    def node_qhat(self, z):
        return cosine_normalize(self.node_q(z))

    def advance_bn(self, *zs):
        """lin_self's running statistics and num_batches_tracked as further train-mode calls on zs would leave them (no output)."""
        if self.training:
            with torch.no_grad():
                for z in zs:
                    self.lin_self(z.detach())

    def _scores(self, z1, z2, idx1, idx2):
        if self.training:
            raise RuntimeError("Similar: train-mode pair scores go through cos_pair_losses (the loss is fused into the pair pass)")
        with torch.no_grad():
            q1 = self.node_qhat(z1)
            q2 = q1 if z2 is z1 else self.node_qhat(z2)
            idx1, idx2 = idx1.long().contiguous(), idx2.long().contiguous()
            if idx1.numel() == 0:
                return torch.empty(0, dtype=torch.float32, device=z1.device)
            y = torch.zeros(idx1.shape[0], dtype=torch.uint8, device=z1.device)
            return ops.pair_cos_loss(q1.contiguous(), q2.contiguous(), idx1, idx2, y)[0]

    def similarity_cross_domain(self, x_src, x_tar, idx1, idx2):
        return self._scores(x_src, x_tar, idx1, idx2)

    def similarity(self, x, idx1, idx2):
        return self._scores(x, x, idx1, idx2)

    def forward_cross_domain(self, x_src, x_tar, idx1, idx2):
        lp_src = lp_tar = None
        if self.use_clf:
            lp_src, lp_tar = self.classify(x_src), self.classify(x_tar)
        return self.similarity_cross_domain(x_src, x_tar, idx1, idx2).unsqueeze(-1), lp_src, lp_tar

    def forward(self, x, idx1, idx2):
        lp = self.classify(x) if self.use_clf else None
        return self.similarity(x, idx1, idx2).unsqueeze(-1), lp


class Source_Learner(nn.Module):
    """models/models.py:576-622"""

    def __init__(self, data, dim_hidden=64, norm_mode="None", norm_scale=1, use_clf=True, dropout=True):
        super().__init__()
        self.dim_in, self.num_classes, self.dim_hidden = data.num_features, int(data.y.max().item()) + 1, dim_hidden
        self.backbone = GraphEncoder(self.dim_in, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True, norm_mode=norm_mode,
                                     norm_scale=norm_scale, log_softmax=False, dropout=dropout)
        self.sim_net = Similar(dim_hidden, num_clf_classes=self.num_classes, dropout=0.6, use_clf=use_clf, train_dropout=dropout)
        self.reset_parameters()

    def reset_parameters(self):
        self.backbone.reset_parameters()
        self.sim_net.reset_parameters()

    def forward(self, data, idx1, idx2, return_representation=False):
        h = self.backbone(data.x, data.edge_index)
        probs_pair, logits_clf = self.sim_net(h, idx1, idx2)
        return (probs_pair, logits_clf, h) if return_representation else (probs_pair, logits_clf)


class Target_Learner_AE(nn.Module):
    """models/models.py:704-750"""

    def __init__(self, data, dim_eq_trans=128, dim_hidden=64, norm_mode="None", norm_scale=1, dropout=True):
        super().__init__()
        self.dim_in, self.dim_eq_trans = data.num_features, dim_eq_trans
        self.num_classes, self.dim_hidden = int(data.y.max().item()) + 1, dim_hidden
        self.equavilent_trans_layer = nn.Sequential(Linear(self.dim_in, dim_eq_trans, bias=True),
                                                    PairNorm(mode=norm_mode, scale=norm_scale), nn.Tanh())
        self.encoder = GraphEncoder(dim_eq_trans, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True, norm_mode=norm_mode,
                                    norm_scale=norm_scale, log_softmax=False, dropout=dropout)
        self.decoder = Decoder(dim_hidden, dim_hidden, dim_eq_trans, num_layer=2, use_norm=True, dropout=0.5, act_fn="relu",
                               norm_mode=norm_mode, norm_scale=norm_scale)
        self.reset_parameters()

    def reset_parameters(self):
        self.encoder.reset_parameters()
        self.decoder.reset_parameters()

    def encode(self, data):
        h0 = self.equavilent_trans_layer(data.x)
        return self.encoder(h0, data.edge_index), h0

    def decode(self, z):
        return torch.tanh(self.decoder(z))

    def forward(self, data):
        z, h0 = self.encode(data)
        return h0, z, self.decode(z)


class Adversarial_Learner(nn.Module):
    """models/models.py:815-844.  `dropout=False` switches every dropout off (tests)."""

    def __init__(self, data_src, data_tar, dim_hidden=64, num_layer=2, source_clf=True, norm_mode="PN", norm_scale=1., dropout=True):
        super().__init__()
        self.num_layer, self.source_clf = num_layer, source_clf
        self.source_learner = Source_Learner(data_src, dim_hidden=dim_hidden, norm_mode=norm_mode, norm_scale=norm_scale,
                                             use_clf=source_clf, dropout=dropout)
        self.target_learner = Target_Learner_AE(data_tar, dim_eq_trans=128, dim_hidden=dim_hidden, norm_mode=norm_mode,
                                                norm_scale=norm_scale, dropout=dropout)
        self.discriminator = Discriminator(dim_hidden, dim_hidden, num_layer=2, use_pair_norm=False, dropout=0.5, act_fn="relu",
                                           sigmoid_output=True, norm_mode=norm_mode, norm_scale=norm_scale)

    def get_probs_within_domain(self, data, idx1, idx2, domain="target"):
        if domain == "source":
            probs_pair, log_probs_clf = self.source_learner(data, idx1, idx2, return_representation=False)
        else:
            z, _ = self.target_learner.encode(data)
            probs_pair, log_probs_clf = self.source_learner.sim_net(z, idx1, idx2)
        if not self.source_clf:
            log_probs_clf = torch.zeros((data.x.shape[0], int(data.y.max().item()) + 1), device=data.x.device)
        return probs_pair, log_probs_clf.exp()

    def get_probs_cross_domain(self, data_src, data_tar, idx1, idx2, return_representation=False):
        z_src = self.source_learner.backbone(data_src.x, data_src.edge_index)
        z_tar, _ = self.target_learner.encode(data_tar)
        probs_pair, lp_src, lp_tar = self.source_learner.sim_net.forward_cross_domain(z_src, z_tar, idx1, idx2)
        if not self.source_clf:
            lp_src = torch.zeros((z_src.shape[0], int(data_src.y.max().item()) + 1), device=z_src.device)
            lp_tar = torch.zeros((z_tar.shape[0], int(data_tar.y.max().item()) + 1), device=z_tar.device)
        if return_representation:
            return probs_pair, lp_src.exp(), lp_tar.exp(), z_src.detach(), z_tar.detach()
        return probs_pair, lp_src.exp(), lp_tar.exp()


def twitter_self_loops(data_src):
    """main_bridged_graph.py:335-340: for the twitter datasets the source graph's edges are replaced by one self loop per node.
    Returns the original edge_index; data_src is changed in place."""
    ori = data_src.edge_index
    n = int(data_src.x.shape[0])
    ar = torch.arange(n, device=ori.device)
    data_src.edge_index = torch.stack((ar, ar), dim=0)
    return ori


# ---- training / evaluation (scripts.py) ---------------------------------------------------------------------------------------------
def train_adv_few_shot(epoch, data_src, data_tar, model, optimizer_src_tar, optimizer_D, metric="f1", pair_enumerator_src_train=None,
                       pair_enumerator_tar_train=None, pair_enumerator_cross_train=None, max_class_num=2, sample_size=10000,
                       use_clf=False, verbose=False):
    """scripts.py:28-94 with the v1 model: one step of the similarity learner + auto-encoder, then one discriminator step.
    -> (loss_sim, (f1_src, f1_tar, f1_cross), loss_d, loss_ae, loss_g, loss_recons) like the reference.
    lin_self runs in train mode on h_src and h_tar once each; its BatchNorms are then advanced twice more (src, tar), as the
    reference's similarity_cross_domain recomputes both."""
    if metric != "f1":
        _unsupported(f"metric={metric!r}")
    model.train()
    dev = data_src.x.device
    sim = model.source_learner.sim_net
    optimizer_src_tar.zero_grad()
    i1s, i2s = (_dev_idx(t, dev) for t in pair_enumerator_src_train.sampling(max_class_num=max_class_num, sample_size=sample_size,
                                                                             shuffle=False))
    h_src = model.source_learner.backbone(data_src.x, data_src.edge_index)
    lp_src = sim.classify(h_src) if sim.use_clf else None
    q_src = sim.node_qhat(h_src)
    i1t, i2t = (_dev_idx(t, dev) for t in pair_enumerator_tar_train.sampling(max_class_num=max_class_num, sample_size=sample_size,
                                                                             shuffle=False))
    h0_tar, h_tar, recons = model.target_learner(data_tar)
    lp_tar = sim.classify(h_tar) if sim.use_clf else None
    q_tar = sim.node_qhat(h_tar)
    i1c, i2c = (_dev_idx(t, dev) for t in pair_enumerator_cross_train.sampling(max_class_num=max_class_num, sample_size=sample_size,
                                                                               shuffle=False))
    sim.advance_bn(h_src, h_tar)
    ys, yt = data_src.y, data_tar.y
    (loss_src, loss_tar, loss_cross), cnt = cos_pair_losses(
        (q_src, q_tar), ((0, 0), (1, 1), (0, 1)),
        ((i1s, i2s, ys[i1s] == ys[i2s]), (i1t, i2t, yt[i1t] == yt[i2t]), (i1c, i2c, ys[i1c] == yt[i2c])))
    loss_recons = F.mse_loss(recons, h0_tar)
    g_labels = torch.ones((h_tar.shape[0], 1), device=dev)
    loss_g = F.binary_cross_entropy(model.discriminator(h_tar), g_labels)
    loss_ae = loss_g + loss_recons * 0.1
    loss_sim = loss_src + loss_tar + loss_cross + loss_ae
    if use_clf:
        tm_s, tm_t = data_src.train_mask, data_tar.train_mask
        loss_clf_src = F.nll_loss(lp_src[tm_s], data_src.y[tm_s])
        loss_clf_tar = F.nll_loss(lp_tar[tm_t], data_tar.y[tm_t])
        loss_sim = loss_sim + loss_clf_src + loss_clf_tar
        if verbose:
            print("Loss_sim:{:.4f} | Loss_clf_src:{:.4f} | Loss_clf_tar:{:.4f}".format(loss_sim.item(), loss_clf_src.item(),
                                                                                        loss_clf_tar.item()))
    loss_sim.backward()
    optimizer_src_tar.step()
    c = cnt.tolist()
    eval_pair = tuple(f1_from_counts(*c[k]) for k in range(3))
    optimizer_D.zero_grad()
    real_loss = F.binary_cross_entropy(model.discriminator(h_src.detach()), torch.ones((h_src.shape[0], 1), device=dev))
    fake_loss = F.binary_cross_entropy(model.discriminator(h_tar.detach()), torch.zeros((h_tar.shape[0], 1), device=dev))
    loss_d = (real_loss + fake_loss) / 2
    loss_d.backward()
    optimizer_D.step()
    return loss_sim.item(), eval_pair, loss_d.item(), loss_ae.item(), loss_g.item(), loss_recons.item()


def _check_eval(conf_lower_bound):
    if conf_lower_bound is not None:
        _unsupported("conf_lower_bound")


def _rows(mask):
    return torch.nonzero(mask).reshape(-1).contiguous()


def _tables(model, data_src=None, data_tar=None):
    """eval-mode (z, q^) of each given domain"""
    sim = model.source_learner.sim_net
    out = []
    if data_src is not None:
        z = model.source_learner.backbone(data_src.x, data_src.edge_index)
        out.append((z, sim.node_qhat(z).contiguous()))
    if data_tar is not None:
        z, _ = model.target_learner.encode(data_tar)
        out.append((z, sim.node_qhat(z).contiguous()))
    return out


def _clf_score(model, data, z, mask_2):
    y2 = data.y[mask_2]
    if model.source_clf:
        pred = model.source_learner.sim_net.classify(z)[mask_2].max(1)[1]
    else:
        pred = torch.zeros_like(y2)
    if int(data.y.max().item()) <= 1:             # f1_score(average='binary' if max(y) <= 1 else 'macro'), scripts.py:177
        yb, pb = y2 == 1, pred == 1
        return f1_from_counts((yb & pb).sum().item(), (~yb & pb).sum().item(), (yb & ~pb).sum().item())
    return macro_f1(y2, pred)


def _within(data, model, mode, z, qh):
    mask_1 = data.train_mask | data.val_mask | data.test_mask
    mask_2 = data.val_mask if mode == "val" else data.test_mask
    y = data.y.long().contiguous()
    counts = ops.pair_cos_count(qh, qh, _rows(mask_1), _rows(mask_2), y, y)
    tp, fp, fn, _ = counts.tolist()
    return f1_from_counts(tp, fp, fn), _clf_score(model, data, z, mask_2)


def _cross_counts(data_src, data_tar, mode, qs, qt):
    """the two Cartesian products of eval_cross_domain (scripts.py:100-116) -> int64 [4] TP, FP, FN, TN"""
    if mode == "val":
        m_s1, m_t1 = data_src.val_mask, data_tar.train_mask | data_tar.val_mask
        m_s2, m_t2 = data_src.train_mask, data_tar.val_mask
    else:
        m_s1, m_t1 = data_src.test_mask, data_tar.train_mask | data_tar.test_mask | data_tar.val_mask
        m_s2, m_t2 = data_src.train_mask | data_src.val_mask, data_tar.test_mask
    ys, yt = data_src.y.long().contiguous(), data_tar.y.long().contiguous()
    return ops.pair_cos_count(qs, qt, _rows(m_s1), _rows(m_t1), ys, yt) + ops.pair_cos_count(qs, qt, _rows(m_s2), _rows(m_t2), ys, yt)


def eval_within_domain(data, model, mode="test", domain="target", conf_lower_bound=None):
    """scripts.py:144-190 -> (pair f1 over all labelled nodes x the val / test nodes, classifier f1 on the split)"""
    _check_eval(conf_lower_bound)
    with torch.no_grad():
        model.eval()
        (z, qh), = _tables(model, data, None) if domain == "source" else _tables(model, None, data)
        return _within(data, model, mode, z, qh)


def eval_cross_domain(data_src, data_tar, model, mode="test", conf_lower_bound=None):
    """scripts.py:98-141 -> pair f1 over the two concatenated Cartesian products"""
    _check_eval(conf_lower_bound)
    with torch.no_grad():
        model.eval()
        (_, qs), (_, qt) = _tables(model, data_src, data_tar)
        tp, fp, fn, _ = _cross_counts(data_src, data_tar, mode, qs, qt).tolist()
    return f1_from_counts(tp, fp, fn)


def eval_adv(data_src, data_tar, model, mode="test"):
    """scripts.py:192-196 -> (pair_src, clf_src, pair_tar, clf_tar, pair_cross).  Each domain is encoded once for all three."""
    with torch.no_grad():
        model.eval()
        (zs, qs), (zt, qt) = _tables(model, data_src, data_tar)
        ps, cs = _within(data_src, model, mode, zs, qs)
        pt, ct = _within(data_tar, model, mode, zt, qt)
        tp, fp, fn, _ = _cross_counts(data_src, data_tar, mode, qs, qt).tolist()
    return ps, cs, pt, ct, f1_from_counts(tp, fp, fn)


def main_adv(args, data_src, data_tar, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, metric="f1",
             use_clf=True, norm_mode="PN", norm_scale=1., eval_per_epoch=1, start_eval_epoch=0, sim_mode="mlp", backbone="mlp",
             device=None, ckpt_dir="../ckpt", dropout=True, verbose=True):
    """scripts.py:199-309 with args.version 'v1': Adversarial_Learner (norm_scale 1, as the reference hard-codes), max_class_num 2,
    sample_size 40000.  Trains `repeat` runs (model init seed = run - 1, or `seed`), evaluating from `start_eval_epoch` every
    `eval_per_epoch` epochs and keeping the epoch with the best cross-domain validation f1 (strict >).  With `save`, writes
    {ckpt_dir}/model_AdvLearner_{args.dataset_name}_best.ckpt at every improvement and _final.ckpt after each run (state_dicts).
    sim_mode / backbone are accepted and ignored, as the reference's v1 branch ignores them.  -> (state_dict of the last run's
    best epoch (CPU tensors; None if no epoch was evaluated), best_acc as the reference leaves it)."""
    from .utils import set_random_seed
    assert device is not None
    if metric != "f1":
        _unsupported(f"metric={metric!r}")
    if save:
        os.makedirs(ckpt_dir, exist_ok=True)
    data_src, data_tar = _to(data_src, device), _to(data_tar, device)
    final_acc = {"train": [], "val": [], "test": []}
    best_state = None
    for train_id in range(1, 1 + repeat):
        set_random_seed(train_id - 1 if seed is None else seed)
        model = Adversarial_Learner(data_src, data_tar, dim_hidden=hidden, num_layer=2, source_clf=use_clf, norm_mode=norm_mode,
                                    norm_scale=1., dropout=dropout).to(device)
        optimizer_src_tar, optimizer_D = make_optimizers(model)
        best_acc = {"epoch": -1, "train": (0, 0, 0), "val": (0, 0, 0), "test": (0, 0, 0), "loss": 666}
        enu = (Pair_Enumerator(data_src, mode="train"), Pair_Enumerator(data_tar, mode="train"),
               Pair_Enumerator_cross(data_src, data_tar, mode="train"))
        for epoch in range(1, 1 + num_epoch):
            loss_sim, eval_pair_train, loss_d, loss_ae, loss_g, loss_recons = train_adv_few_shot(
                epoch, data_src, data_tar, model, optimizer_src_tar, optimizer_D, metric=metric, pair_enumerator_src_train=enu[0],
                pair_enumerator_tar_train=enu[1], pair_enumerator_cross_train=enu[2], max_class_num=2, sample_size=40000,
                use_clf=use_clf)
            if verbose:
                print("[AE]Epoch: {:03d}, Loss_ae:{:.4f} | Loss_recons:{:.4f} | Loss_g:{:.4f} | Loss_d:{:.4f}".format(
                    epoch, loss_ae, loss_recons, loss_g, loss_d))
            if epoch >= start_eval_epoch and epoch % eval_per_epoch == 0:
                ps_v, cs_v, pt_v, ct_v, pc_v = eval_adv(data_src, data_tar, model, mode="val")
                ps_t, cs_t, pt_t, ct_t, pc_t = eval_adv(data_src, data_tar, model, mode="test")
                if verbose:
                    print("[Sim]Epoch: {:03d}, Loss:{:.4f} | Train Pair:{:.4f}/{:.4f}/{:.4f} | Val Pair:{:.4f}/{:.4f}/{:.4f} | "
                          "Test Pair:{:.4f}/{:.4f}/{:.4f} | Val CLF:{:.4f}/{:.4f} | Test CLF:{:.4f}/{:.4f}".format(
                              epoch, loss_sim, *eval_pair_train, ps_v, pt_v, pc_v, ps_t, pt_t, pc_t, cs_v, ct_v, cs_t, ct_t))
                if pc_v > best_acc["val"][2]:
                    best_acc.update(train=eval_pair_train, val=(ps_v, pt_v, pc_v), test=(ps_t, pt_t, pc_t), loss=loss_sim, epoch=epoch)
                    best_state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
                    if save:
                        torch.save(model.state_dict(), os.path.join(ckpt_dir, f"model_AdvLearner_{args.dataset_name}_best.ckpt"))
        if save:
            torch.save(model.state_dict(), os.path.join(ckpt_dir, f"model_AdvLearner_{args.dataset_name}_final.ckpt"))
        if verbose:
            print("[Run-{} score] {}".format(train_id, best_acc))
        for key in final_acc:
            final_acc[key].append(best_acc[key])
    for key in final_acc:
        best_acc[key] = max(final_acc[key])
    return best_state, best_acc
