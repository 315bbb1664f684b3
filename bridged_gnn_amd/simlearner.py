"""Step 1 of the bridged-graph recipe: training the v2 similarity learner (`Adversarial_Learner_v2` with the mlp backbone and the
mlp pair scorer, models/models.py:852-1142; `train_adv_few_shot` / `eval_adv_v2` / `main_adv_v2`, scripts.py:28-94, :313-555).

Modules keep the reference's class names, constructor arguments and state_dict keys, so a checkpoint written here loads into the
reference with strict=True and into `bridge.BridgeScorer` without conversion.  The pair part of the scorer -- BN1 -> Linear(2H,
128) -> BN2 -> ReLU -> Linear(128, 1) -> sigmoid -> BCE over 40 000-pair lists -- runs as per-node products plus the HIP pair
passes of csrc/bgnn_pair_mlp.hip (`_PairMlpFn`; derivation in DESIGN.md section 11).  Everything else is per-node torch.

Supported: version v2, backbone 'mlp', sim_mode 'mlp', eval_mode 'sampling' (balanced pair lists, what the office recipes run,
run.sh #2/#3) and 'all' (every pair of the Cartesian split products, counted by the product pass of csrc/bgnn_pair_mlp.hip without
a pair list), evaluation metrics 'f1' and 'acc', shuffle=False samplers.  sim_mode 'cosine', backbone 'gnn', shuffling, metric
'auc', conf_lower_bound and a training metric other than 'f1' raise NotImplementedError.  The v1 learner (Adversarial_Learner, the
cosine scorer Similar) is bridged_gnn_amd.simlearner_v1.
"""
import copy
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ktgnn import Linear

__all__ = ["PairNorm", "MLP", "Decoder", "Discriminator", "Similar_v2", "Source_Learner_v2", "Target_Learner_AE_v2",
           "Adversarial_Learner_v2", "Pair_Enumerator", "Pair_Enumerator_cross", "pair_enumeration", "f1_from_counts",
           "macro_f1", "train_adv_few_shot", "eval_within_domain_v2", "eval_cross_domain_v2", "eval_adv_v2", "main_adv_v2"]

U = ops.PAIR_MLP_WIDTH


def _unsupported(what):
    raise NotImplementedError(f"{what} is not supported by bridged_gnn_amd.simlearner (v2 / mlp backbone / mlp scorer only)")


class PairNorm(nn.Module):
    """models/models.py:29-64"""

    def __init__(self, mode="PN", scale=10):
        assert mode in ["None", "PN", "PN-SI", "PN-SCS"]
        super().__init__()
        self.mode, self.scale = mode, scale

    def forward(self, x):
        if self.mode == "None":
            return x
        col_mean = x.mean(dim=0)
        if self.mode == "PN":
            x = x - col_mean
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1).mean()).sqrt()
        if self.mode == "PN-SI":
            x = x - col_mean
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1, keepdim=True)).sqrt()
        if self.mode == "PN-SCS":
            x = self.scale * x / (1e-6 + x.pow(2).sum(dim=1, keepdim=True)).sqrt() - col_mean
        return x


def _act(name):
    if name == "relu":
        return nn.ReLU()
    if name == "leakyrelu":
        return nn.LeakyReLU(0.2, inplace=False)
    if name == "tanh":
        return nn.Tanh()
    if name == "sigmoid":
        return nn.Sigmoid()
    raise NotImplementedError("Not Implemented Activation Function:{}".format(name))


class MLP(nn.Module):
    """models/models.py:852-893.  `dropout=False` switches off the 0.5 dropout after the hidden layer (tests)."""

    def __init__(self, dim_in, dim_out, dim_hidden=64, layer_num=2, root_weight=True, use_norm=False, norm_mode="PN-SCS",
                 norm_scale=1, log_softmax=False, dropout=True):
        super().__init__()
        self.layers = nn.ModuleList()
        if layer_num == 1:
            self.layers.append(Linear(dim_in, dim_out, weight_initializer="glorot"))
        else:
            for num in range(layer_num):
                a = dim_in if num == 0 else dim_hidden
                b = dim_out if num == layer_num - 1 else dim_hidden
                self.layers.append(Linear(a, b, weight_initializer="glorot"))
        if use_norm:
            self.norm = PairNorm(mode=norm_mode, scale=norm_scale)
        self.use_norm, self.log_softmax, self.dropout = use_norm, log_softmax, dropout

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()

    def forward(self, x, edge_index=None):
        for ind, layer in enumerate(self.layers):
            x = layer(x)
            if ind != len(self.layers) - 1:
                if self.use_norm:
                    x = self.norm(x)
                x = F.relu(x)
                if self.dropout:
                    x = F.dropout(x, p=0.5, training=self.training)
        return F.log_softmax(x, dim=1) if self.log_softmax else x


class Decoder(nn.Module):
    """models/models.py:653-702 (no dropout is applied, as in the reference)."""

    def __init__(self, dim_in, dim_hidden, dim_out, num_layer=2, use_norm=False, dropout=0.5, act_fn="relu", norm_mode="PN",
                 norm_scale=1.):
        super().__init__()
        self.layers = nn.ModuleList()
        self.use_norm, self.dropout, self.num_layer = use_norm, dropout, num_layer
        if num_layer == 1:
            self.layers.append(Linear(dim_in, dim_out, bias=True))
        else:
            self.layers.append(Linear(dim_in, dim_hidden, bias=True))
            for _ in range(num_layer - 2):
                self.layers.append(Linear(dim_hidden, dim_hidden, bias=True))
            self.layers.append(Linear(dim_hidden, dim_out, bias=True))
        if use_norm:
            self.pair_norm = PairNorm(norm_mode, norm_scale)
        self.act_fn = _act(act_fn)
        self.reset_parameters()

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()

    def forward(self, z):
        x = z
        for idx in range(self.num_layer - 1):
            x = self.layers[idx](x)
            if self.use_norm:
                x = self.pair_norm(x)
            x = self.act_fn(x)
        return self.layers[-1](x)


class Discriminator(nn.Module):
    """models/models.py:753-813 (no dropout is applied, as in the reference)."""

    def __init__(self, dim_in, dim_hidden, num_layer=2, use_bn=False, use_pair_norm=False, dropout=0.5, act_fn="leakyrelu",
                 sigmoid_output=True, norm_mode="PN", norm_scale=1.):
        super().__init__()
        self.layers = nn.ModuleList()
        self.use_bn, self.dropout, self.num_layer, self.sigmoid_output = use_bn, dropout, num_layer, sigmoid_output
        if num_layer == 1:
            self.layers.append(Linear(dim_in, 1, bias=True))
        else:
            self.layers.append(Linear(dim_in, dim_hidden, bias=True))
            for _ in range(num_layer - 2):
                self.layers.append(Linear(dim_hidden, dim_hidden, bias=True))
            self.layers.append(Linear(dim_hidden, 1, bias=True))
        self.use_pair_norm = use_pair_norm
        if use_pair_norm:
            self.pair_norm = PairNorm(mode=norm_mode, scale=norm_scale)
        if use_bn:
            self.bns = nn.ModuleList([nn.BatchNorm1d(dim_hidden) for _ in range(num_layer - 1)])
        self.act_fn = _act(act_fn)
        self.reset_parameters()

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()
        if self.use_bn:
            for bn in self.bns:
                bn.reset_parameters()

    def forward(self, z):
        x = z
        for idx in range(self.num_layer - 1):
            x = self.layers[idx](x)
            if self.use_bn:
                x = self.bns[idx](x)
            elif self.use_pair_norm:
                x = self.pair_norm(x)
            x = self.act_fn(x)
        logits = self.layers[-1](x)
        return torch.sigmoid(logits) if self.sigmoid_output else logits


# ---- the pair part of Similar_v2(mode='mlp') ------------------------------------------------------------------------------------
def _bn1_half(z, c, P, weight, bias, bn, cols, eps, momentum):
    """BN1 in train mode on one half of the concatenation [z1[idx1] || z2[idx2]]: its batch statistics are count-weighted per-node
    sums (c[n] = pairs that reference node n).  Updates bn's running statistics on `cols`; -> (x_hat fp32, BN output, rstd)."""
    zd = z.detach().double()
    cw = c[:, None]
    mu = (zd * cw).sum(0) / P                              # fp64 reductions, not fp64 GEMVs (the library's are slow)
    var = ((zd - mu).square() * cw).sum(0) / P
    with torch.no_grad():
        bn.running_mean[cols].mul_(1.0 - momentum).add_(mu.float(), alpha=momentum)
        bn.running_var[cols].mul_(1.0 - momentum).add_((var * (P / (P - 1.0))).float(), alpha=momentum)
    rstd = (var + eps).rsqrt()
    xh = ((zd - mu) * rstd).float()
    return xh, xh * weight.detach()[cols] + bias.detach()[cols], rstd.float()


def _bn1_half_bwd(D, xh, rstd, c, gamma, P):
    """BN1's train-mode backward of one half in per-node form: D = S W1_half ([N, H]) ->
    (dz [N, H], dgamma, dbeta)."""
    Dd = D.double()
    s_d = Dd.sum(0)
    s_dx = (xh.double() * Dd).sum(0)
    dz = (gamma.double() * rstd.double()) * (Dd - c[:, None] * (s_d / P + xh.double() * (s_dx / P)))
    return dz.float(), s_dx.float(), s_d.float()


class _PairMlpFn(torch.autograd.Function):
    """(p, mean BCE, [TP, FP, FN]) of Similar_v2(mode='mlp') in train mode on the pairs (z1[idx1], z2[idx2]) with labels y (uint8).
    Updates the running statistics of both BatchNorms and their num_batches_tracked like one nn.BatchNorm1d call each.
    z1 may be z2 (autograd adds the two halves' gradients).  p and the counts are not differentiable."""

    @staticmethod
    def forward(ctx, z1, z2, idx1, idx2, y, g1, be1, W1, b1, g2, be2, w2, b2, bn1, bn2):
        P = int(idx1.shape[0])
        if P <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{P}, {2 * z1.shape[1]}]")
        H = int(z1.shape[1])
        N1, N2 = int(z1.shape[0]), int(z2.shape[0])
        eps, mom = float(bn1.eps), float(bn1.momentum)
        rp1, pm1 = ops.pair_csr(idx1, idx2, N1, N2)
        rp2, pm2 = ops.pair_csr(idx2, idx1, N2, N1)
        c1 = (rp1[1:] - rp1[:-1]).double()
        c2 = (rp2[1:] - rp2[:-1]).double()
        ha, hb = slice(0, H), slice(H, 2 * H)
        xh1, a_in, r1 = _bn1_half(z1, c1, P, g1, be1, bn1, ha, eps, mom)
        xh2, b_in, r2 = _bn1_half(z2, c2, P, g1, be1, bn1, hb, eps, mom)
        W1d = W1.detach()
        A = (a_in @ W1d[:, :H].t()).contiguous()
        B = torch.addmm(b1.detach(), b_in, W1d[:, H:].t()).contiguous()
        w2v, g2d, be2d, b2d = w2.detach().reshape(-1).contiguous(), g2.detach().contiguous(), be2.detach().contiguous(), b2.detach()
        stats = ops.pair_mlp_stats(A, B, idx1, idx2, bn2.momentum, bn2.running_mean, bn2.running_var)
        p, dl, sums = ops.pair_mlp_loss(A, B, idx1, idx2, y, stats, g2d, be2d, w2v, b2d.reshape(-1).contiguous(), float(bn2.eps))
        with torch.no_grad():
            bn1.num_batches_tracked.add_(1)
            bn2.num_batches_tracked.add_(1)
        loss = (sums[3 * U + 1] / P).to(torch.float32)
        counts = sums[3 * U + 2:3 * U + 5]
        ctx.save_for_backward(A, B, idx1, idx2, dl, stats, sums, xh1, xh2, a_in, b_in, r1, r2, c1, c2, rp1, pm1, rp2, pm2, g1, W1d,
                              g2d, be2d, w2v)
        ctx.P, ctx.H, ctx.eps2 = P, H, float(bn2.eps)
        ctx.shapes = (w2.shape, b2.shape)
        ctx.mark_non_differentiable(p, counts)
        return p, loss, counts

    @staticmethod
    def backward(ctx, gp, gloss, gcounts):
        (A, B, idx1, idx2, dl, stats, sums, xh1, xh2, a_in, b_in, r1, r2, c1, c2, rp1, pm1, rp2, pm2, g1, W1, g2, be2,
         w2v) = ctx.saved_tensors
        P, H = ctx.P, ctx.H
        S1 = ops.pair_mlp_segsum(A, B, rp1, pm1, idx2, dl, stats, sums, g2, be2, w2v, ctx.eps2)
        S2 = ops.pair_mlp_segsum(B, A, rp2, pm2, idx1, dl, stats, sums, g2, be2, w2v, ctx.eps2)
        g = gloss.to(torch.float32)
        dW1 = torch.cat((S1.t() @ a_in, S2.t() @ b_in), dim=1)
        db1 = S1.double().sum(0).float()
        dz1, dg1a, db1a = _bn1_half_bwd(S1 @ W1[:, :H], xh1, r1, c1, g1.detach()[:H], P)
        dz2, dg1b, db1b = _bn1_half_bwd(S2 @ W1[:, H:], xh2, r2, c2, g1.detach()[H:], P)
        f = lambda t: (t.float() * g)                                                       # noqa: E731
        dw2 = f(sums[2 * U:3 * U]).reshape(ctx.shapes[0])
        db2 = f(sums[3 * U:3 * U + 1]).reshape(ctx.shapes[1])
        return (f(dz1), f(dz2), None, None, None, f(torch.cat((dg1a, dg1b))), f(torch.cat((db1a, db1b))), f(dW1), f(db1),
                f(sums[U:2 * U]), f(sums[:U]), dw2, db2, None, None)


class Similar_v2(nn.Module):
    """models/models.py:895-997, mode='mlp'.  Keys lin_self.{0,1,2,4}.* and lin_clf.* as in the reference.  `train_dropout=False`
    switches off the 0.6 dropout before lin_clf (tests)."""

    def __init__(self, in_channels, num_clf_classes, dropout=0.6, use_clf=True, mode="mlp", train_dropout=True):
        super().__init__()
        if mode != "mlp":
            _unsupported(f"Similar_v2(mode={mode!r})")
        self.mode = mode
        self.lin_self = nn.Sequential(
            nn.BatchNorm1d(in_channels * 2),
            Linear(in_channels * 2, U, bias=True, weight_initializer="glorot"),
            nn.BatchNorm1d(U),
            nn.ReLU(),
            Linear(U, 1, bias=True, weight_initializer="glorot"),
        )
        self.use_clf = use_clf
        if use_clf:
            self.lin_clf = Linear(in_channels, num_clf_classes, bias=True, weight_initializer="glorot")
        self.dropout, self.train_dropout = dropout, train_dropout
        self.reset_parameters()

    def reset_parameters(self):
        if self.use_clf:
            self.lin_clf.reset_parameters()
        for m in self.lin_self:
            if isinstance(m, nn.Linear):          # the reference's test: its PyG Linear layers are not nn.Linear, so none is re-drawn
                m.reset_parameters()

    def classify(self, z):
        """log_softmax(lin_clf(dropout(relu(z)))) (:936-940)"""
        h = F.relu(z)
        if self.train_dropout:
            h = F.dropout(h, p=self.dropout, training=self.training)
        return F.log_softmax(self.lin_clf(h), dim=-1)

    def pair_bce(self, z1, z2, idx1, idx2, y_pair):
        """Train mode: (p [P], F.binary_cross_entropy(p, y) as the reference computes it after `similarity`, [TP, FP, FN] at
        p > 0.5) through the HIP pair passes; one BN call each (running statistics, num_batches_tracked).  Eval mode: the
        running-statistics scores, loss None."""
        idx1, idx2 = idx1.contiguous(), idx2.contiguous()
        y = y_pair.to(torch.uint8).reshape(-1).contiguous()
        if not self.training:
            p, counts = self.pair_scores(z1, z2, idx1, idx2, y)
            return p, None, counts
        bn1, l1, bn2, _, l2 = self.lin_self
        return _PairMlpFn.apply(z1, z2, idx1, idx2, y, bn1.weight, bn1.bias, l1.weight, l1.bias, bn2.weight, bn2.bias, l2.weight,
                                l2.bias, bn1, bn2)

    def _eval_tables(self, z1, z2):
        """The eval-mode separable form (running statistics): u = A[i] + B[j] per pair, then BN2 as the per-column affine
        (scale2, shift2) -> (A [n1, 128], B [n2, 128], scale2, shift2, w2 [128], b2 [1])."""
        bn1, l1, bn2, _, l2 = self.lin_self
        H = z1.shape[1]
        s1 = bn1.weight / torch.sqrt(bn1.running_var + bn1.eps)
        t1 = bn1.bias - bn1.running_mean * s1
        A = F.linear(z1 * s1[:H] + t1[:H], l1.weight[:, :H]).contiguous()
        B = F.linear(z2 * s1[H:] + t1[H:], l1.weight[:, H:], l1.bias).contiguous()
        s2 = (bn2.weight / torch.sqrt(bn2.running_var + bn2.eps)).contiguous()
        t2 = (bn2.bias - bn2.running_mean * s2).contiguous()
        return A, B, s2, t2, l2.weight.reshape(-1).contiguous(), l2.bias.reshape(-1).contiguous()

    def pair_scores(self, z1, z2, idx1, idx2, y_pair=None):
        """Eval-mode (running statistics) sigmoid scores of the pairs and, with labels, [TP, FP, FN] -- no autograd."""
        with torch.no_grad():
            A, B, s2, t2, w2, b2 = self._eval_tables(z1, z2)
            y = None if y_pair is None else y_pair.to(torch.uint8).reshape(-1).contiguous()
            return ops.pair_mlp_eval(A, B, idx1.contiguous(), idx2.contiguous(), s2, t2, w2, b2, y)

    def pair_counts(self, z1, z2, rows1, rows2, lab1, lab2):
        """Eval-mode int64 [TP, FP, FN, TN] of (score > 0.5) against lab1[rows1[i]] == lab2[rows2[j]] over the whole product
        rows1 x rows2 (int64 row ids into z1 / z2; lab1 / lab2 per node) -- no pair list, no autograd."""
        with torch.no_grad():
            A, B, s2, t2, w2, b2 = self._eval_tables(z1, z2)
            return ops.pair_mlp_count(A, B, rows1, rows2, lab1.long().contiguous(), lab2.long().contiguous(), s2, t2, w2, b2)

    def _scores(self, z1, z2, idx1, idx2):
        if self.training:
            raise RuntimeError("Similar_v2: train-mode pair scores go through pair_bce (the loss is fused into the pair passes)")
        return self.pair_scores(z1, z2, idx1, idx2)[0]

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


class Source_Learner_v2(nn.Module):
    """models/models.py:999-1052"""

    def __init__(self, data, dim_hidden=64, norm_mode="None", norm_scale=1, use_clf=True, use_norm=True, backbone="mlp", mode="mlp",
                 dropout=True):
        super().__init__()
        if backbone != "mlp":
            _unsupported(f"backbone={backbone!r}")
        self.dim_in, self.num_classes, self.dim_hidden = data.num_features, int(data.y.max().item()) + 1, dim_hidden
        self.backbone = MLP(self.dim_in, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True, use_norm=use_norm,
                            norm_mode=norm_mode, norm_scale=norm_scale, log_softmax=False, dropout=dropout)
        self.sim_net = Similar_v2(dim_hidden, num_clf_classes=self.num_classes, dropout=0.6, use_clf=use_clf, mode=mode,
                                  train_dropout=dropout)
        self.reset_parameters()

    def reset_parameters(self):
        self.backbone.reset_parameters()
        self.sim_net.reset_parameters()

    def forward(self, data, idx1, idx2, return_representation=False):
        h = self.backbone(data.x, data.edge_index)
        probs_pair, logits_clf = self.sim_net(h, idx1, idx2)
        return (probs_pair, logits_clf, h) if return_representation else (probs_pair, logits_clf)


class Target_Learner_AE_v2(nn.Module):
    """models/models.py:1055-1107"""

    def __init__(self, data, dim_eq_trans=128, dim_hidden=64, use_norm=True, norm_mode="None", norm_scale=1, backbone="mlp",
                 dropout=True):
        super().__init__()
        if backbone != "mlp":
            _unsupported(f"backbone={backbone!r}")
        self.dim_in, self.dim_eq_trans = data.num_features, dim_eq_trans
        self.num_classes, self.dim_hidden = int(data.y.max().item()) + 1, dim_hidden
        self.equavilent_trans_layer = nn.Sequential(Linear(self.dim_in, dim_eq_trans, bias=True),
                                                    PairNorm(mode=norm_mode, scale=norm_scale), nn.Tanh())
        self.use_norm = use_norm
        self.encoder = MLP(dim_eq_trans, dim_hidden, dim_hidden=dim_hidden, layer_num=2, root_weight=True, use_norm=use_norm,
                           norm_mode=norm_mode, norm_scale=norm_scale, log_softmax=False, dropout=dropout)
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


class Adversarial_Learner_v2(nn.Module):
    """models/models.py:1110-1142.  Only sim_mode='mlp' / backbone='mlp'; `dropout=False` switches every dropout off (tests)."""

    def __init__(self, data_src, data_tar, dim_hidden=64, num_layer=2, source_clf=True, use_norm=True, norm_mode="PN", norm_scale=1.,
                 backbone="mlp", sim_mode="mlp", dropout=True):
        super().__init__()
        self.num_layer, self.source_clf = num_layer, source_clf
        self.source_learner = Source_Learner_v2(data_src, dim_hidden=dim_hidden, norm_mode=norm_mode, norm_scale=norm_scale,
                                                use_clf=source_clf, use_norm=use_norm, backbone=backbone, mode=sim_mode, dropout=dropout)
        self.target_learner = Target_Learner_AE_v2(data_tar, dim_eq_trans=128, dim_hidden=dim_hidden, norm_mode=norm_mode,
                                                   use_norm=use_norm, norm_scale=norm_scale, backbone=backbone, dropout=dropout)
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


# ---- samplers (models/models.py:284-512) ----------------------------------------------------------------------------------------
def pair_enumeration(x1, x2):
    """models/models.py:265-282: [x1 tiled n2 times || each x2 row repeated n1 times]"""
    assert x1.ndimension() == 2 and x2.ndimension() == 2, "Input dimension must be 2"
    x1_ = x1.repeat(x2.size(0), 1)
    x2_ = x2.repeat(1, x1.size(0)).view(-1, x1.size(1))
    return torch.cat((x1_, x2_), dim=1)


def _buckets(y, mask, num_classes):
    """class -> int64 numpy array of the masked node ids of that class, ascending (the reference's per-class boolean selection)"""
    y, mask = y.detach().cpu().long(), mask.detach().cpu().bool()
    ids = torch.nonzero(mask).reshape(-1)
    lab = y[ids]
    order = torch.sort(lab, stable=True).indices
    ids, lab = ids[order].numpy(), lab[order].numpy()
    bounds = np.searchsorted(lab, np.arange(num_classes + 1))
    return [ids[bounds[c]:bounds[c + 1]] for c in range(num_classes)]


def _split_mask(data, mode):
    if mode == "all":
        _unsupported("Pair enumerator mode 'all'")
    if mode not in ("train", "val", "test"):
        raise NotImplementedError("Not Implemented Mode:{}".format(mode))
    return getattr(data, mode + "_mask")


def _choose_classes(num_classes, max_class_num):
    if num_classes > max_class_num:
        return np.random.choice(np.arange(num_classes), replace=False, size=max_class_num)
    return np.arange(num_classes).astype(np.int8)


def _balanced(b1, b2, num_classes, max_class_num, sample_size, shuffle):
    """balanced_sampling (:324-357 / :461-494): the same np.random calls in the same order as the reference"""
    if shuffle:
        _unsupported("shuffle=True")
    sel = _choose_classes(num_classes, max_class_num)
    same = int(0.5 * sample_size / max_class_num)
    diff = int(0.5 * sample_size / (max_class_num * (max_class_num - 1)))
    s1, s2 = [], []
    for l1 in sel:
        for l2 in sel:
            n = same if l1 == l2 else diff
            s1.append(np.random.choice(b1[int(l1)], size=n))
            s2.append(np.random.choice(b2[int(l2)], size=n))
    return torch.from_numpy(np.concatenate(s1).astype(np.int64)), torch.from_numpy(np.concatenate(s2).astype(np.int64))


def _sampling(b1, b2, num_classes, max_class_num, sample_size, shuffle):
    """sampling (:358-375 / :495-512): per selected class sqrt(sample_size) / max_class_num draws per side, then the Cartesian
    enumeration"""
    if shuffle:
        _unsupported("shuffle=True")
    sel = _choose_classes(num_classes, max_class_num)
    per = int(np.sqrt(sample_size) / max_class_num)
    s1, s2 = [], []
    for lbl in sel:
        s1.append(np.random.choice(b1[int(lbl)], size=per))
        s2.append(np.random.choice(b2[int(lbl)], size=per))
    s1 = torch.from_numpy(np.concatenate(s1).astype(np.int64))
    s2 = torch.from_numpy(np.concatenate(s2).astype(np.int64))
    return s1.repeat(s2.shape[0]), s2.repeat_interleave(s1.shape[0])


class Pair_Enumerator:
    """models/models.py:428-512: label-balanced pair lists inside one domain (int64 CPU index tensors)."""

    def __init__(self, data, mode="train"):
        self.num_classes = int(data.y.max().item()) + 1
        self.mode = mode
        self.class_bucket = _buckets(data.y, _split_mask(data, mode), self.num_classes)

    def balanced_sampling(self, max_class_num=2, sample_size=10000, shuffle=True):
        return _balanced(self.class_bucket, self.class_bucket, self.num_classes, max_class_num, sample_size, shuffle)

    def sampling(self, max_class_num=2, sample_size=10000, shuffle=True):
        return _sampling(self.class_bucket, self.class_bucket, self.num_classes, max_class_num, sample_size, shuffle)


class Pair_Enumerator_cross:
    """models/models.py:284-375: (source, target) pair lists."""

    def __init__(self, data_src, data_tar, mode="train"):
        self.num_classes = int(data_src.y.max().item()) + 1
        self.mode = mode
        self.class_bucket_src = _buckets(data_src.y, _split_mask(data_src, mode), self.num_classes)
        self.class_bucket_tar = _buckets(data_tar.y, _split_mask(data_tar, mode), self.num_classes)

    def balanced_sampling(self, max_class_num=2, sample_size=10000, shuffle=True):
        return _balanced(self.class_bucket_src, self.class_bucket_tar, self.num_classes, max_class_num, sample_size, shuffle)

    def sampling(self, max_class_num=2, sample_size=10000, shuffle=True):
        return _sampling(self.class_bucket_src, self.class_bucket_tar, self.num_classes, max_class_num, sample_size, shuffle)


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def f1_from_counts(tp, fp, fn):
    """binary f1 (sklearn's f1_score(average='binary'), zero_division -> 0)"""
    tp, fp, fn = float(tp), float(fp), float(fn)
    den = 2.0 * tp + fp + fn
    return 0.0 if den == 0.0 else 2.0 * tp / den


def macro_f1(y_true, y_pred):
    """sklearn's f1_score(average='macro'): mean over the labels present in y_true or y_pred"""
    y_true, y_pred = y_true.long().reshape(-1), y_pred.long().reshape(-1)
    if y_true.numel() == 0:
        return 0.0
    labels = torch.unique(torch.cat((y_true, y_pred)))
    n = int(labels.max().item()) + 1
    tp = torch.bincount(y_true[y_true == y_pred], minlength=n).double()
    t = torch.bincount(y_true, minlength=n).double()
    p = torch.bincount(y_pred, minlength=n).double()
    f1 = 2.0 * tp / (t + p)
    return float(f1[labels].mean().item())


def _f1(counts):
    tp, fp, fn = counts.tolist()
    return f1_from_counts(tp, fp, fn)


# ---- training / evaluation (scripts.py) ---------------------------------------------------------------------------------------------
def _dev_idx(t, dev):
    return t.to(dev, non_blocking=True).long().contiguous()


def train_adv_few_shot(epoch, data_src, data_tar, model, optimizer_src_tar, optimizer_D, metric="f1", pair_enumerator_src_train=None,
                       pair_enumerator_tar_train=None, pair_enumerator_cross_train=None, max_class_num=2, sample_size=10000,
                       use_clf=False, verbose=False):
    """scripts.py:28-94: one step of the similarity learner + auto-encoder, then one discriminator step.  -> (loss_sim,
    (f1_src, f1_tar, f1_cross), loss_d, loss_ae, loss_g, loss_recons) like the reference."""
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
    _, loss_src, cnt_src = sim.pair_bce(h_src, h_src, i1s, i2s, data_src.y[i1s] == data_src.y[i2s])
    i1t, i2t = (_dev_idx(t, dev) for t in pair_enumerator_tar_train.sampling(max_class_num=max_class_num, sample_size=sample_size,
                                                                             shuffle=False))
    h0_tar, h_tar, recons = model.target_learner(data_tar)
    lp_tar = sim.classify(h_tar) if sim.use_clf else None
    _, loss_tar, cnt_tar = sim.pair_bce(h_tar, h_tar, i1t, i2t, data_tar.y[i1t] == data_tar.y[i2t])
    i1c, i2c = (_dev_idx(t, dev) for t in pair_enumerator_cross_train.sampling(max_class_num=max_class_num, sample_size=sample_size,
                                                                               shuffle=False))
    _, loss_cross, cnt_cross = sim.pair_bce(h_src, h_tar, i1c, i2c, data_src.y[i1c] == data_tar.y[i2c])
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
    eval_pair = (_f1(cnt_src), _f1(cnt_tar), _f1(cnt_cross))
    optimizer_D.zero_grad()
    real_loss = F.binary_cross_entropy(model.discriminator(h_src.detach()), torch.ones((h_src.shape[0], 1), device=dev))
    fake_loss = F.binary_cross_entropy(model.discriminator(h_tar.detach()), torch.zeros((h_tar.shape[0], 1), device=dev))
    loss_d = (real_loss + fake_loss) / 2
    loss_d.backward()
    optimizer_D.step()
    return loss_sim.item(), eval_pair, loss_d.item(), loss_ae.item(), loss_g.item(), loss_recons.item()


def _check_eval(metric, eval_mode, conf_lower_bound):
    if eval_mode not in ("sampling", "all"):
        raise NotImplementedError("Not Implemented Eval Mode:{}".format(eval_mode))
    if metric == "auc":
        _unsupported(f"metric={metric!r}")
    if metric not in ("f1", "acc"):
        raise NotImplementedError("NotImplemented Metric:{}".format(metric))
    if conf_lower_bound is not None:
        _unsupported("conf_lower_bound")


def _rows(mask):
    return torch.nonzero(mask).reshape(-1).contiguous()


def _all_masks_within(data, split):
    """eval_mode='all' inside one domain (scripts.py:374-375): (mask of rows1 = every labelled node, mask of rows2 = the split)"""
    return data.train_mask | data.val_mask | data.test_mask, data.val_mask if split == "val" else data.test_mask


def _all_masks_cross(data_src, data_tar, split):
    """eval_mode='all' across the domains (scripts.py:317-318, :326-327): the two products ((source mask, target mask), ...)"""
    if split == "val":
        return ((data_src.val_mask, data_tar.train_mask | data_tar.val_mask),
                (data_src.train_mask, data_tar.val_mask))
    return ((data_src.test_mask, data_tar.train_mask | data_tar.test_mask | data_tar.val_mask),
            (data_src.train_mask | data_src.val_mask, data_tar.test_mask))


def _pair_score(tp, fp, fn, tn, metric):
    """f1_score(average='binary') / accuracy_score of the pair predictions from their confusion counts"""
    if metric == "f1":
        return f1_from_counts(tp, fp, fn)
    total = float(tp) + float(fp) + float(fn) + float(tn)
    return 0.0 if total == 0.0 else (float(tp) + float(tn)) / total


def _list_score(counts, P, metric):
    """the list pass counts [TP, FP, FN] of P pairs; TN is the rest"""
    tp, fp, fn = counts.tolist()
    return _pair_score(tp, fp, fn, P - tp - fp - fn, metric)


def _clf_score(model, data, z, mask_2, metric):
    """macro f1 (metric 'f1') or accuracy (metric 'acc', scripts.py:411-413) of the node classifier on the split"""
    y2 = data.y[mask_2]
    pred = model.source_learner.sim_net.classify(z)[mask_2].max(1)[1] if model.source_clf else torch.zeros_like(y2)
    if metric == "acc":
        return 0.0 if y2.numel() == 0 else float((pred == y2).double().mean().item())
    return macro_f1(y2, pred)


def _encode(model, data, domain):
    if domain == "source":
        return model.source_learner.backbone(data.x, data.edge_index)
    return model.target_learner.encode(data)[0]


def _within_all(data, model, split, z, metric):
    mask_1, mask_2 = _all_masks_within(data, split)
    tp, fp, fn, tn = model.source_learner.sim_net.pair_counts(z, z, _rows(mask_1), _rows(mask_2), data.y, data.y).tolist()
    return _pair_score(tp, fp, fn, tn, metric), _clf_score(model, data, z, mask_2, metric)


def _cross_all_counts(data_src, data_tar, model, split, z_src, z_tar):
    """int64 [TP, FP, FN, TN] over the two products of eval_cross_domain_v2's concatenated 'all' list"""
    sim = model.source_learner.sim_net
    (m_s1, m_t1), (m_s2, m_t2) = _all_masks_cross(data_src, data_tar, split)
    return (sim.pair_counts(z_src, z_tar, _rows(m_s1), _rows(m_t1), data_src.y, data_tar.y)
            + sim.pair_counts(z_src, z_tar, _rows(m_s2), _rows(m_t2), data_src.y, data_tar.y))


def eval_within_domain_v2(data, model, pair_enumerator=None, split="test", domain="target", conf_lower_bound=None, metric="f1",
                          eval_mode="sampling"):
    """scripts.py:372-416 -> (pair score, classifier score on the split); metric 'f1' (binary f1 / macro f1) or 'acc'.
    eval_mode='sampling' scores a balanced list from `pair_enumerator`; 'all' counts every pair of (train | val | test) x split
    and does not use `pair_enumerator`."""
    _check_eval(metric, eval_mode, conf_lower_bound)
    if eval_mode == "all":
        with torch.no_grad():
            model.eval()
            return _within_all(data, model, split, _encode(model, data, domain), metric)
    mask_2 = data.val_mask if split == "val" else data.test_mask
    num_classes = int(data.y.max().item()) + 1
    dev = data.x.device
    idx1, idx2 = (_dev_idx(t, dev) for t in pair_enumerator.balanced_sampling(max_class_num=num_classes, sample_size=100000,
                                                                              shuffle=False))
    with torch.no_grad():
        model.eval()
        z = _encode(model, data, domain)
        _, counts = model.source_learner.sim_net.pair_scores(z, z, idx1, idx2, data.y[idx1] == data.y[idx2])
        score_clf = _clf_score(model, data, z, mask_2, metric)
    return _list_score(counts, int(idx1.shape[0]), metric), score_clf


def eval_cross_domain_v2(data_src, data_tar, model, pair_enumerator=None, split="test", conf_lower_bound=None, metric="f1",
                         eval_mode="sampling"):
    """scripts.py:315-367 -> pair score ('f1' or 'acc').  eval_mode='all' counts the reference's two products (source split x
    target, source train(+val) x target split) and does not use `pair_enumerator`."""
    _check_eval(metric, eval_mode, conf_lower_bound)
    if eval_mode == "all":
        with torch.no_grad():
            model.eval()
            z_src, z_tar = _encode(model, data_src, "source"), _encode(model, data_tar, "target")
            return _pair_score(*_cross_all_counts(data_src, data_tar, model, split, z_src, z_tar).tolist(), metric)
    num_classes = int(data_tar.y.max().item()) + 1
    dev = data_src.x.device
    idx1, idx2 = (_dev_idx(t, dev) for t in pair_enumerator.balanced_sampling(max_class_num=num_classes, sample_size=100000,
                                                                              shuffle=False))
    with torch.no_grad():
        model.eval()
        z_src, z_tar = _encode(model, data_src, "source"), _encode(model, data_tar, "target")
        _, counts = model.source_learner.sim_net.pair_scores(z_src, z_tar, idx1, idx2, data_src.y[idx1] == data_tar.y[idx2])
    return _list_score(counts, int(idx1.shape[0]), metric)


def eval_adv_v2(data_src, data_tar, model, split="test", metric="f1", enu_list=None, eval_mode="sampling"):
    """scripts.py:418-426 -> (pair_src, clf_src, pair_tar, clf_tar, pair_cross).  With eval_mode='all' each domain is encoded
    once for the three evaluations and `enu_list` is not used."""
    if eval_mode == "all":
        _check_eval(metric, eval_mode, None)
        with torch.no_grad():
            model.eval()
            z_src, z_tar = _encode(model, data_src, "source"), _encode(model, data_tar, "target")
            ps, cs = _within_all(data_src, model, split, z_src, metric)
            pt, ct = _within_all(data_tar, model, split, z_tar, metric)
            pc = _pair_score(*_cross_all_counts(data_src, data_tar, model, split, z_src, z_tar).tolist(), metric)
        return ps, cs, pt, ct, pc
    enu_src, enu_tar, enu_cross = enu_list
    ps, cs = eval_within_domain_v2(data_src, model, split=split, domain="source", metric=metric, pair_enumerator=enu_src,
                                   eval_mode=eval_mode)
    pt, ct = eval_within_domain_v2(data_tar, model, split=split, domain="target", metric=metric, pair_enumerator=enu_tar,
                                   eval_mode=eval_mode)
    pc = eval_cross_domain_v2(data_src, data_tar, model, split=split, metric=metric, pair_enumerator=enu_cross, eval_mode=eval_mode)
    return ps, cs, pt, ct, pc


def _to(data, dev):
    d = copy.copy(data)
    for k, v in list(vars(d).items()):
        if torch.is_tensor(v):
            setattr(d, k, v.to(dev))
    return d


def make_optimizers(model):
    """scripts.py:470-479"""
    lr, b1, b2 = 1e-3, 0.5, 0.999
    opt = torch.optim.Adam([
        {"params": model.source_learner.parameters(), "lr": 1e-2, "weight_decay": 5e-3},
        {"params": model.target_learner.parameters(), "lr": lr, "betas": (b1, b2)},
    ])
    return opt, torch.optim.Adam(model.discriminator.parameters(), lr=lr, betas=(b1, b2))


def main_adv_v2(args, data_src, data_tar, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, metric="f1",
                use_clf=True, norm_mode="PN", norm_scale=1., eval_per_epoch=1, start_eval_epoch=0, max_class_num=5, sample_size=40000,
                sim_mode="mlp", backbone="mlp", use_norm=True, eval_mode="sampling", device=None, ckpt_dir="../ckpt", dropout=True,
                verbose=True):
    """scripts.py:432-555.  Trains `repeat` runs (model init seed = run - 1, or `seed`), evaluating from `start_eval_epoch` every
    `eval_per_epoch` epochs and keeping the epoch with the best cross-domain validation f1 (:524).  With `save`, writes
    {ckpt_dir}/model_AdvLearner_{args.dataset_name}_best.ckpt at every improvement and _final.ckpt after each run, in the
    reference's format (a state_dict).  -> (state_dict of the last run's best epoch (CPU tensors; None if no epoch was evaluated),
    best_acc as the reference leaves it)."""
    from .utils import set_random_seed
    assert device is not None
    if save:
        os.makedirs(ckpt_dir, exist_ok=True)
    data_src, data_tar = _to(data_src, device), _to(data_tar, device)
    final_acc = {"train": [], "val": [], "test": []}
    best_state = None
    for train_id in range(1, 1 + repeat):
        model_init_seed = train_id - 1 if seed is None else seed
        set_random_seed(model_init_seed)
        model = Adversarial_Learner_v2(data_src, data_tar, dim_hidden=hidden, num_layer=num_layer, use_norm=use_norm, source_clf=use_clf,
                                       norm_mode=norm_mode, norm_scale=norm_scale, sim_mode=sim_mode, backbone=backbone,
                                       dropout=dropout).to(device)
        optimizer_src_tar, optimizer_D = make_optimizers(model)
        best_acc = {"epoch": -1, "train": (0, 0, 0), "val": (0, 0, 0), "test": (0, 0, 0), "loss": 666}
        enu_train = (Pair_Enumerator(data_src, mode="train"), Pair_Enumerator(data_tar, mode="train"),
                     Pair_Enumerator_cross(data_src, data_tar, mode="train"))
        enu_val = (Pair_Enumerator(data_src, mode="val"), Pair_Enumerator(data_tar, mode="val"),
                   Pair_Enumerator_cross(data_src, data_tar, mode="val"))
        enu_test = (Pair_Enumerator(data_src, mode="test"), Pair_Enumerator(data_tar, mode="test"),
                    Pair_Enumerator_cross(data_src, data_tar, mode="test"))
        for epoch in range(1, 1 + num_epoch):
            loss_sim, eval_pair_train, loss_d, loss_ae, loss_g, loss_recons = train_adv_few_shot(
                epoch, data_src, data_tar, model, optimizer_src_tar, optimizer_D, metric=metric, pair_enumerator_src_train=enu_train[0],
                pair_enumerator_tar_train=enu_train[1], pair_enumerator_cross_train=enu_train[2], max_class_num=max_class_num,
                sample_size=sample_size, use_clf=use_clf)
            if verbose:
                print("[AE]Epoch: {:03d}, Loss_ae:{:.4f} | Loss_recons:{:.4f} | Loss_g:{:.4f} | Loss_d:{:.4f}".format(
                    epoch, loss_ae, loss_recons, loss_g, loss_d))
            if epoch >= start_eval_epoch and epoch % eval_per_epoch == 0:
                ps_v, cs_v, pt_v, ct_v, pc_v = eval_adv_v2(data_src, data_tar, model, split="val", metric=metric, enu_list=enu_val,
                                                           eval_mode=eval_mode)
                ps_t, cs_t, pt_t, ct_t, pc_t = eval_adv_v2(data_src, data_tar, model, split="test", metric=metric, enu_list=enu_test,
                                                           eval_mode=eval_mode)
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
