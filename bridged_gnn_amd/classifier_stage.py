"""The classifier stage of KT-GNN (reference models/KTGNN.py:432-435: `clf_base(h)`, `clf_target(T(h))`, `clf_target(h)`,
`log_softmax`) -- everything the four drivers share about it: `KTGNN_no_complement.forward` (eval and training),
`dist.PartitionedKTGNN` and `dist_train.PartitionedTrainer`.

The three convs share the graph, so their six narrow tables are interleaved per node and ONE CSR walk serves all three:
  head 0 = clf_base(h), head 1 = clf_target(h), head 2 = clf_target(T(h)) ("target-hat");
  a table row = [base | target | target-hat] x pad4(C) floats; the forward's return order is (head 0, head 1, head 2).
The drivers keep what differs: where the domain sums come from, the halo exchange and the eval walk's launches.  Nothing here
syncs with the host except `composed_target_pack` (once per weight version).
"""
import os

import torch
import torch.nn.functional as F

from . import ops
from .ktgnn import _AggregateFn, _AggregateHeadsFn, _AggregateWideHeadsFn, _TransformPairFn, _pad_cols4, _plist


class ClassifierStage:
    """the stage of one `KTGNN_no_complement` (`model._stage`) and its host-side caches"""

    def __init__(self, model):
        base = model.clf_base
        self.model, self.convs = model, (base, model.clf_target, model.clf_target)         # head order
        self.C, self.ld, self.slope = base.out_channels, ops.pad4(base.out_channels), base.negative_slope
        self.plain = not (base.root_weight or base.normalize)        # the only classifier convs the shared walks cover
        self.fused_log_softmax = ops.heads_log_softmax_supported(3, self.C)      # KTGNN.py:435 inside the eval walk's epilogue
        self.drop_caches()

    def drop_caches(self):
        self._a3_key = self._tf_key = self._tf_pack = None

    # ---- heads -------------------------------------------------------------------------------------------------------
    def views(self, t2s, s2t):
        """(h_t2s, h_s2t) column views of head j = 0, 1, 2 in two interleaved [rows, 3 * pad4(C)] tables"""
        ld = self.ld
        return [(t2s[:, j * ld:(j + 1) * ld], s2t[:, j * ld:(j + 1) * ld]) for j in range(3)]

    # ---- 32-byte rows (C <= 2): [h0c0 h0c1 h1c0 h1c1 | h2c0 h2c1 0 0] per node and table -----------------------------------------
    def rows32_eligible(self, dtype=torch.float32, training=False):
        """the host half of the layout decision: a plain stage of at most two classes, fp32, the eval forward"""
        return self.plain and self.C <= 2 and dtype == torch.float32 and not training

    @staticmethod
    def rows32_views(t2s, s2t):
        """(h_t2s, h_s2t) column views of head j = 0, 1, 2 in two [rows, 8] tables; head 2's view takes the padding along"""
        return [(t2s[:, 0:2], s2t[:, 0:2]), (t2s[:, 2:4], s2t[:, 2:4]), (t2s[:, 4:8], s2t[:, 4:8])]

    @staticmethod
    def rows32_pack(tab):
        """[rows, 3 * 4] padded table (at most two real columns per head) -> [rows, 8]"""
        t = tab.view(tab.shape[0], 3, 4)
        return torch.cat((t[:, 0, :2], t[:, 1, :2], t[:, 2, :]), dim=1).contiguous()

    @staticmethod
    def rows32_unpack(tab8):
        """[rows, 8] -> the padded [rows, 3 * 4] table with the same values, zeros in the padding"""
        out = tab8.new_zeros(tab8.shape[0], 3, 4)
        out[:, 0, :2], out[:, 1, :2], out[:, 2, :] = tab8[:, 0:2], tab8[:, 2:4], tab8[:, 4:8]
        return out.view(tab8.shape[0], 12)

    def eval_tables_rows32(self, x, mask_u8, sums_h, csr, arena):
        """the two tables of the eval forward as 32-byte rows, filled -> (t2s, s2t), or None where the stage, the one-pass
        producer or the walk's plan (one window, no hub rows, BGNN_HEADS_ROWS32) does not take them: the caller then builds
        the padded tables.  Decided before anything is written -- no other kernel reads this layout."""
        if not self.rows32_eligible(x.dtype) or x.stride(1) != 1:
            return None
        ops_a = self._one_pass_operands(x, sums_h)
        if ops_a is None:
            return None
        both = torch.empty(2, x.shape[0], 8, dtype=torch.float32, device=x.device)       # one allocation: one window
        t2s, s2t = both[0], both[1]
        if not ops.heads_rows32_plan(t2s, s2t, csr, self.C, self.slope, row_end=x.shape[0]):
            return None
        a = self.one_pass(x, mask_u8, sums_h, None, arena, rows32=(t2s, s2t), operands=ops_a)
        self.target_stage_b(a, mask_u8, self.rows32_views(t2s, s2t)[2], rows32=True)
        return t2s, s2t

    def attention(self, autograd=False):
        """(a_t2s, a_s2t) of the three heads as [3, C]: stacked under autograd for training, else detached and re-packed only when
        a weight changes"""
        if autograd:
            return (torch.stack([c.a_f_t2s.weight.reshape(-1) for c in self.convs]),
                    torch.stack([c.a_f_s2t.weight.reshape(-1) for c in self.convs]))
        key = (self.convs[0]._versions(), self.convs[1]._versions())
        if self._a3_key != key:
            self._a3 = (torch.stack([c.a_f_t2s.weight.detach().reshape(-1) for c in self.convs]).contiguous(),
                        torch.stack([c.a_f_s2t.weight.detach().reshape(-1) for c in self.convs]).contiguous())
            self._a3_key = key
        return self._a3

    def finish(self, out3):
        """the eval walk's [n, 3 * pad4(C)] output -> (logp_base, logp_target, logp_target_hat)"""
        logp = out3.view(out3.shape[0], 3, self.ld)[:, :, :self.C]
        if not self.fused_log_softmax:
            logp = F.log_softmax(logp, dim=2)                                    # one launch for the three heads
        return logp[:, 0], logp[:, 1], logp[:, 2]

    # ---- clf_transformer in eval mode ----------------------------------------------------------------------------------
    def fold_transformer(self):
        """eval BatchNorm of clf_transformer folded into its first Linear (re-folded when a parameter / buffer changes)."""
        l0, bn, _, l3 = self.model.clf_transformer
        key = tuple((p.data_ptr(), p._version) for p in _plist(self.model.clf_transformer)) + \
            (bn.running_mean._version, bn.running_var._version)
        if self._tf_key != key:
            s = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
            self._tf_w0 = (l0.weight.detach() * s[:, None]).float().contiguous()
            self._tf_w0t = self._tf_w0.t().contiguous()
            self._tf_b0 = (l0.bias.detach() * s + bn.bias.detach() - bn.running_mean * s).float().contiguous()
            self._tf_key = key
            self._tf_pack = None

    def transformer_hidden_eval(self, x, mask_u8=None, want_sums=False, sums_out=None):
        """h1 = relu(BN(Linear0(x))) of clf_transformer (eval; BN folded: BN(Wx+b) = (s*W)x + (s*b + t)).  Inside the
        envelope of `ops.linear` the W-stationary MFMA kernel applies bias + ReLU and, with `want_sums`, accumulates the
        per-domain column sums of h1 in its epilogue; other shapes go through the library GEMM."""
        self.fold_transformer()
        sums = None
        dout, din = self._tf_w0.shape
        if x.dtype == torch.float32 and x.stride(1) == 1 and ops.linear_supported(din, dout):
            if want_sums:
                sums = sums_out if sums_out is not None else torch.zeros(2 * dout + 2, dtype=torch.float64, device=x.device)
            h1 = ops.linear(x, self._tf_w0, self._tf_b0, relu=True, mask_u8=mask_u8 if want_sums else None, colsum=sums)
        elif hasattr(torch, "_addmm_activation"):
            h1 = torch._addmm_activation(self._tf_b0, x, self._tf_w0t, use_gelu=False)
        else:
            h1 = F.relu(torch.addmm(self._tf_b0, x, self._tf_w0t))
        return (h1, sums) if want_sums else h1

    def transformer_eval(self, x):
        """clf_transformer in eval mode (BatchNorm folded into the first Linear -- exact algebra:
        BN(Wx+b) = (s*W)x + (s*b + t))."""
        l3 = self.model.clf_transformer[3]
        return F.linear(self.transformer_hidden_eval(x), l3.weight, l3.bias)

    def composed_target_pack(self, din_pad):
        """clf_target evaluated on x' = h1.W3^T + b3 without materialising x' (the last Linear of clf_transformer is
        affine): W x' + b = (W W3) h1 + (W b3 + b); [x' || d'].g = h1.(W3^T g_x) + b3.g_x + d.(W3^T g_d) with d the
        domain-mean difference of h1 (d' = W3 d).  Packed once per weight version.  The gate constants b3.g_x stay 0-dim device
        tensors (`pack_transform_heads` copies them into its fp32 table: the same value as through a Python float), so a re-pack
        after a weight update does not wait for the device."""
        c, l3 = self.convs[1], self.model.clf_transformer[3]
        key = (din_pad, c._versions(), l3.weight._version, l3.bias._version, l3.weight.data_ptr())
        if self._tf_pack is None or self._tf_pack[0] != key:
            W3, b3 = l3.weight.detach(), l3.bias.detach()
            hd = c.head()
            din = W3.shape[0]

            def comp_gate(g):
                g = g.reshape(-1)
                return torch.cat((W3.t() @ g[:din], W3.t() @ g[din:])), (b3 * g[:din]).sum()
            g1, c1 = comp_gate(hd["g_s2t"])
            g2, c2 = comp_gate(hd["g_t2s"])
            head = {"W_s": hd["W_s"] @ W3, "W_t": hd["W_t"] @ W3,
                    "b_s": hd["W_s"] @ b3 + (hd["b_s"] if hd["b_s"] is not None else 0),
                    "b_t": hd["W_t"] @ b3 + (hd["b_t"] if hd["b_t"] is not None else 0),
                    "g_s2t": g1, "g_t2s": g2, "gate_const": (c1, c2)}
            self._tf_pack = (key, ops.pack_transform_heads([head], din_pad))
        return self._tf_pack[1]

    # ---- eval tables -----------------------------------------------------------------------------------------------------
    def _one_pass_operands(self, x, sums_h):
        """(pair, pack_t) of `one_pass`, or None outside the kernel's envelope"""
        if sums_h is None or x.dtype != torch.float32 or x.stride(1) != 1:
            return None
        self.fold_transformer()
        dout, din = self._tf_w0.shape
        if x.shape[1] != din or dout != 128:
            return None
        pack_t = self.composed_target_pack(ops.pad4(dout))
        pair = self.convs[0].packed(x.shape[1], self.convs[1])
        if not ops.classifier_stage_supported(x, pair, self._tf_w0, pack_t):
            return None
        return pair, pack_t

    def one_pass(self, x, mask_u8, sums_h, views, arena, rows32=None, operands=None):
        """heads 0 / 1 and stage A of head 2 from ONE pass over x (bgnn_classifier_stage_f32); needs the GLOBAL domain sums of x
        up front.  -> stage A's result (see `target_stage_a`), or None outside the kernel's envelope.  `rows32` = (t2s, s2t):
        heads 0 / 1 into tables of 32-byte rows instead of `views`."""
        if operands is None:
            operands = self._one_pass_operands(x, sums_h)
        if operands is None:
            return None
        pair, pack_t = operands
        n_s = 2 * ops.pad4(self._tf_w0.shape[0]) + 2
        sums_t = arena.take(n_s) if arena is not None else torch.zeros(n_s, dtype=torch.float64, device=x.device)
        outs = [views[0], views[1]] if rows32 is None else None
        raw = ops.classifier_stage(x, mask_u8, sums_h, pair, outs, self._tf_w0, self._tf_b0, sums_t, pack_t, relu=True, rows32=rows32)
        return raw, None, sums_t

    def pair_tables(self, x, mask_u8, sums_h, views):
        """heads 0 / 1: clf_base and clf_target on x from one pass over it; `sums_h` = the global domain sums of x"""
        self.convs[0].transform(x, mask_u8, sums=sums_h, partner=self.convs[1], out=[views[0], views[1]])

    def target_stage_a(self, x, mask_u8, sums_out=None):
        """head 2, clf_target on clf_transformer(x) (:433), the half that needs rank-local data only -> (raw, h1, sums of h1).
        Inside the envelope of the fused pair h1 = relu(BN(Linear0(x))) never reaches HBM: `raw` holds the per-row products and
        the zeroed float64 accumulator `sums_out` receives the local domain sums of h1.  Otherwise (or without an accumulator) h1
        is materialised, column-padded; T's last Linear is folded into the packed weights either way."""
        self.fold_transformer()
        dout, din = self._tf_w0.shape
        pack = self.composed_target_pack(ops.pad4(dout))
        if (sums_out is not None and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] == din
                and ops.linear_narrow_supported(din, dout, pack) and os.environ.get("BGNN_FUSED_TARGET", "1") != "0"):
            return ops.linear_narrow_transform(x, self._tf_w0, self._tf_b0, mask_u8, sums_out, pack, relu=True), None, sums_out
        h1, sums1 = self.transformer_hidden_eval(x, mask_u8, want_sums=True, sums_out=sums_out)
        h1 = _pad_cols4(h1)
        if sums1 is None or sums1.numel() != 2 * h1.shape[1] + 2:
            sums1 = ops.domain_sums(h1, mask_u8)
        return None, h1, sums1

    def target_stage_b(self, stage_a, mask_u8, out, sums_t=None, rows32=False):
        """head 2's (h_t2s, h_s2t) tables into `out` from stage A's result; `sums_t`: the GLOBAL domain sums of h1 where stage A's
        are one rank's share; `rows32` (raw form only): `out` is the second half of 32-byte rows"""
        raw, h1, sums_t = (*stage_a[:2], sums_t if sums_t is not None else stage_a[2])
        if raw is not None:
            ops.narrow_transform_finish(raw, mask_u8, sums_t, self.composed_target_pack(ops.pad4(self._tf_w0.shape[0])), out, rows32=rows32)
        else:
            assert not rows32
            ops.adaptedconv_transform(h1, mask_u8, None, self.composed_target_pack(h1.shape[1]), out=[out], sums=sums_t)

    def target_tables(self, x, mask_u8, out, arena=None, sums_out=None):
        """stage A and stage B back to back (one device: the local sums of h1 are the global ones)"""
        if sums_out is None:
            n_s = 2 * ops.pad4(self.model.clf_transformer[0].weight.shape[0]) + 2
            sums_out = arena.take(n_s) if arena is not None else torch.zeros(n_s, dtype=torch.float64, device=x.device)
        self.target_stage_b(self.target_stage_a(x, mask_u8, sums_out), mask_u8, out)

    def eval_tables(self, x, mask_u8, sums_h, views, arena):
        """the six narrow tables of rows x on one device, `sums_h` = the domain sums of x"""
        a = self.one_pass(x, mask_u8, sums_h, views, arena)
        if a is not None:
            return self.target_stage_b(a, mask_u8, views[2])
        self.pair_tables(x, mask_u8, sums_h, views)
        self.target_tables(x, mask_u8, views[2], arena)

    # ---- training --------------------------------------------------------------------------------------------------------
    def train_walk(self, opt_in=False):
        """which training walk serves the three heads at this C: "narrow" (C <= 4), "wide" (C <= 32) or "convs" (one walk per
        conv on the shared tables).  `opt_in` (single device, where the convs' own forward is the alternative): the environment
        decides as well -- BGNN_FUSED_TRAIN_HEADS (default on), BGNN_WIDE_TRAIN_HEADS (default off) -- and None = neither."""
        if ops.heads_log_softmax_supported(3, self.C) and not (opt_in and os.environ.get("BGNN_FUSED_TRAIN_HEADS", "1") == "0"):
            return "narrow"
        if ops.wide_heads_supported(3, self.C) and not (opt_in and os.environ.get("BGNN_WIDE_TRAIN_HEADS", "0") != "1"):
            return "wide"
        return None if opt_in else "convs"

    def train_tables(self, x, mask_u8, sums_x, bn, sums_of=None, mean_hook=None):
        """the six autograd tables (h_t2s, h_s2t of head 0, 1, 2) of rows x (main_graph_knowledge_transfer.py:39-68).  `sums_x`: the
        global domain sums of x, formed once for both convs on x; `bn(x, bn_module, relu, p_drop)`: train-mode BatchNorm -> ReLU of
        clf_transformer; `sums_of(xt)`: the global domain sums of T(x) (None: the transform forms them); `mean_hook`: see
        `_TransformFn`.  `_TransformPairFn` has no such hook: one device only."""
        base, target, _ = self.convs
        l0, bnm, _, l3 = self.model.clf_transformer
        xt = l3(bn(l0(x), bnm, True, 0.0)).contiguous()
        sums_t = sums_of(xt) if sums_of is not None else None
        if mean_hook is None and _TransformPairFn.supported(x, base, target):
            prm = [t for c in (base, target)
                   for t in (c.lin_s.weight, c.lin_s.bias, c.lin_t.weight, c.lin_t.bias, c.a_g_s2t.weight, c.a_g_t2s.weight)]
            tabs_x = _TransformPairFn.apply(x, mask_u8, base, target, sums_x, *prm)
        else:
            tabs_x = (*base._transform_autograd(x, mask_u8, sums_x, mean_hook), *target._transform_autograd(x, mask_u8, sums_x, mean_hook))
        return (*tabs_x, *target._transform_autograd(xt, mask_u8, sums_t, mean_hook))

    def train_aggregate(self, walk, csr, mask_u8, tables, n_rows=None):
        """`tables` (six [rows, pad4(C)] tensors in `train_tables` order) -> the three heads' log-probs of the first `n_rows` rows"""
        C = self.C
        a_t, a_s = self.attention(autograd=True)
        if walk == "convs":
            return tuple(F.log_softmax(_AggregateFn.apply(tables[2 * j], tables[2 * j + 1], a_t[j], a_s[j], csr, mask_u8, C,
                                                          c.negative_slope)[:n_rows, :C], dim=1) for j, c in enumerate(self.convs))
        fn = _AggregateHeadsFn if walk == "narrow" else _AggregateWideHeadsFn
        logp = fn.apply(csr, mask_u8, C, self.slope, a_t, a_s, *tables)[:n_rows, :, :C]
        return logp[:, 0], logp[:, 1], logp[:, 2]
