"""One sha256 per case over the outputs of the three step-2 convs' kernels, to compare two trees bit for bit:

    python profiles/conv_common/digests.py --root TREE > digests.txt      (TREE: a checkout with its library built)

Graph: synth.random_multigraph(3000 nodes, 30000 edges, seed 1) as a by-destination CSR with one self loop per row, and its
by-source view.  Widths 1, 2, 5, 31, 64, 128, 132; every epilogue; p_drop 0 and, after the activation, 0.5; GCN with and without
hub tables (threshold 16, segments of 8 edges); GAT at H = 1 and 3 with C up to 128; rows_segment_add over the by-source view."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

DS = (1, 2, 5, 31, 64, 128, 132)
N, E = 3000, 30000


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.gcn import GcnGraph
    dev = torch.device("cuda:0")
    ei, _ = synth.random_multigraph(N, E, n_isolated=30, seed=1)
    g = GcnGraph(torch.from_numpy(ei.astype(np.int64)).to(dev), N)
    rowptr, col = g.csr.rowptr, g.col
    t_rowptr, t_eid, t_dst = g.csr.transposed()
    hubs = (16,) + tuple(g.csr.hub_tables(16, 8)[:3])
    t_hubs = (16,) + tuple(g.csr.transposed_hub_tables(16, 8)[:3])
    gen = torch.Generator().manual_seed(5)
    word = torch.tensor([77], dtype=torch.int64, device=dev)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    for D in DS:
        Dp = ops.pad4(D)
        T, root, bias, dy = rnd(N, Dp), rnd(N, Dp), rnd(Dp), rnd(N, Dp)
        dy[:, D:] = 0
        for epi in (None, "relu", "log_softmax"):
            if epi == "log_softmax" and D > 128:
                continue
            for p in ((0.0, 0.5) if epi == "relu" else (0.0,)):
                kw = dict(epilogue=epi, p_drop=p)
                tag = f"D={D} epi={epi} p={p}"
                y = ops.sage_mean_aggregate(T, rowptr, col, N, D, root=root, seed=11, seed_dev=word if p else None, **kw)
                print(f"sage_fwd {tag} {sha(y)}")
                print(f"sage_bwd {tag} {sha(*ops.sage_mean_aggregate_bwd(y, dy, rowptr, t_rowptr, t_dst, N, D, **kw))}")
                for hb, thb, ht in ((None, None, "plain"), (hubs, t_hubs, "hubs")):
                    y = ops.gcn_aggregate(T, rowptr, col, g.dinv, N, D, bias=bias, seed=11, seed_dev=word if p else None, hubs=hb, **kw)
                    print(f"gcn_fwd {ht} {tag} {sha(y)}")
                    print(f"gcn_bwd {ht} {tag} {sha(*ops.gcn_aggregate_bwd(y, dy, t_rowptr, t_dst, g.dinv, N, D, hubs=thb, **kw))}")
        print(f"sage_bwd D={D} epi=None y=None {sha(*ops.sage_mean_aggregate_bwd(None, dy, rowptr, t_rowptr, t_dst, N, D))}")
        rows = torch.randperm(N, generator=gen).to(torch.int32).to(dev)
        for acc in (False, True):
            dst = rnd(N, Dp)
            dst[:, D:] = 0
            print(f"rows_segment_add D={D} accumulate={acc} {sha(ops.rows_segment_add(T, t_rowptr, t_dst, rows, dst, D=D, accumulate=acc))}")

    for H in (1, 3):
        for C in (c for c in DS if c <= 128):
            W = ops.pad4(H * C)
            T, bias, dy = rnd(N, W), rnd(W), rnd(N, W)
            dy[:, H * C:] = 0
            s_src, s_dst = ops.gat_scores(T, rnd(H * C), rnd(H * C), H, C)
            for epi in (None, "elu", "log_softmax"):
                if epi == "log_softmax" and H != 1:
                    continue
                for p in ((0.0, 0.5) if epi == "elu" else (0.0,)):
                    kw = dict(bias=bias, p_att=0.5 if p else 0.0, seed_att=3, epilogue=epi, p_drop=p, seed=11)
                    tag = f"H={H} C={C} epi={epi} p={p}"
                    out, state, pre, alpha = ops.gat_aggregate(T, s_src, s_dst, rowptr, col, N, H, C, want_pre=True, return_alpha=True, **kw)
                    print(f"gat_fwd {tag} {sha(out, state, pre, alpha)}")
                    got = ops.gat_aggregate_bwd(T, s_src, s_dst, state, alpha, pre, dy, rowptr, col, t_rowptr, t_eid, t_dst, H, C, **kw)
                    print(f"gat_bwd {tag} {sha(*got)}")


if __name__ == "__main__":
    main()
