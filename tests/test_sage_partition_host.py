"""CPU: the host side of partitioned GraphSAGE (bridged_gnn_amd.dist_sage.SagePartition) -- the owned rows, the extended CSR,
the halo slots and the segment CSR of the gradient return -- and an fp64 numpy simulation of the partitioned forward and
backward (exchange by row copies, exactly as all_to_all_single delivers them) against the whole-graph fp64 GraphSAGE on the
reference's small fixture."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub

SMALL_MODELS = (("l2h8", 2), ("l1", 1), ("l3h6", 3))


def _graph(n, e, seed):
    from bridged_gnn_amd import synth
    ei, mask = synth.random_multigraph(n, e, n_isolated=max(n // 20, 1), seed=seed)
    extra = [ei, ei[:, : e // 10], np.stack([np.arange(0, n, 5), np.arange(0, n, 5)])]   # duplicate edges + self loops
    return np.concatenate(extra, axis=1).astype(np.int64), mask


def _parts(ei, n, world, owner_kind, mask=None):
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_sage import SagePartition
    owner = partition_nodes(mask, world) if owner_kind == "domain_blocks" else None
    return [SagePartition(ei, n, r, world, owner=owner) for r in range(world)]


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("owner_kind", ["contiguous", "domain_blocks"])
def test_partition_tables(world, owner_kind):
    n = 700
    ei, mask = _graph(n, 5000, seed=world)
    parts = _parts(ei, n, world, owner_kind, mask)
    # the owned rows form a partition
    own = np.concatenate([p.owned_global for p in parts])
    assert np.array_equal(np.sort(own), np.arange(n))
    # whole-graph in-edge lists in input order (the SageGraph CSR keeps duplicates, self loops and input order)
    order = np.argsort(ei[1], kind="stable")
    g_src, g_dst = ei[0][order], ei[1][order]
    g_ptr = np.searchsorted(g_dst, np.arange(n + 1))
    for p in parts:
        ext = p.ext_global()
        assert p.rowptr.shape == (p.n_ext + 1,) and p.col.shape == (p.num_edges,)
        assert (p.rowptr[p.n_local:] == p.num_edges).all(), "halo rows have no in-edges"
        assert ((p.col >= 0) & (p.col < p.n_ext)).all()
        for i, v in enumerate(p.owned_global):
            got = ext[p.col[p.rowptr[i]:p.rowptr[i + 1]]]
            assert np.array_equal(got, g_src[g_ptr[v]:g_ptr[v + 1]]), f"rank {p.rank} row {v}"
        # one halo slot per node, all remote, all actually read
        assert np.unique(p.halo_global).shape[0] == p.n_halo
        assert not np.isin(p.halo_global, p.owned_global).any()
        read = np.zeros(p.n_ext, dtype=bool)
        read[p.col] = True
        assert read[p.n_local:].all()
        # the segment CSR covers every send entry exactly once, each under its own row
        assert np.array_equal(np.sort(p.seg_idx), np.arange(p.send_rows.shape[0]))
        assert np.unique(p.seg_row).shape[0] == p.seg_row.shape[0]
        for s in range(p.seg_row.shape[0]):
            ks = p.seg_idx[p.seg_ptr[s]:p.seg_ptr[s + 1]]
            assert ks.size > 0 and (np.diff(ks) > 0).all() and (p.send_rows[ks] == p.seg_row[s]).all()
    # the splits pair up: what q sends to r is what r receives from q, and it is what r's halo holds
    for r, p in enumerate(parts):
        assert sum(p.recv_splits) == p.n_halo
        got = np.concatenate([q.owned_global[_chunk(q.send_rows, q.send_splits, r)] for q in parts])
        assert np.array_equal(got, p.halo_global)
    assert sum(p.n_halo for p in parts) > 0


def _chunk(a, splits, k):
    o = int(sum(splits[:k]))
    return a[o:o + int(splits[k])]


def _a2a(parts, bufs, fwd=True):
    """all_to_all_single by row copies: forward sends (send order, send_splits) -> halo order; reverse the other way"""
    out = []
    for r, p in enumerate(parts):
        s_key, r_key = ("send_splits", "recv_splits") if fwd else ("recv_splits", "send_splits")
        out.append(np.concatenate([_chunk(bufs[k], getattr(q, s_key), r) for k, q in enumerate(parts)]
                                  + [np.zeros((0,) + bufs[r].shape[1:])]))
        assert out[-1].shape[0] == sum(getattr(p, r_key))
    return out


def _simulate(parts, P, x, y, tm, L):
    """the partitioned forward and backward of dist_sage in fp64 numpy -> (loss summed over ranks, gradients summed over ranks)"""
    cnt = max(int(tm.sum()), 1)
    W = [(P[f"convs.{l}.lin_l.weight"], P[f"convs.{l}.lin_l.bias"], P[f"convs.{l}.lin_r.weight"]) for l in range(L)]
    h = [x[p.owned_global] for p in parts]                 # input of the conv (own rows)
    saved = []
    for l, (wl, bl, wr) in enumerate(W):
        if l == 0:                                         # resident input halo: own + halo rows transformed locally
            xin = [np.concatenate([x[p.owned_global], x[p.halo_global]]) for p in parts]
            tl = [xi @ wl.T for xi in xin]
        else:                                              # own rows transformed, T_l of the send rows exchanged
            xin = h
            tl_own = [hi @ wl.T for hi in h]
            halo = _a2a(parts, [t[p.send_rows] for t, p in zip(tl_own, parts)])
            tl = [np.concatenate([t, hh]) for t, hh in zip(tl_own, halo)]
        outs, pres = [], []
        for r, p in enumerate(parts):
            nl = p.n_local
            deg = np.diff(p.rowptr[:nl + 1])
            rows = np.repeat(np.arange(nl), deg)
            s = np.zeros((nl, wl.shape[0]))
            np.add.at(s, rows, tl[r][p.col])
            pre = s / np.maximum(deg, 1)[:, None] + h[r] @ wr.T + bl
            pres.append(pre)
            if l == L - 1:
                z = pre - pre.max(1, keepdims=True)
                outs.append(z - np.log(np.exp(z).sum(1, keepdims=True)))
            else:
                outs.append(np.maximum(pre, 0))
        saved.append((xin, pres, outs))
        h = outs
    loss = 0.0
    dy = []
    for r, p in enumerate(parts):
        yl, tml = y[p.owned_global], tm[p.owned_global].astype(np.float64)
        loss += -(h[r][np.arange(p.n_local), yl] * tml).sum() / cnt
        g = np.zeros_like(h[r])
        g[np.arange(p.n_local), yl] = -tml / cnt
        dy.append(g)
    grads = {}
    for l in reversed(range(L)):
        wl, bl, wr = W[l]
        xin, pres, outs = saved[l]
        d_tl, d_tr = [], []
        for r, p in enumerate(parts):
            nl = p.n_local
            if l == L - 1:
                g = dy[r] - np.exp(outs[r]) * dy[r].sum(1, keepdims=True)
            else:
                g = dy[r] * (pres[r] > 0)
            deg = np.diff(p.rowptr[:nl + 1])
            rows = np.repeat(np.arange(nl), deg)
            dt = np.zeros((p.n_ext, g.shape[1]))
            np.add.at(dt, p.col, (g / np.maximum(deg, 1)[:, None])[rows])
            d_tl.append(dt)
            d_tr.append(g)
        if l > 0:                                          # reverse exchange + fold into the owners' rows (segment CSR)
            back = _a2a(parts, [dt[p.n_local:] for dt, p in zip(d_tl, parts)], fwd=False)
            for r, p in enumerate(parts):
                own = d_tl[r][:p.n_local]
                for s in range(p.seg_row.shape[0]):
                    own[p.seg_row[s]] += back[r][p.seg_idx[p.seg_ptr[s]:p.seg_ptr[s + 1]]].sum(0)
                d_tl[r] = own
        gwl = sum(dt.T @ xi for dt, xi in zip(d_tl, xin))
        gwr = sum(g.T @ xi[:p.n_local] for g, xi, p in zip(d_tr, xin, parts))
        gbl = sum(g.sum(0) for g in d_tr)
        grads.update({f"convs.{l}.lin_l.weight": gwl, f"convs.{l}.lin_l.bias": gbl, f"convs.{l}.lin_r.weight": gwr})
        if l > 0:
            dy = [dt[:p.n_local] @ wl + g @ wr for dt, g, p in zip(d_tl, d_tr, parts)]
    return loss, grads


def _whole_graph(P, x, ei, y, tm, L):
    """the whole-graph fp64 GraphSAGE (torch autograd): loss and gradients"""
    Pt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in P.items()}
    src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    n = x.shape[0]
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64)).clamp(min=1)
    h = torch.from_numpy(x)
    for l in range(L):
        c = f"convs.{l}."
        agg = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add_(0, dst, h[src]) / cnt[:, None]
        h = agg @ Pt[c + "lin_l.weight"].t() + Pt[c + "lin_l.bias"] + h @ Pt[c + "lin_r.weight"].t()
        h = torch.relu(h) if l < L - 1 else torch.log_softmax(h, 1)
    tmt = torch.from_numpy(tm)
    loss = F.nll_loss(h[tmt], torch.from_numpy(y)[tmt])
    gs = torch.autograd.grad(loss, list(Pt.values()))
    return loss.item(), {k: g.numpy() for k, g in zip(Pt, gs)}


@pytest.mark.parametrize("world", [2, 3, 4])
def test_fp64_partitioned_simulation_reproduces_whole_graph(world):
    d = load_golden("graphsage_small.npz")
    x, y, tm, ei = d["x"].astype(np.float64), d["y"].astype(np.int64), d["train_mask"].astype(bool), d["edge_index"].astype(np.int64)
    n = x.shape[0]
    rng = np.random.default_rng(world)
    # the fixture's graph as shipped, and with extra duplicates, self loops and nodes without in-edges
    ei_adv = np.concatenate([ei, ei[:, rng.choice(ei.shape[1], 200)], np.stack([np.arange(0, n, 3)] * 2)], axis=1)
    ei_adv = ei_adv[:, ~np.isin(ei_adv[1], np.arange(7, n, 37))]          # nodes without in-edges
    assert (np.bincount(ei_adv[1], minlength=n) == 0).sum() >= n // 37
    for graph_name, e in (("raw", ei), ("adversarial", ei_adv)):
        for owner_kind in ("contiguous", "domain_blocks"):
            parts = _parts(e, n, world, owner_kind, rng.random(n) < 0.4)
            for name, L in SMALL_MODELS:
                P = {k: v.astype(np.float64) for k, v in sub(d, f"{name}/param/").items()}
                loss_ref, g_ref = _whole_graph(P, x, e, y, tm, L)
                if graph_name == "raw":                # the whole-graph restatement is the reference's (fixture)
                    assert abs(loss_ref - float(d[f"raw/{name}/loss"])) <= 1e-12 * abs(loss_ref)
                loss, g = _simulate(parts, P, x, y, tm, L)
                what = f"world {world} {graph_name} {owner_kind} {name}"
                assert abs(loss - loss_ref) <= 1e-12 * abs(loss_ref), what
                assert sorted(g) == sorted(g_ref)
                for k in g_ref:
                    err = np.abs(g[k] - g_ref[k]).max()
                    assert err <= 1e-12 * max(np.abs(g_ref[k]).max(), 1e-300), f"{what} {k}: {err:.3e}"
