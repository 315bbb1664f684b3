"""CPU: the host side of partitioned GCN (bridged_gnn_amd.dist_gcn.GcnPartition) -- the owned rows, the extended CSR of A' + I,
the global-degree `dinv_ext` of owned rows and halo slots, the send / receive lists and the segment CSR of the gradient return --
against a numpy brute force and the degrees of test_gcn_host.norm_adj; the one aggregation entry that takes the row ids (ABI 116:
no `_rows` twin, for GCN and for GraphSAGE) and the package exports."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gatv2_partition_host import _abi_116, _one_entry
from test_gcn_host import norm_adj


@functools.lru_cache(maxsize=None)
def _case(name):
    """(edge_index, n, central mask, reference) -- built once per graph: the small GCN fixture's graph (duplicates, repeated self
    loops, nodes without in-edges) or a bridged graph of about 2000 nodes with duplicates and self loops added"""
    if name == "small":
        d = load_golden("gcn_small.npz")
        n = d["x"].shape[0]
        ei = d["edge_index"].astype(np.int64)
        return ei, n, np.arange(n) < n // 2, _reference(ei, n)
    from bridged_gnn_amd import synth
    ei, mask = synth.bridged_graph(1200, 800, 4, 8, 3000, cluster=128, p_local=0.8, seed=5)
    n = 2000
    loops = np.arange(0, n, 9)
    ei = np.concatenate([ei, ei[:, :300], np.stack([loops, loops]), np.stack([loops[:7], loops[:7]])], axis=1)
    ei = ei.astype(np.int64)
    return ei, n, mask, _reference(ei, n)


def _reference(ei, n):
    """brute force: (src, dst) of A' + I (input self loops dropped, one per node, duplicates counted) and the single-GPU dinv from
    the degrees of the fp64 dense restatement (A^ = dinv A dinv has the diagonal 1 / deg_i: exactly one loop per node)"""
    keep = ei[0] != ei[1]
    loops = np.arange(n, dtype=np.int64)
    src, dst = np.concatenate([ei[0][keep], loops]), np.concatenate([ei[1][keep], loops])
    deg = np.rint(1.0 / torch.diagonal(norm_adj(torch.from_numpy(ei), n)).numpy()).astype(np.int64)
    assert np.array_equal(deg, np.bincount(dst, minlength=n))
    return src, dst, (deg.astype(np.float64) ** -0.5).astype(np.float32)


def _chunk(a, splits, k):
    o = int(sum(splits[:k]))
    return a[o:o + int(splits[k])]


@pytest.mark.parametrize("owner_kind", ["contiguous", "domain_blocks"])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("graph", ["small", "synth"])
def test_partition_tables(graph, world, owner_kind):
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gcn import GcnPartition
    ei, n, mask, (src, dst, dinv_ref) = _case(graph)
    owner = partition_nodes(mask, world) if owner_kind == "domain_blocks" else None
    parts = [GcnPartition(ei, n, r, world, owner=owner) for r in range(world)]
    # the owned sets partition the nodes
    own = np.concatenate([p.owned_global for p in parts])
    assert np.array_equal(np.sort(own), np.arange(n))
    for p in parts:
        ext = p.ext_global()
        assert p.n_ext == p.n_local + p.n_halo and ext.shape == (p.n_ext,)
        assert p.rowptr.shape == (p.n_ext + 1,) and p.col.shape == (p.num_edges,)
        assert p.rowptr.dtype == np.int32 and p.col.dtype == np.int32
        assert (p.rowptr[p.n_local:] == p.num_edges).all(), "halo slots have no in-edges"
        assert ((p.col >= 0) & (p.col < p.n_ext)).all()
        # exactly the in-edges of the owned rows, as multisets of (global src, global dst)
        rows = np.repeat(np.arange(p.n_ext), np.diff(p.rowptr))
        got = np.sort(ext[rows] * n + ext[p.col])
        mine = np.isin(dst, p.owned_global)
        assert np.array_equal(got, np.sort(dst[mine] * n + src[mine])), f"rank {p.rank}"
        n_loops = np.bincount(rows[ext[rows] == ext[p.col]], minlength=p.n_ext)
        assert (n_loops[:p.n_local] == 1).all(), "exactly one self loop per owned row"
        # dinv of owned rows and halo slots alike: the single-GPU factor (fp64 rsqrt of the GLOBAL degree, rounded to fp32)
        assert p.dinv_ext.dtype == np.float32 and p.dinv_ext.shape == (p.n_ext,)
        assert np.array_equal(p.dinv_ext, dinv_ref[ext]), f"rank {p.rank}"
        # one halo slot per node, all remote, all actually read
        assert np.unique(p.halo_global).shape[0] == p.n_halo
        assert not np.isin(p.halo_global, p.owned_global).any()
        read = np.zeros(p.n_ext, dtype=bool)
        read[p.col] = True
        assert read[p.n_local:].all()
        # the segment CSR covers every send entry exactly once, each under its own row
        assert np.array_equal(np.sort(p.seg_idx), np.arange(p.send_rows.shape[0]))
        assert np.unique(p.seg_row).shape[0] == p.seg_row.shape[0]
        assert p.seg_ptr[0] == 0 and p.seg_ptr[-1] == p.send_rows.shape[0]
        for s in range(p.seg_row.shape[0]):
            ks = p.seg_idx[p.seg_ptr[s]:p.seg_ptr[s + 1]]
            assert ks.size > 0 and (np.diff(ks) > 0).all() and (p.send_rows[ks] == p.seg_row[s]).all()
    # the splits pair up: what q sends to r is what r receives from q, and it is what r's halo holds
    for r, p in enumerate(parts):
        assert sum(p.recv_splits) == p.n_halo and len(p.send_splits) == len(p.recv_splits) == world
        assert sum(p.send_splits) == p.send_rows.shape[0]
        assert [q.send_splits[r] for q in parts] == list(p.recv_splits)
        got = np.concatenate([q.owned_global[_chunk(q.send_rows, q.send_splits, r)] for q in parts])
        assert np.array_equal(got, p.halo_global)
    assert (sum(p.n_halo for p in parts) > 0) == (world > 1)


def test_rows_entry_is_exported_and_bound():
    for plain, twin, n_args in (("bgnn_gcn_aggregate_f32", "bgnn_gcn_aggregate_rows_f32", 26),
                                ("bgnn_sage_mean_aggregate_f32", "bgnn_sage_mean_aggregate_rows_f32", 18)):
        names, args = _one_entry(plain, twin)
        assert names[-4:] == ["row_id_opt", "out", "ldo", "stream"] and args[-4] is ctypes.c_void_p     # the ids sit before `out`
        assert len(names) == n_args
    _abi_116()


def test_package_exports_and_wrapper_keyword():
    import inspect

    import bridged_gnn_amd
    from bridged_gnn_amd import GcnPartition, PartitionedGCN, dist_gcn, ops
    assert PartitionedGCN is dist_gcn.PartitionedGCN and GcnPartition is dist_gcn.GcnPartition
    assert bridged_gnn_amd.PartitionedGCN is PartitionedGCN
    params = list(inspect.signature(ops.gcn_aggregate).parameters)
    assert params[-1] == "row_ids" and inspect.signature(ops.gcn_aggregate).parameters["row_ids"].default is None
    for name in ("forward", "get_emb", "get_logits", "nll_loss", "sync_grads", "invalidate_input_cache"):
        assert callable(getattr(PartitionedGCN, name))
