"""CPU: the host side of partitioned GAT (bridged_gnn_amd.dist_gat.GatPartition) -- `SagePartition`'s invariants over A' + I and
`edge_base`, the position of every owned row's first edge in the whole graph's by-destination CSR, against a numpy stable sort:
over all ranks the positions edge_base[i] + k cover the whole graph's edges exactly once and name the same sources, which is what
lets a rank hash the attention dropout where the single-GPU call hashes it; the one entry per aggregation that takes the ids (ABI
116: no `_rows` twin), the package exports and the wrappers' keywords."""
import ctypes
import inspect

import numpy as np
import pytest

from test_gatv2_partition_host import _abi_116, _one_entry
from test_gcn_partition_host import _case, _chunk


def _whole_graph_csr(ei, n):
    """(rowptr, src) of the whole graph's by-destination CSR as the device builds it: input self loops dropped, the other edges
    sorted by destination with a STABLE sort (input order inside a row), one self loop appended as the last edge of every row"""
    keep = ei[0] != ei[1]
    s, d = ei[0][keep], ei[1][keep]
    loops = np.arange(n, dtype=np.int64)
    s, d = np.concatenate([s, loops]), np.concatenate([d, loops])        # the loops come last in the input: last in their rows
    order = np.argsort(d, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=n))]).astype(np.int64)
    return rowptr, s[order]


@pytest.mark.parametrize("owner_kind", ["contiguous", "domain_blocks"])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
@pytest.mark.parametrize("graph", ["small", "synth"])
def test_partition_tables_and_edge_base(graph, world, owner_kind):
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gat import GatPartition
    ei, n, mask, (src, dst, _) = _case(graph)
    rowptr_g, src_g = _whole_graph_csr(ei, n)
    E = src_g.shape[0]
    assert E == src.shape[0] == int((ei[0] != ei[1]).sum()) + n
    owner = partition_nodes(mask, world) if owner_kind == "domain_blocks" else None
    parts = [GatPartition(ei, n, r, world, owner=owner) for r in range(world)]
    own = np.concatenate([p.owned_global for p in parts])
    assert np.array_equal(np.sort(own), np.arange(n))
    covered = np.zeros(E, dtype=np.int64)
    for p in parts:
        ext = p.ext_global()
        # SagePartition's invariants over A' + I
        assert p.n_ext == p.n_local + p.n_halo and ext.shape == (p.n_ext,)
        assert p.rowptr.shape == (p.n_ext + 1,) and p.col.shape == (p.num_edges,)
        assert p.rowptr.dtype == np.int32 and p.col.dtype == np.int32
        assert (p.rowptr[p.n_local:] == p.num_edges).all(), "halo slots have no in-edges"
        assert ((p.col >= 0) & (p.col < p.n_ext)).all()
        rows = np.repeat(np.arange(p.n_ext), np.diff(p.rowptr))
        got = np.sort(ext[rows] * n + ext[p.col])
        mine = np.isin(dst, p.owned_global)
        assert np.array_equal(got, np.sort(dst[mine] * n + src[mine])), f"rank {p.rank}"
        last = p.col[p.rowptr[1:p.n_local + 1] - 1]
        assert np.array_equal(ext[last], p.owned_global), "the self loop is the last edge of every owned row"
        n_loops = np.bincount(rows[ext[rows] == ext[p.col]], minlength=p.n_ext)
        assert (n_loops[:p.n_local] == 1).all(), "exactly one self loop per owned row"
        assert np.unique(p.halo_global).shape[0] == p.n_halo and not np.isin(p.halo_global, p.owned_global).any()
        read = np.zeros(p.n_ext, dtype=bool)
        read[p.col] = True
        assert read[p.n_local:].all()
        assert np.array_equal(np.sort(p.seg_idx), np.arange(p.send_rows.shape[0]))
        assert p.seg_ptr[0] == 0 and p.seg_ptr[-1] == p.send_rows.shape[0]
        for s in range(p.seg_row.shape[0]):
            ks = p.seg_idx[p.seg_ptr[s]:p.seg_ptr[s + 1]]
            assert ks.size > 0 and (np.diff(ks) > 0).all() and (p.send_rows[ks] == p.seg_row[s]).all()
        # edge_base: the whole graph's rowptr at the owned rows; the rows have the whole graph's degrees
        assert p.edge_base.dtype == np.int64 and p.edge_base.shape == (p.n_local,) and p.edge_base.flags["C_CONTIGUOUS"]
        assert np.array_equal(p.edge_base, rowptr_g[p.owned_global]), f"rank {p.rank}"
        deg = np.diff(p.rowptr)[:p.n_local]
        assert np.array_equal(deg, np.diff(rowptr_g)[p.owned_global])
        # edge k of owned row i is edge edge_base[i] + k of the whole graph: same position, same source
        pos = np.repeat(p.edge_base - p.rowptr[:p.n_local], deg) + np.arange(p.num_edges)
        np.add.at(covered, pos, 1)
        assert np.array_equal(src_g[pos], ext[p.col]), f"rank {p.rank}: a row's edges are not in the whole graph's order"
    assert (covered == 1).all(), "the ranks' positions cover 0 .. E'-1 exactly once"
    for r, p in enumerate(parts):
        assert sum(p.recv_splits) == p.n_halo and sum(p.send_splits) == p.send_rows.shape[0]
        assert [q.send_splits[r] for q in parts] == list(p.recv_splits)
        got = np.concatenate([q.owned_global[_chunk(q.send_rows, q.send_splits, r)] for q in parts])
        assert np.array_equal(got, p.halo_global)
    assert (sum(p.n_halo for p in parts) > 0) == (world > 1)


def test_rows_entries_are_exported_and_bound():
    P = ctypes.c_void_p
    # forward: the ids sit immediately before the first output (state); backward: before the first output (g), after the workspace
    names, args = _one_entry("bgnn_gat_aggregate_f32", "bgnn_gat_aggregate_rows_f32")
    assert names[-11:-8] == ["row_id_opt", "edge_base_opt", "state"] and args[-11:-9] == [P, P]
    assert names[-12] == "seed_dev_opt" and len(names) == 31
    names, args = _one_entry("bgnn_gat_aggregate_bwd_f32", "bgnn_gat_aggregate_bwd_rows_f32")
    assert names[-11:-6] == ["ws", "ws_bytes", "row_id_opt", "edge_base_opt", "g"] and args[-9:-7] == [P, P]
    assert names[:3] == ["tbl", "ldt", "n_src"] and len(names) == 40
    _abi_116()


def test_package_exports_and_wrapper_keywords():
    import torch

    import bridged_gnn_amd
    from bridged_gnn_amd import GatPartition, PartitionedGAT, dist_gat, ops
    assert PartitionedGAT is dist_gat.PartitionedGAT and GatPartition is dist_gat.GatPartition
    assert bridged_gnn_amd.PartitionedGAT is PartitionedGAT
    fwd = inspect.signature(ops.gat_aggregate).parameters
    bwd = inspect.signature(ops.gat_aggregate_bwd).parameters
    assert list(fwd)[-2:] == ["row_ids", "edge_base"] and list(bwd)[-3:] == ["n_rows", "row_ids", "edge_base"]
    assert all(fwd[k].default is None for k in ("row_ids", "edge_base"))
    assert all(bwd[k].default is None for k in ("n_rows", "row_ids", "edge_base"))
    for name in ("forward", "get_emb", "nll_loss", "sync_grads", "invalidate_input_cache"):
        assert callable(getattr(PartitionedGAT, name))
    # the ids are given together: one alone is refused before anything reaches the device
    ids, f, i32 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 4), torch.zeros(5, dtype=torch.int32)
    for kw in (dict(row_ids=ids), dict(edge_base=ids)):
        with pytest.raises(ValueError, match="together"):
            ops.gat_aggregate(f, f[:, :1], f[:, :1], i32, i32[:4], 4, 1, 4, **kw)
        with pytest.raises(ValueError, match="together"):
            ops.gat_aggregate_bwd(f, f[:, :1], f[:, :1], f[:, :2], f[:, :1], f, f, i32, i32[:4], i32, i32[:4], i32[:4], 1, 4, **kw)
