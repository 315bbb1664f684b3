"""CPU: the host side of the segmented GIN walk and of GIN on a node partition (bridged_gnn_amd.dist_gin, models/backbones.py:26-57)
-- the three additive C entries are declared, bound, argument-counted and cited while the ABI revision stays 116 and the three
earlier GIN entries keep their arity; bgnn_gin.hip still has no atomics and keeps its Makefile and hash position; the facts of a
GIN partition (`dist_sage.SagePartition(rewrite_self_loops=False)`) on gin_small's graph at worlds 1, 2 and 3; the refusals that
need no GPU; and a numpy restatement of the hub tables' invariants at (threshold, segment) = (8, 5) on the small graph."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgnn_gin_aggregate_hub_workspace_bytes", "bgnn_gin_aggregate_hub_f32", "bgnn_gin_aggregate_bwd_hub_f32")
OLD = {"bgnn_gin_aggregate_f32": 18, "bgnn_gin_aggregate_bwd_workspace_bytes": 2, "bgnn_gin_aggregate_bwd_f32": 23}
HUB_ARGS = ["hub_threshold", "hub_rows_opt", "n_hubs", "hub_seg_ptr_opt", "seg_bounds_opt", "n_seg"]
DS = types.SimpleNamespace(num_features=37, num_classes=5)


def _decl_args(code, name):
    decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert decl, f"{name} is not declared in bgnn.h"
    return [a.strip() for a in decl.group(1).split(",") if a.strip()]


def _names(args):
    return [a.split()[-1].lstrip("*") for a in args]


# ---- C ABI -------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_cited_and_the_abi_stays():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        args = _decl_args(code, name)
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name][1]) == len(args), name
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)
    for name, arity in OLD.items():                          # the earlier entries keep their argument lists
        assert len(_decl_args(code, name)) == arity == len(_lib.SIGNATURES[name][1]), name
    # the forward takes the old forward's arguments plus the hub arguments in bgnn_gcn_aggregate_f32's order, then the workspace
    old, new, gcn = (_names(_decl_args(code, k)) for k in ("bgnn_gin_aggregate_f32", NEW[1], "bgnn_gcn_aggregate_f32"))
    assert [a for a in new if a in old] == old
    extra = [a for a in new if a not in old]
    assert extra == HUB_ARGS + ["ws_opt", "ws_bytes"] and [a for a in gcn if a in extra] == extra
    oldb, newb = (_names(_decl_args(code, k)) for k in ("bgnn_gin_aggregate_bwd_f32", NEW[2]))
    assert [a for a in newb if a in oldb] == oldb and [a for a in newb if a not in oldb] == HUB_ARGS
    # one self-contained comment block cites the reference for both new walks and states their formulas
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if NEW[2] + " (" in b]
    assert len(blocks) == 1 and blocks[0].count("backbones.py:26-57") >= 2 and blocks[0].count("(1 + eps)") >= 2
    for word in (NEW[0], NEW[1], "ROWS", "SEGMENT", "FINISH", "hub_rows[h]", "row_id[hub_rows[h]]"):
        assert word in blocks[0], word
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_gin.hip")).read()
    for name in NEW + tuple(OLD):
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    assert "atomicAdd" not in src and "atomic" not in re.sub(r"//.*", "", src)
    assert "clamp_row" in src and src.count("MODE_SEGMENT") >= 3 and src.count("MODE_FINISH") >= 3


def test_source_keeps_its_makefile_and_hash_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert srcs.count("bgnn_gin.hip") == 1 and srcs.index("bgnn_gin.hip") == _lib._HASHED_SOURCES.index("bgnn_gin.hip")
    assert srcs[srcs.index("bgnn_gin.hip") - 1] == "bgnn_edge_filter.hip" and srcs[srcs.index("bgnn_gin.hip") + 1] == "bgnn_jk.hip"


def test_ops_and_model_surface():
    import bridged_gnn_amd
    from bridged_gnn_amd import dist_gin, gin, ops
    assert (ops.GIN_HUB_THRESHOLD, ops.GIN_HUB_SEGMENT) == (ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT) == (256, 128)
    base = list(inspect.signature(ops.gin_aggregate).parameters)
    sig = inspect.signature(ops.gin_aggregate_hubs).parameters
    assert list(sig) == base + ["hubs"] and sig["hubs"].default is None
    base = list(inspect.signature(ops.gin_aggregate_bwd).parameters)
    sig = inspect.signature(ops.gin_aggregate_bwd_hubs).parameters
    assert list(sig) == base + ["hubs"] and sig["hubs"].default is None
    for fn in (ops.gin_aggregate_hubs, ops.gin_aggregate_bwd_hubs):
        assert "backbones.py:26-57" in fn.__doc__ and "bgnn.h" in fn.__doc__
    with pytest.raises(ValueError, match="D >= 1"):
        ops.gin_aggregate_hubs(None, None, None, None, 2, 0, hubs=None)
    with pytest.raises(ValueError, match="D <= 128"):
        ops.gin_aggregate_bwd_hubs(None, None, None, None, None, None, 2, 129, epilogue="log_softmax")
    assert inspect.signature(gin.GINNet.__init__).parameters["segment_hubs"].default is False
    assert inspect.signature(gin.GINConv.run).parameters["hubs"].default is None
    assert gin.GINNet(DS, 2, 8).segment_hubs is False and gin.GINNet(DS, 2, 8, segment_hubs=True).segment_hubs is True
    assert bridged_gnn_amd.PartitionedGIN is dist_gin.PartitionedGIN
    sig = inspect.signature(dist_gin.PartitionedGIN.__init__).parameters
    assert sig["hub_cfg"].default == (ops.GIN_HUB_THRESHOLD, ops.GIN_HUB_SEGMENT) and sig["graphed"].default is False
    assert issubclass(dist_gin.PartitionedGIN, __import__("bridged_gnn_amd.dist_sage", fromlist=["_RankModel"])._RankModel)


# ---- the partition -----------------------------------------------------------------------------------------------
def _small():
    d = load_golden("gin_small.npz")
    return np.asarray(d["edge_index"]).astype(np.int64), int(d["x"].shape[0])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("owners", ["blocks", "scattered"])
def test_partition_facts_on_the_small_graph(world, owners):
    from bridged_gnn_amd.dist_sage import SagePartition
    ei, n = _small()
    E = ei.shape[1]
    assert (ei[0] == ei[1]).sum() >= 3 and np.unique(ei[0] * n + ei[1]).size < E          # self loops and duplicates to keep
    owner = None if owners == "blocks" else (np.arange(n) * 7 % world).astype(np.int32)
    parts = [SagePartition(ei, n, r, world, owner=owner, rewrite_self_loops=False) for r in range(world)]
    seen = np.zeros(n, dtype=np.int64)
    edges = []
    for part in parts:
        ext = part.ext_global()
        assert ext.shape == (part.n_ext,) and part.n_ext == part.n_local + part.n_halo
        seen[part.owned_global] += 1
        for i, gid in enumerate(part.owned_global):
            got = ext[part.col[part.rowptr[i]:part.rowptr[i + 1]]]
            want = ei[0][ei[1] == gid]
            assert sorted(got.tolist()) == sorted(want.tolist()), (part.rank, gid)        # as given: loops and duplicates kept
            edges += [(int(s), int(gid)) for s in got]
        assert (part.rowptr[part.n_local:] == part.rowptr[part.n_local]).all()            # halo slots have no in-edges
        assert part.num_edges == part.rowptr[part.n_local]
        assert sorted(part.halo_global.tolist()) == sorted(set(ext[part.col[:part.num_edges]].tolist()) - set(part.owned_global.tolist()))
        # the segment CSR covers the send list: every send entry once, grouped by its owned row
        ns = part.send_rows.shape[0]
        assert sum(part.send_splits) == ns and sum(part.recv_splits) == part.n_halo
        assert sorted(part.seg_idx.tolist()) == list(range(ns)) and part.seg_ptr[0] == 0 and part.seg_ptr[-1] == ns
        for s, row in enumerate(part.seg_row):
            idx = part.seg_idx[part.seg_ptr[s]:part.seg_ptr[s + 1]]
            assert idx.size >= 1 and (part.send_rows[idx] == row).all() and (np.diff(idx) > 0).all()
        assert np.unique(part.seg_row).size == part.seg_row.size
    assert (seen == 1).all()
    assert sorted(edges) == sorted(zip(ei[0].tolist(), ei[1].tolist()))                     # every edge is owned exactly once
    for a in range(world):                                   # the send and receive splits agree across ranks, and so do the rows
        for b in range(world):
            assert parts[a].send_splits[b] == parts[b].recv_splits[a]
            so, ro = sum(parts[a].send_splits[:b]), sum(parts[b].recv_splits[:a])
            k = parts[a].send_splits[b]
            sent = parts[a].owned_global[parts[a].send_rows[so:so + k]]
            assert np.array_equal(sent, parts[b].halo_global[ro:ro + k])
    if world == 1:
        assert parts[0].n_halo == 0 and parts[0].send_rows.size == 0


def test_refusals_that_need_no_gpu():
    from bridged_gnn_amd.dist_gin import PartitionedGIN
    from bridged_gnn_amd.gin import GINNet
    ei, n = _small()
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedGIN(GINNet(DS, 2, 8), ei, n, 0, 1, "cpu")
    with pytest.raises(NotImplementedError, match="graphed"):
        PartitionedGIN(GINNet(DS, 2, 8), ei, n, 0, 1, "cuda:0", graphed=True)
    with pytest.raises(ValueError, match="hub_cfg"):
        PartitionedGIN(GINNet(DS, 2, 8), ei, n, 0, 1, "cuda:0", hub_cfg=(8,))
    # a wrong row count is refused before anything touches the device
    pg = object.__new__(PartitionedGIN)
    pg.model, pg.n_local = GINNet(DS, 2, 8), n
    with pytest.raises(ValueError, match=f"this rank owns {n}"):
        pg.forward(torch.zeros(n - 1, 37))
    with pytest.raises(RuntimeError, match="no CPU"):
        pg.forward(torch.zeros(n, 37))


# ---- hub tables --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_source", [False, True])
def test_hub_tables_tile_each_hub_row_exactly(by_source):
    """`DstCSR.hub_tables` / `transposed_hub_tables` at (8, 5) on the small graph against a numpy restatement: the hubs are the
    rows of at least 8 edges, the segments of a hub tile its edge range exactly, in order, each of 5 edges but a ragged last one"""
    from bridged_gnn_amd import ops
    ei, n = _small()
    THR, SEG = 8, 5
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n))]).astype(np.int32)
    csr = ops.DstCSR(torch.from_numpy(rowptr), torch.from_numpy(ei[0][order].astype(np.int32)), None, ei.shape[1], n)
    if by_source:
        tabs = csr.transposed_hub_tables(THR, SEG)
        rp = csr.transposed()[0].numpy().astype(np.int64)
        assert np.array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n))]))
    else:
        tabs = csr.hub_tables(THR, SEG)
        rp = rowptr.astype(np.int64)
    assert tabs is not None, "the small graph has no row of 8 edges"
    rows, seg_ptr, bounds, seg_node = (t.numpy().astype(np.int64) for t in tabs)
    assert all(t.dtype == torch.int32 for t in tabs)
    deg = rp[1:] - rp[:-1]
    assert np.array_equal(rows, np.nonzero(deg >= THR)[0])
    assert seg_ptr[0] == 0 and seg_ptr.shape[0] == rows.shape[0] + 1 and bounds.shape[0] == 2 * seg_ptr[-1]
    b = bounds.reshape(-1, 2)
    ragged = False
    for h, r in enumerate(rows):
        segs = b[seg_ptr[h]:seg_ptr[h + 1]]
        assert segs.shape[0] == -(-deg[r] // SEG) >= 2
        assert segs[0, 0] == rp[r] and segs[-1, 1] == rp[r + 1]                          # the row's range, exactly
        assert np.array_equal(segs[1:, 0], segs[:-1, 1])                                # in order, no gap, no overlap
        assert ((segs[:-1, 1] - segs[:-1, 0]) == SEG).all() and 1 <= segs[-1, 1] - segs[-1, 0] <= SEG
        ragged = ragged or segs[-1, 1] - segs[-1, 0] < SEG
        assert (seg_node[seg_ptr[h]:seg_ptr[h + 1]] == r).all()
    assert ragged, "no hub of the small graph has a ragged last segment"
    assert ops.DstCSR(torch.from_numpy(rowptr), csr.col, None, ei.shape[1], n).hub_tables(10 ** 6, SEG) is None
