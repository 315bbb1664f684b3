"""CPU: the partitioned GCNII baseline's host side (bridged_gnn_amd.dist_gcn2) -- the additive C entry bgnn_gcn2_conv_rows_f32 is
declared (citing the reference), bound with the header's argument count and defined at ABI 116 while bgnn_gcn2_conv_f32 keeps its
argument list; the class is exported lazily; what needs no GPU to be refused is refused; and on a 12-node hand-written graph the
rank's tables hold every owned row's in-edges plus one self loop, with the fp64-then-fp32 global deg^-1/2 at `ext_global()`."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "bgnn_gcn2_conv_rows_f32"
DS = types.SimpleNamespace(num_features=6, num_classes=3)


def _decl_args(code, name):
    decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert decl, f"{name} is not declared in bgnn.h"
    return [a.strip() for a in decl.group(1).split(",") if a.strip()]


def test_entry_is_declared_bound_defined_and_the_abi_stays():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    args = _decl_args(code, ENTRY)
    assert ENTRY in _lib.SIGNATURES, f"{ENTRY} is not bound in _lib.SIGNATURES"
    assert len(_lib.SIGNATURES[ENTRY][1]) == len(args)
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if "RECTANGULAR graph (GCN2" in b]
    assert len(blocks) == 1 and "backbones.py:163-197" in blocks[0] and "row_ids_opt" in blocks[0] and "n_tbl" in blocks[0]
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)
    # the square entry keeps its 28 arguments; the new one takes n_tbl and row_ids_opt next to them
    old = _decl_args(code, "bgnn_gcn2_conv_f32")
    assert len(old) == 28 == len(_lib.SIGNATURES["bgnn_gcn2_conv_f32"][1]) and len(args) == 30
    names = lambda decl: [a.split()[-1].lstrip("*") for a in decl]
    assert [a for a in names(args) if a not in names(old)] == ["n_tbl", "row_ids_opt"]
    assert [a for a in names(args) if a in names(old)] == names(old)
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_gcn2.hip")).read()
    for name in (ENTRY, "bgnn_gcn2_conv_f32"):
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    assert src.count("dispatch_conv<MODE_ROWS>") == 1, "both entries share one launch sequence"
    assert "atomicAdd" not in src


def test_export_and_refusals():
    import bridged_gnn_amd
    from bridged_gnn_amd import dist_gcn2, ops
    from bridged_gnn_amd.gcn2 import GCN2
    assert bridged_gnn_amd.PartitionedGCN2 is dist_gcn2.PartitionedGCN2
    ei, n = _multigraph()
    with pytest.raises(RuntimeError, match="no CPU"):
        dist_gcn2.PartitionedGCN2(GCN2(DS, 8, 2, 0.1, 0.5), ei, n, 0, 1, "cpu")
    with pytest.raises(NotImplementedError, match="graphed"):
        dist_gcn2.PartitionedGCN2(GCN2(DS, 8, 2, 0.1, 0.5), ei, n, 0, 1, "cuda:0", graphed=True)
    with pytest.raises(NotImplementedError):
        GCN2(DS, 8, 2, 0.1, 0.5, shared_weights=False)
    rowptr, col, dinv = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU"):                     # a rectangular call with ids, host tensors
        ops.gcn2_conv(torch.zeros(3, 4), torch.zeros(2, 4), torch.eye(4), rowptr, col, dinv, 2, 4, 0.1, row_ids=torch.arange(2))
    with pytest.raises(ValueError, match="H <= 128"):
        ops.gcn2_conv(None, None, None, None, None, None, 2, 129, 0.1, row_ids=None)


def _multigraph():
    """12 nodes: duplicate edges, input self loops (one of them twice), a node without in-edges, one without out-edges; asymmetric"""
    e = [(0, 1), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (0, 10), (1, 10), (10, 0),
         (3, 3), (3, 3), (7, 7), (2, 9), (9, 2), (9, 2), (4, 0), (5, 0), (6, 1), (8, 1), (10, 5), (2, 6), (11, 4)]
    return np.array(e, dtype=np.int64).T, 12


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("owners", ["blocks", "scattered"])
def test_rank_tables_hold_the_owned_rows_of_the_normalised_graph(world, owners):
    """what `PartitionedGCN2` builds on the host (`dist_gcn.GcnPartition`, the partition of `PartitionedGCN`)"""
    from bridged_gnn_amd import dist_gcn2
    assert dist_gcn2.GcnPartition.__module__ == "bridged_gnn_amd.dist_gcn"
    ei, n = _multigraph()
    owner = None if owners == "blocks" else (np.arange(n) * 7 % world).astype(np.int32)
    nl = ei[:, ei[0] != ei[1]]
    deg = np.bincount(nl[1], minlength=n).astype(np.float64) + 1.0
    dinv = (1.0 / np.sqrt(deg)).astype(np.float32)                          # fp64, then rounded
    seen = np.zeros(n, dtype=np.int64)
    for r in range(world):
        part = dist_gcn2.GcnPartition(ei, n, r, world, owner=owner)
        ext = part.ext_global()
        assert ext.shape == (part.n_ext,) and part.n_ext == part.n_local + part.n_halo
        seen[part.owned_global] += 1
        for i, gid in enumerate(part.owned_global):
            got = sorted(ext[part.col[part.rowptr[i]:part.rowptr[i + 1]]].tolist())
            want = sorted(nl[0][nl[1] == gid].tolist() + [int(gid)])          # the in-edges (duplicates kept) plus ONE self loop
            assert got == want, (r, gid)
            assert part.col[part.rowptr[i + 1] - 1] == i                     # the self loop closes the row
        assert part.dinv_ext.dtype == np.float32 and np.array_equal(part.dinv_ext, dinv[ext])
        assert (part.rowptr[part.n_local:] == part.rowptr[part.n_local]).all()        # halo slots have no in-edges
        assert sorted(part.halo_global.tolist()) == sorted(set(ext[part.col].tolist()) - set(part.owned_global.tolist()))
    assert (seen == 1).all()
