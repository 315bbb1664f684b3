"""CPU: the partitioned APPNP baseline's host side (bridged_gnn_amd.dist_appnp) -- the three additive C entries are declared and
bound with equal argument counts at ABI 116; the transposed partition holds exactly the flipped edges of A' + I, once each, under
the forward partition's owners and with the forward partition's (in-degree) factors; and what is out of scope is refused."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bgnn_appnp_step_f32", "bgnn_feature_dropout_rows_f32", "bgnn_feature_dropout_rows_bwd_f32")
DS = types.SimpleNamespace(num_features=6, num_classes=3)


def test_entries_are_declared_bound_and_the_abi_stays():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert decl, f"{name} is not declared in bgnn.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.group(1).split(",") if a.strip()]), name
    for block in re.findall(r"/\*.*?\*/", txt, flags=re.S):
        if "One step of the APPNP propagation" in block or "on a rank's rows of a partitioned activation" in block:
            assert "backbones.py:110-128" in block
    assert txt.count("backbones.py:110-128") >= 6
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_appnp.hip")).read()
    for name in ENTRIES:
        assert re.search(r'extern "C" int ' + name + r"\(", src), name


def _multigraph():
    """12 nodes: duplicate edges, input self loops (one of them twice), a node without in-edges, one without out-edges; asymmetric"""
    e = [(0, 1), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (0, 10), (1, 10), (10, 0),
         (3, 3), (3, 3), (7, 7), (2, 9), (9, 2), (9, 2), (4, 0), (5, 0), (6, 1), (8, 1), (10, 5), (2, 6), (11, 4)]
    return np.array(e, dtype=np.int64).T, 12


def _global_edges(part):
    """(src, dst) global ids of every edge of a partition's owned rows"""
    ext = part.ext_global()
    rows = np.repeat(np.arange(part.n_local), np.diff(part.rowptr[:part.n_local + 1]))
    return np.stack([ext[part.col[:rows.shape[0]]], part.owned_global[rows]])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("owners", ["blocks", "scattered"])
def test_transposed_partition(world, owners):
    from bridged_gnn_amd.dist_appnp import AppnpPartition
    ei, n = _multigraph()
    owner = None if owners == "blocks" else (np.arange(n) * 7 % world).astype(np.int32)
    nl = ei[:, ei[0] != ei[1]]
    loops = np.arange(n)
    full = np.concatenate([nl, np.stack([loops, loops])], axis=1)             # A' + I, duplicates kept
    want_t = sorted(map(tuple, full[::-1].T.tolist()))                         # its flipped edges
    deg = np.bincount(nl[1], minlength=n) + 1.0
    dinv = (1.0 / np.sqrt(deg)).astype(np.float32)
    parts = [AppnpPartition(ei, n, r, world, owner=owner) for r in range(world)]
    got_f, got_t, seen = [], [], np.zeros(n, dtype=np.int64)
    for p in parts:
        assert sorted(p.owned_global.tolist()) == sorted(p.t.owned_global.tolist())      # the same owned set, maybe another order
        assert np.array_equal(p.owned_global[p.t_from_f], p.t.owned_global)
        assert np.array_equal(p.t.owned_global[p.f_from_t], p.owned_global)
        seen[p.owned_global] += 1
        got_f += map(tuple, _global_edges(p).T.tolist())
        got_t += map(tuple, _global_edges(p.t).T.tolist())
        # the factors of the ORIGINAL graph's in-degrees on both partitions, halo slots included
        assert np.array_equal(p.dinv_ext, dinv[p.ext_global()])
        assert np.array_equal(p.t.dinv_ext, dinv[p.t.ext_global()])
        assert p.t.dinv_ext.dtype == np.float32 and p.t.dinv_ext.shape == (p.t.n_ext,)
        # every row of either partition ends in its self loop
        for q in (p, p.t):
            last = q.col[q.rowptr[1:q.n_local + 1] - 1]
            assert np.array_equal(last, np.arange(q.n_local))
    assert (seen == 1).all()
    assert sorted(got_f) == sorted(map(tuple, full.T.tolist()))
    assert sorted(got_t) == want_t
    out_deg = np.bincount(nl[0], minlength=n) + 1.0
    assert not np.array_equal(out_deg, deg), "the flipped graph's own degrees differ on this graph"
    if world > 1:
        assert sum(p.n_halo for p in parts) > 0 and sum(p.t.n_halo for p in parts) > 0


def test_refusals():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.appnp import APPNP_Net
    from bridged_gnn_amd.dist_appnp import PartitionedAPPNP
    import bridged_gnn_amd
    assert bridged_gnn_amd.PartitionedAPPNP is PartitionedAPPNP
    ei, n = _multigraph()
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedAPPNP(APPNP_Net(DS, hidden=8), ei, n, 0, 1, "cpu")
    with pytest.raises(NotImplementedError, match="graphed"):
        PartitionedAPPNP(APPNP_Net(DS, hidden=8), ei, n, 0, 1, "cuda:0", graphed=True)
    with pytest.raises(NotImplementedError, match="128 classes"):
        PartitionedAPPNP(APPNP_Net(types.SimpleNamespace(num_features=6, num_classes=129), hidden=8), ei, n, 0, 1, "cuda:0")
    rowptr, col, dinv = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.appnp_step(torch.zeros(3, 4), torch.zeros(2, 4), rowptr, col, dinv, 2, 4, 0.1, True, "state")
    ids = torch.arange(2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.feature_dropout(torch.zeros(2, 4), 0.5, 1, row_ids=ids)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.feature_dropout_bwd(torch.zeros(2, 4), 0.5, 1, row_ids=ids)


def test_dist_transfer_refusals_are_unchanged():
    from bridged_gnn_amd import dist_transfer
    src = open(dist_transfer.__file__).read()
    assert "the plain backbones train on a partition through bridged_gnn_amd.dist_sage / dist_gcn" in src
    assert "KTGNN only; GraphSAGE and GCN train on a partition through" in src
