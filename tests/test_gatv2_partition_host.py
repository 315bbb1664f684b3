"""CPU: the host side of partitioned GATv2 (bridged_gnn_amd.dist_gatv2) -- the one entry per aggregation that takes the ids (ABI
116: no `_rows` twin in the library, the binding or the header), its ctypes binding against the prototype of include/bgnn.h, what `ops.gatv2_aggregate` / `ops.gatv2_aggregate_bwd` refuse
before anything reaches a device (one id array without the other, ids of another dtype or length, host tensors), the package
export and the CPU-device refusal of the driver.  The partition itself is `dist_gat.GatPartition`: tests/test_gat_partition_host.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "float": ctypes.c_float,
         "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def _prototype(name):
    """(restype, argtypes, argument names) of `name` as include/bgnn.h declares it; every pointer is a c_void_p"""
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*)\);", txt, re.M)
    assert m, f"{name} is not declared in bgnn.h"
    types, names = [], []
    for arg in m.group(2).replace("\n", " ").split(","):
        arg = arg.strip()
        names.append(re.search(r"(\w+)$", arg).group(1))
        types.append(ctypes.c_void_p if "*" in arg else CTYPE[arg.replace("const ", "").split()[0]])
    return CTYPE[m.group(1)], types, names


def _one_entry(plain, twin):
    """`plain` is the one entry (exported, bound as bgnn.h declares it) and its former twin is gone from the library, the binding
    and the header -> the argument names of `plain`"""
    from bridged_gnn_amd import _lib
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(lib, plain) and not hasattr(lib, twin), f"{plain} exported, {twin} not"
    assert plain in _lib.SIGNATURES and twin not in _lib.SIGNATURES
    assert twin not in open(os.path.join(ROOT, "include", "bgnn.h")).read(), f"{twin} is still named in bgnn.h"
    res, args, names = _prototype(plain)
    assert (res, args) == (_lib.SIGNATURES[plain][0], list(_lib.SIGNATURES[plain][1])), f"{plain}: SIGNATURES against bgnn.h"
    assert len(names) == len(set(names))
    return names, args


def _abi_116():
    """the library, the binding and the header's revision comment are at 116"""
    from bridged_gnn_amd import _lib
    assert ctypes.CDLL(_lib.SO_PATH).bgnn_version() == 116 == _lib.ABI_VERSION
    head = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    assert "#define BGNN_VERSION 116\n" in head
    note = " ".join(head[head.index("116 is NOT call-compatible with 115"):head.index("#define BGNN_VERSION")].replace("*", " ").split())
    assert "take the ids (and n_src) for every caller; the _rows_ entries are gone" in note
    for name in ("bgnn_sage_mean_aggregate_f32", "bgnn_gcn_aggregate_f32", "bgnn_gat_aggregate_f32", "bgnn_gat_aggregate_bwd_f32",
                 "bgnn_gatv2_aggregate_f32", "bgnn_gatv2_aggregate_bwd_f32"):
        assert name in note, name


def test_rows_entries_are_exported_bound_and_declared():
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    # forward: the two ids sit immediately before the first output (state)
    names, args = _one_entry("bgnn_gatv2_aggregate_f32", "bgnn_gatv2_aggregate_rows_f32")
    assert names[-9:-6] == ["row_id_opt", "edge_base_opt", "state"] and args[-9:-7] == [P, P]
    assert names[-10] == "seed_dev_opt" and len(names) == 28
    # backward: n_src third, after the table's leading dimension; the two ids after the workspace, immediately before g
    names, args = _one_entry("bgnn_gatv2_aggregate_bwd_f32", "bgnn_gatv2_aggregate_bwd_rows_f32")
    assert names[:3] == ["tbl", "ldt", "n_src"] and args[2] is I64
    assert names[-10:-5] == ["ws", "ws_bytes", "row_id_opt", "edge_base_opt", "g"] and args[-8:-6] == [P, P]
    assert len(names) == 37
    _abi_116()


def test_wrapper_keywords_and_refusals():
    from bridged_gnn_amd import ops
    fwd = inspect.signature(ops.gatv2_aggregate).parameters
    bwd = inspect.signature(ops.gatv2_aggregate_bwd).parameters
    assert list(fwd)[-2:] == ["row_ids", "edge_base"] and list(bwd)[-3:] == ["n_rows", "row_ids", "edge_base"]
    assert all(fwd[k].default is None for k in ("row_ids", "edge_base"))
    assert all(bwd[k].default is None for k in ("n_rows", "row_ids", "edge_base"))
    n, H, C = 4, 1, 4
    ids, T, att = torch.zeros(n, dtype=torch.int64), torch.zeros(n, 8), torch.zeros(1, 1, 4)
    rp, col = torch.zeros(n + 1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    state, rows = torch.zeros(n, 1, 2), torch.zeros(n, 4)

    def f(**kw):
        return ops.gatv2_aggregate(T, att, rp, col, n, H, C, **kw)

    def b(**kw):
        return ops.gatv2_aggregate_bwd(T, att, state, rows, rows, rp, col, rp, col, col, H, C, **kw)

    for call in (f, b):
        # the ids are given together: one alone is refused before anything reaches the device
        for kw in (dict(row_ids=ids), dict(edge_base=ids)):
            with pytest.raises(ValueError, match="together"):
                call(**kw)
        # dtype and length
        with pytest.raises(ValueError, match="row_ids must be a contiguous torch.int64 tensor of shape"):
            call(row_ids=ids.int(), edge_base=ids)
        with pytest.raises(ValueError, match="edge_base must be a contiguous torch.int64 tensor of shape"):
            call(row_ids=ids, edge_base=ids.float())
        with pytest.raises(ValueError, match=r"row_ids must be .* shape \(4,\)"):
            call(row_ids=ids[:3], edge_base=ids)
        with pytest.raises(ValueError, match=r"edge_base must be .* shape \(4,\)"):
            call(row_ids=ids, edge_base=torch.zeros(n + 1, dtype=torch.int64))
        # host tensors: there is no CPU path, with ids or without
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(row_ids=ids, edge_base=ids)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    # the backward's ids are over n_rows, and n_rows lies inside the table
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        b(n_rows=3, row_ids=ids, edge_base=ids)
    with pytest.raises(ValueError, match="n_rows = 5 must lie in"):
        b(n_rows=5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        b(n_rows=3, row_ids=ids[:3].contiguous(), edge_base=ids[:3].contiguous())


def test_package_export_and_cpu_device_refusal():
    import bridged_gnn_amd
    from bridged_gnn_amd import PartitionedGATv2, dist_gatv2
    from bridged_gnn_amd.gatv2 import GATv2
    assert PartitionedGATv2 is dist_gatv2.PartitionedGATv2 and bridged_gnn_amd.PartitionedGATv2 is dist_gatv2.PartitionedGATv2
    for name in ("forward", "nll_loss", "sync_grads", "invalidate_input_cache"):
        assert callable(getattr(PartitionedGATv2, name))
    assert not hasattr(PartitionedGATv2, "get_emb"), "the model has none"
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 0]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        PartitionedGATv2(GATv2(8, 4, 3, 2, 2, 0.0, 0.0), ei, 4, 0, 1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        PartitionedGATv2(GATv2(8, 4, 3, 2, 2, 0.0, 0.0), ei.numpy(), 4, 0, 2, torch.device("cpu"))
