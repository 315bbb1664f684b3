"""CPU: the host side of the partitioned step-2 driver (`dist_transfer`) and of the split-phase BatchNorm entries: the header declares
them and the library exports them, argument errors come back before any launch, the command line is `transfer`'s, rank / world /
device come from the environment, and the modes the driver does not offer are refused before a device is touched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgnn_bn_colstats_f32", "bgnn_bn_apply_rows_f32", "bgnn_bn_bwd_reduce_rows_f32", "bgnn_bn_bwd_apply_rows_f32")


def test_header_declares_and_library_exports_the_split_phase_entries():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(bgnn_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.SO_PATH)
    for n in NEW:
        assert n in declared, f"{n} is not declared in include/bgnn.h"
        assert hasattr(lib, n), f"{n} declared in bgnn.h but not exported"
        assert n in _lib.SIGNATURES
    assert "bgnn_norm.hip" in _lib._HASHED_SOURCES
    assert _lib.lib().bgnn_version() == _lib.ABI_VERSION          # additive entries: the revision did not move
    head = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    assert "models/KTGNN.py:420-430, :364-367" in head


def test_argument_errors_come_back_before_any_launch():
    """BGNN_E_NULL (-1) / BGNN_E_SHAPE (-2) / BGNN_E_ALIGN (-4) from host pointers that are never dereferenced"""
    from bridged_gnn_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                          # 16-byte aligned by the allocator for 512 bytes
    assert ctypes.addressof(buf) % 16 == 0
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    N, D = 8, 8
    # colstats
    assert L.bgnn_bn_colstats_f32(None, N, D, D, p, None) == -1
    assert L.bgnn_bn_colstats_f32(p, N, D, D, None, None) == -1
    for bad_d in (0, 6, 1028):
        assert L.bgnn_bn_colstats_f32(p, N, bad_d, 1028, p, None) == -2
    assert L.bgnn_bn_colstats_f32(p, N, D, 6, p, None) == -2       # ld < D / ld % 4 != 0
    assert L.bgnn_bn_colstats_f32(p, -1, D, D, p, None) == -2
    assert L.bgnn_bn_colstats_f32(odd, N, D, D, p, None) == -4
    # apply: (x, n, D, ldx, totals, n_total, gamma, beta, eps, relu, p, seed, seed_dev, row_ids, row_base, mom, rm, rv, y, ldy, stream)
    ap = lambda x=p, n=N, d=D, tot=p, nt=N, pd=0.5, base=0, rm=None, rv=None, y=p, ldy=D: L.bgnn_bn_apply_rows_f32(
        x, n, d, d if d > 0 else 4, tot, nt, None, None, 1e-5, 1, pd, 7, None, None, base, 0.1, rm, rv, y, ldy, None)
    assert ap(x=None) == -1 and ap(tot=None) == -1 and ap(y=None) == -1
    assert ap(rm=p) == -1 and ap(rv=p) == -1                       # running buffers: both or neither
    assert ap(d=6) == -2 and ap(d=1028) == -2 and ap(ldy=6) == -2
    assert ap(nt=0) == -2 and ap(nt=N - 1) == -2                   # the totals run over at least this rank's rows
    assert ap(pd=1.0) == -2 and ap(pd=-0.1) == -2 and ap(base=-1) == -2
    assert ap(x=odd) == -4 and ap(y=odd) == -4
    # backward reduce / apply
    red = lambda x=p, g=p, tot=p, nt=N, d=D, acc=p: L.bgnn_bn_bwd_reduce_rows_f32(x, g, N, d, d, d, tot, nt, None, None, 1e-5, 1, 0.5, 7, None, None, 0, acc, None)
    assert red(x=None) == -1 and red(g=None) == -1 and red(tot=None) == -1 and red(acc=None) == -1
    assert red(d=12, nt=4) == -2 and red(d=2) == -2 and red(g=odd) == -4
    bw = lambda x=p, g=p, tot=p, gt=p, nt=N, d=D, gx=p: L.bgnn_bn_bwd_apply_rows_f32(x, g, N, d, d, d, tot, gt, nt, None, None, 1e-5, 1, 0.5, 7, None, None, 0, gx, d, None)
    assert bw(x=None) == -1 and bw(g=None) == -1 and bw(tot=None) == -1 and bw(gt=None) == -1 and bw(gx=None) == -1
    assert bw(d=6) == -2 and bw(nt=0) == -2 and bw(gx=odd) == -4


def test_ops_refuse_host_tensors():
    from bridged_gnn_amd import ops
    x = torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.bn_colstats(x)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.bn_apply_rows(x, torch.zeros(16, dtype=torch.float64), 8, None, None, 1e-5, True, 0.5, 1)


def test_command_line_is_transfers():
    from bridged_gnn_amd import dist_transfer, transfer
    assert dist_transfer.build_parser is transfer.build_parser
    a = dist_transfer.build_parser().parse_args(["--num_epoch", "7", "--hidden_dim", "32", "--to_undirected"])
    assert (a.num_epoch, a.hidden_dim, a.to_undirected, a.model_name, a.no_dtc) == (7, 32, True, "KTGNN", False)


def test_rank_world_and_device_come_from_the_environment():
    from bridged_gnn_amd.dist_transfer import ranks_from_env
    env = {"RANK": "5", "WORLD_SIZE": "8", "LOCAL_RANK": "5", "LOCAL_WORLD_SIZE": "8"}
    assert ranks_from_env(env, n_devices=8) == (5, 8, torch.device("cuda", 5), "nccl")
    # two nodes of four GPUs
    env = {"RANK": "6", "WORLD_SIZE": "8", "LOCAL_RANK": "2", "LOCAL_WORLD_SIZE": "4"}
    assert ranks_from_env(env, n_devices=4) == (6, 8, torch.device("cuda", 2), "nccl")
    # ranks sharing one device: RCCL refuses that, the group is gloo
    env = {"RANK": "2", "WORLD_SIZE": "3", "LOCAL_RANK": "2"}
    assert ranks_from_env(env, n_devices=1) == (2, 3, torch.device("cuda", 0), "gloo")
    assert ranks_from_env({}, n_devices=1) == (0, 1, torch.device("cuda", 0), "nccl")
    with pytest.raises(ValueError):
        ranks_from_env({"RANK": "3", "WORLD_SIZE": "3"}, n_devices=8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ranks_from_env({}, n_devices=0)


def test_modes_the_driver_does_not_offer_are_refused_first():
    from bridged_gnn_amd import dist_transfer
    with pytest.raises(NotImplementedError, match="dist_sage / dist_gcn"):
        dist_transfer.main(["--no_dtc"])
    with pytest.raises(NotImplementedError, match="graphed"):
        dist_transfer.main(["--graphed"])
    with pytest.raises(NotImplementedError, match="auc"):
        dist_transfer.main(["--eval_metric", "auc"])
    import types
    with pytest.raises(NotImplementedError, match="auc"):
        dist_transfer.train_gnn_partitioned(types.SimpleNamespace(dataset_name="x"), None, None, 0, 1, "cuda:0", gnn="KTGNN", metric="auc")
    with pytest.raises(NotImplementedError, match="dist_sage / dist_gcn"):
        dist_transfer.train_gnn_partitioned(types.SimpleNamespace(dataset_name="x"), None, None, 0, 1, "cuda:0", gnn="GraphSAGE")
