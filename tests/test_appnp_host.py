"""CPU: the APPNP baseline's host side (bridged_gnn_amd.appnp, models/backbones.py:110-128) -- the new C entries are declared and
bound, the new source is built and hashed, APPNP_Net carries the reference's state_dict and draws its parameters in the
reference's order, everything but PyG's defaults is refused, host tensors are refused, and the CLI has step 2's flags plus
--K / --alpha."""
import os
import re
import types

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bgnn_appnp_propagate_workspace_bytes", "bgnn_appnp_propagate_f32", "bgnn_appnp_log_softmax_bwd_f32",
           "bgnn_feature_dropout_f32", "bgnn_feature_dropout_bwd_f32")
DS = types.SimpleNamespace(num_features=37, num_classes=5)


def test_entries_are_declared_bound_and_cite_the_reference():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in bgnn.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    # the propagation has no backward entry: the same call walks the other view
    assert "bgnn_appnp_propagate_bwd_f32" not in code and "bgnn_appnp_propagate_bwd_f32" not in _lib.SIGNATURES
    # the comment blocks in front of the entries cite the reference lines
    for block in re.findall(r"/\*.*?\*/", txt, flags=re.S):
        if "APPNP propagation (" in block or "Feature dropout of APPNP_Net" in block:
            assert "backbones.py:110-128" in block
    assert txt.count("backbones.py:110-128") >= 4
    # argument counts of the binding follow the header
    for name in ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(",") if a.strip()]), name
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)


def test_source_is_built_and_hashed_in_the_same_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "bgnn_appnp.hip" in srcs and "bgnn_appnp.hip" in _lib._HASHED_SOURCES
    assert list(_lib._HASHED_SOURCES[:len(srcs)]) == srcs
    assert os.path.exists(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_appnp.hip"))


def test_state_dict_is_the_reference_layout():
    from bridged_gnn_amd.appnp import APPNP, APPNP_Net
    m = APPNP_Net(DS, hidden=16)
    sd = m.state_dict()
    assert list(sd) == ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"]
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"lin1.weight": (16, 37), "lin1.bias": (16,), "lin2.weight": (5, 16),
                                                          "lin2.bias": (5,)}
    assert isinstance(m.prop1, APPNP) and (m.prop1.K, m.prop1.alpha) == (10, 0.1) and not list(m.prop1.state_dict())
    assert m.dropout == 0.5


def test_parameters_are_drawn_in_the_reference_order():
    from bridged_gnn_amd.appnp import APPNP_Net
    torch.manual_seed(7)
    m = APPNP_Net(DS, hidden=16)
    torch.manual_seed(7)
    l1, l2 = nn.Linear(37, 16), nn.Linear(16, 5)
    for got, want in ((m.lin1.weight, l1.weight), (m.lin1.bias, l1.bias), (m.lin2.weight, l2.weight), (m.lin2.bias, l2.bias)):
        assert torch.equal(got, want)
    torch.manual_seed(7)
    m.reset_parameters()
    assert torch.equal(m.lin1.weight, l1.weight) and torch.equal(m.lin2.bias, l2.bias)


@pytest.mark.parametrize("kw", [dict(dropout=0.1), dict(cached=True), dict(add_self_loops=False), dict(normalize=False)])
def test_non_default_arguments_are_refused(kw):
    from bridged_gnn_amd.appnp import APPNP
    with pytest.raises(NotImplementedError):
        APPNP(10, 0.1, **kw)


def test_edge_weight_is_refused_and_defaults_build():
    from bridged_gnn_amd.appnp import APPNP
    prop = APPNP(10, 0.1, dropout=0., cached=False, add_self_loops=True, normalize=True)
    with pytest.raises(NotImplementedError):
        prop(torch.zeros(2, 3), torch.tensor([[0, 1], [1, 0]]), edge_weight=torch.ones(2))
    import bridged_gnn_amd
    assert bridged_gnn_amd.APPNP is APPNP


def test_host_tensors_are_refused():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.appnp import APPNP, APPNP_Net
    from bridged_gnn_amd.data import Data
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU"):
        APPNP(10, 0.1)(torch.zeros(2, 4), ei)
    with pytest.raises(RuntimeError, match="no CPU"):
        APPNP_Net(DS, hidden=8).eval()(Data(x=torch.zeros(2, 37), edge_index=ei))
    rowptr, col, dinv = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.appnp_propagate(torch.zeros(2, 4), rowptr, col, dinv, 2, 4, 10, 0.1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.appnp_log_softmax_bwd(torch.zeros(2, 4), torch.zeros(2, 4), 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.feature_dropout(torch.zeros(2, 4), 0.5, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.feature_dropout_bwd(torch.zeros(2, 4), 0.5, 1)


def test_cli_defaults_are_step_twos_plus_k_and_alpha():
    from bridged_gnn_amd import appnp, transfer
    a = appnp.build_parser().parse_args([])
    assert (a.K, a.alpha) == (10, 0.1)
    base = transfer.build_parser().parse_args([])
    for k, v in vars(base).items():
        assert getattr(a, k) == v, k
    b = appnp.build_parser().parse_args(["--path_data", "x_bridged_graph.dat", "--to_undirected", "--graphed", "--K", "3",
                                         "--alpha", "0.25"])
    assert b.to_undirected and b.graphed and (b.K, b.alpha, b.path_data) == (3, 0.25, "x_bridged_graph.dat")


def test_graphed_driver_is_refused():
    from bridged_gnn_amd import appnp
    with pytest.raises(NotImplementedError, match="graphed"):
        appnp.train_appnp_noDTC(types.SimpleNamespace(dataset_name="x"), DS, None, graphed=True)


def test_train_gnn_nodtc_is_unchanged():
    """the plain driver keeps its two backbones; APPNP runs through its own driver"""
    import inspect
    from bridged_gnn_amd import appnp, transfer
    assert transfer._FLAGS["baseline"][2] == ("GraphSAGE", "GCN")
    sig = inspect.signature(appnp.train_appnp_noDTC).parameters
    assert (sig["hidden"].default, sig["K"].default, sig["alpha"].default, sig["dropout"].default, sig["graphed"].default,
            sig["history"].default) == (64, 10, 0.1, 0.5, False, None)
