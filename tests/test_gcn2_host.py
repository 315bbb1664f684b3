"""CPU: the GCNII baseline's host side (bridged_gnn_amd.gcn2, models/backbones.py:163-197) -- the new C entries are declared, bound
and argument-counted at ABI 116, the new source is built and hashed at one position, GCN2 carries the reference's state_dict and
draws its parameters in the reference's order (lins, then convs; weight1 by glorot), beta follows PyG's rule, everything the
layer does not implement is refused, host tensors are refused, `graphed=True` is refused and the CLI has step 2's flags plus
--alpha / --theta / --dropout."""
import math
import os
import re
import types

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bgnn_gcn2_conv_workspace_bytes", "bgnn_gcn2_conv_f32", "bgnn_gcn2_conv_bwd_f32")
DS = types.SimpleNamespace(num_features=37, num_classes=5)


def test_entries_are_declared_bound_and_cite_the_reference():
    from bridged_gnn_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in bgnn.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(",") if a.strip()]), name
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if "bgnn_gcn2_conv_bwd_f32 (" in b]
    assert blocks and all(b.count("backbones.py:163-197") >= 2 for b in blocks)      # the forward's and the backward's citation
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)
    # the library's source defines what the header declares
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_gcn2.hip")).read()
    for name in ENTRIES:
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in src and "bgnn_conv_common.h" in src and "atomicAdd" not in src


def test_source_is_built_and_hashed_in_the_same_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "bgnn_gcn2.hip" in srcs and "bgnn_gcn2.hip" in _lib._HASHED_SOURCES
    assert srcs.index("bgnn_gcn2.hip") == _lib._HASHED_SOURCES.index("bgnn_gcn2.hip")
    assert list(_lib._HASHED_SOURCES[:len(srcs)]) == srcs


def test_state_dict_is_the_reference_layout():
    from bridged_gnn_amd.gcn2 import GCN2, GCN2Conv
    m = GCN2(DS, 16, 3, 0.1, 0.5, dropout=0.25)
    sd = m.state_dict()
    assert list(sd) == ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias", "convs.0.weight1", "convs.1.weight1",
                        "convs.2.weight1"]
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "lins.0.weight": (16, 37), "lins.0.bias": (16,), "lins.1.weight": (5, 16), "lins.1.bias": (5,),
        "convs.0.weight1": (16, 16), "convs.1.weight1": (16, 16), "convs.2.weight1": (16, 16)}
    assert all(isinstance(c, GCN2Conv) and c.alpha == 0.1 and c.weight2 is None for c in m.convs)
    assert [c.beta for c in m.convs] == [math.log(0.5 / (l + 1) + 1) for l in range(3)]
    assert m.dropout == 0.25
    import bridged_gnn_amd
    assert bridged_gnn_amd.GCN2 is GCN2 and bridged_gnn_amd.GCN2Conv is GCN2Conv
    assert bridged_gnn_amd.train_gcn2_noDTC.__module__ == "bridged_gnn_amd.gcn2"


def test_parameters_are_drawn_in_the_reference_order():
    from bridged_gnn_amd.gcn2 import GCN2

    def restated():
        l0, l1 = nn.Linear(37, 16), nn.Linear(16, 5)                     # lins first ...
        a = math.sqrt(6.0 / (16 + 16))
        ws = [torch.empty(16, 16).uniform_(-a, a) for _ in range(2)]     # ... then every conv's weight1 by glorot
        return [l0.weight, l0.bias, l1.weight, l1.bias] + ws
    torch.manual_seed(7)
    m = GCN2(DS, 16, 2, 0.1, 0.5)
    torch.manual_seed(7)
    want = restated()
    got = [m.lins[0].weight, m.lins[0].bias, m.lins[1].weight, m.lins[1].bias, m.convs[0].weight1, m.convs[1].weight1]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    torch.manual_seed(7)
    m.reset_parameters()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("theta,layer", [(0.5, 1), (0.5, 4), (1.0, 2), (1.5, 64), (None, None)])
def test_beta(theta, layer):
    from bridged_gnn_amd.gcn2 import GCN2Conv
    c = GCN2Conv(8, 0.2, theta, layer)
    assert c.beta == (1.0 if theta is None else math.log(theta / layer + 1)) and c.alpha == 0.2
    assert list(c.state_dict()) == ["weight1"] and c.weight1.shape == (8, 8)


@pytest.mark.parametrize("kw", [dict(shared_weights=False), dict(cached=True)])
def test_non_default_arguments_are_refused(kw):
    from bridged_gnn_amd.gcn2 import GCN2, GCN2Conv
    with pytest.raises(NotImplementedError):
        GCN2Conv(8, 0.1, 0.5, 1, **kw)
    if "shared_weights" in kw:
        with pytest.raises(NotImplementedError):
            GCN2(DS, 8, 2, 0.1, 0.5, shared_weights=False)


def test_normalize_is_accepted_either_way():
    from bridged_gnn_amd.gcn2 import GCN2Conv
    GCN2Conv(8, 0.1, 0.5, 1, normalize=False)
    GCN2Conv(8, 0.1, 0.5, 1, normalize=True)
    with pytest.raises(NotImplementedError):
        GCN2Conv(8, 0.1)(torch.zeros(2, 8), torch.zeros(2, 8), torch.tensor([[0, 1], [1, 0]]), edge_weight=torch.ones(2))


def test_host_tensors_are_refused():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.gcn2 import GCN2, GCN2Conv
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU"):
        GCN2Conv(4, 0.1, 0.5, 1)(torch.zeros(2, 4), torch.zeros(2, 4), ei)
    with pytest.raises(RuntimeError, match="no CPU"):
        GCN2Conv(4, 0.1, 0.5, 1).run(torch.zeros(2, 4), torch.zeros(2, 4), None)
    with pytest.raises(RuntimeError, match="no CPU"):
        GCN2(DS, 8, 2, 0.1, 0.5).eval()(Data(x=torch.zeros(2, 37), edge_index=ei))
    rowptr, col, dinv = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gcn2_conv(torch.zeros(2, 4), torch.zeros(2, 4), torch.eye(4), rowptr, col, dinv, 2, 4, 0.1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gcn2_conv_bwd(torch.zeros(2, 4), torch.zeros(2, 4), torch.eye(4), 4, 0.1, 0.0)


def test_envelope_of_the_ops():
    from bridged_gnn_amd import ops
    assert [ops.gcn2_supported(h) for h in (0, 1, 5, 128, 129)] == [False, True, True, True, False]
    with pytest.raises(ValueError, match="H <= 128"):
        ops.gcn2_conv(None, None, None, None, None, None, 2, 129, 0.1)
    with pytest.raises(ValueError, match="H <= 128"):
        ops.gcn2_conv_bwd(None, None, None, 0, 0.1, 0.0)


def test_cli_defaults_are_step_twos_plus_alpha_theta_and_dropout():
    from bridged_gnn_amd import gcn2, transfer
    a = gcn2.build_parser().parse_args([])
    assert (a.alpha, a.theta, a.dropout) == (0.1, 0.5, 0.5)
    base = transfer.build_parser().parse_args([])
    for k, v in vars(base).items():
        assert getattr(a, k) == v, k
    b = gcn2.build_parser().parse_args(["--path_data", "x_bridged_graph.dat", "--to_undirected", "--graphed", "--alpha", "0.25",
                                        "--theta", "1.5", "--dropout", "0.1"])
    assert b.to_undirected and b.graphed and (b.alpha, b.theta, b.dropout, b.path_data) == (0.25, 1.5, 0.1, "x_bridged_graph.dat")


def test_graphed_driver_is_refused():
    import inspect
    from bridged_gnn_amd import gcn2
    with pytest.raises(NotImplementedError, match="graphed"):
        gcn2.train_gcn2_noDTC(types.SimpleNamespace(dataset_name="x"), DS, None, graphed=True)
    sig = inspect.signature(gcn2.train_gcn2_noDTC).parameters
    assert (sig["num_layer"].default, sig["hidden"].default, sig["alpha"].default, sig["theta"].default, sig["dropout"].default,
            sig["graphed"].default, sig["history"].default) == (2, 64, 0.1, 0.5, 0.5, False, None)
