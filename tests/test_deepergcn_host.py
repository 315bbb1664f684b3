"""CPU: the DeeperGCN baseline's host side (bridged_gnn_amd.deepergcn, models/backbones.py:130-161) -- the three new C entries are
declared, bound and argument-counted at ABI 116 and cite the reference, the new source is built and hashed at one position,
DeeperGCN carries the reference's state_dict at 1 and 3 layers and draws its parameters in the reference's order, every
configuration the layers do not implement is refused, the ops validate what can be validated without a device and refuse host
tensors, `graphed=True` is refused and the CLI has step 2's flags with --num_layer 3 / --hidden_dim 64 plus --dropout."""
import inspect
import os
import re
import types

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bgnn_gen_softmax_aggregate_f32", "bgnn_gen_softmax_aggregate_workspace_bytes", "bgnn_gen_softmax_aggregate_bwd_f32")
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
    blocks = [b for b in re.findall(r"/\*.*?\*/", txt, flags=re.S) if "bgnn_gen_softmax_aggregate_bwd_f32 (" in b]
    assert blocks and all(b.count("backbones.py:130-161") >= 2 for b in blocks)      # the forward's and the backward's citation
    assert _lib.ABI_VERSION == 116 and re.search(r"#define\s+BGNN_VERSION\s+116\b", txt)          # additive: the revision stays
    src = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "bgnn_gen.hip")).read()
    for name in ENTRIES:
        assert re.search(r'extern "C" \w+ ' + name + r"\(", src), name
    assert "bgnn_conv_common.h" in src and "lf_ladder" in src and "clamp_row" in src and "atomicAdd" not in src
    # the temperature is a device pointer in both entries
    for name in (ENTRIES[0], ENTRIES[2]):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1)
        assert re.search(r"const\s+float\s*\*\s*t\b", decl), name


def test_source_is_built_and_hashed_in_the_same_position():
    from bridged_gnn_amd import _lib
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "bgnn_gen.hip" in srcs and "bgnn_gen.hip" in _lib._HASHED_SOURCES
    assert srcs.index("bgnn_gen.hip") == _lib._HASHED_SOURCES.index("bgnn_gen.hip")
    assert list(_lib._HASHED_SOURCES[:len(srcs)]) == srcs


def _want_keys(L, H=16):
    want = {"node_encoder.weight": (H, 37), "node_encoder.bias": (H,)}
    for i in range(L):
        c = f"layers.{i}.conv."
        want.update({c + "t": (1,), c + "mlp.0.weight": (2 * H, H), c + "mlp.0.bias": (2 * H,), c + "mlp.1.weight": (2 * H,),
                     c + "mlp.1.bias": (2 * H,), c + "mlp.4.weight": (H, 2 * H), c + "mlp.4.bias": (H,),
                     f"layers.{i}.norm.weight": (H,), f"layers.{i}.norm.bias": (H,)})
    want.update({"lin.weight": (5, H), "lin.bias": (5,)})
    return want


@pytest.mark.parametrize("L", [1, 3])
def test_state_dict_is_the_reference_layout(L):
    import bridged_gnn_amd
    from bridged_gnn_amd.deepergcn import DeepGCNLayer, DeeperGCN, GENConv
    m = DeeperGCN(DS, 16, L)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == _want_keys(L)
    # the reference's order: node_encoder, the layers (conv before norm; a module's own t before its children's), lin
    assert list(sd)[:2] == ["node_encoder.weight", "node_encoder.bias"] and list(sd)[-2:] == ["lin.weight", "lin.bias"]
    assert list(sd)[2:11] == ["layers.0.conv.t"] + [f"layers.0.conv.mlp.{k}.{w}" for k in (0, 1, 4) for w in ("weight", "bias")] + \
        ["layers.0.norm.weight", "layers.0.norm.bias"]
    assert m.dropout == 0.1 and len(m.layers) == L
    for i, layer in enumerate(m.layers):
        assert isinstance(layer, DeepGCNLayer) and isinstance(layer.conv, GENConv) and isinstance(layer.norm, nn.LayerNorm)
        assert layer.block == "res+" and layer.dropout == 0.1 and layer.ckpt_grad == (i + 1) % 3
        assert layer.conv.t.requires_grad and layer.conv.t.item() == 1.0
        assert isinstance(layer.conv.mlp[2], nn.ReLU) and isinstance(layer.conv.mlp[3], nn.Dropout) and layer.conv.mlp[3].p == 0.0
    assert bridged_gnn_amd.DeeperGCN is DeeperGCN and bridged_gnn_amd.GENConv is GENConv and bridged_gnn_amd.DeepGCNLayer is DeepGCNLayer
    assert bridged_gnn_amd.train_deepergcn_noDTC.__module__ == "bridged_gnn_amd.deepergcn"


def test_reset_parameters_redraws_every_member_and_restores_t():
    """node_encoder, every layer's conv (mlp and t) and norm, then lin, in that order: the same seed gives the same draw, and the
    order is the restated one (PyG's GENConv draws its mlp in the constructor and again in its own reset_parameters, so a fresh
    model is NOT what one reset gives)"""
    from bridged_gnn_amd.deepergcn import DeeperGCN
    from bridged_gnn_amd.ktgnn import Linear
    m = DeeperGCN(DS, 16, 2)
    with torch.no_grad():
        for layer in m.layers:
            layer.conv.t.fill_(3.0)
            layer.norm.weight.fill_(2.0)
            layer.conv.mlp[1].bias.fill_(2.0)
    torch.manual_seed(7)
    m.reset_parameters()
    torch.manual_seed(7)
    enc = Linear(37, 16)
    mlps = [[nn.Linear(16, 32), nn.Linear(32, 16)] for _ in range(2)]
    lin = Linear(16, 5)
    sd = m.state_dict()
    assert torch.equal(sd["node_encoder.weight"], enc.weight) and torch.equal(sd["node_encoder.bias"], enc.bias)
    assert torch.equal(sd["lin.weight"], lin.weight) and torch.equal(sd["lin.bias"], lin.bias)
    for i, (a, b) in enumerate(mlps):
        c = f"layers.{i}.conv."
        assert torch.equal(sd[c + "mlp.0.weight"], a.weight) and torch.equal(sd[c + "mlp.0.bias"], a.bias)
        assert torch.equal(sd[c + "mlp.4.weight"], b.weight) and torch.equal(sd[c + "mlp.4.bias"], b.bias)
        assert float(sd[c + "t"]) == 1.0
        assert bool((sd[c + "mlp.1.weight"] == 1).all()) and bool((sd[c + "mlp.1.bias"] == 0).all())
        assert bool((sd[f"layers.{i}.norm.weight"] == 1).all()) and bool((sd[f"layers.{i}.norm.bias"] == 0).all())


@pytest.mark.parametrize("kw", [dict(aggr="power"), dict(aggr="add"), dict(msg_norm=True), dict(learn_p=True), dict(learn_t=False),
                                dict(norm="batch"), dict(num_layers=3), dict(eps=1e-6)])
def test_unsupported_genconv_configurations_raise(kw):
    from bridged_gnn_amd.deepergcn import GENConv
    cfg = dict(aggr="softmax", t=1.0, learn_t=True, num_layers=2, norm="layer")
    GENConv(8, 8, **cfg)
    cfg.update(kw)
    with pytest.raises(NotImplementedError):
        GENConv(8, 8, **cfg)


def test_unsupported_calls_and_blocks_raise():
    from bridged_gnn_amd.deepergcn import DeepGCNLayer, GENConv
    conv = GENConv(8, 8, aggr="softmax", t=1.0, learn_t=True, num_layers=2, norm="layer")
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(2, 8), ei, edge_attr=torch.zeros(2, 8))
    for block in ("res", "dense", "plain"):
        with pytest.raises(NotImplementedError):
            DeepGCNLayer(conv, nn.LayerNorm(8), nn.ReLU(), block=block)
    with pytest.raises(NotImplementedError):
        DeepGCNLayer(conv, nn.LayerNorm(8), nn.ELU(), block="res+")
    DeepGCNLayer(conv, nn.LayerNorm(8), nn.ReLU(inplace=True), block="res+", dropout=0.1, ckpt_grad=2)       # accepted and ignored


def test_host_tensors_are_refused():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.deepergcn import DeepGCNLayer, DeeperGCN, GENConv
    ei = torch.tensor([[0, 1], [1, 0]])
    conv = GENConv(4, 4, aggr="softmax", t=1.0, learn_t=True, num_layers=2, norm="layer")
    with pytest.raises(RuntimeError, match="no CPU"):
        conv(torch.zeros(2, 4), ei)
    with pytest.raises(RuntimeError, match="no CPU"):
        DeepGCNLayer(conv, nn.LayerNorm(4), nn.ReLU())(torch.zeros(2, 4), ei)
    with pytest.raises(RuntimeError, match="no CPU"):
        DeeperGCN(DS, 8, 2).eval()(Data(x=torch.zeros(2, 37), edge_index=ei))
    rowptr, col, t = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32), torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gen_softmax_aggregate(torch.zeros(2, 4), rowptr, col, t, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.gen_softmax_aggregate_bwd(torch.zeros(2, 4), torch.zeros(2, 4), (torch.zeros(2, 4), torch.zeros(2, 4)), rowptr, col, t, 4)


def test_width_is_validated_before_anything_else():
    from bridged_gnn_amd import ops
    with pytest.raises(ValueError, match="H >= 1"):
        ops.gen_softmax_aggregate(None, None, None, None, 2, 0)
    with pytest.raises(ValueError, match="H >= 1"):
        ops.gen_softmax_aggregate_bwd(None, None, (None, None), None, None, None, 0)
    sig = inspect.signature(ops.gen_softmax_aggregate).parameters
    assert list(sig)[:7] == ["x", "rowptr", "col", "t", "n_rows", "H", "save"] and sig["save"].default is None
    for fn in (ops.gen_softmax_aggregate, ops.gen_softmax_aggregate_bwd):
        assert "backbones.py:130-161" in fn.__doc__ and "bgnn.h" in fn.__doc__


def test_cli_defaults_are_step_twos_with_three_layers_of_64():
    from bridged_gnn_amd import deepergcn, transfer
    a = deepergcn.build_parser().parse_args([])
    assert (a.num_layer, a.hidden_dim, a.dropout) == (3, 64, 0.1)
    base = transfer.build_parser().parse_args([])
    for k, v in vars(base).items():
        if k not in ("num_layer", "hidden_dim"):
            assert getattr(a, k) == v, k
    b = deepergcn.build_parser().parse_args(["--path_data", "x_bridged_graph.dat", "--to_undirected", "--graphed", "--num_layer", "5",
                                             "--hidden_dim", "128", "--dropout", "0.2"])
    assert b.to_undirected and b.graphed and (b.num_layer, b.hidden_dim, b.dropout, b.path_data) == (5, 128, 0.2, "x_bridged_graph.dat")


def test_graphed_driver_is_refused():
    from bridged_gnn_amd import deepergcn
    with pytest.raises(NotImplementedError, match="graphed"):
        deepergcn.train_deepergcn_noDTC(types.SimpleNamespace(dataset_name="x"), DS, None, graphed=True)
    sig = inspect.signature(deepergcn.train_deepergcn_noDTC).parameters
    assert (sig["num_layer"].default, sig["hidden"].default, sig["dropout"].default, sig["graphed"].default,
            sig["history"].default) == (3, 64, 0.1, False, None)
