"""CPU: step 1's driver (`bridged_gnn_amd.bridged_graph`): flag table, `prepare_datasets`, the refusal of the fused filters on host
tensors, and the C ABI of csrc/bgnn_edge_filter.hip."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# main_bridged_graph.py:361-387: name -> (default, choices)
REFERENCE_FLAGS = {
    "gpu": (0, None), "dataset_name": ("twitter_unrelational", None), "save": (False, None), "check_within": (False, None),
    "check_cross": (False, None), "norm_mode": ("None", None), "version": ("v1", ["v1", "v2"]), "norm_scale": (1.0, None),
    "num_epoch": (400, None), "start_eval_epoch": (300, None), "eval_per_epoch": (1, None), "num_layer": (2, None),
    "hidden_dim": (64, None), "sim_mode": ("mlp", ["cosine", "mlp"]), "backbone": ("mlp", ["gnn", "mlp"]), "seed": (0, None),
    "epsilon": (0.5, None), "thres_conf_quantile": (0.1, None), "thres_feat_sim": (0.8, None), "k_within": (6, None),
    "k_cross": (20, None), "batch_size": (1000, None), "repeat": (1, None), "max_class_num": (10, None),
    "eval_mode": ("sampling", ["all", "sampling"]), "sample_size": (40000, None),
}
OWN_FLAGS = {"data_root": "../datasets", "path_dataset": None, "ckpt_dir": "../ckpt", "out_dir": "../data_bridged_graph",
             "skip_train": False, "reference_filter_quirk": False, "no_fused": False, "quiet": False}


def test_parser_carries_the_reference_flags():
    from bridged_gnn_amd.bridged_graph import build_parser
    ap = build_parser()
    actions = {a.dest: a for a in ap._actions if a.dest != "help"}
    assert set(actions) == set(REFERENCE_FLAGS) | set(OWN_FLAGS)
    for name, (default, choices) in REFERENCE_FLAGS.items():
        a = actions[name]
        assert a.default == default and type(a.default) is type(default), name
        assert (list(a.choices) if a.choices is not None else None) == choices, name
    for name, default in OWN_FLAGS.items():
        assert actions[name].default == default, name
    ns = ap.parse_args(["--hidden_dim", "128", "--k_within", "3", "--save", "--dataset_name", "office_amazon2dslr", "--version", "v2",
                        "--check_within", "--check_cross"])                        # a line of the reference's run.sh
    assert (ns.hidden_dim, ns.k_within, ns.k_cross, ns.save, ns.version, ns.check_cross) == (128, 3, 20, True, "v2", True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--version", "v3"])


def write_office_standin(path, mask_name="central_mask"):
    """the office A->D stand-in as a VS-graph .dat: fixture x / y / masks, one self loop per node"""
    from bridged_gnn_amd.data import Data, save_bridged_graph
    g = load_golden("office_a2d_graph.npz")
    n = g["x"].shape[0]
    ar = torch.arange(n)
    d = Data(x=torch.from_numpy(g["x"]), edge_index=torch.stack((ar, ar)), y=torch.from_numpy(g["y"]).long(),
             **{k: torch.from_numpy(g[k]).bool() for k in ("train_mask", "val_mask", "test_mask")})
    setattr(d, mask_name, torch.from_numpy(g["central_mask"]).bool())
    save_bridged_graph(d, str(path))
    return g


def test_prepare_datasets_on_a_vs_graph_file(tmp_path):
    from bridged_gnn_amd.bridge import reorder
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, prepare_datasets
    g = write_office_standin(tmp_path / DATASET_FILES["office_amazon2dslr"][0])
    out = prepare_datasets("office_amazon2dslr", data_root=str(tmp_path))
    assert len(out) == 5
    ds, dt, data, ms, mt = out
    cm = g["central_mask"].astype(bool)
    assert ds.x.shape[0] == 2817 and dt.x.shape[0] == 591 and data.x.shape[0] == 3408
    for key in ("train_mask", "val_mask", "test_mask"):                          # split_data=False: the file's own target split
        assert np.array_equal(getattr(dt, key).numpy(), g[key].astype(bool)[~cm]), key
    assert np.array_equal(ds.x.numpy(), g["x"][cm]) and np.array_equal(dt.y.numpy(), g["y"][~cm])
    assert np.array_equal(ds.edge_index.numpy(), np.stack([np.arange(2817)] * 2))
    # the mappers invert reorder: [sources ; targets] goes back to the file's node order
    from bridged_gnn_amd.data import Data
    merged = Data(x=torch.cat([ds.x, dt.x]), y=torch.cat([ds.y, dt.y]), edge_index=torch.zeros(2, 0, dtype=torch.long))
    back = reorder(merged, ds, ms, mt)
    assert torch.equal(back.x, data.x) and torch.equal(back.y, data.y)
    assert ms[int(np.flatnonzero(cm)[5])] == 5 and mt[int(np.flatnonzero(~cm)[7])] == 7
    # an explicit path wins over data_root
    out2 = prepare_datasets("office_amazon2dslr", data_root="/nonexistent", path=str(tmp_path / DATASET_FILES["office_amazon2dslr"][0]))
    assert torch.equal(out2[0].x, ds.x)


def test_prepare_datasets_fb_source_mask_and_twitter(tmp_path):
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, prepare_datasets
    name = "fb_hamilton2caltech"
    assert DATASET_FILES[name][1]
    g = write_office_standin(tmp_path / DATASET_FILES[name][0], mask_name="source_mask")
    ds, dt, data, _, _ = prepare_datasets(name, data_root=str(tmp_path))
    assert hasattr(data, "central_mask") and not hasattr(data, "source_mask")
    assert np.array_equal(data.central_mask.numpy(), g["central_mask"].astype(bool)) and ds.x.shape[0] == 2817
    with pytest.raises(NotImplementedError, match="path_dataset"):
        prepare_datasets("twitter_unrelational", data_root=str(tmp_path))
    with pytest.raises(NotImplementedError, match="Not Recognized"):
        prepare_datasets("no_such_dataset", data_root=str(tmp_path))
    # a twitter name with a ready file: self loops (unrelational) and a freshly drawn target split
    p = tmp_path / "tw.dat"
    write_office_standin(p)
    ds, dt, data, _, _ = prepare_datasets("twitter_unrelational", path=str(p))
    assert np.array_equal(data.edge_index.numpy(), np.stack([np.arange(3408)] * 2))
    lab = dt.y != -1
    assert bool(((dt.train_mask | dt.val_mask | dt.test_mask) == lab).all())


def test_fused_filters_refuse_host_tensors():
    from bridged_gnn_amd import bridge
    from bridged_gnn_amd.data import Data
    d = Data(x=torch.randn(4, 8), y=torch.tensor([0, 1, -1, 0]), train_mask=torch.tensor([True, False, False, True]))
    ei, es, pc = torch.tensor([[0, 1], [2, 3]]), torch.tensor([0.6, 0.7]), torch.rand(4, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bridge.check_added_edges_cross_domain_validity(ei, es, d, d, pc, pc, fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bridge.check_added_edges_within_domain_validity(ei, es, d, pc, fused=True)
    out, counts = bridge.check_added_edges_within_domain_validity(ei, es, d, pc, 0.1, -2.0, return_counts=True)   # the torch path counts too
    assert len(counts) == 5 and counts == sorted(counts) and out.shape[1] == 2 - counts[-1]


def test_edge_filter_entries_are_declared_and_exported():
    from bridged_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgnn.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("bgnn_quantile_workspace_bytes", "bgnn_quantile_f32", "bgnn_row_inv_norms_f32", "bgnn_edge_validity_f32",
                 "bgnn_edge_rule1_counts_f32"):
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in bgnn.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "bgnn_edge_filter.hip" in _lib._HASHED_SOURCES
    assert _lib.lib().bgnn_quantile_workspace_bytes(1 << 30) <= 16384            # the select's scratch does not grow with n
    assert _lib.ABI_VERSION == 116
