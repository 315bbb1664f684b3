"""GPU: step 1 end to end (`bridged_gnn_amd.bridged_graph.main`) on the office A->D stand-in: train, checkpoint, bridge, fused
filters, merge, reorder, save; the torch filters (`--no_fused`) on the same checkpoint give the same graph; the v1 learner runs."""
import os

import numpy as np
import pytest
import torch

from test_bridged_graph_host import write_office_standin

pytestmark = pytest.mark.gpu
NAME = "office_amazon2dslr"


def _argv(tmp_path, *extra):
    return ["--dataset_name", NAME, "--data_root", str(tmp_path / "datasets"), "--ckpt_dir", str(tmp_path / "ckpt"),
            "--out_dir", str(tmp_path / "out"), "--quiet", *extra]


def _edge_keys(ei, n):
    return set((ei[0].cpu().numpy().astype(np.int64) * n + ei[1].cpu().numpy()).tolist())


def test_step1_driver_office_v2_and_torch_filters_agree(tmp_path):
    from bridged_gnn_amd import bridge, load_bridged_graph
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, main, prepare_datasets
    os.makedirs(tmp_path / "datasets")
    g = write_office_standin(tmp_path / "datasets" / DATASET_FILES[NAME][0])
    recipe = ["--version", "v2", "--hidden_dim", "128", "--num_epoch", "3", "--start_eval_epoch", "1", "--k_within", "3", "--k_cross", "20",
              "--check_within", "--check_cross", "--save"]
    merged = main(_argv(tmp_path, *recipe))
    ckpt = tmp_path / "ckpt" / f"model_AdvLearner_{NAME}_best.ckpt"
    assert ckpt.exists()
    scorer = bridge.BridgeScorer(torch.load(ckpt, map_location="cpu", weights_only=True), "cuda:0")
    assert scorer.version == "v2" and scorer.sim_mode == "mlp" and scorer.use_clf
    d = load_bridged_graph(str(tmp_path / "out" / f"{NAME}_bridged_graph.dat"))
    n = 3408
    assert d.x.shape[0] == n and torch.equal(d.edge_index, merged.edge_index.cpu())
    assert np.array_equal(d.x.numpy(), g["x"]) and np.array_equal(d.y.numpy(), g["y"])             # the input file's node order
    cm = g["central_mask"].astype(bool)
    assert np.array_equal(d.central_mask.numpy(), cm)
    for key in ("val_mask", "test_mask"):
        assert np.array_equal(getattr(d, key).numpy(), g[key].astype(bool) & ~cm), key
    assert np.array_equal(d.train_mask.numpy()[~cm], g["train_mask"].astype(bool)[~cm])
    assert np.array_equal(d.train_mask.numpy()[cm], g["y"][cm] != -1)
    key = d.edge_index[0] * n + d.edge_index[1]
    assert bool((key[1:] > key[:-1]).all()), "edge list is not coalesced"
    keys = _edge_keys(d.edge_index, n)
    assert all(i * n + i in keys for i in range(n)), "the input's edges (self loops) are missing"
    # rule 4 on the saved graph: no bridge edge joins nodes whose predicted classes differ
    ds, dt, _, ms, mt = prepare_datasets(NAME, data_root=str(tmp_path / "datasets"))
    ds, dt = ds.to("cuda:0"), dt.to("cuda:0")
    pred = torch.empty(n, dtype=torch.int64)
    pred[ms.orig] = scorer.class_probs(scorer.encode_source(ds)).argmax(1).cpu()
    pred[mt.orig] = scorer.class_probs(scorer.encode_target(dt)).argmax(1).cpu()
    cmt = torch.from_numpy(cm)
    cross = cmt[d.edge_index[0]] != cmt[d.edge_index[1]]
    assert int(cross.sum()) > 0 and bool(cmt[d.edge_index[0]][cross].all())                          # bridge edges run source -> target
    assert bool((pred[d.edge_index[0]][cross] == pred[d.edge_index[1]][cross]).all())
    # the torch filters on the same checkpoint
    merged_t = main(_argv(tmp_path, *recipe[:-1], "--skip_train", "--no_fused"))
    a, b = keys, _edge_keys(merged_t.edge_index, n)
    print(f"office driver: {len(a)} edges fused, {len(b)} torch, symmetric difference {len(a ^ b)}")
    assert len(a ^ b) <= 1e-3 * len(a)


def test_step1_driver_v1_runs_and_saves(tmp_path):
    from bridged_gnn_amd import load_bridged_graph
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, main
    os.makedirs(tmp_path / "datasets")
    write_office_standin(tmp_path / "datasets" / DATASET_FILES[NAME][0])
    main(_argv(tmp_path, "--version", "v1", "--hidden_dim", "64", "--num_epoch", "2", "--start_eval_epoch", "1", "--k_within", "0",
               "--check_within", "--check_cross", "--save"))
    d = load_bridged_graph(str(tmp_path / "out" / f"{NAME}_bridged_graph.dat"))
    assert d.x.shape[0] == 3408 and d.edge_index.shape[1] >= 3408


def test_driver_keeps_the_trainers_refusals(tmp_path):
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, main
    os.makedirs(tmp_path / "datasets")
    write_office_standin(tmp_path / "datasets" / DATASET_FILES[NAME][0])
    with pytest.raises(NotImplementedError):
        main(_argv(tmp_path, "--version", "v2", "--sim_mode", "cosine", "--num_epoch", "1"))
    with pytest.raises(FileNotFoundError, match="best.ckpt"):
        main(_argv(tmp_path, "--skip_train"))
