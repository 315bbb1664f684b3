"""Step 1 of Bridged-GNN end to end: `python -m bridged_gnn_amd.bridged_graph` (main_bridged_graph.py:325-357 + datasets.py:16-66).

Dataset -> source / target split -> similarity learner (simlearner_v1.main_adv / simlearner.main_adv_v2) -> checkpoint ->
`BridgeScorer` -> kNN bridge, edge-validity filters (the fused HIP pass unless --no_fused), merge, reorder -> diagnostics ->
`{out_dir}/{dataset_name}_bridged_graph.dat`, the file step 2 (`python -m bridged_gnn_amd.transfer`) reads.

The flags are the reference's, with its defaults and choices; the paths it hard-codes (`../datasets`, `../ckpt`,
`../data_bridged_graph`) are flags here with those values as defaults.  The twitter datasets are built by the reference from raw
files (datasets/dataset_ktgnn.py); that builder is out of scope, so a twitter name needs `--path_dataset`, a ready VS-graph file."""
import argparse
import os

import torch

from . import bridge
from .data import load_bridged_graph, save_bridged_graph
from .utils import set_random_seed

__all__ = ["DATASET_FILES", "build_parser", "prepare_datasets", "main"]

# datasets.py:30-49: name -> (file under data_root, the file calls its source mask `source_mask`)
DATASET_FILES = {
    "office_amazon2dslr": ("office_amazon2dslr_pyg.dat", False),
    "office_amazon2webcam": ("office_amazon2webcam_pyg.dat", False),
    "fb_hamilton2caltech": ("dataset_FB(Hamilton->Caltech)_pyg_relational_intra.dat", True),
    "fb_howard2simmons": ("dataset_FB(Howard->Simmons)_pyg_relational_intra.dat", True),
}
_TWITTER = ("twitter_unrelational", "twitter_relational_intra_inter")       # datasets.py:17-29: split_data=True

# name -> (type (None: store_true), default, choices, help)
_FLAGS = {
    "gpu": (int, 0, None, "index of the GPU to run on"),
    "dataset_name": (str, "twitter_unrelational", None, "dataset; also names the checkpoint and the output file"),
    "save": (None, False, None, "write the checkpoints and the bridged graph"),
    "check_within": (None, False, None, "filter the added within-domain edges"),
    "check_cross": (None, False, None, "filter the added cross-domain edges"),
    "norm_mode": (str, "None", None, "PairNorm mode of the encoders"),
    "version": (str, "v1", ("v1", "v2"), "version of the similarity learner"),
    "norm_scale": (float, 1.0, None, None),
    "num_epoch": (int, 400, None, None),
    "start_eval_epoch": (int, 300, None, None),
    "eval_per_epoch": (int, 1, None, None),
    "num_layer": (int, 2, None, None),
    "hidden_dim": (int, 64, None, None),
    "sim_mode": (str, "mlp", ("cosine", "mlp"), "pair scorer of the v2 learner"),
    "backbone": (str, "mlp", ("gnn", "mlp"), "encoder of the v2 learner"),
    "seed": (int, 0, None, None),
    "epsilon": (float, 0.5, None, "accepted for compatibility; unused by the reference as well"),
    "thres_conf_quantile": (float, 0.1, None, "rule 1: drop cross edges below this quantile of the scorer's confidence"),
    "thres_feat_sim": (float, 0.8, None, "rule 5: drop cross edges whose raw-feature cosine is below this"),
    "k_within": (int, 6, None, "within-domain neighbours per node (0: none)"),
    "k_cross": (int, 20, None, "source neighbours per target node"),
    "batch_size": (int, 1000, None, "accepted for compatibility; batching is internal to the kernels"),
    "repeat": (int, 1, None, None),
    "max_class_num": (int, 10, None, None),
    "eval_mode": (str, "sampling", ("all", "sampling"), None),
    "sample_size": (int, 40000, None, None),
    # this package's own
    "data_root": (str, "../datasets", None, "directory of the dataset files"),
    "path_dataset": (str, None, None, "an explicit VS-graph .dat (x, edge_index, y, masks, central_mask) instead of data_root's file"),
    "ckpt_dir": (str, "../ckpt", None, "where model_AdvLearner_{dataset_name}_best.ckpt is written and read"),
    "out_dir": (str, "../data_bridged_graph", None, "where {dataset_name}_bridged_graph.dat is written"),
    "skip_train": (None, False, None, "do not train: use the checkpoint already in --ckpt_dir"),
    "reference_filter_quirk": (None, False, None, "feed the filters the top-k-ordered similarity vector, as the reference does"),
    "no_fused": (None, False, None, "run the edge filters as torch ops instead of the fused HIP pass"),
    "quiet": (None, False, None, "no per-epoch / per-stage lines"),
}


def build_parser():
    """the reference's flags with its defaults and choices (main_bridged_graph.py:361-387), plus this package's path / mode flags"""
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.bridged_graph",
                                 description="Step 1 of Bridged-GNN: train the similarity learner and build the bridged graph")
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=default, choices=choices, help=text)
    return ap


def prepare_datasets(dataset_name="twitter_unrelational", data_root="../datasets", path=None):
    """datasets.py:16-66 -> (data_src, data_tar, data, mapper_idx_src, mapper_idx_tar).  The .dat is read with the restricted loader
    of `data.py` (no torch_geometric).  fb files: `source_mask` becomes `central_mask` (:41-42).  `*_unrelational`: one self loop per
    node replaces the edges (:61-62).  office / fb keep the file's own target split, twitter draws one (`split_data`)."""
    if dataset_name in DATASET_FILES:
        fname, _ = DATASET_FILES[dataset_name]
        split_data = False
        path = os.path.join(data_root, fname) if path is None else path
    elif dataset_name in _TWITTER:
        split_data = True
        if path is None:
            raise NotImplementedError(
                f"{dataset_name}: the reference builds the twitter graph from raw files, which this package does not do; "
                "pass --path_dataset with a ready VS-graph .dat (x, edge_index, y, train / val / test masks, central_mask)")
    else:
        raise NotImplementedError("Not Recognized Dataset Name:{}".format(dataset_name))
    data = load_bridged_graph(path)
    if hasattr(data, "source_mask"):                                             # :41-42, :47-48
        data.central_mask = data.source_mask
        del data.source_mask
    if not hasattr(data, "central_mask"):
        raise ValueError(f"{path} has neither central_mask nor source_mask: not a VS-graph file")
    if dataset_name.split("_")[-1] == "unrelational":                            # :61-62
        ar = torch.arange(data.num_nodes)
        data.edge_index = torch.stack((ar, ar), dim=0)
    data_src, data_tar, mapper_idx_src, mapper_idx_tar = bridge.dataset_conversion(data, seed=1, dataset_name=dataset_name,
                                                                                   split_data=split_data)
    return data_src, data_tar, data, mapper_idx_src, mapper_idx_tar


def _say(quiet, *a):
    if not quiet:
        print(*a)


def main(argv=None):
    """main_bridged_graph.py:325-357.  `argv`: a list of command-line words, a parsed namespace, or None (sys.argv).
    -> the merged, reordered bridged graph (`Data`, on the GPU)."""
    args = argv if isinstance(argv, argparse.Namespace) else build_parser().parse_args(argv)
    quiet = bool(getattr(args, "quiet", False))
    set_random_seed(0)                                                           # :326
    data_src, data_tar, data, mapper_idx_src, mapper_idx_tar = prepare_datasets(args.dataset_name, args.data_root, args.path_dataset)
    _say(quiet, data)
    if not torch.cuda.is_available():
        raise RuntimeError("bridged_gnn_amd.bridged_graph needs an MI355X; there is no CPU path")
    device = torch.device("cuda:{}".format(args.gpu))
    _say(quiet, "Device:", device)
    with torch.cuda.device(device):
        if args.dataset_name.split("_")[0] == "twitter":                         # :335-340
            from .simlearner_v1 import twitter_self_loops
            twitter_self_loops(data_src)
        _say(quiet, data_src, data_tar)
        if not args.skip_train:
            common = dict(save=args.save, repeat=args.repeat, num_epoch=args.num_epoch, seed=args.seed, num_layer=args.num_layer,
                          hidden=args.hidden_dim, metric="f1", use_clf=True, norm_mode=args.norm_mode, norm_scale=args.norm_scale,
                          eval_per_epoch=args.eval_per_epoch, start_eval_epoch=args.start_eval_epoch, device=device,
                          ckpt_dir=args.ckpt_dir, verbose=not quiet)
            if args.version == "v1":                                             # :346-349
                from .simlearner_v1 import main_adv
                main_adv(args, data_src, data_tar, **common)
            else:                                                                # :350-354
                from .simlearner import main_adv_v2
                main_adv_v2(args, data_src, data_tar, max_class_num=args.max_class_num, sample_size=args.sample_size,
                            sim_mode=args.sim_mode, backbone=args.backbone, use_norm=True, eval_mode=args.eval_mode, **common)
        path_ckpt = os.path.join(args.ckpt_dir, f"model_AdvLearner_{args.dataset_name}_best.ckpt")      # :356
        if not os.path.exists(path_ckpt):
            raise FileNotFoundError(f"{path_ckpt} does not exist: train with --save (a checkpoint is written when an evaluated epoch "
                                    "improves the cross-domain validation score), or point --ckpt_dir at an existing one")
        model = bridge.BridgeScorer(torch.load(path_ckpt, map_location="cpu", weights_only=True), device, norm_mode=args.norm_mode,
                                    norm_scale=args.norm_scale)
        data_src, data_tar = data_src.to(device), data_tar.to(device)
        merged = bridge.gen_bridged_graph(data_src, data_tar, model, k_cross=args.k_cross, k_within=args.k_within,
                                          check_cross=args.check_cross, check_within=args.check_within,
                                          thres_conf_quantile=args.thres_conf_quantile, thres_feat_sim=args.thres_feat_sim,
                                          mapper_idx_src=mapper_idx_src, mapper_idx_tar=mapper_idx_tar,
                                          reference_filter_quirk=args.reference_filter_quirk, verbose=not quiet, fused=not args.no_fused)
        bridge.eval_homophily(merged, verbose=not quiet)                         # :315
        bridge.eval_bridged_Graph(merged, verbose=not quiet)                     # :316
        if args.save:                                                            # :317-320
            os.makedirs(args.out_dir, exist_ok=True)
            save_bridged_graph(merged, os.path.join(args.out_dir, f"{args.dataset_name}_bridged_graph.dat"))
    return merged


if __name__ == "__main__":
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
