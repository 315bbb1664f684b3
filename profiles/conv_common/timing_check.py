"""The speed criterion of this comparison over the JSON lines in a directory (`<tool>_<parent|branch>_<run>.json` written by
tools/sage_time.py, tools/gcn_time.py, tools/gat_time.py and tools/gatv2_time.py with --out): every branch median must lie inside the parent's
min-to-max range widened by that range's own width on each side.

    python profiles/conv_common/timing_check.py profiles/conv_common/timing"""
import glob
import json
import os
import sys

import numpy as np

FIGURES = {
    "sage": ("eval_forward_ms", "train_step_ms", "aggregations.D64.fwd_ms", "aggregations.D64.bwd_ms", "aggregations.D2.fwd_ms",
             "aggregations.D2.bwd_ms"),
    "gcn": ("widths.D64.fused_fwd_ms", "widths.D64.fused_bwd_ms", "widths.D4.fused_fwd_ms", "widths.D4.fused_bwd_ms",
            "office_epoch_ms.eager", "office_epoch_ms.graphed"),
    "gat": ("shapes.H3C64.fused_fwd_ms", "shapes.H3C64.fused_fwd_bwd_ms", "shapes.H1C2.fused_fwd_ms", "shapes.H1C2.fused_fwd_bwd_ms",
            "office_epoch_ms.eager", "office_epoch_ms.graphed"),
    "gatv2": ("shapes.H1C64.fused_fwd_ms", "shapes.H1C64.fused_fwd_bwd_ms", "shapes.H1C2.fused_fwd_ms", "shapes.H1C2.fused_fwd_bwd_ms",
              "office_epoch_ms.eager", "office_epoch_ms.graphed"),
}


def get(d, path):
    for k in path.split("."):
        d = d[k]
    return float(d)


def main(folder):
    bad = 0
    print("| tool | figure | parent runs | branch runs | branch median | allowed | |")
    print("|---|---|---|---|---|---|---|")
    for tool, figures in FIGURES.items():
        runs = {tree: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(folder, f"{tool}_{tree}_*.json")))]
                for tree in ("parent", "branch")}
        if not runs["parent"] or not runs["branch"]:
            print(f"| {tool} | no runs | | | | | |")
            continue
        for fig in figures:
            p, b = [get(r, fig) for r in runs["parent"]], [get(r, fig) for r in runs["branch"]]
            lo, hi = min(p), max(p)
            w = hi - lo
            med = float(np.median(b))
            ok = lo - w <= med <= hi + w
            bad += not ok
            print(f"| {tool} | {fig} | {' '.join(f'{v:.4f}' for v in p)} | {' '.join(f'{v:.4f}' for v in b)} | {med:.4f} | "
                  f"{lo - w:.4f} .. {hi + w:.4f} | {'ok' if ok else 'OUTSIDE'} |")
    print(f"\n{bad} figure(s) outside")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
