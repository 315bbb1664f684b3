"""Times step 1's edge-validity filters and its driver; prints one JSON line (method of tools/sage_time.py: device events,
alternating blocks, medians).
  filter_1m / filter_8m: `check_added_edges_cross_domain_validity` with fused=True against fused=False (the torch ops) in the same
          process on a synthetic coalesced cross list, F = 300, k = 20, both fed the same per-edge similarity vector; also the fused
          pass fed the [Nq, k] tables (what replaces `align_e_sim_to_edges`) and the kernel launch alone (`ops.edge_validity`);
  filter_20m: the fused filter alone at E = 20M (the torch path's quantile raises there);
  quantile: `ops.quantile_f32` against `torch.quantile` at 8M values, and alone at 20M;
  driver:   wall time of `bridged_graph.main` on the office stand-in (tests/golden/office_a2d_graph.npz), 3 epochs, and of the
            bridge stage alone (--skip_train).
Without --step every step runs as a child process under its own `timeout -k 10`, chained: the first failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"filter_1m": 240, "filter_8m": 420, "filter_20m": 300, "quantile": 240, "driver": 420}       # seconds allowed
SHAPES = {"filter_1m": (50_000, 50_000), "filter_8m": (100_000, 400_000), "filter_20m": (200_000, 1_000_000)}
DEV = "cuda:0"


def cross_case(ns, nt, feat=300, k=20, n_cls=10, seed=0):
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = torch.randn(n_cls, feat, device=DEV, generator=g)

    def domain(n):
        cls = torch.arange(n, device=DEV) % n_cls
        x = centres[cls] + (0.1 + 1.4 * torch.rand(n, 1, device=DEV, generator=g)) * torch.randn(n, feat, device=DEV, generator=g)
        y = cls.clone()
        y[torch.rand(n, device=DEV, generator=g) < 0.2] = -1
        probs = torch.softmax(torch.randn(n, n_cls, device=DEV, generator=g) + 2.5 * F.one_hot(cls, n_cls), dim=1)
        return Data(x=x, y=y, train_mask=torch.rand(n, device=DEV, generator=g) < 0.5), probs
    (ds, ps), (dt, pt) = domain(ns), domain(nt)
    q_cls = (torch.arange(nt, device=DEV) % n_cls).unsqueeze(1)
    idx = torch.cat([torch.randint(0, ns // n_cls, (nt, k // 2), device=DEV, generator=g) * n_cls + q_cls,
                     torch.randint(0, ns, (nt, k - k // 2), device=DEV, generator=g)], dim=1)
    sim = torch.sigmoid(torch.randn(nt, k, device=DEV, generator=g) * 2)
    ei = ops.coalesce(ops.topk_edges(idx))
    flat = torch.sigmoid(torch.randn(ei.shape[1], device=DEV, generator=g) * 2)
    return ei, flat, sim, idx, ds, dt, ps, pt


def step_filter(name, a):
    from bridged_gnn_amd import bridge
    from tools.sage_time import alternate, timed
    ns, nt = SHAPES[name]
    ei, flat, sim, idx, ds, dt, ps, pt = cross_case(ns, nt)
    E = int(ei.shape[1])
    fused = lambda: bridge.check_added_edges_cross_domain_validity(ei, flat, ds, dt, ps, pt, 0.1, 0.8, fused=True)
    tables = lambda: bridge.check_added_edges_cross_domain_validity(ei, (sim, idx), ds, dt, ps, pt, 0.1, 0.8, fused=True)
    plain = lambda: bridge.check_added_edges_cross_domain_validity(ei, flat, ds, dt, ps, pt, 0.1, 0.8)
    out = {"edges": E, "F": 300, "k": 20}
    fused(); tables()
    if name == "filter_20m":
        out["fused_ms"] = round(timed(fused, a.reps), 3)
    else:
        plain()
        torch.cuda.synchronize()
        kept_f, kept_t = fused(), plain()
        out["kept_fused"], out["kept_torch"] = int(kept_f.shape[1]), int(kept_t.shape[1])
        t_f, t_t = alternate(fused, plain, a.rounds, a.reps)
        out.update(fused_ms=round(t_f, 3), torch_ms=round(t_t, 3), speedup=round(t_t / t_f, 2))
    out["fused_tables_ms"] = round(timed(tables, a.reps), 3)
    nodes_to = bridge._node_tables(dt, pt, ei.device, True)
    nodes_from = bridge._node_tables(ds, ps, ei.device, False)
    from bridged_gnn_amd import ops
    out["pass_only_ms"] = round(timed(lambda: ops.edge_validity(ei, nodes_from, nodes_to, False, 0.1, 0.8, e_sim=flat), a.reps), 3)
    out["gathered_GB"] = round(E * 2 * 4 * 300 / 1e9, 2)          # bytes the rule-5 dot asks for, before any cache
    return out


def step_quantile(a):
    from bridged_gnn_amd import ops
    from tools.sage_time import alternate, timed
    g = torch.Generator(device=DEV).manual_seed(0)
    v8 = torch.sigmoid(torch.randn(8_000_000, device=DEV, generator=g) * 2)
    v20 = torch.sigmoid(torch.randn(20_000_000, device=DEV, generator=g) * 2)
    same = bool(ops.quantile_f32(v8, 0.1).item() == torch.quantile(v8, 0.1).item())
    t_s, t_t = alternate(lambda: ops.quantile_f32(v8, 0.1), lambda: torch.quantile(v8, 0.1), a.rounds, a.reps)
    return {"n": 8_000_000, "select_ms": round(t_s, 4), "torch_ms": round(t_t, 4), "speedup": round(t_t / t_s, 2), "equal": same,
            "select_20m_ms": round(timed(lambda: ops.quantile_f32(v20, 0.1), a.reps), 4)}


def step_driver(a):
    from bridged_gnn_amd.bridged_graph import DATASET_FILES, main
    from bridged_gnn_amd.data import Data, save_bridged_graph
    og = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    n = og["x"].shape[0]
    ar = torch.arange(n)
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.stack((ar, ar)), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]).bool() for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    with tempfile.TemporaryDirectory() as tmp:
        name = "office_amazon2dslr"
        save_bridged_graph(d, os.path.join(tmp, DATASET_FILES[name][0]))
        argv = ["--dataset_name", name, "--data_root", tmp, "--ckpt_dir", tmp, "--out_dir", tmp, "--quiet", "--version", "v2",
                "--hidden_dim", "128", "--num_epoch", "3", "--start_eval_epoch", "1", "--k_within", "3", "--k_cross", "20",
                "--check_within", "--check_cross", "--save"]
        main(argv)                                                   # warm-up: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merged = main(argv)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        main(argv + ["--skip_train"])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    return {"dataset": "office stand-in", "nodes": n, "edges_out": int(merged.edge_index.shape[1]), "epochs": 3,
            "wall_s": round(t1 - t0, 3), "bridge_only_wall_s": round(t2 - t1, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    if a.step is not None:
        assert torch.cuda.is_available(), "bridged_graph_time needs an MI355X"
        res = step_quantile(a) if a.step == "quantile" else step_driver(a) if a.step == "driver" else step_filter(a.step, a)
        print(json.dumps({a.step: res, "device": torch.cuda.get_device_name(0)}), flush=True)
        return 0
    line = {"tool": "bridged_graph_time"}
    for step, limit in STEPS.items():                                # chained: a step that fails or runs out of time ends the run
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps),
                            "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(json.dumps(dict(line, failed=step, exit_code=r.returncode)), flush=True)
            return r.returncode
        line.update(json.loads(r.stdout.strip().splitlines()[-1]))
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
