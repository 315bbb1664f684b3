"""The reference's step-2 schedule on the config-3 stand-in (300 epochs, Adam lr 1e-3 wd 5e-3, dropout 0.5, StepLR(100, 0.1);
main_graph_knowledge_transfer.py:143-262) through `bridged_gnn_amd.transfer.train_gnn`: the fused HIP loss, one eval forward and one
metric-count launch per epoch, nothing read back before the last epoch.  Prints wall time, the loss curve's end points and the scores
of the best epoch (lowest loss_target)."""
import os, sys, time, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bridged_gnn_amd import synth, transfer
from bridged_gnn_amd.data import Data
dev = "cuda:0"
x, ei, y, m = synth.twitter_standin(seed=0)
n = x.shape[0]
yt = torch.from_numpy(y).to(dev)
cm = torch.from_numpy(m).to(dev)
lab = yt >= 0
g = torch.Generator(device=dev).manual_seed(0)
u = torch.rand(n, device=dev, generator=g)
data = Data(x=torch.from_numpy(x).to(dev), edge_index=torch.from_numpy(ei).to(dev).long(), y=yt.long(), central_mask=cm,
            train_mask=(u < 0.6) & lab, val_mask=(u >= 0.6) & (u < 0.8) & lab & ~cm, test_mask=(u >= 0.8) & lab & ~cm)
data.to_undirected_()
hist = {}
torch.cuda.synchronize(); t0 = time.perf_counter()
lb, each = transfer.train_gnn(types.SimpleNamespace(dataset_name="twitter_standin"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=300,
                              gnn="KTGNN", seed=0, num_layer=2, hidden=128, metric="f1", verbose=False, history=hist)
torch.cuda.synchronize(); t1 = time.perf_counter()
L = lb["source&target"]
print(f"300 epochs (train + eval each): {t1 - t0:.3f} s | loss {L[0]:.4f} -> {L[-1]:.4f} | best epoch {hist['best_epoch'] + 1}: "
      f"train / val / test F1 {hist['best_acc']['train']:.3f} / {hist['best_acc']['val']:.3f} / {hist['best_acc']['test']:.3f} | "
      f"finite {all(v == v for v in L)}", flush=True)
