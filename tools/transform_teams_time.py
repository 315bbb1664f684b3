"""Team mode of the hidden transform on a target-only launch: 500k rows, every tile needs h_s2t only (one run over all tiles).
  python tools/transform_teams_time.py [LIB.so | -]      with BGNN_TS_TEAMS=0 or 1 in the environment
Prints the hip-event time per call (W.delta kernel + transform).  With a library whose bgnn_transform_stream.hip was built with
-DTS_STAMP (tools/build_variant.sh) the kernel also prints its per-phase cycle stamps every 12 launches."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from bridged_gnn_amd import _lib
if len(sys.argv) > 1 and sys.argv[1] != "-":
    _lib.SO_PATH = os.path.abspath(sys.argv[1])
from bridged_gnn_amd import ops
from test_gpu_classifier_stage import dev_head, domain_sums64, make_head
dev = "cuda:0"
n, din, D = 500_000, 128, 128
g = torch.Generator().manual_seed(1)
x = torch.randn(n, din, generator=g)
m = torch.zeros(n, dtype=torch.bool); 
sums = domain_sums64(torch.cat((x[:1000], x[:1000] + 1)), torch.cat((torch.ones(1000, dtype=torch.bool), torch.zeros(1000, dtype=torch.bool)))).to(dev)
packed = ops.pack_transform_heads([dev_head(make_head(g, D, din, True))], din)
need = torch.ones((n + 31) // 32, dtype=torch.int32, device=dev)
xd, m8 = x.to(dev), m.to(dev, torch.uint8)
out = [(torch.empty(n, 128, device=dev), torch.empty(n, 128, device=dev))]
print("teams env", os.environ.get("BGNN_TS_TEAMS"), "plan", ops.transform_team_runs(n, torch.device(dev), need), flush=True)
for _ in range(12):
    ops.adaptedconv_transform(xd, m8, None, packed, out=out, sums=sums, tile_need=need)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(25)]
for k in range(24):
    ev[k].record(); ops.adaptedconv_transform(xd, m8, None, packed, out=out, sums=sums, tile_need=need)
ev[24].record(); torch.cuda.synchronize()
t = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(24))
print(f"target-only transform, {n} rows: per call (wd kernel + transform) min {t[0]*1e3:.1f} us  median {t[12]*1e3:.1f} us  max {t[-1]*1e3:.1f} us", flush=True)
