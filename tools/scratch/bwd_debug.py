import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from bridged_gnn_amd import _lib as L, ops, synth
DEV = "cuda:0"
n, D, deg = 64, 128, 5
rng = np.random.default_rng(0)
ei, mask = synth.random_multigraph(n, deg * n, frac_src=0.5, n_isolated=1, seed=0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
csr = ops.build_dst_csr(t(ei), n)
both = torch.zeros(2, n, D, device=DEV)
hS, hT = both[0], both[1]
hS.copy_(t(rng.standard_normal((n, D)).astype(np.float32))); hT.copy_(t(rng.standard_normal((n, D)).astype(np.float32)))
a1, a2 = t((rng.standard_normal(D) * 0.3 * float(os.environ.get("ASCALE", "1"))).astype(np.float32)), t((rng.standard_normal(D) * 0.3 * float(os.environ.get("ASCALE", "1"))).astype(np.float32))
m8 = t(mask).to(torch.uint8)
out, alpha = ops.adaptedconv_aggregate(hS, hT, a1, a2, csr, m8, D, 0.1, want_alpha=True)
g = t(rng.standard_normal((n, D)).astype(np.float32))
lib = L.lib()
E = csr.num_edges
t_rowptr, t_eid, t_dst = csr.transposed()
wsb = lib.bgnn_aggregate_bwd_pull_workspace_bytes(n, E, D, D, 0, 0)
ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
dS, dT = torch.empty_like(hS), torch.empty_like(hT)
da1, da2 = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
rc = lib.bgnn_adaptedconv_aggregate_bwd_pull_f32(L.ptr_rows(hS), L.ptr_rows(hT), D, L.ptr(a1), L.ptr(a2), L.ptr(csr.rowptr), L.ptr(csr.col), L.ptr(m8),
        L.ptr(t_rowptr), L.ptr(t_eid), L.ptr(t_dst), n, E, D, 0.1, L.ptr(out), D, L.ptr(alpha), L.ptr(g), D, L.ptr(dS), L.ptr(dT), L.ptr(da1), L.ptr(da2),
        0, None, 0, None, None, None, 0, None, 0, None, None, None, 0, L.ptr(ws), wsb, L.stream())   # no hub rows
print("rc", rc)
torch.cuda.synchronize()
rec = ws[:32 * E].view(torch.int32).view(E, 8).cpu()
recf = ws[:32 * E].view(torch.float32).view(E, 8).cpu()
off = (32 * E + 255) // 256 * 256
dstside = ws[off:off + n * D * 4].view(torch.float32).view(n, D).cpu()
# expected
rp, col = csr.rowptr.cpu().long(), csr.col.cpu().long()
H = torch.where(torch.from_numpy(mask)[:, None], hS.cpu(), hT.cpu())   # table by domain of destination? table rows used: H_dom(i)[j]
hS_c, hT_c, gc, oc, al = hS.cpu().double(), hT.cpu().double(), g.cpu().double(), out.cpu().double(), alpha.cpu().double()
bad = 0
for i in range(n):
    T = hS_c if mask[i] else hT_c
    a = (a1 if mask[i] else a2).cpu().double()
    ti = (gc[i] * oc[i]).sum()
    dd = torch.zeros(D, dtype=torch.float64)
    for e in range(rp[i], rp[i + 1]):
        j = col[e]
        c = (gc[i] * T[j]).sum()
        de = al[e] * (c - ti)
        z = T[j] + T[i]
        lp = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.1))
        dd += de * a * lp
        # record check
        als, der = recf[e, 4].item(), recf[e, 5].item()
        bits = [(rec[e, c_].item() & 0xFFFFFFFF) for c_ in range(4)]
        exp_bits = [0, 0, 0, 0]
        for l in range(32):
            for c_ in range(4):
                if z[4 * l + c_] > 0: exp_bits[c_] |= (1 << l)
        if abs(abs(als) - al[e].item()) > 1e-6 or (als < 0 or (als == 0 and np.signbit(als))) != bool(mask[i]) or abs(der - de.item()) > 1e-4 * (1 + abs(de.item())) or bits != exp_bits:
            if bad < 5: print("rec mismatch edge", e, "i", i, "al", als, al[e].item(), "de", der, de.item(), [hex(b) for b in bits], [hex(b) for b in exp_bits])
            bad += 1
    err = (dstside[i].double() - dd).abs().max().item()
    if err > 1e-4 and bad < 8:
        print("dstside mismatch row", i, err, dstside[i, :6], dd[:6]); bad += 1
print("bad", bad)
# expected dH (fp64), per source j
expS = torch.zeros(n, D, dtype=torch.float64); expT = torch.zeros(n, D, dtype=torch.float64)
for i in range(n):
    T = hS_c if mask[i] else hT_c
    a = (a1 if mask[i] else a2).cpu().double()
    ti = (gc[i] * oc[i]).sum()
    tgt = expS if mask[i] else expT
    for e in range(rp[i], rp[i + 1]):
        j = col[e]
        c = (gc[i] * T[j]).sum()
        de = al[e] * (c - ti)
        z = T[j] + T[i]
        lp = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.1))
        tgt[j] += al[e] * gc[i] + de * a * lp
        tgt[i] += de * a * lp
errS = (dS.cpu().double() - expS).abs().max(1).values
errT = (dT.cpu().double() - expT).abs().max(1).values
print("max err S", errS.max().item(), "T", errT.max().item())
trp = t_rowptr.cpu()
for j in range(n):
    if errS[j] > 1e-4 or errT[j] > 1e-4:
        print("row", j, "outdeg", int(trp[j + 1] - trp[j]), "errS", errS[j].item(), "errT", errT[j].item(), "mask", bool(mask[j]))
