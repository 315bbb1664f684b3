"""One sha256 per case over the outputs of the dense-transform entries, to compare two trees bit for bit:

    python profiles/transform_entry/digests.py --root TREE > digests.txt      (TREE: a checkout with its library built)

Only `ops` is used, so the same script runs on a tree with four transform entries and on one with a single entry.  N in
{1, 33, 300} rows, a random domain mask, fixed seeds.  Transform cases (Din, heads, D) reach every branch of the route (stream,
W-stationary block kernel at 2 / 4 / 8 column tiles, skinny, the three tiled GEMMs), each in delta form and in sums form; in sums
form also two tail groups and a random need mask, of which only the rows a consumer may read are hashed.  `ops.linear` and
`ops.linear_narrow_transform` + `narrow_transform_finish` over Din in {64, 128} x Dout in {64, 128, 256}.  The fp64-atomic
`colsum` outputs get lines of their own: their summation order is not fixed from run to run."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

NS = (1, 33, 300)
# (Din, heads, D): route
CASES = ((100, 1, 64), (128, 1, 128),                       # stream
         (64, 1, 32), (64, 1, 64), (32, 2, 32), (128, 2, 64),   # W-stationary block kernel: 2, 4, 4, 8 column tiles
         (100, 1, 4), (64, 2, 4),                           # skinny
         (64, 2, 5), (256, 1, 4), (256, 1, 32), (132, 1, 64), (256, 1, 100))    # tiled GEMM <32>, <32>, <64>, <128>, <128>
TAIL = (37, 50)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from bridged_gnn_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(115)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen)

    def inputs(n, din):
        """x, the domain mask, its float64 domain sums (counts of an empty domain raised to 1) and the float32 delta"""
        m = torch.rand(n, generator=gen) < 0.45
        x = rnd(n, din)
        x[m] += 0.5 * rnd(din)
        x64 = x.double()
        ns, nt = max(int(m.sum()), 1), max(int((~m).sum()), 1)
        sums = torch.cat([x64[m].sum(0), x64[~m].sum(0), torch.tensor([ns, nt], dtype=torch.float64)])
        delta = ((sums[:din] / ns).float() - (sums[din:2 * din] / nt).float())
        return x.to(dev), m.to(dev, torch.uint8), sums.to(dev), delta.to(dev)

    def head(D, din):
        return {"W_s": rnd(D, din).to(dev) / din ** 0.5, "b_s": rnd(D).to(dev), "W_t": rnd(D, din).to(dev) / din ** 0.5, "b_t": rnd(D).to(dev),
                "g_s2t": rnd(2 * din).to(dev) / din ** 0.5, "g_t2s": rnd(2 * din).to(dev) / din ** 0.5,
                "gate_const": (float(rnd(1)), float(rnd(1)))}

    def tables(n, packed):
        H, ldh = packed[2].shape[0], packed[4]
        return [(torch.zeros(n, ldh, device=dev), torch.zeros(n, ldh, device=dev)) for _ in range(H)]

    for din, H, D in CASES:
        packed = ops.pack_transform_heads([head(D, din) for _ in range(H)], din)
        for n in NS:
            x, m8, sums, delta = inputs(n, din)
            tag = f"Din={din} heads={H} D={D} N={n}"
            out = ops.adaptedconv_transform(x, m8, delta, packed, out=tables(n, packed))
            print(f"transform delta {tag} {sha(*[t for pair in out for t in pair])}")
            out = ops.adaptedconv_transform(x, m8, None, packed, out=tables(n, packed), sums=sums)
            print(f"transform sums {tag} {sha(*[t for pair in out for t in pair])}")
            if (din, H, D) in ((128, 1, 128), (64, 1, 32)) and n == 300:
                # rows [0, both) need both tables, the next TAIL[0] rows h_t2s only, the last TAIL[1] rows h_s2t only
                (t2s, s2t), = ops.adaptedconv_transform(x, m8, None, packed, out=tables(n, packed), sums=sums, tail_single=TAIL)
                both = n - TAIL[0] - TAIL[1]
                print(f"transform tail={TAIL} {tag} {sha(t2s[:both + TAIL[0]], s2t[:both], s2t[both + TAIL[0]:])}")
            if (din, H, D) == (128, 1, 128):
                need = torch.randint(0, 4, ((n + 31) // 32,), generator=gen, dtype=torch.int32).to(dev)
                (t2s, s2t), = ops.adaptedconv_transform(x, m8, None, packed, out=tables(n, packed), sums=sums, tile_need=need)
                rows = need[torch.arange(n, device=dev) // 32]              # bit 0: h_s2t is read, bit 1: h_t2s
                print(f"transform need {tag} {sha(need, s2t[(rows & 1) != 0], t2s[(rows & 2) != 0])}")

    for din in (64, 128):
        for dout in (64, 128, 256):
            W, b = rnd(dout, din).to(dev) / din ** 0.5, rnd(dout).to(dev)
            narrow = ops.pack_transform_heads([head(3, dout)], dout)
            fin_sums = torch.cat([rnd(2 * dout).double() * 40, torch.tensor([100.0, 150.0], dtype=torch.float64)]).to(dev)
            for n in NS:
                x, m8, _, _ = inputs(n, din)
                for relu in (False, True):
                    tag = f"Din={din} Dout={dout} relu={int(relu)} N={n}"
                    print(f"linear {tag} {sha(ops.linear(x, W, b, relu=relu))}")
                    colsum = torch.zeros(2 * dout + 2, dtype=torch.float64, device=dev)
                    print(f"linear+colsum out {tag} {sha(ops.linear(x, W, b, relu=relu, mask_u8=m8, colsum=colsum))}")
                    print(f"linear+colsum colsum {tag} {sha(colsum)}")
                    colsum = torch.zeros(2 * dout + 2, dtype=torch.float64, device=dev)
                    raw = ops.linear_narrow_transform(x, W, b, m8, colsum, narrow, relu=relu)
                    print(f"narrow raw {tag} {sha(raw)}")
                    print(f"narrow colsum {tag} {sha(colsum)}")
                    fin = ops.narrow_transform_finish(raw, m8, fin_sums, narrow, (torch.zeros(n, 4, device=dev), torch.zeros(n, 4, device=dev)))
                    print(f"narrow finish {tag} {sha(*fin)}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
