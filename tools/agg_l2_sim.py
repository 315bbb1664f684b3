#!/usr/bin/env python3
"""CPU model of the hidden aggregation's L2 traffic: replay agg_wide_fast_kernel's tile schedule through an LRU cache.

The launch is bound by the rate of 512-byte row gathers, and a gather that misses the XCD's L2 costs more than twice a hit
(DESIGN 4.1), so what a tile schedule is worth shows in its miss rate.  This script walks one XCD's share of the tiles the way
the resident blocks of that XCD do -- every block takes its next tile by the schedule's rule, a tile of 8 rows gathers 4 edges
per row and step, a step takes a jittered time -- and sends every gathered row (and each destination's own row) through a
row-granular, fully associative LRU of `--cache-rows` rows.  It prints the miss rate and the fabric reads scaled to eight XCDs.

Schedules (csrc/bgnn_aggregate.hip, launch_wide_fast):
  chunk   claim k of an XCD = `--chunk` tiles; with `--interleave` (the default) tiles r, r + G, .. of super-chunk k // G,
          else consecutive tiles
  tile    single tiles from `--subqueues` striped counters: counter c = slot % NQ hands out positions NQ * k + c;
          `--ahead` tiles are claimed before they are walked (2 in the kernel, 0 = claimed when needed)
  static  position slot + k * G

    python tools/agg_l2_sim.py --schedule chunk --cache-rows 3072
    python tools/agg_l2_sim.py --schedule tile --subqueues 4 --ahead 2 --cache-rows 3072

The model knows nothing of sets, sectors or the Infinity Cache: `--cache-rows` is an EFFECTIVE size.  3072 rows (1.5 MB) is the
size at which the chunk schedule reproduces the counters measured on the C4 graph (profiles/r03)."""
import argparse
import heapq
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS_PER_TILE = 8
EDGES_PER_STEP = 4


def dst_csr(ei, n):
    """by-destination CSR with one self loop per node, last in its row (what bgnn_build_dst_csr makes of edge_index)"""
    src, dst = ei[0], ei[1]
    keep = src != dst
    src = np.concatenate([src[keep], np.arange(n, dtype=np.int64)])
    dst = np.concatenate([dst[keep], np.arange(n, dtype=np.int64)])
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return rowptr, src[order]


class Layout:
    """positions of one XCD's sequence -> global tiles (launch_wide_fast's xcd_segments mapping)"""

    def __init__(self, ntiles, xcd, segments=8):
        self.ntiles, self.xcd, self.nseg = ntiles, xcd, max(segments, 1)
        self.per_x = (ntiles + 7) // 8
        self.seg_len = (self.per_x + self.nseg - 1) // self.nseg
        self.npos = self.nseg * self.seg_len if self.nseg > 1 else max(min((xcd + 1) * self.per_x, ntiles) - xcd * self.per_x, 0)

    def tile(self, pos):
        """global tile of position `pos`, or -1 for a padded position"""
        if self.nseg == 1:
            return self.xcd * self.per_x + pos
        sg, r = divmod(pos, self.seg_len)
        gt = (sg * 8 + self.xcd) * self.seg_len + r
        return gt if gt < self.ntiles else -1


class Claims:
    """the next position of block `slot` (of G on the XCD) under a schedule; None when the block is done"""

    def __init__(self, schedule, npos, G, chunk=4, interleave=True, subqueues=4, ahead=2):
        self.schedule, self.npos, self.G = schedule, npos, G
        self.chunk, self.interleave, self.nq, self.ahead = chunk, interleave, max(min(subqueues, G), 1), ahead      # (a counter needs a block)
        self.counter = [0] * max(subqueues, 1)
        self.pending = [[] for _ in range(G)]          # positions a block holds and has not walked
        self.static_k = [0] * G
        self.done = [False] * G

    def _claim(self, slot):
        if self.schedule == "static":
            pos = slot + self.static_k[slot] * self.G
            self.static_k[slot] += 1
            return [pos]
        if self.schedule == "chunk":
            k = self.counter[0]
            self.counter[0] += 1
            if self.interleave:
                sc, r = divmod(k, self.G)
                return [sc * self.chunk * self.G + r + j * self.G for j in range(self.chunk)]
            return [k * self.chunk + j for j in range(self.chunk)]
        c = slot % self.nq
        k = self.counter[c]
        self.counter[c] += 1
        return [self.nq * k + c]

    def next(self, slot):
        q = self.pending[slot]
        while not self.done[slot]:
            want = 1 + (self.ahead if self.schedule == "tile" else 0)
            while len(q) < want:
                got = self._claim(slot)
                q.extend((pos, j == 0) for j, pos in enumerate(got))
            pos, first = q.pop(0)
            if pos < self.npos:
                return pos
            if first:                                      # a claim that starts behind the end: the block is done
                self.done[slot] = True
            else:                                          # a later tile of a chunk behind the end: the kernel drops the rest, claims again
                q.clear()
        return None


def simulate(rowptr, col, mask, schedule, cache_rows, blocks=160, xcds=(0,), jitter=0.0, seed=0, segments=8, **kw):
    """-> dict(miss_rate, fabric_gb (scaled to 8 XCDs), accesses, misses, visited = global tiles in visiting order)"""
    n = rowptr.shape[0] - 1
    ntiles = (n + ROWS_PER_TILE - 1) // ROWS_PER_TILE
    rng = np.random.default_rng(seed)
    accesses = misses = 0
    visited = []
    for xcd in xcds:
        lay = Layout(ntiles, xcd, segments)
        G = min(blocks, max((min(ntiles, 8 * blocks) + 7) // 8, 1))
        claims = Claims(schedule, lay.npos, G, **kw)
        lru = OrderedDict()
        heap = [(float(rng.random()) * 1e-3, slot, -1, 0, 0) for slot in range(G)]      # (time, slot, tile, step, steps)
        heapq.heapify(heap)
        while heap:
            t, slot, tile, step, steps = heapq.heappop(heap)
            if step >= steps:                              # take the next tile
                tile = -1
                while tile < 0:
                    pos = claims.next(slot)
                    if pos is None:
                        break
                    tile = lay.tile(pos)
                if tile < 0:
                    continue
                visited.append(tile)
                r0, r1 = tile * ROWS_PER_TILE, min((tile + 1) * ROWS_PER_TILE, n)
                deg = rowptr[r0 + 1:r1 + 1] - rowptr[r0:r1]
                steps = int((deg.max() + EDGES_PER_STEP - 1) // EDGES_PER_STEP)
                step = 0
                keys = [(r << 1) | int(mask[r]) for r in range(r0, r1)]                 # each destination's own row of its table
            else:
                r0, r1 = tile * ROWS_PER_TILE, min((tile + 1) * ROWS_PER_TILE, n)
                keys = []
                for r in range(r0, r1):
                    b = rowptr[r] + step * EDGES_PER_STEP
                    e = min(b + EDGES_PER_STEP, rowptr[r + 1])
                    if b < e:
                        dom = int(mask[r])
                        keys.extend((int(c) << 1) | dom for c in col[b:e])
                step += 1
            for key in keys:
                accesses += 1
                if key in lru:
                    lru.move_to_end(key)
                else:
                    misses += 1
                    lru[key] = None
                    if len(lru) > cache_rows:
                        lru.popitem(last=False)
            heapq.heappush(heap, (t + 1.0 + jitter * float(rng.standard_normal()) if jitter else t + 1.0, slot, tile, step, steps))
    scale = 8.0 / max(len(xcds), 1)
    return dict(miss_rate=misses / max(accesses, 1), fabric_gb=misses * 512 * scale / 1e9, accesses=accesses, misses=misses, visited=visited)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--graph", choices=["local", "uniform"], default="local", help="synth.bridged_graph as bench.py's C4 builds it")
    ap.add_argument("--schedule", choices=["chunk", "tile", "static"], default="tile")
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--no-interleave", action="store_true")
    ap.add_argument("--subqueues", type=int, default=4)
    ap.add_argument("--ahead", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=160, help="resident blocks per XCD (5 per CU x 32 CUs)")
    ap.add_argument("--cache-rows", type=int, default=3072, help="effective L2 size in 512-byte rows")
    ap.add_argument("--jitter", type=float, default=0.0, help="standard deviation of a step's time, in steps")
    ap.add_argument("--xcds", type=int, default=1, help="XCDs to simulate (the result is scaled to eight)")
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from bridged_gnn_amd import synth
    n_src = args.nodes // 2
    n_tar = args.nodes - n_src
    extra = args.edges - 6 * args.nodes - 20 * n_tar
    ei, mask = synth.bridged_graph(n_src, n_tar, k_within=6, k_cross=20, n_extra=max(extra, 0), cluster=1024,
                                   p_local=0.9 if args.graph == "local" else 0.0, seed=0)
    rowptr, col = dst_csr(ei, args.nodes)
    r = simulate(rowptr, col, mask, args.schedule, args.cache_rows, blocks=args.blocks, xcds=tuple(range(args.xcds)), jitter=args.jitter,
                 seed=args.seed, segments=args.segments, chunk=args.chunk, interleave=not args.no_interleave, subqueues=args.subqueues,
                 ahead=args.ahead)
    print(f"schedule={args.schedule} chunk={args.chunk} interleave={int(not args.no_interleave)} subqueues={args.subqueues} ahead={args.ahead} "
          f"blocks={args.blocks} cache_rows={args.cache_rows} ({args.cache_rows * 512 / 2**20:.2f} MB) jitter={args.jitter}: "
          f"miss rate {r['miss_rate']:.3f}, fabric reads {r['fabric_gb']:.2f} GB ({r['accesses']} row reads on {args.xcds} XCD)")


if __name__ == "__main__":
    main()
