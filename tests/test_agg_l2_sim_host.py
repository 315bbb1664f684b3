"""CPU: tools/agg_l2_sim.py -- every tile schedule the simulator knows visits every tile of a clustered graph exactly once."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim():
    spec = importlib.util.spec_from_file_location("agg_l2_sim", os.path.join(ROOT, "tools", "agg_l2_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def graph():
    from bridged_gnn_amd import synth
    sim = _sim()
    n = 20001                                                 # 2501 tiles, the last one partial; per_x = 313 pads the XCD segments
    ei, mask = synth.bridged_graph(n // 2, n - n // 2, k_within=3, k_cross=4, n_extra=0, cluster=1024, p_local=0.9, seed=1)
    return sim, n, sim.dst_csr(ei, n), mask


SCHEDULES = [dict(schedule="chunk", chunk=4, interleave=True), dict(schedule="chunk", chunk=4, interleave=False),
             dict(schedule="chunk", chunk=1, interleave=False), dict(schedule="chunk", chunk=3, interleave=True),
             dict(schedule="tile", subqueues=4, ahead=2), dict(schedule="tile", subqueues=4, ahead=0),
             dict(schedule="tile", subqueues=1, ahead=2), dict(schedule="tile", subqueues=2, ahead=2),
             dict(schedule="tile", subqueues=8, ahead=2), dict(schedule="static")]


@pytest.mark.parametrize("kw", SCHEDULES, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
@pytest.mark.parametrize("blocks,segments", [(12, 8), (5, 1)])
def test_every_schedule_visits_every_tile_exactly_once(graph, kw, blocks, segments):
    sim, n, (rowptr, col), mask = graph
    r = sim.simulate(rowptr, col, mask, cache_rows=256, blocks=blocks, xcds=tuple(range(8)), segments=segments, **kw)
    ntiles = (n + 7) // 8
    assert sorted(r["visited"]) == list(range(ntiles))
    assert r["accesses"] == int(rowptr[-1]) + n               # every edge's row and every destination's own row, once
    assert 0.0 < r["miss_rate"] < 1.0


def test_more_cache_never_misses_more(graph):
    sim, n, (rowptr, col), mask = graph
    miss = [sim.simulate(rowptr, col, mask, "tile", c, blocks=12, xcds=(0,), jitter=0.0)["misses"] for c in (64, 512, 4096)]
    assert miss[0] >= miss[1] >= miss[2]                      # (LRU is a stack algorithm; the visiting order does not depend on the cache)
