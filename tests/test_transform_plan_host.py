"""Host (no GPU): the planner of the hidden transform's team mode, `ops.single_table_runs` and `ops.transform_team_runs`, on CPU
tensors.  The planner needs the device only for its CU count, which it reads from `ops._N_CU`: the tests put G there (256, and
8 to show that nothing is tied to 256).  Need masks are written as segments (value, tiles); N = 32 * ntiles - 7, so the last tile
is partial.  What is pinned: the longest run per table and at most two runs, ordered by first tile; the rule of 4 tiles per
block, exactly at its boundary; tiles that need neither table next to and between runs; the tail groups rounded to whole tiles;
and the cache on the need mask, which an in-place edit must invalidate -- a stale plan makes the kernel skip a table that a tile
now needs."""
import pytest
import torch

CPU = torch.device("cpu")
GS = (256, 8)


@pytest.fixture(params=GS)
def G(request, monkeypatch):
    from bridged_gnn_amd import ops
    monkeypatch.setitem(ops._N_CU, CPU, request.param)
    return request.param


def need_of(segments):
    """-> (need mask int32 [ntiles], N)"""
    need = torch.cat([torch.full((int(k),), int(v), dtype=torch.int32) for v, k in segments])
    return need, 32 * need.numel() - 7


def plan_of(segments):
    from bridged_gnn_amd import ops
    need, n = need_of(segments)
    return ops.transform_team_runs(n, CPU, need)


def test_two_separated_runs(G):
    plan = plan_of([(3, 37), (2, 4 * G + 3), (3, 5), (1, 4 * G + G // 2), (3, 2)])
    assert plan == [(37, 4 * G + 40, 1), (4 * G + 45, 8 * G + G // 2 + 45, 0)]


def test_directly_adjacent_runs_to_the_partial_last_tile(G):
    segs = [(3, 37), (2, 4 * G + 3), (1, 4 * G + G // 2)]
    need, n = need_of(segs)
    ntiles = (n + 31) // 32
    assert ntiles == need.numel() == 8 * G + G // 2 + 40 and n % 32 != 0
    assert plan_of(segs) == [(37, 4 * G + 40, 1), (4 * G + 40, ntiles, 0)]


def test_table_0_first_from_tile_0_with_a_gap_of_unneeded_tiles(G):
    plan = plan_of([(1, 4 * G), (0, 3), (2, 5 * G + 1), (3, 1)])
    assert plan == [(0, 4 * G, 0), (4 * G + 3, 9 * G + 4, 1)]


def test_admission_boundary_is_exactly_4_tiles_per_block(G):
    plan = plan_of([(3, 1), (1, 4 * G - 1), (3, 1), (2, 4 * G), (3, 1)])
    assert plan == [(4 * G + 1, 8 * G + 1, 1)]


def test_two_stretches_of_one_table_give_the_longer_one(G):
    plan = plan_of([(3, 3), (1, 4 * G), (3, 2), (1, 4 * G + 9), (3, 2)])
    assert plan == [(4 * G + 5, 8 * G + 14, 0)]


def test_candidates_before_the_4_tile_rule(G):
    """`single_table_runs` alone: one candidate per table whatever its length, by first tile; tiles that need neither table or both
    end a run"""
    from bridged_gnn_amd import ops
    need, _ = need_of([(2, 2), (0, 1), (2, 3), (1, 1), (3, 1), (1, 2), (0, 4)])
    assert ops.single_table_runs(need) == [(3, 6, 1), (8, 10, 0)]
    assert ops.single_table_runs(torch.full((5,), 3, dtype=torch.int32)) == []
    assert ops.single_table_runs(torch.zeros(5, dtype=torch.int32)) == []


def test_in_place_edit_of_the_need_mask_replans(G):
    from bridged_gnn_amd import ops
    need, n = need_of([(3, 37), (2, 4 * G + 3), (3, 5), (1, 4 * G + G // 2), (3, 2)])
    both = [(37, 4 * G + 40, 1), (4 * G + 45, 8 * G + G // 2 + 45, 0)]
    first = ops.transform_team_runs(n, CPU, need)
    assert first == both
    assert ops.transform_team_runs(n, CPU, need) is first, "no edit: the cached list"
    need[40] = 3                                        # the table-1 run falls apart into 3 and 4G - 1 tiles
    second = ops.transform_team_runs(n, CPU, need)
    assert second == [both[1]]
    assert ops.transform_team_runs(n, CPU, need) is second
    assert ops.single_table_runs(need) == [(41, 4 * G + 40, 1), both[1]]
    need[40] = 2                                        # and back: the plan follows the mask, not the history
    assert ops.transform_team_runs(n, CPU, need) == both


def _tail(G, own, n_t2s, n_s2t):
    from bridged_gnn_amd import ops
    n = own + n_t2s + n_s2t
    return ops.transform_team_runs(n, CPU, None, (n_t2s, n_s2t)), own, own + n_t2s, (n + 31) // 32


def test_tail_groups_both_qualify(G):
    plan, t2s_begin, s2t_begin, ntiles = _tail(G, 5003, 32 * (4 * G + 7) + 5, 32 * (4 * G + 2) + 9)
    assert t2s_begin % 32 and s2t_begin % 32
    assert plan == [((t2s_begin + 31) // 32, s2t_begin // 32, 1), ((s2t_begin + 31) // 32, ntiles, 0)]
    assert plan[0][1] + 1 == plan[1][0], "the tile that holds rows of both groups is in neither run"


def test_tail_without_a_t2s_group(G):
    plan, _, s2t_begin, ntiles = _tail(G, 5003, 0, 32 * (4 * G + 2) + 9)
    assert plan == [((s2t_begin + 31) // 32, ntiles, 0)]


def test_tail_groups_both_short(G):
    plan, t2s_begin, s2t_begin, ntiles = _tail(G, 5003, 32 * (4 * G - 1), 32 * (4 * G - 2) + 9)
    assert s2t_begin // 32 - (t2s_begin + 31) // 32 == 4 * G - 2 and ntiles - (s2t_begin + 31) // 32 == 4 * G - 2
    assert plan == []


def test_no_rows(G):
    from bridged_gnn_amd import ops
    assert ops.transform_team_runs(0, CPU, torch.zeros(0, dtype=torch.int32)) == []
    assert ops.transform_team_runs(0, CPU, None, (0, 0)) == []
    assert ops.single_table_runs(torch.zeros(0, dtype=torch.int32)) == []
