"""GPU: the integer plumbing of csrc/bgnn_csr.hip past its grid cap and at its edges -- `bgnn_build_dst_csr`, `bgnn_coalesce_i64`,
`bgnn_topk_edges_i64`, `bgnn_gather_rows_f32` and `ops.pair_csr`.  Every launch of that file goes through
`grid_for`: at most 4096 blocks of 256 threads, the rest in a grid-stride loop, so a block takes a second trip above
CAP = 1 048 576 items (slots of E + N, edges, pairs, 16-byte chunks).  Each test restates CAP and asserts that its shape is past it.
Everything here is integer work (or a copy of bits): every comparison is exact, against oracle/oracle_np.py or a few lines of
numpy, never against another kernel of the library.  Every index handed to a kernel lies inside its table."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 4096 * 256                 # bgnn_csr.hip grid_for: g > 4096 ? 4096 : g blocks of 256 threads, one item per thread and trip
E_SHAPE, E_WORKSPACE, E_RANGE = -2, -3, -5          # include/bgnn.h


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _check_csr(ei, n):
    """all four outputs of the rewriting build against O.dst_csr"""
    from bridged_gnn_amd import ops
    csr = ops.build_dst_csr(_t(ei), n, rewrite_self_loops=True, want_eperm=True)
    rowptr, col, eperm = O.dst_csr(ei, np.zeros(n, bool))
    assert csr.num_edges == col.shape[0] == int((ei[0] != ei[1]).sum()) + n
    assert csr.rowptr.dtype == csr.col.dtype == csr.eperm.dtype == torch.int32
    assert np.array_equal(_np(csr.rowptr), rowptr)
    assert np.array_equal(_np(csr.col), col)
    assert np.array_equal(_np(csr.eperm), eperm)
    return csr


# ---- build_dst_csr past the cap ----------------------------------------------------------------------------------------
BIG = {"uniform": (1000, 1_100_000), "three_rows": (3, 1_100_000), "many_nodes": (1_050_000, 10)}
_BIG = {}


def _big(name):
    """uniform random over [0, N): self loops (a third of the list at N = 3) and duplicates; built once, never written to"""
    if name not in _BIG:
        n, e = BIG[name]
        assert e + n > CAP                                                # slots of the rewriting build
        ei = np.random.default_rng(sorted(BIG).index(name)).integers(0, n, size=(2, e))
        ei[:, 0] = n - 1                                                  # a self loop at the last node
        if name != "many_nodes":
            assert (ei[0] == ei[1]).sum() > e // (2 * n) and np.unique(ei[0] * n + ei[1]).shape[0] < e
        _BIG[name] = (n, ei)
    return _BIG[name]


@pytest.mark.parametrize("name", sorted(BIG))
def test_build_dst_csr_past_the_grid_cap(name):
    n, ei = _big(name)
    if name == "three_rows":
        assert np.bincount(ei[1][ei[0] != ei[1]], minlength=n).min() > 200_000       # the order inside a row spans many radix blocks
    if name == "many_nodes":
        assert n > CAP                                                    # the appended loops alone reach the second trip
    _check_csr(ei, n)


@pytest.mark.parametrize("name", sorted(BIG))
def test_build_dst_csr_without_rewrite_past_the_grid_cap(name):
    """every edge kept: the position in the rewritten list is the input position, so eperm is the stable argsort itself"""
    from bridged_gnn_amd import ops
    n, ei = _big(name)
    e = ei.shape[1]
    assert e > CAP or name == "many_nodes"                               # without the rewrite the slots are the edges alone
    csr = ops.build_dst_csr(_t(ei), n, rewrite_self_loops=False, want_eperm=True)
    order = np.argsort(ei[1], kind="stable")
    assert csr.num_edges == e
    assert np.array_equal(_np(csr.rowptr), np.concatenate(([0], np.cumsum(np.bincount(ei[1], minlength=n)))))
    assert np.array_equal(_np(csr.col), ei[0][order])
    assert np.array_equal(_np(csr.eperm), order)


@pytest.mark.parametrize("n", [2, 255, 256, 257, 65535, 65536, 65537])
def test_build_dst_csr_node_counts_around_powers_of_two(n):
    """at N = 2^k the dropped bucket (key N) needs one more bit than the node ids: it must still sort last, behind the edges
    into node N - 1"""
    e = 4 * n
    rng = np.random.default_rng(n)
    ei = rng.integers(0, n, size=(2, e))
    loops = max(n // 8, 1)
    ei[:, :loops] = rng.integers(0, n, size=loops)                       # self loops, the first at node N - 1
    ei[:, 0] = n - 1
    ei[:, -1] = (0, n - 1)                                                # ordinary edges into the last and into the first node
    ei[:, -2] = (n - 1, 0)
    assert (ei[0] == ei[1]).sum() >= n // 8 and ei[0, 0] == ei[1, 0] == n - 1
    _check_csr(ei, n)


def test_build_dst_csr_degenerate_lists():
    n = 300
    rng = np.random.default_rng(5)
    # every edge a self loop: what is left is the appended loops
    s = rng.integers(0, n, size=1000)
    csr = _check_csr(np.stack([s, s]), n)
    assert csr.num_edges == n
    assert np.array_equal(_np(csr.col), np.arange(n)) and np.array_equal(_np(csr.eperm), np.arange(n))
    assert np.array_equal(_np(csr.rowptr), np.arange(n + 1))
    # no self loop at all
    s = rng.integers(0, n, size=2000)
    d = (s + rng.integers(1, n, size=2000)) % n
    assert (s != d).all()
    assert _check_csr(np.stack([s, d]), n).num_edges == 2000 + n
    # every edge into one node (some of them its self loop)
    ei = np.stack([rng.integers(0, n, size=2000), np.full(2000, 17)])
    assert (ei[0] == 17).any()
    csr = _check_csr(ei, n)
    assert int(csr.rowptr[18]) - int(csr.rowptr[17]) == int((ei[0] != 17).sum()) + 1
    # one edge; one self loop
    _check_csr(np.array([[5], [299]]), n)
    _check_csr(np.array([[299], [299]]), n)


# ---- refusals that launch nothing --------------------------------------------------------------------------------------
def test_edge_list_entry_points_refuse_shapes_outside_their_envelope():
    from bridged_gnn_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = torch.zeros(64, dtype=torch.int64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    two31 = 1 << 31
    # build: E + N >= 2^31 (either way round), then a workspace one byte short
    assert L.bgnn_build_dst_csr(p(i64), two31 - 10, 10, 1, p(i32), p(i32), p(i32), p(i64), p(ws), ws.numel(), None) == E_SHAPE
    assert L.bgnn_build_dst_csr(p(i64), 10, two31 - 10, 1, p(i32), p(i32), p(i32), p(i64), p(ws), ws.numel(), None) == E_SHAPE
    need = L.bgnn_csr_workspace_bytes(10, 20)
    assert 0 < need <= ws.numel()
    assert L.bgnn_build_dst_csr(p(i64), 20, 10, 1, p(i32), p(i32), p(i32), p(i64), p(ws), need - 1, None) == E_WORKSPACE
    # coalesce: E >= 2^31; num_nodes one past the largest n with n * n < 2^63
    assert L.bgnn_coalesce_i64(p(i64), two31, 100, p(i64), p(ws), ws.numel(), None) == E_SHAPE
    assert 3_037_000_499 ** 2 < 1 << 63 <= 3_037_000_500 ** 2
    assert L.bgnn_coalesce_i64(p(i64), 20, 3_037_000_500, p(i64), p(ws), ws.numel(), None) == E_RANGE
    # top-k -> coalesced edges: fewer candidates than k; Nq * k >= 2^31
    assert L.bgnn_topk_edges_coalesced_i64(p(i64), 8, 4, 3, 0, 0, p(i64), p(ws), ws.numel(), None) == E_SHAPE
    assert L.bgnn_topk_edges_coalesced_i64(p(i64), 1 << 30, 2, 10, 0, 0, p(i64), p(ws), ws.numel(), None) == E_SHAPE
    torch.cuda.synchronize()
    assert int(i64.abs().sum()) == 0 and int(i32.abs().sum()) == 0       # nothing ran


# ---- coalesce ----------------------------------------------------------------------------------------------------------
def _check_coalesce(r, n):
    from bridged_gnn_amd import ops
    arg = _t(r)
    got = ops.coalesce(arg, num_nodes=n)
    want = O.coalesce(r, n)
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert np.array_equal(_np(got), want)
    assert np.array_equal(_np(arg), r)                                    # the argument is untouched
    return want


def test_coalesce_past_the_grid_cap_with_duplicates():
    n, e = 700, 1_200_000
    assert e > CAP
    r = np.random.default_rng(0).integers(0, n, size=(2, e))
    want = _check_coalesce(r, n)
    assert want.shape[1] < 0.4 * e                                        # more than 60 % duplicates: flag, scan and compact all move
    assert r.max() == n - 1
    assert np.array_equal(_check_coalesce(r, None), want)                 # num_nodes inferred = max + 1 = n
    # one edge, E times
    one = np.empty((2, 1_100_000), np.int64)
    one[0], one[1] = 123, 45
    assert one.shape[1] > CAP
    assert _check_coalesce(one, n).tolist() == [[123], [45]]


def test_coalesce_sorted_reversed_and_single():
    n = 5000
    r = np.random.default_rng(1).integers(0, n, size=(2, 200_000))
    c = O.coalesce(r, n)
    assert 0 < c.shape[1] < r.shape[1]
    assert np.array_equal(_check_coalesce(c, n), c)                       # already coalesced: unchanged
    assert np.array_equal(_check_coalesce(np.ascontiguousarray(c[:, ::-1]), n), c)
    assert _check_coalesce(np.array([[3], [2]]), 7).tolist() == [[3], [2]]


def test_coalesce_63_bit_keys():
    """num_nodes = 3 037 000 499, the largest the entry takes, and ids in the 50 values below it: keys row * n + col just under 2^63"""
    n = 3_037_000_499
    r = np.random.default_rng(0).integers(n - 50, n, size=(2, 4000))
    key = r[0].astype(object) * n + r[1].astype(object)                  # exact integers
    assert (1 << 62) < min(key) and max(key) < (1 << 63)
    want = _check_coalesce(r, n)
    assert 0 < want.shape[1] <= 2500 and want.shape[1] == len(set(key))


# ---- top-k table -> edges ----------------------------------------------------------------------------------------------
def test_topk_edges_past_the_grid_cap():
    from bridged_gnn_amd import ops
    nq, k, nc = 60_000, 20, 1000
    assert nq * k > CAP
    idx = np.random.default_rng(2).integers(0, nc, size=(nq, k))
    d = _t(idx)
    for cb, qb in ((0, 0), (7, 123)):
        got = ops.topk_edges(d, cand_base=cb, query_base=qb)
        assert got.dtype == torch.int64 and got.shape == (2, nq * k)
        assert np.array_equal(_np(got[0]), idx.reshape(-1) + cb)          # from = the selected candidate
        assert np.array_equal(_np(got[1]), np.repeat(np.arange(nq), k) + qb)   # to = the query
    assert np.array_equal(_np(d), idx)


# ---- gather_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,src_rows", [(40_000, 128, 5000), (1_100_000, 4, 70_000)])
def test_gather_rows_past_the_grid_cap(n, w, src_rows):
    from bridged_gnn_amd import ops
    assert n * (w // 4) > CAP                                             # one thread per 16-byte chunk
    g = torch.Generator(device=DEV).manual_seed(w)
    table = torch.randn(src_rows, w, device=DEV, generator=g)
    idx = torch.randint(0, src_rows, (n,), device=DEV, generator=g)
    idx[0], idx[1], idx[-1], idx[-2] = src_rows - 1, 0, 0, src_rows - 1
    assert n > src_rows and int(idx.min()) == 0 and int(idx.max()) == src_rows - 1    # repeats; both ends of the table
    want = table.index_select(0, idx).view(torch.int32)
    assert torch.equal(ops.gather_rows(table, idx).view(torch.int32), want)
    # out= a column slice of a wider buffer (the partitioned drivers' halo rows): the pad columns are not written
    buf = torch.full((n, w + 4), float("nan"), device=DEV)
    out = ops.gather_rows(table, idx, out=buf[:, :w])
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :w].contiguous().view(torch.int32), want)
    assert bool(torch.isnan(buf[:, w:]).all())


# ---- pair_csr ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_by,n_other,P", [(500, 40, 1_100_000), (40, 500, 50_000), (3000, 2000, 300_007), (1, 1, 5)])
def test_pair_csr_rowptr_and_perm(n_by, n_other, P):
    """pairs grouped by `idx_by`, input order inside a node; pairs with idx_by == idx_other are ordinary pairs"""
    from bridged_gnn_amd import ops
    if n_by == 500:
        assert P > CAP                                                    # no rewrite: the slots are the pairs
    rng = np.random.default_rng(P)
    by = rng.integers(0, n_by - 100 if n_by == 3000 else n_by, size=P)   # (3000, ...): the last 100 nodes receive no pair
    other = rng.integers(0, n_other, size=P)
    by[-1] = other[-1] = 0
    assert (by == other).any()
    rowptr, perm = ops.pair_csr(_t(by), _t(other), n_by, n_other)
    assert rowptr.dtype == perm.dtype == torch.int32
    assert rowptr.shape == (n_by + 1,) and perm.shape == (P,)
    assert np.array_equal(_np(rowptr), np.concatenate(([0], np.cumsum(np.bincount(by, minlength=n_by)))))
    assert np.array_equal(_np(perm), np.argsort(by, kind="stable"))
    assert int(rowptr[-1]) == P
