"""Host: the torch views on top of a by-destination CSR -- `DstCSR.transposed()`, `DstCSR.hub_tables()` and
`DstCSR.transposed_hub_tables()` -- on CPU tensors against a few lines of numpy.  The rows carry chosen in-degrees at every
boundary of the hub arithmetic: 0, 1, threshold - 1, threshold, threshold + 1, an exact multiple of the segment and one past it.
Everything is integer work, so every comparison is exact."""
import numpy as np
import pytest
import torch

from bridged_gnn_amd import ops
from bridged_gnn_amd.ops import DstCSR

KEYS = ((ops.HUB_THRESHOLD, ops.HUB_SEGMENT), (16, 8))


def _csr_cpu(src, dst, n):
    """what bgnn_build_dst_csr returns without the self-loop rewrite, on CPU tensors"""
    order = np.argsort(dst, kind="stable")
    col = src[order].astype(np.int32)
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(dst, minlength=n)))).astype(np.int32)
    return DstCSR(torch.from_numpy(rowptr), torch.from_numpy(col), None, col.shape[0], n)


def _graph(threshold, segment, seed, n=400):
    """(DstCSR, src, dst in CSR order, in-degrees).  Rows 0..6 have the boundary in-degrees, the rest fewer than 6; source 11 has
    exactly `threshold` out-edges and source 12 `5 * segment + 1`, every other source far fewer."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 6, n)
    deg[:7] = (0, 1, threshold - 1, threshold, threshold + 1, 5 * segment, 5 * segment + 1)
    deg[n - 1] = 2 * threshold + 3                                       # a hub in the last row: rowptr[N] is its end
    dst = np.repeat(np.arange(n), deg)
    rng.shuffle(dst)                                                     # input order is not row order
    E = dst.shape[0]
    src = rng.integers(13, n, E)                                         # about E / n out-edges each
    pick = rng.permutation(E)
    src[pick[:threshold]] = 11
    src[pick[threshold:threshold + 5 * segment + 1]] = 12
    assert np.bincount(src, minlength=n)[13:].max() < threshold          # no other source is a hub
    csr = _csr_cpu(src, dst, n)
    order = np.argsort(dst, kind="stable")
    return csr, src[order], dst[order], deg


def _check_hub_tables(tables, rowptr, deg, threshold, segment):
    hub_rows, hub_seg_ptr, seg_bounds, seg_node = (t.numpy() for t in tables)
    assert all(t.dtype == torch.int32 for t in tables)
    want_rows = np.flatnonzero(deg >= threshold)
    assert np.array_equal(hub_rows, want_rows)                           # exactly the rows at or above the threshold, ascending
    nseg = -(-deg[want_rows] // segment)
    assert np.array_equal(hub_seg_ptr, np.concatenate(([0], np.cumsum(nseg))))
    assert seg_bounds.shape == (2 * nseg.sum(),) and seg_node.shape == (nseg.sum(),)
    b = seg_bounds.reshape(-1, 2)
    for i, h in enumerate(want_rows):
        lo, hi = hub_seg_ptr[i], hub_seg_ptr[i + 1]
        assert (seg_node[lo:hi] == h).all()
        assert b[lo, 0] == rowptr[h] and b[hi - 1, 1] == rowptr[h + 1]
        assert np.array_equal(b[lo + 1:hi, 0], b[lo:hi - 1, 1])          # contiguous
        lens = b[lo:hi, 1] - b[lo:hi, 0]
        assert (lens[:-1] == segment).all() and 0 < lens[-1] <= segment  # only the last may be shorter
    return want_rows


@pytest.mark.parametrize("threshold,segment", KEYS)
def test_transposed_is_the_stable_by_source_view(threshold, segment):
    csr, src, dst, _ = _graph(threshold, segment, seed=1)
    n = csr.num_nodes
    t_rowptr, t_eid, t_dst = csr.transposed()
    assert t_rowptr.dtype == t_eid.dtype == t_dst.dtype == torch.int32
    order = np.argsort(src, kind="stable")
    assert np.array_equal(t_eid.numpy(), order)
    assert np.array_equal(t_dst.numpy(), dst[order])
    assert np.array_equal(t_rowptr.numpy(), np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n)))))
    assert csr.transposed() is csr.transposed()                          # built once


@pytest.mark.parametrize("threshold,segment", KEYS)
def test_hub_tables_cut_rows_at_the_threshold_into_segments(threshold, segment):
    csr, _, _, deg = _graph(threshold, segment, seed=2)
    hubs = _check_hub_tables(csr.hub_tables(threshold, segment), csr.rowptr.numpy(), deg, threshold, segment)
    assert set((3, 4, csr.num_nodes - 1)) <= set(hubs.tolist()) and 2 not in hubs     # threshold - 1 is no hub, threshold is
    if (threshold, segment) == KEYS[0]:
        assert csr.hub_tables() is csr.hub_tables(threshold, segment)    # the defaults are this key


@pytest.mark.parametrize("threshold,segment", KEYS)
def test_transposed_hub_tables_cut_sources_the_same_way(threshold, segment):
    csr, src, _, _ = _graph(threshold, segment, seed=3)
    outdeg = np.bincount(src, minlength=csr.num_nodes)
    assert outdeg[11] == threshold and outdeg[12] == 5 * segment + 1
    hubs = _check_hub_tables(csr.transposed_hub_tables(threshold, segment), csr.transposed()[0].numpy(), outdeg, threshold, segment)
    assert hubs.tolist() == ([11, 12] if 5 * segment + 1 >= threshold else [11])


def test_no_row_at_the_threshold_gives_none_and_the_cache_is_keyed():
    csr, src, _, deg = _graph(*KEYS[0], seed=4)
    assert csr.hub_tables(int(deg.max()) + 1, 8) is None
    assert csr.hub_tables(int(deg.max()), 8) is not None                 # >=, not >
    outdeg = np.bincount(src, minlength=csr.num_nodes)
    assert csr.transposed_hub_tables(int(outdeg.max()) + 1, 8) is None
    a, b = csr.hub_tables(16, 8), csr.hub_tables()
    assert a is not None and b is not None
    assert a[0].numel() > b[0].numel() and a[2].numel() > b[2].numel()   # different keys, different tables
    _check_hub_tables(a, csr.rowptr.numpy(), deg, 16, 8)                 # rows of the other key's graph: 127 = 15 * 8 + 7, 128 = 16 * 8
    assert csr.hub_tables(16, 8) is a and csr.hub_tables(*KEYS[0]) is b
    ta = csr.transposed_hub_tables(16, 8)
    assert ta is not a and not (ta[0].shape == a[0].shape and torch.equal(ta[0], a[0]))   # the by-source key is its own
    # a graph of isolated nodes and one of a single edge
    empty = _csr_cpu(np.zeros(0, np.int64), np.zeros(0, np.int64), 5)
    assert empty.hub_tables(1, 1) is None and empty.transposed_hub_tables(1, 1) is None
    one = _csr_cpu(np.array([2]), np.array([4]), 5)
    hr, sp, bd, sn = one.hub_tables(1, 64)
    assert hr.tolist() == [4] and sp.tolist() == [0, 1] and bd.tolist() == [0, 1] and sn.tolist() == [4]
    hr, sp, bd, sn = one.transposed_hub_tables(1, 64)
    assert hr.tolist() == [2] and sp.tolist() == [0, 1] and bd.tolist() == [0, 1] and sn.tolist() == [2]
