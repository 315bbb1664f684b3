"""CPU: the host half of the 32-byte-row layout of the eval classifier stage (classifier_stage.py: rows32_*): when the stage offers
the layout, and the pack / unpack / views of a [rows, 8] table against the padded [rows, 3 * 4] one.  No kernel runs here; the
walk's own plan (one window, hub rows, the environment switches) is a GPU-side question: tests/test_gpu_heads_rows32.py."""
import pytest
import torch

from bridged_gnn_amd.classifier_stage import ClassifierStage
from bridged_gnn_amd.ktgnn import KTGNN_no_complement


def _stage(C, root_weight=False):
    return KTGNN_no_complement(8, C, 2, 16, root_weight=root_weight, dim_share=8)._stage


@pytest.mark.parametrize("C,want", [(1, True), (2, True), (3, False)])
def test_layout_by_class_count(C, want):
    assert _stage(C).rows32_eligible() is want


def test_layout_needs_a_plain_stage_fp32_and_the_eval_forward():
    assert not _stage(2, root_weight=True).rows32_eligible()          # the convs' own forward: padded tables
    st = _stage(2)
    assert st.rows32_eligible(torch.float32, training=False)
    assert not st.rows32_eligible(torch.float32, training=True)
    assert not st.rows32_eligible(torch.float16) and not st.rows32_eligible(torch.float64)


def test_eval_tables_rows32_declines_without_touching_anything():
    """outside the host conditions the stage answers None before it looks at the device"""
    x = torch.zeros(5, 16, dtype=torch.float64)
    assert _stage(2).eval_tables_rows32(x, None, None, None, None) is None
    assert _stage(3).eval_tables_rows32(x.float(), None, None, None, None) is None
    assert _stage(2).eval_tables_rows32(x.float(), None, None, None, None) is None          # no domain sums: no one-pass producer


@pytest.mark.parametrize("C", [1, 2])
def test_pack_unpack_and_views(C):
    g = torch.Generator().manual_seed(C)
    padded = torch.zeros(7, 3, 4)
    padded[:, :, :C] = torch.randn(7, 3, C, generator=g)
    padded = padded.view(7, 12)
    t8 = ClassifierStage.rows32_pack(padded)
    assert t8.shape == (7, 8) and t8.is_contiguous()
    assert torch.equal(t8[:, 0:2], padded[:, 0:2]) and torch.equal(t8[:, 2:4], padded[:, 4:6]) and torch.equal(t8[:, 4:8], padded[:, 8:12])
    assert torch.equal(ClassifierStage.rows32_unpack(t8), padded)
    other = ClassifierStage.rows32_pack(-padded)
    views = ClassifierStage.rows32_views(t8, other)
    for j, (a, b) in enumerate(views):
        assert a.stride(0) == b.stride(0) == 8 and a.data_ptr() == t8.data_ptr() + 8 * j and b.data_ptr() == other.data_ptr() + 8 * j
        assert torch.equal(a[:, :C], padded[:, 4 * j:4 * j + C]) and torch.equal(b[:, :C], -padded[:, 4 * j:4 * j + C])
    assert views[2][0].shape[1] == 4                                   # head 2's view takes the padding along: one 16-byte store
