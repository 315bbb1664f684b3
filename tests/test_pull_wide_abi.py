"""CPU: the pull-form backward has ONE entry and one workspace function per operation (single head, interleaved heads) in the
declared C ABI (include/bgnn.h) and in the ctypes binding; test_library_exports_every_declared_symbol then covers the export itself."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = ("bgnn_aggregate_bwd_pull_workspace_bytes", "bgnn_adaptedconv_aggregate_bwd_pull_f32",
        "bgnn_aggregate_heads_bwd_workspace_bytes", "bgnn_adaptedconv_aggregate_heads_bwd_f32")
GONE = ("bgnn_aggregate_bwd_pull_hub_workspace_bytes", "bgnn_adaptedconv_aggregate_bwd_pull_hub_f32",
        "bgnn_aggregate_bwd_pull_wide_workspace_bytes", "bgnn_adaptedconv_aggregate_bwd_pull_wide_f32",
        "bgnn_aggregate_heads_bwd_hub_workspace_bytes", "bgnn_adaptedconv_aggregate_heads_bwd_hub_f32")


def test_wide_pull_entries_are_declared_and_bound():
    from bridged_gnn_amd import _lib
    raw = open(os.path.join(ROOT, "include", "bgnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in KEPT:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in bgnn.h"
        assert name in _lib.SIGNATURES
    for name in GONE:
        assert name not in raw, f"{name} still in bgnn.h"
        assert name not in _lib.SIGNATURES
    # both entries end in the same hub-table argument group, workspace and stream (16 arguments), as the header says
    assert _lib.SIGNATURES[KEPT[1]][1][-16:] == _lib.SIGNATURES[KEPT[3]][1][-16:]
    assert len(_lib.SIGNATURES[KEPT[1]][1]) == 40 and len(_lib.SIGNATURES[KEPT[3]][1]) == 38
    assert "bgnn_aggregate_bwd_wide.hip" in _lib._HASHED_SOURCES
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    assert "bgnn_aggregate_bwd_wide.hip" in mk
    # the shared conv header is hashed, and the Makefile's digest reads the same files in the same order as the loader's
    assert "bgnn_conv_common.h" in _lib._HASHED_SOURCES
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    hashed = re.search(r"^HASHED\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(SRCS)", " ".join(srcs)).split()
    assert [os.path.normpath(f) for f in hashed] == [os.path.normpath(f) for f in _lib._HASHED_SOURCES]
