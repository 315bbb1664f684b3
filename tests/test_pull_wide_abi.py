"""CPU: the D > 128 pull-form backward is part of the declared C ABI (include/bgnn.h) and of the ctypes binding;
test_library_exports_every_declared_symbol then covers the export itself."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bgnn_aggregate_bwd_pull_wide_workspace_bytes", "bgnn_adaptedconv_aggregate_bwd_pull_wide_f32")


def test_wide_pull_entries_are_declared_and_bound():
    from bridged_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgnn.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} not declared in bgnn.h"
        assert name in _lib.SIGNATURES
    # the argument list of bgnn_adaptedconv_aggregate_bwd_pull_hub_f32, as the header says
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES["bgnn_adaptedconv_aggregate_bwd_pull_hub_f32"]
    assert "bgnn_aggregate_bwd_wide.hip" in _lib._HASHED_SOURCES
    mk = open(os.path.join(ROOT, "bridged_gnn_amd", "csrc", "Makefile")).read()
    assert "bgnn_aggregate_bwd_wide.hip" in mk
