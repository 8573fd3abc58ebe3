"""CPU: the C-ABI shared library loads and exports exactly what include/vlg_hip.h declares
(no compute calls - there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "vlg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef VLG_DIAG.*?#endif", "", text, flags=re.S)      # diagnostic-build-only entry points
    return sorted(set(re.findall(r"\b(vlg_[a-z0-9_]+)\s*\(", text)))


def test_header_lists_entry_points():
    names = declared_symbols()
    assert len(names) >= 24 and "vlg_linear_fwd" in names and "vlg_adam_step" in names


def test_library_exports_every_declared_symbol():
    from vlg import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.fail("libvlg_hip.so is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), "missing export " + name


def test_binding_covers_header_and_types_resolve():
    from vlg import hip
    assert sorted(hip.SIGNATURES) == declared_symbols()
    lib = hip.load()
    assert lib.vlg_abi_version() == 1
    assert lib.vlg_build_arch() == b"gfx950"
    # pure host-side planners can be called without a GPU
    assert lib.vlg_embed_bwd_slabs() > 0
    assert 1 <= lib.vlg_linear_wgrad_slabs(32768, 768, 256) <= 128
    assert lib.vlg_linear_wgrad_slabs(128, 64, 64) == 1
    plan = (ctypes.c_int64 * 12)()                                                            # sizeof(vlg_gemm_plan) = 80
    assert lib.vlg_linear_plan(2, 32768, 768, 256, 0, 768, 256, 0, 0, plan) == 0            # the weight gradient's plan
    ints = (ctypes.c_int * 24).from_buffer(plan)                                              # family, launches, problems, fused, p[0] ...
    assert list(ints[:4]) == [0, 1, 1, 0] and ints[8] == lib.vlg_linear_wgrad_slabs(32768, 768, 256)
    assert lib.vlg_linear_plan(2, 32768, 770, 256, 0, 770, 256, 0, 0, plan) == 1001          # N not a multiple of 4
    assert lib.vlg_layout_loss_scratch() > 4 and lib.vlg_image_loss_scratch() > 4


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(ROOT, "video-layout-generation_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dirpath, f)
                assert "layout_spec" not in src and "vlg_oracle" not in src, os.path.join(dirpath, f)


def test_product_library_has_no_debug_setters():
    """include/vlg_hip.h promises a library without mutable process-wide state: the vlg_debug_set_* switches exist only in
    the diagnostic build (make diag, -DVLG_DIAG), never in the library the product loads."""
    from vlg import hip
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("vlg_debug_set_clock_probe", "vlg_debug_set_conv_probe", "vlg_debug_set_gemm_bk", "vlg_debug_set_gemm_run"):
        assert not hasattr(lib, name), name


def test_product_library_reads_no_tuning_variables():
    """Every kernel and slab plan of the product library follows from the call's arguments: the development tuning
    variables (VLG_TUNE in csrc/common.h) are read by the diagnostic build only, so their names are not in the product .so."""
    from vlg import hip
    data = open(hip.LIB_PATH, "rb").read()
    for name in ("VLG_GEMM_BK", "VLG_GEMM_SMALL", "VLG_GEMM_SMALL_BELOW", "VLG_GEMM_SMALL_BELOW_WGRAD", "VLG_WGRAD_SMALL_SLOTS",
                 "VLG_GEMM_PAIR", "VLG_CONV_NARROW_BK", "VLG_CONV_TAIL", "VLG_CONV_WGRAD_TALL", "VLG_EMBED_PREFETCH"):
        assert name.encode() not in data, name
