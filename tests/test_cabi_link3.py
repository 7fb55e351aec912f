"""The 3-D batch link at the C ABI, without a GPU: ``ysmr_tracker_prepare3`` is declared in the header, exported by the
library and bound by ``_lib``; link mode 2 is a mode the library knows (a NULL handle fails on the handle, not on the mode)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ysmr_hip.h")


@pytest.fixture(scope="module")
def lib():
    """The library as tests/test_cabi.py loads it: built if it is absent, and every failure to load or bind it is a failure."""
    from ysmr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_prepare3_is_declared_with_the_third_coordinate_between_det_and_count():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+ysmr_tracker_prepare3\s*\(([^)]*)\)\s*;", text)
    assert m, "ysmr_tracker_prepare3 is not declared in include/ysmr_hip.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["ysmr_tracker *t", "void *stream", "const float *det_dev", "const double *third_dev",
                    "const int32_t *det_count_dev", "int batch", "int slot"]
    assert re.search(r"#define\s+YSMR_ABI_VERSION\s+15\b", text), "the export was added without a new ABI number"


def test_prepare3_is_exported_and_bound(lib):
    import ctypes
    from ysmr_amd import _lib
    L = lib
    assert "ysmr_tracker_prepare3" in _lib.EXPORTS
    assert hasattr(L, "ysmr_tracker_prepare3")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(L.ysmr_tracker_prepare3.argtypes) == [vp, vp, vp, vp, vp, ci, ci]
    assert L.ysmr_abi_version() == _lib.ABI_VERSION == 15


def test_null_handle_fails_on_the_handle_not_on_the_mode(lib):
    from ysmr_amd import _lib
    L = lib
    for mode in (0, 1, 2):
        assert L.ysmr_tracker_link_mode(None, mode) == _lib.YSMR_ERR_ARG
        assert b"handle is NULL" in L.ysmr_last_error()
    assert L.ysmr_tracker_prepare3(None, None, None, None, None, 1, 0) == _lib.YSMR_ERR_ARG
    assert b"handle is NULL" in L.ysmr_last_error()
