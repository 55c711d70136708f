"""The short-MSM entry points through the layers that need no GPU: the header, the library's exports, the Python binding."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pcdhip_msm_short", "pcdhip_msm_short_dev", "pcdhip_msm_set_short"]


def test_header_declares_the_three_functions():
    text = open(os.path.join(ROOT, "include", "pcdhip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*pcdhip_ctx\s*\*", text), name


def test_library_exports_and_binding_list():
    from pcd_amd import capi
    lib = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name


def test_null_context_is_an_argument_error():
    from pcd_amd import capi
    lib = capi.lib()
    out = (C.c_uint64 * 64)()
    z = C.c_size_t(0)
    assert lib.pcdhip_msm_short(None, None, z, None, z, out) == -1
    assert lib.pcdhip_msm_short_dev(None, None, z, None, z, z, out) == -1
    assert lib.pcdhip_msm_set_short(None, C.c_size_t(64)) == -1


def test_context_has_both_methods():
    from pcd_amd import capi
    assert callable(getattr(capi.Context, "msm_short", None))
    assert callable(getattr(capi.Context, "msm_set_short", None))
