"""akz_fetch_pyramid on the host side: exported, declared by the binding, and its argument checks run before anything
touches a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AKZ_ERR_INVALID_ARG = -1


def test_fetch_pyramid_is_exported_and_declared(amd):
    L = amd.lib()
    assert hasattr(L, "akz_fetch_pyramid")
    assert "akz_fetch_pyramid" in L._declared
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "akaze_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+akz_fetch_pyramid\s*\(\s*const akz_result\*\s*res,\s*uint64_t img,\s*float\* const\* dst,"
                     r"\s*uint64_t n_dst,\s*uint64_t\* bytes_out\s*\)", hdr)


def test_fetch_pyramid_rejects_a_null_result_without_a_device(amd):
    L = amd.lib()
    assert L.akz_fetch_pyramid(None, 0, None, 0, None) == AKZ_ERR_INVALID_ARG
    assert L.akz_last_error()  # the message says why
