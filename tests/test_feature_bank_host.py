"""The feature bank without a GPU: the new entry points are exported, declared in the headers and bound with the documented
signatures; every refusal that the C ABI makes before it touches a device; and the refusals the Python wrappers make themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1

# name -> the parameter types of include/akaze_hip.h, as written there
DOCUMENTED = {
    "akz_bank_create_from_results": ["akz_ctx*", "const akz_result* const*", "uint64_t", "akz_bank**"],
    "akz_bank_create_from_sets": ["akz_ctx*", "const akz_feature_set*", "uint64_t", "uint64_t", "akz_bank**"],
    "akz_bank_info": ["const akz_bank*", "uint64_t*", "uint64_t*", "uint64_t*"],
    "akz_bank_set_info": ["const akz_bank*", "uint64_t", "uint64_t*", "uint64_t*", "uint64_t*"],
    "akz_bank_device": ["const akz_bank*", "const uint8_t**", "const float**", "const float**"],
    "akz_bank_free": ["akz_bank*"],
    "akz_match_features_seeded_bank_pairs": ["akz_ctx*", "const akz_bank*", "const uint64_t*", "uint64_t", "const akz_ransac_options*", "int",
                                             "akz_match*", "uint64_t*", "float*", "int*", "uint32_t*", "uint64_t*"],
    "akz_match_features_seeded_pose_bank_pairs": ["akz_ctx*", "const akz_bank*", "const akz_camera*", "const uint64_t*", "uint64_t",
                                                  "const akz_ransac_options*", "int", "akz_match*", "uint64_t*", "float*", "int*", "uint32_t*",
                                                  "uint64_t*", "akz_pose*", "float*"],
}


def prototypes(text):
    """name -> [parameter type, ...] of every `int name(...);` of a header, comments removed, parameter names dropped"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(akz_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?[\*\s])(\w+)$", a)  # the trailing identifier is the parameter's name
            types.append((m.group(1) if m else a).replace(" *", "*").strip())
        out[name] = types
    return out


def test_symbols_exported_declared_and_bound_as_documented(amd):
    L = amd.lib()
    protos = prototypes(open(os.path.join(ROOT, "include", "akaze_hip.h")).read())
    for name, want in DOCUMENTED.items():
        assert hasattr(L, name) and name in L._declared, name
        assert protos.get(name) == want, (name, protos.get(name))
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(want) and fn.restype is C.c_int, name
        for got, doc in zip(fn.argtypes, want):  # a scalar is bound as that scalar, a pointer as some pointer
            scalar = {"uint64_t": C.c_uint64, "int": C.c_int}.get(doc)
            assert got is scalar if scalar else got not in (C.c_uint64, C.c_int, C.c_uint32), (name, doc, got)
    debug = prototypes(open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read())
    assert debug.get("akz_debug_bank_gather") == ["akz_ctx*", "const uint8_t*", "uint64_t", "uint64_t", "uint8_t*"]
    assert "akz_debug_bank_gather" in L._declared and len(L.akz_debug_bank_gather.argtypes) == 5
    assert amd.KERNEL_ROW_KINDS[14] == "k_bank_gather"


def test_c_refusals_that_need_no_device(amd):
    L = amd.lib()
    out = C.c_void_p(0xdead)
    one = (C.c_void_p * 1)(None)
    fake_ctx = C.c_void_p(0)  # (every case below is refused before the context is looked at)
    assert L.akz_bank_create_from_results(fake_ctx, one, 1, C.byref(out)) == INVALID_ARG and out.value is None
    assert "null" in L.akz_last_error().decode()
    out = C.c_void_p(0xdead)
    assert L.akz_bank_create_from_results(None, None, 0, C.byref(out)) == INVALID_ARG and out.value is None
    assert L.akz_bank_create_from_results(None, one, 1, None) == INVALID_ARG
    # from sets: the refusals akz_match_features_pairs makes for a set, for every set
    kp = np.zeros(2, amd.KEYPOINT_DTYPE)
    d = np.zeros((3, 61), np.uint8)
    sets = (amd.FeatureSet * 2)()
    sets[0] = amd.FeatureSet(kp.ctypes.data, 2, d.ctypes.data, 2)
    for bad, word in ((amd.FeatureSet(kp.ctypes.data, 2, d.ctypes.data, 3), "more descriptors than keypoints"),
                      (amd.FeatureSet(None, 2, d.ctypes.data, 2), "null keypoints or descriptors"),
                      (amd.FeatureSet(kp.ctypes.data, 2, None, 2), "null keypoints or descriptors")):
        sets[1] = bad
        out = C.c_void_p(0xdead)
        assert L.akz_bank_create_from_sets(None, C.cast(sets, C.c_void_p), 2, 61, C.byref(out)) == INVALID_ARG and out.value is None
        msg = L.akz_last_error().decode()
        assert word in msg and "set 1" in msg, msg
    sets[1] = sets[0]
    for nb in (0, 65):
        assert L.akz_bank_create_from_sets(None, C.cast(sets, C.c_void_p), 2, nb, C.byref(out)) == INVALID_ARG
        assert "desc_bytes" in L.akz_last_error().decode()
    assert L.akz_bank_create_from_sets(None, None, 2, 61, C.byref(out)) == INVALID_ARG
    assert L.akz_bank_create_from_sets(None, C.cast(sets, C.c_void_p), 2, 61, None) == INVALID_ARG
    assert L.akz_bank_create_from_sets(None, C.cast(sets, C.c_void_p), 2, 61, C.byref(out)) == INVALID_ARG  # a null context, last
    assert "null context" in L.akz_last_error().decode()
    # accessors and calls on a null bank
    n = C.c_uint64(77)
    assert L.akz_bank_info(None, C.byref(n), None, None) == INVALID_ARG and n.value == 77
    assert L.akz_bank_set_info(None, 0, C.byref(n), None, None) == INVALID_ARG and n.value == 77
    assert L.akz_bank_device(None, None, None, None) == INVALID_ARG
    assert L.akz_bank_free(None) == 0
    opt = amd.RansacOptions()
    pairs = np.array([0, 1], np.uint64)
    cnt = np.full(1, 99, np.uint64)
    assert L.akz_match_features_seeded_bank_pairs(None, None, pairs.ctypes.data, 1, C.byref(opt), 0, None,
                                                  cnt.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None, None) == INVALID_ARG
    assert "null bank" in L.akz_last_error().decode() and cnt[0] == 99
    assert L.akz_match_features_seeded_pose_bank_pairs(None, None, None, pairs.ctypes.data, 1, C.byref(opt), 0, None,
                                                       cnt.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None, None, None, None) == INVALID_ARG
    assert "null bank" in L.akz_last_error().decode() and cnt[0] == 99


class _Ctx:
    """stands in for a Context where the wrapper must refuse before it reaches the library"""
    _h = None


def _fake_bank(amd, ctx, rows=(3, 0, 2)):
    class Fake(amd.FeatureBank):
        def info(self):
            sets, at = [], 0
            for r in rows:
                sets.append(dict(n_keypoints=r, n_descriptors=r, row0=at))
                at += r
            return dict(n_sets=len(rows), desc_bytes=61, rows=at, sets=sets)

    return Fake(ctx, None)


def test_python_refusals(amd):
    c = _Ctx()
    for bad in ("features.bin", b"x", 7, None):
        with pytest.raises(TypeError):
            amd.Context.feature_bank(c, bad)
    with pytest.raises(TypeError, match="host set"):
        amd.Context.feature_bank(c, [np.zeros((2, 61), np.uint8)])
    with pytest.raises(ValueError, match="descriptor lengths differ"):
        amd.Context.feature_bank(c, [(np.zeros(2, amd.KEYPOINT_DTYPE), np.zeros((2, 61), np.uint8)),
                                     (np.zeros(2, amd.KEYPOINT_DTYPE), np.zeros((2, 21), np.uint8))])
    bank = _fake_bank(amd, c)
    with pytest.raises(TypeError):
        amd.Context.feature_bank(c, bank)
    with pytest.raises(ValueError):  # an odd number of indices is no list of pairs
        amd.Context.match_features_seeded_pairs(c, bank, [0, 1, 2])
    with pytest.raises(ValueError):
        amd.Context.match_features_seeded_pose_pairs(c, bank, [(1, 1, 0, 0)] * 3, [0, 1, 2])
    with pytest.raises(ValueError, match="3 feature sets but 2 cameras"):
        amd.Context.match_features_seeded_pose_pairs(c, bank, [(1, 1, 0, 0)] * 2, [(0, 2)])
    with pytest.raises(ValueError, match="another context"):
        amd.Context.match_features_seeded_pairs(_Ctx(), bank, [(0, 2)])
    with pytest.raises(TypeError, match="seeded pairs calls"):  # the host-draw calls have no bank form
        amd.Context.match_features_pairs(c, bank, [(0, 2)], 0.86, 100, 0.02)
    with pytest.raises(TypeError):
        amd.Context.match_features_seeded_pairs(c, 5, [(0, 1)])
    # the layout the wrapper hands to the library: fixed room per pair from the bank's counts, none for an index beyond it
    a = amd._PairsArgs(c, bank, [(0, 2), (1, 0), (2, 2), (5, 0)], bank_ok=True)
    assert a.rows == [3, 0, 2, 0] and len(a.out) == 5 and a.n_sets == 3 and len(a.head) == 4
