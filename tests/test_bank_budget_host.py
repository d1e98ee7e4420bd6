"""The feature bank under a keypoint budget without a GPU: the new entry points are exported, declared in the headers and bound with
the documented signatures; every refusal that the C ABI makes before it touches a device -- each made with a NULL context, which
shows that it comes before the context is read; and the refusals the Python wrappers make themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1

# name -> the parameter types of include/akaze_hip.h, as written there
DOCUMENTED = {
    "akz_bank_create_from_results_budget": ["akz_ctx*", "const akz_result* const*", "uint64_t", "const akz_keypoint_budget*", "akz_bank**"],
    "akz_bank_create_from_sets_budget": ["akz_ctx*", "const akz_feature_set*", "uint64_t", "uint64_t", "const akz_keypoint_budget*", "akz_bank**"],
    "akz_bank_set_indices": ["const akz_bank*", "uint64_t", "uint64_t*"],
}
DEBUG_HOOK = ["akz_ctx*", "const uint8_t*", "const float*", "const float*", "uint64_t", "const uint64_t*", "const uint64_t*", "const uint32_t*",
              "uint64_t", "uint8_t*", "float*", "float*", "uint32_t*"]


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


def bound_as(fn, want):
    """a scalar is bound as that scalar, a pointer as some pointer"""
    assert len(fn.argtypes) == len(want) and fn.restype is C.c_int
    for got, doc in zip(fn.argtypes, want):
        scalar = {"uint64_t": C.c_uint64, "int": C.c_int}.get(doc)
        assert got is scalar if scalar else got not in (C.c_uint64, C.c_int, C.c_uint32), (doc, got)


def test_symbols_exported_declared_and_bound_as_documented(amd):
    L = amd.lib()
    protos = prototypes(open(os.path.join(ROOT, "include", "akaze_hip.h")).read())
    for name, want in DOCUMENTED.items():
        assert hasattr(L, name) and name in L._declared, name
        assert protos.get(name) == want, (name, protos.get(name))
        bound_as(getattr(L, name), want)
    debug_text = open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read()
    assert prototypes(debug_text).get("akz_debug_bank_select") == DEBUG_HOOK
    assert hasattr(L, "akz_debug_bank_select") and "akz_debug_bank_select" in L._declared
    bound_as(L.akz_debug_bank_select, DEBUG_HOOK)
    # the kernel row: appended, and the numbers before it have not moved
    assert re.search(r"\bAKZ_KR_BANK_SELECT\s*=\s*15\b", debug_text)
    assert re.search(r"\bAKZ_KR_MASK_CANDIDATES\s*=\s*13\b", debug_text) and re.search(r"\bAKZ_KR_BANK_GATHER\s*=\s*14\b", debug_text)
    assert amd.KERNEL_ROW_KINDS[15] == "k_bank_select" and amd.KERNEL_ROW_KINDS[14] == "k_bank_gather"


def two_sets(amd, n=(3, 2)):
    kps = [np.zeros(k, amd.KEYPOINT_DTYPE) for k in n]
    for k in kps:
        k["x"], k["y"], k["response"] = np.arange(len(k)), 1.0, 0.5
    ds = [np.ones((k, 61), np.uint8) for k in n]
    sets = (amd.FeatureSet * len(n))()
    for i, (k, d) in enumerate(zip(kps, ds)):
        sets[i] = amd.FeatureSet(k.ctypes.data, len(k), d.ctypes.data, len(d))
    return sets, kps, ds


def from_sets(amd, sets, n_sets, budget, desc_bytes=61):
    """the from-sets form with a NULL context -> (status, *out, the message)"""
    out = C.c_void_p(0xdead)
    status = amd.lib().akz_bank_create_from_sets_budget(None, C.cast(sets, C.c_void_p) if sets is not None else None, n_sets, desc_bytes,
                                                        C.byref(budget) if budget is not None else None, C.byref(out))
    return status, out.value, amd.lib().akz_last_error().decode()


def test_c_refusals_that_need_no_device(amd):
    L = amd.lib()
    sets, kps, ds = two_sets(amd)
    good = amd.KeypointBudget(2, amd.BUDGET_SPREAD, 0.9)
    # the budget's option refusals
    status, out, msg = from_sets(amd, sets, 2, None)
    assert status == INVALID_ARG and out is None and "null options" in msg, msg
    status, out, msg = from_sets(amd, sets, 2, amd.KeypointBudget(2, 7, 0.9))
    assert status == INVALID_ARG and out is None and "unknown mode 7" in msg, msg
    for robust in (0.0, 1.5, float("nan")):
        status, out, msg = from_sets(amd, sets, 2, amd.KeypointBudget(2, amd.BUDGET_SPREAD, robust))
        assert status == INVALID_ARG and out is None and "robust" in msg, (robust, msg)
        status, out, msg = from_sets(amd, sets, 2, amd.KeypointBudget(2, amd.BUDGET_STRONGEST, robust))  # STRONGEST does not read it
        assert status == INVALID_ARG and out is None and "null context" in msg, (robust, msg)
    # ... and those of a set: a value that is not finite, named by its set
    for field, bad in (("response", np.inf), ("response", np.nan), ("x", -np.inf), ("y", np.nan)):
        keep = kps[1][field][1]
        kps[1][field][1] = bad
        status, out, msg = from_sets(amd, sets, 2, good)
        kps[1][field][1] = keep
        assert status == INVALID_ARG and out is None and "set 1" in msg and "keypoint 1" in msg and "not finite" in msg, (field, msg)
    # the budget is defined over keypoints that all have a row
    sets[1] = amd.FeatureSet(kps[1].ctypes.data, 2, ds[1].ctypes.data, 1)
    status, out, msg = from_sets(amd, sets, 2, good)
    assert status == INVALID_ARG and out is None and "set 1" in msg and "1 descriptors for 2 keypoints" in msg, msg
    # the refusals of akz_bank_create_from_sets
    sets[1] = amd.FeatureSet(None, 2, ds[1].ctypes.data, 2)
    status, out, msg = from_sets(amd, sets, 2, good)
    assert status == INVALID_ARG and out is None and "null keypoints or descriptors" in msg and "set 1" in msg, msg
    sets[1] = amd.FeatureSet(kps[1].ctypes.data, 2, ds[1].ctypes.data, 2)
    for nb in (0, 65):
        status, out, msg = from_sets(amd, sets, 2, good, desc_bytes=nb)
        assert status == INVALID_ARG and out is None and "desc_bytes" in msg
    status, out, msg = from_sets(amd, None, 2, good)
    assert status == INVALID_ARG and out is None and "null sets" in msg
    assert L.akz_bank_create_from_sets_budget(None, C.cast(sets, C.c_void_p), 2, 61, C.byref(good), None) == INVALID_ARG
    status, out, msg = from_sets(amd, sets, 2, good)  # a null context, last
    assert status == INVALID_ARG and out is None and "null context" in msg, msg
    # from results: the budget's options come before the context and the results are looked at
    one = (C.c_void_p * 1)(None)
    for budget, word in ((None, "null options"), (amd.KeypointBudget(2, 7, 0.9), "unknown mode"), (amd.KeypointBudget(2, amd.BUDGET_SPREAD, 0.0), "robust")):
        out = C.c_void_p(0xdead)
        assert L.akz_bank_create_from_results_budget(None, one, 1, C.byref(budget) if budget is not None else None, C.byref(out)) == INVALID_ARG
        assert out.value is None and word in L.akz_last_error().decode(), L.akz_last_error().decode()
    out = C.c_void_p(0xdead)
    assert L.akz_bank_create_from_results_budget(None, one, 1, C.byref(good), C.byref(out)) == INVALID_ARG and out.value is None
    assert "null" in L.akz_last_error().decode()
    assert L.akz_bank_create_from_results_budget(None, one, 1, C.byref(good), None) == INVALID_ARG
    # the indices of a null bank
    idx = np.full(4, 77, np.uint64)
    assert L.akz_bank_set_indices(None, 0, idx.ctypes.data_as(C.POINTER(C.c_uint64))) == INVALID_ARG and np.all(idx == 77)
    assert "null bank" in L.akz_last_error().decode()


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
    sets = [(np.zeros(2, amd.KEYPOINT_DTYPE), np.zeros((2, 61), np.uint8))] * 2
    for bad in (1000, (1000, amd.BUDGET_SPREAD, 0.9), dict(max_keypoints=1000), "spread", amd.RansacOptions()):
        with pytest.raises(TypeError, match="KeypointBudget"):
            amd.Context.feature_bank(c, sets, budget=bad)
    with pytest.raises(TypeError, match="host set"):  # the source is still looked at as before
        amd.Context.feature_bank(c, [np.zeros((2, 61), np.uint8)], budget=amd.KeypointBudget(1, amd.BUDGET_STRONGEST, 0.9))
    with pytest.raises(amd.AkazeError, match="null context"):  # a budget of the right type reaches the library
        amd.Context.feature_bank(c, sets, budget=amd.KeypointBudget(1, amd.BUDGET_STRONGEST, 0.9))
    bank = _fake_bank(amd, c)
    for bad in (3, -1, 99):
        with pytest.raises(IndexError):
            bank.indices(bad)
    for call in (lambda: bank.indices(0), lambda: bank.indices(1), lambda: bank.indices()):  # in range: the library's to answer
        with pytest.raises(amd.AkazeError, match="null bank"):
            call()
