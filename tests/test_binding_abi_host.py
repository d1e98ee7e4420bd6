"""The Python binding against the C headers and at its smallest shapes (host only, no GPU call): every declared function's
argtypes and restype against its prototype by ABI class, the refusal of two descriptor widths in the descriptor-only calls, and
the pair packer over row counts {0, 1, 2}^2 against a numpy Hamming scan written here."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENUMS = ("akz_status", "akz_plane", "akz_frame_format", "akz_stage")  # the enums of the headers: int in the ABI
C_CLASS = {"uint64_t": "u64", "size_t": "u64", "uint32_t": "u32", "int": "i32", "int32_t": "i32", "float": "f32", "double": "f64",
           **{e: "i32" for e in ENUMS}}
CTYPES_CLASS = {C.c_uint64: "u64", C.c_size_t: "u64", C.c_uint32: "u32", C.c_int: "i32", C.c_int32: "i32", C.c_float: "f32",
                C.c_double: "f64", C.c_void_p: "ptr", C.c_char_p: "ptr", None: "void"}


def c_class(decl):
    """ABI class of a C parameter or return type: 'const uint8_t* d0', 'uint64_t out[6]', 'akz_plane plane', 'void'"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w not in ("const", "unsigned", "struct", "enum")]
    assert words and words[0] in C_CLASS or words == ["void"], f"unknown C type in {decl!r}"
    return "void" if words == ["void"] else C_CLASS[words[0]]


def ctypes_class(t):
    if t is not None and issubclass(t, C._Pointer):
        return "ptr"
    assert t in CTYPES_CLASS, f"unknown ctypes type {t!r}"
    return CTYPES_CLASS[t]


def prototypes():
    """{name: (return class, [parameter classes])} of every akz_* function the two headers declare"""
    protos = {}
    for name in ("akaze_hip.h", "akaze_hip_debug.h"):
        hdr = open(os.path.join(ROOT, "include", name)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # (as tests/test_host.py and tools/check_shim.py do)
        hdr = re.sub(r"//[^\n]*", "", hdr)
        hdr = re.sub(r"^\s*#[^\n]*", "", hdr, flags=re.M)
        for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(akz_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
            ret, fn, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
            assert fn not in protos, f"{fn} is declared twice"
            args = [] if params in ("", "void") else [c_class(p.strip()) for p in params.split(",")]
            protos[fn] = (c_class(ret), args)
    return protos


def test_every_declared_function_matches_its_prototype(amd):
    L = amd.lib()
    protos = prototypes()
    assert sorted(protos) == list(L._declared), (sorted(set(protos) ^ set(L._declared)))
    assert len(protos) >= 216
    bad = []
    for name, (ret, args) in protos.items():
        fn = getattr(L, name)
        got = [ctypes_class(t) for t in fn.argtypes]
        if got != args:
            bad.append(f"{name}: binding {got}, header {args}")
        if ctypes_class(fn.restype) != ret:
            bad.append(f"{name}: binding returns {ctypes_class(fn.restype)}, header {ret}")
    assert not bad, "\n".join(bad)


def test_the_parser_reads_what_it_should():
    """the classes of a few prototypes, written out by hand: an enum, an array parameter, a void and a pointer return"""
    p = prototypes()
    assert p["akz_last_error"] == ("ptr", []) and p["akz_image_free"] == ("void", ["ptr"]) and p["akz_ctx_stream"] == ("ptr", ["ptr"])
    assert p["akz_fetch_plane"] == ("i32", ["ptr", "u64", "u64", "i32", "ptr", "ptr"])
    assert p["akz_debug_resource_counts"] == ("i32", ["ptr"])
    assert p["akz_gaussian_kernel"] == ("i32", ["f32", "u64", "ptr"])
    assert p["akz_match_features_fundamental_refined_guided_pairs"] == (
        "i32", ["ptr", "ptr", "u64", "ptr", "u64", "u64", "f64", "u64", "f32", "u32", "f32", "f64", "ptr", "ptr", "ptr", "ptr", "ptr"])


# ---- the numpy statement: feature_matching.rs:37-81 ------------------------------------------------------------------------
def np_match(d0, d1, threshold=10000, ratio=0.86):
    out = []
    for i in range(len(d0)):
        mn = second = threshold
        mj = 0
        for j in range(len(d1)):
            d = int(np.unpackbits(d0[i] ^ d1[j]).sum())
            if d < mn:
                second, mn, mj = mn, d, j
            elif d < second:
                second = d
        if float(mn) < float(second) * (ratio * ratio) and mn < threshold:
            out.append((i, mj, float(mn)))
    return out


def np_cross(d0, d1):
    back = {(i, j) for j, i, _ in np_match(d1, d0)}
    return [m for m in np_match(d0, d1) if (m[0], m[1]) in back]


def _as_list(m):
    return [(int(a), int(b), float(c)) for a, b, c in zip(m["index_0"], m["index_1"], m["distance"])]


def _rows(n0, n1, nb):
    """n0 and n1 rows of nb bytes: row 0 of the second set is row n0 - 1 of the first with one bit flipped, the rest is random"""
    rng = np.random.default_rng(1000 * nb + 10 * n0 + n1)
    d0 = rng.integers(0, 256, (n0, nb), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, nb), dtype=np.uint8)
    if n0 and n1:
        d1[0] = d0[n0 - 1]
        d1[0, nb // 2] ^= 4
    return d0, d1


EMPTY_FORMS = [(0, 61), (0, 32), (0,)]


# ---- two widths are refused once both sides have rows; an empty side of any form is not ---------------------------------------
def test_the_descriptor_only_calls_refuse_two_widths(amd):
    d0, d1 = np.zeros((2, 61), np.uint8), np.zeros((2, 32), np.uint8)
    for a, b in ((d0, d1), (d1, d0)):
        with pytest.raises(ValueError, match="descriptor lengths differ"):
            amd.descriptor_match_cross_host(a, b)
        with pytest.raises(ValueError, match="descriptor lengths differ"):
            amd.descriptor_match_knn_host(a, b, 2)


@pytest.mark.parametrize("empty", EMPTY_FORMS)
@pytest.mark.parametrize("nb", [61, 32])
def test_an_empty_side_is_not_a_width(amd, nb, empty):
    full, _ = _rows(2, 0, nb)
    none = np.zeros(empty, np.uint8)
    for d0, d1 in ((full, none), (none, full), (none, none)):
        n0 = len(d0) if d0.ndim == 2 else 0
        m = amd.descriptor_match_cross_host(d0, d1)
        assert m.dtype == amd.MATCH_DTYPE and len(m) == 0
        rec, cnt = amd.descriptor_match_knn_host(d0, d1, 3)
        assert rec.shape == (n0, 3) and rec.dtype == amd.MATCH_DTYPE and cnt.shape == (n0,) and cnt.dtype == np.uint32
        assert not cnt.any() and np.all(rec["index_1"] == 2**64 - 1) and np.all(np.isinf(rec["distance"]))  # every slot unused


# ---- the pair packer at its smallest shapes ---------------------------------------------------------------------------------
ALL_PASS = np.eye(3, dtype=np.float32)  # H = I with a radius beyond every distance: the gate passes every pair


def _keypoints(amd, n, empty_list):
    if n == 0:
        return [] if empty_list else np.zeros(0, amd.KEYPOINT_DTYPE)
    k = np.zeros(n, amd.KEYPOINT_DTYPE)
    k["x"], k["y"] = np.arange(n) * 3.0, np.arange(n) * 2.0
    return k


@pytest.mark.parametrize("empty_list", [False, True])
@pytest.mark.parametrize("nb", [61, 32])
@pytest.mark.parametrize("n0,n1", list(itertools.product(range(3), repeat=2)))
def test_the_packer_at_its_smallest_shapes(amd, n0, n1, nb, empty_list):
    d0, d1 = _rows(n0, n1, nb)
    exp = np_match(d0, d1)
    if n0 and n1:
        assert (n0 - 1, 0, 1.0) in exp  # (the planted row matches: the comparison below is not one of empty lists)
    k0, k1 = _keypoints(amd, n0, empty_list), _keypoints(amd, n1, empty_list)
    got = amd.descriptor_match_guided_host(k0, d0, k1, d1, ALL_PASS, amd.GUIDED_HOMOGRAPHY, 1e6)
    assert got.dtype == amd.MATCH_DTYPE and _as_list(got) == exp
    cross = amd.descriptor_match_cross_host(d0, d1)
    assert cross.dtype == amd.MATCH_DTYPE and _as_list(cross) == np_cross(d0, d1)
    if n0 == 0 or n1 == 0:  # the empty side in its other forms
        for form in EMPTY_FORMS:
            e0 = np.zeros(form, np.uint8) if n0 == 0 else d0
            e1 = np.zeros(form, np.uint8) if n1 == 0 else d1
            assert len(amd.descriptor_match_guided_host(k0, e0, k1, e1, ALL_PASS, amd.GUIDED_HOMOGRAPHY, 1e6)) == 0
            assert len(amd.descriptor_match_cross_host(e0, e1)) == 0
