"""The detection mask on the CPU: the statement (tests/mask_numpy.py: the unmasked statement with one line added) against the
oracle's keypoints, the masks that tell it from a filter over finished keypoints, the geometry of odd sizes, and what the binding
refuses before any call.  Everything is compared for equality; no GPU call."""
import functools
import os
import re

import numpy as np
import pytest

import extrema_numpy as E
import mask_numpy as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("x", "y", "response", "size", "octave", "class_id")
W, H = 320, 240
INDICES = (100, 126, 143)  # synth_frame indices at which checker8 and rows2 both give keypoints a post-filter lacks (asserted below)
NEW_SYMBOLS = ("akz_extract_device_frames_masked", "akz_extract_begin_device_frames_masked", "akz_extract_gray_u8_masked",
               "akz_debug_mask_candidates", "akz_debug_mask_counts")


def keys(kps):
    return set(zip(kps["x"].view(np.uint32).tolist(), kps["y"].view(np.uint32).tolist(), kps["class_id"].tolist()))


@functools.lru_cache(maxsize=None)
def oracle(w, h, idx):
    """(cfg, levels, Ldet planes, keypoints, extrema count) of the CPU oracle on synth_frame(w, h, idx), computed once"""
    import akaze_amd
    import akaze_ref
    akaze_ref.build()
    cfg = akaze_ref.default_config()
    rf = akaze_ref.extract(akaze_amd.synth_frame(w, h, idx), cfg)
    infos = [rf.level_info(l) for l in range(rf.num_levels)]
    levels = [(i["w"], i["h"], i["octave"], i["esigma"]) for i in infos]
    ldets = [rf.plane(l, "Ldet") for l in range(rf.num_levels)]
    out = (cfg, levels, ldets, rf.keypoints().copy(), rf.num_extrema)
    rf.close()
    return out


def assert_keypoints(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in FIELDS:
        ga, ea = np.asarray(got[f]), np.asarray(exp[f])
        if ga.dtype.kind == "f":
            ga, ea = ga.view(np.uint32), ea.view(np.uint32)
        assert np.array_equal(ga, ea), (what, f)


@pytest.mark.parametrize("idx", INDICES)
def test_all_ones_is_the_oracle_and_zeros_is_nothing(amd, ref, idx):
    cfg, levels, ldets, want, n_ext = oracle(W, H, idx)
    got, got_ext = M.detect_masked(ldets, levels, cfg, M.make_mask("ones", W, H))
    assert len(want) >= 15 and got_ext == n_ext
    assert_keypoints(got, want, idx)
    none, none_ext = M.detect_masked(ldets, levels, cfg, M.make_mask("zeros", W, H))
    assert len(none) == 0 and none_ext == 0


@pytest.mark.parametrize("name", ["left_half", "disc"])
@pytest.mark.parametrize("idx", INDICES)
def test_region_masks_equal_the_post_filter_here(amd, ref, idx, name):
    """masks whose border is crossed by few suppression pairs: on these frames the statement and the post-filter agree keypoint for
    keypoint, which pins the mask pixel (a shifted one would move the border)"""
    cfg, levels, ldets, want, _ = oracle(W, H, idx)
    mask = M.make_mask(name, W, H)
    got, _ = M.detect_masked(ldets, levels, cfg, mask)
    assert 0 < len(got) < len(want)
    assert_keypoints(got, M.post_filter(want, mask), (idx, name))


@pytest.mark.parametrize("name", ["checker8", "rows2"])
@pytest.mark.parametrize("idx", INDICES)
def test_fine_masks_differ_from_a_post_filter(amd, ref, idx, name):
    """a removed candidate no longer suppresses its neighbour: keypoints that filtering the oracle's list by the mask cannot have"""
    cfg, levels, ldets, want, _ = oracle(W, H, idx)
    mask = M.make_mask(name, W, H)
    got, _ = M.detect_masked(ldets, levels, cfg, mask)
    extra = keys(got) - keys(M.post_filter(want, mask))
    print(f"{idx} {name}: {len(got)} keypoints, {len(extra)} that the post-filter lacks")
    assert len(extra) >= 1, (idx, name)
    # ... and every masked keypoint's CANDIDATE pixel is unmasked (refinement may move the keypoint itself by up to a level pixel)
    for kp in got:
        lv = levels[int(kp["class_id"])]
        r = E.F(2.0) ** E.F(lv[2])
        half = E.F(0.5) * (r - E.F(1.0))
        cx, cy = (kp["x"] - half) / r, (kp["y"] - half) / r
        near = [(int(np.floor(cx)) + dx, int(np.floor(cy)) + dy) for dx in (-1, 0, 1, 2) for dy in (-1, 0, 1, 2)]
        assert any(0 <= x < lv[0] and 0 <= y < lv[1] and mask[M.mask_pixel(x, y, lv[2])[::-1]] != 0 and abs(x - cx) <= 1 and abs(y - cy) <= 1
                   for x, y in near), (idx, name, kp)


def test_odd_size_maps_inside_the_mask(amd, ref):
    """321 x 241: the last column and row of every level map inside the mask, and the library plans the same levels"""
    w, h = 321, 241
    cfg, levels, ldets, want, _ = oracle(w, h, 100)
    assert [(p["w"], p["h"], p["octave"]) for p in amd.plan_levels(w, h, amd.Config())] == [lv[:3] for lv in levels]
    assert max(lv[2] for lv in levels) >= 1
    for lw, lh, o, _ in levels:
        assert (lw, lh) == (w >> o, h >> o)
        mx, my = M.mask_pixel(lw - 1, lh - 1, o)
        assert mx < w and my < h, (lw, lh, o)
        assert M.mask_pixel(0, 0, o) == ((1 << o) >> 1, (1 << o) >> 1)
    got, _ = M.detect_masked(ldets, levels, cfg, M.make_mask("ones", w, h))
    assert_keypoints(got, want, "odd")
    # a mask that keeps ONLY the last row and column's mask pixels of every level drops every candidate (none lies on a level's edge)
    edge = np.zeros((h, w), np.uint8)
    for lw, lh, o, _ in levels:
        mx, my = M.mask_pixel(np.arange(lw), np.full(lw, lh - 1), o)
        edge[my, mx] = 1
        mx, my = M.mask_pixel(np.full(lh, lw - 1), np.arange(lh), o)
        edge[my, mx] = 1
    assert len(M.detect_masked(ldets, levels, cfg, edge)[0]) == 0


def test_keep_records_is_the_rule(amd):
    """the record form of the rule (what the GPU tests compare the kernel with) against keep() per level"""
    rng = np.random.default_rng(3)
    w, h = 161, 81
    levels = E.plan_levels(w, h)
    masks = (rng.random((3, h, w)) < 0.5).astype(np.uint8)
    rec = np.zeros(500, amd.CANDIDATE_IMG_DTYPE)
    rec["level"] = rng.integers(0, len(levels), len(rec))
    rec["img"] = rng.integers(0, 3, len(rec))
    for i, r in enumerate(rec):
        rec["idx"][i] = rng.integers(0, levels[r["level"]][0] * levels[r["level"]][1])
    got = M.keep_records(rec, levels, masks)
    for i, r in enumerate(rec):
        assert got[i] == M.keep([r["idx"]], levels[r["level"]], masks[r["img"]])[0]
    assert 100 < got.sum() < 400
    assert np.array_equal(M.keep_records(rec, levels, masks[1]), M.keep_records(rec, levels, np.stack([masks[1]] * 3)))


def test_binding_refuses_wrong_masks(amd):
    ok = np.ones((H, W), np.uint8)
    lay, n_masks = amd.mask_layout_of(ok, 3, H, W)
    assert (lay.format, lay.width, lay.height, lay.row_pitch, n_masks) == (amd.FRAME_GRAY8, W, H, W, 1)
    lay, n_masks = amd.mask_layout_of(np.ones((3, H, W + 5), bool)[:, :, :W], 3, H, W)
    assert (lay.row_pitch, lay.frame_stride, n_masks) == (W + 5, H * (W + 5), 3)
    for bad, word in ((ok.astype(np.float32), "uint8 or bool"), (ok[:, :-1], "the mask is"), (ok[:-1], "the mask is"), (np.ones((2, H, W), np.uint8), "2 masks for 3"),
                      (np.ones((1, 1, H, W), np.uint8), "dimensions"), (ok[:, ::2].repeat(2, 1)[:, ::-1], "pixel stride"),
                      (np.ones((H, 2 * W), np.uint8)[:, ::2], "pixel stride")):
        with pytest.raises(ValueError, match=word):
            amd.mask_layout_of(bad, 3, H, W)
    img = np.zeros((H, W), np.uint8)
    for bad, word in ((ok.astype(np.int32), "uint8 or bool"), (ok[:-1], "the mask is")):
        with pytest.raises(ValueError, match=word):
            amd.Context.extract_features_masked(None, img, bad)
    with pytest.raises(ValueError, match="uint8"):
        amd.Context.extract_features_masked(None, img.astype(np.float32), ok)
    with pytest.raises(ValueError, match="CUDA"):
        amd.Context._device_mask(None, ok, 1, lay)


def test_new_symbols_are_declared_and_exported(amd):
    L = amd.lib()
    text = open(os.path.join(ROOT, "include", "akaze_hip.h")).read() + open(os.path.join(ROOT, "include", "akaze_hip_debug.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L._declared and hasattr(L, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"AKZ_KR_MASK_CANDIDATES\s*=\s*13\b", text) and amd.KR_MASK_CANDIDATES == 13
    assert amd.KERNEL_ROW_KINDS[13] == "k_mask_candidates"
    assert L.akz_abi_version() == 6
    # host-side refusals of the masked host call need no GPU: a null mask is refused before anything else
    import ctypes as C
    out = C.c_void_p(0xDEAD)
    assert L.akz_extract_gray_u8_masked(None, None, None, 8, 8, None, 0, C.byref(out)) == -1 and not out.value
    assert "mask" in L.akz_last_error().decode()
