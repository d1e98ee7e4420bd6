"""The detection mask as a statement: detect_keypoints (tests/extrema_numpy.py) with ONE line between candidates() and select().
Imports neither the oracle nor the product.  TEST INFRASTRUCTURE ONLY.

A mask is height x width of the FRAME, nonzero = detect here.  A candidate of level l (octave o, r = 1 << o) at level pixel
(x, y) exists only if mask[(y << o) + (r >> 1), (x << o) + (r >> 1)] != 0 -- the rounded position the reference gives the
unrefined keypoint (x r + 0.5 (r - 1), scale_space_extrema.rs:89-92).  Everything else is the unmasked statement."""
import numpy as np

import extrema_numpy as E


def mask_pixel(x, y, octave):
    """(mx, my): the frame pixel whose mask byte decides the level pixel (x, y) of an octave-`octave` level (arrays allowed)"""
    r = 1 << int(octave)
    return (np.asarray(x, np.int64) << int(octave)) + (r >> 1), (np.asarray(y, np.int64) << int(octave)) + (r >> 1)


def keep(idx, level, mask):
    """the candidates (flat indices of one level) the mask lets through"""
    idx = np.asarray(idx, np.int64)
    mx, my = mask_pixel(idx % level[0], idx // level[0], level[2])
    return np.asarray(mask)[my, mx] != 0


def detect_masked(ldets, levels, cfg, mask):
    """(keypoints with angle 0, extrema count) of the masked detection"""
    thr = E.F(float(cfg.detector_threshold))
    cands = [E.candidates(ldets[l], thr) for l in range(len(levels))]
    cands = [c[keep(c, levels[l], mask)] for l, c in enumerate(cands)]  # <- the mask
    ext, n_ext = E.select(cands, ldets, levels, cfg)
    return E.refine(ext, ldets), n_ext


def post_filter(kps, mask):
    """what a caller without the feature does: the finished keypoints whose own rounded pixel is unmasked"""
    if len(kps) == 0:
        return kps
    h, w = np.asarray(mask).shape
    x = np.clip(E.round_f32(kps["x"]).astype(np.int64), 0, w - 1)
    y = np.clip(E.round_f32(kps["y"]).astype(np.int64), 0, h - 1)
    return kps[np.asarray(mask)[y, x] != 0]


def keep_records(records, levels, masks):
    """the rule on candidate records (akaze_amd.CANDIDATE_IMG_DTYPE); masks: [h, w] (shared) or [n, h, w]"""
    masks = np.asarray(masks)
    out = np.zeros(len(records), bool)
    for l, lv in enumerate(levels):
        sel = np.nonzero(records["level"] == l)[0]
        if len(sel) == 0:
            continue
        idx = records["idx"][sel].astype(np.int64)
        mx, my = mask_pixel(idx % lv[0], idx // lv[0], lv[2])
        out[sel] = (masks[my, mx] if masks.ndim == 2 else masks[records["img"][sel].astype(np.int64), my, mx]) != 0
    return out


# ---- the masks the tests use, by name: uint8 [h, w], nonzero = detect ----------------------------------------------------------
def make_mask(name, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "ones":
        m = np.ones((h, w), bool)
    elif name == "zeros":
        m = np.zeros((h, w), bool)
    elif name == "left_half":
        m = xx < w // 2
    elif name == "disc":
        m = (xx - w // 2) ** 2 + (yy - h // 2) ** 2 <= (min(w, h) * 3 // 8) ** 2
    elif name == "checker8":
        m = ((xx // 8) + (yy // 8)) % 2 == 0
    elif name == "rows2":
        m = yy % 2 == 0
    elif name == "tenth":  # a strip that keeps about a tenth of the frame
        m = xx < w // 10
    else:
        raise KeyError(name)
    return m.astype(np.uint8) * 255


PARTIAL = ("left_half", "disc", "checker8", "rows2")
