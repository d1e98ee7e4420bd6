"""Regenerates the JPEG fixtures of tests/golden/jpeg/ (the input of tests/test_gpu_jpeg.py and tests/test_jpeg_host.py).

Every sampling the host decoder reconstructs differently gets a file: grayscale, 4:4:4, 4:2:2 and 4:2:0 (written by
Pillow), 4:4:0 (h1v2), 4:1:1 (h4v1) and a mixed 3:2:1 horizontal sampling (written by the small baseline encoder of
tests/jpeg_numpy.py, since Pillow cannot), progressive 4:2:0, restart intervals, quality 100, sizes below and above one MCU (1x1, 2x2, 17x9,
chroma one sample wide), and extreme.jpg: 16-bit (pq=1) quantisation tables near 65535 and coefficients near +-32767, so
that dequantised values approach +-2^31.  Deterministic: numpy's seeded generator and fixed encoder settings.
The files the baseline encoder writes are listed in ENCODED with the function that gives their coefficients, so that a test
can state what they decode to.  Run from the repo root:  python tests/golden/make_jpegs.py
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
from jpeg_numpy import dct_matrix, encode  # noqa: E402

OUT = os.path.join(HERE, "jpeg")


def picture(w, h, seed):
    """An RGB test picture: colour gradients, a few saturated discs and rectangles, noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 128 + 100 * np.sin((x + y) / 5.0)], axis=-1)
    for _ in range(max(2, w * h // 400)):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1, max(2, min(w, h) / 3))
        img[(x - cx) ** 2 + (y - cy) ** 2 < r * r] = rng.integers(0, 256, 3)
    img += rng.normal(0, 6, img.shape)
    return np.clip(img + 0.5, 0, 255).astype(np.uint8)


def pillow(name, w, h, seed, mode="RGB", **kw):
    from PIL import Image  # (only the files Pillow writes need it)
    px = picture(w, h, seed)
    im = Image.fromarray(px, "RGB")
    if mode == "L":
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return name, buf.getvalue()


STD_LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
              87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
              72, 92, 95, 98, 112, 100, 103, 99]


def picture_coefs(w, h, seed, factors):
    """Colour picture with Y/Cb/Cr sampling factors [(h, v)] x 3, quality ~75 with the Annex K luma table for all planes:
    the arguments of jpeg_numpy.encode."""
    rgb = picture(w, h, seed).astype(np.float64)
    ycc = [0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2],
           -0.168736 * rgb[..., 0] - 0.331264 * rgb[..., 1] + 0.5 * rgb[..., 2] + 128,
           0.5 * rgb[..., 0] - 0.418688 * rgb[..., 1] - 0.081312 * rgb[..., 2] + 128]
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    q = np.array([max(1, v // 2) for v in STD_LUMA_Q], np.float64)
    D = dct_matrix()
    coefs = []
    for plane, (ch, cv) in zip(ycc, factors):
        # the plane at the component's resolution (box filter over the samples each one covers), edge-padded to whole MCUs
        pw, ph = mcux * ch * 8, mcuy * cv * 8
        ys = (np.arange(ph)[:, None] * vmax) // cv
        xs = (np.arange(pw)[None, :] * hmax) // ch
        acc = np.zeros((ph, pw))
        for dy in range(vmax // cv if vmax % cv == 0 else 1):
            for dx in range(hmax // ch if hmax % ch == 0 else 1):
                acc += plane[np.minimum(ys + dy, h - 1), np.minimum(xs + dx, w - 1)]
        n = (vmax // cv if vmax % cv == 0 else 1) * (hmax // ch if hmax % ch == 0 else 1)
        p = acc / n - 128.0
        blocks = p.reshape(mcuy * cv, 8, mcux * ch, 8).transpose(0, 2, 1, 3)
        d = np.einsum("ij,abjk,lk->abil", D, blocks, D).reshape(mcuy * cv, mcux * ch, 64)
        coefs.append(np.round(d / q).astype(np.int64))
    comps = [(fh, fv, 0) for fh, fv in factors]
    return w, h, comps, coefs, {0: [int(v) for v in q]}


def extreme_coefs():
    """4:2:0, 64x16: 16-bit tables near 65535, AC coefficients of 2^14 .. 2^15 - 1 in magnitude, and DC values that walk
    (in steps of 2047, the largest baseline DC difference) up to 32752 in Y and +-8188 in the chroma blocks: the arguments
    of jpeg_numpy.encode."""
    rng = np.random.default_rng(7)
    mcux, mcuy = 4, 1
    comps = [(2, 2, 0), (1, 1, 1), (1, 1, 1)]
    coefs = []
    for k, (ch, cv, _) in enumerate(comps):
        c = np.zeros((mcuy * cv, mcux * ch, 64), np.int64)
        j = 0
        sign = -1 if k == 2 else 1
        for my in range(mcuy):
            for mx in range(mcux):
                for vv in range(cv):
                    for hh in range(ch):  # (encoding order: the DC differences stay within 2047)
                        blk = c[my * cv + vv, mx * ch + hh]
                        j += 1
                        blk[0] = sign * 2047 * j
                        idx = rng.choice(np.arange(1, 64), size=12, replace=False)
                        blk[idx] = rng.choice([-1, 1], size=12) * rng.integers(1 << 14, 1 << 15, size=12)
        coefs.append(c)
    tabs = {0: [65535 - i for i in range(64)], 1: [65000 + 7 * i for i in range(64)]}
    return 64, 16, comps, coefs, tabs


# the files the baseline encoder writes: name -> the arguments of jpeg_numpy.encode
ENCODED = {
    "s440_45x37.jpg": lambda: picture_coefs(45, 37, 18, [(1, 2), (1, 1), (1, 1)]),
    "s440_3x3.jpg": lambda: picture_coefs(3, 3, 19, [(1, 2), (1, 1), (1, 1)]),
    "s411_53x19.jpg": lambda: picture_coefs(53, 19, 20, [(4, 1), (1, 1), (1, 1)]),
    "s411_3x7.jpg": lambda: picture_coefs(3, 7, 21, [(4, 1), (1, 1), (1, 1)]),
    "s321_41x13.jpg": lambda: picture_coefs(41, 13, 22, [(3, 1), (2, 1), (1, 1)]),
    "s420_custom_29x23.jpg": lambda: picture_coefs(29, 23, 23, [(2, 2), (1, 1), (1, 1)]),
    "extreme.jpg": extreme_coefs,
}


def main():
    os.makedirs(OUT, exist_ok=True)
    files = [
        pillow("gray_17x9.jpg", 17, 9, 1, mode="L", quality=85),
        pillow("gray_1x1.jpg", 1, 1, 2, mode="L", quality=85),
        pillow("gray_131x67.jpg", 131, 67, 3, mode="L", quality=90),
        pillow("s444_33x21.jpg", 33, 21, 4, quality=85, subsampling=0),
        pillow("s444_q100_40x24.jpg", 40, 24, 5, quality=100, subsampling=0),
        pillow("s422_37x19.jpg", 37, 19, 6, quality=85, subsampling=1),
        pillow("s422_2x5.jpg", 2, 5, 7, quality=85, subsampling=1),
        pillow("s420_1x1.jpg", 1, 1, 8, quality=85, subsampling=2),
        pillow("s420_2x2.jpg", 2, 2, 9, quality=85, subsampling=2),
        pillow("s420_17x9.jpg", 17, 9, 10, quality=85, subsampling=2),
        pillow("s420_2x30.jpg", 2, 30, 11, quality=85, subsampling=2),
        pillow("s420_257x189.jpg", 257, 189, 12, quality=90, subsampling=2),
        pillow("s420_q100_45x27.jpg", 45, 27, 13, quality=100, subsampling=2),
        pillow("prog420_97x71.jpg", 97, 71, 14, quality=85, subsampling=2, progressive=True),
        pillow("prog444_31x17.jpg", 31, 17, 15, quality=85, subsampling=0, progressive=True),
        pillow("rst420_120x88.jpg", 120, 88, 16, quality=85, subsampling=2, restart_marker_blocks=3),
        pillow("rst422_65x33.jpg", 65, 33, 17, quality=85, subsampling=1, restart_marker_blocks=1),
    ] + [(name, encode(*args())) for name, args in ENCODED.items()]
    for name, data in files:
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
    print(f"{len(files)} files, {sum(len(d) for _, d in files)} bytes in {OUT}")


if __name__ == "__main__":
    main()
