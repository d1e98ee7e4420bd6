"""Cases shared by test_frames_host.py and test_gpu_frames.py: frames in every akz_frame_format with pitches and strides, laid
out in a poisoned byte buffer, and the numpy statement of to_luma they are held to."""
import numpy as np

POISON = 0xA5
GRAY8, RGB8, BGR8, RGBA8, BGRA8, PLANAR = range(6)
FORMATS = {GRAY8: "gray8", RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8", PLANAR: "rgb8_planar"}
BPP = {GRAY8: 1, RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4, PLANAR: 1}
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257)
HEIGHTS = (1, 2, 3, 17)
BATCHES = (1, 3)
PITCH_EXTRA = (0, 1, 3, 13)
FRAME_PAD = (0, 7)
PLANE_PAD = (0, 5)


def luma_numpy(r, g, b):
    """DynamicImage::to_luma in numpy float32: three products, two sums in this order, truncated"""
    r, g, b = (np.asarray(v, np.float32) for v in (r, g, b))
    return ((np.float32(0.2126) * r + np.float32(0.7152) * g) + np.float32(0.0722) * b).astype(np.uint8)


class Case:
    """n frames of w x h in format fmt inside self.buf (every byte outside the declared rows is POISON)"""

    def __init__(self, fmt, w, h, n, pitch_extra=0, frame_pad=0, plane_pad=0, rng=None, chans=None):
        self.fmt, self.w, self.h, self.n = fmt, w, h, n
        bpp = BPP[fmt]
        tight_row = w * bpp
        self.pitch = tight_row + pitch_extra
        self.plane = self.pitch * h + plane_pad if fmt == PLANAR else 0
        tight_frame = 3 * self.plane if fmt == PLANAR else self.pitch * h
        self.frame = tight_frame + frame_pad
        # what the layout says: 0 wherever the value is the tight one
        self.fields = (fmt, w, h, self.pitch if pitch_extra else 0, self.frame if frame_pad else 0, self.plane if plane_pad else 0)
        last = (2 * self.plane if fmt == PLANAR else 0) + (h - 1) * self.pitch + tight_row
        self.buf = np.full((n - 1) * self.frame + last, POISON, np.uint8)
        nch = 1 if fmt == GRAY8 else 4 if fmt in (RGBA8, BGRA8) else 3
        if chans is None:
            chans = [rng.integers(0, 256, (n, h, w), dtype=np.uint8) for _ in range(nch)]
        self.chans = chans
        order = {GRAY8: (0,), RGB8: (0, 1, 2), BGR8: (2, 1, 0), RGBA8: (0, 1, 2, 3), BGRA8: (2, 1, 0, 3), PLANAR: (0, 1, 2)}[fmt]
        rows = np.arange(h)[:, None] * self.pitch
        cols = np.arange(w)[None, :] * bpp
        for f in range(n):
            for k, c in enumerate(order):  # byte k of a pixel (plane k of a planar frame) holds channel c
                off = f * self.frame + (k * self.plane if fmt == PLANAR else k)
                self.buf[off + rows + cols] = chans[c][f]

    def expected(self):
        return self.chans[0].copy() if self.fmt == GRAY8 else luma_numpy(*self.chans[:3])

    def __repr__(self):
        return f"{FORMATS[self.fmt]} {self.w}x{self.h}x{self.n} pitch {self.pitch} frame {self.frame} plane {self.plane}"


def matrix(fmt, seed=0):
    """every shape x pitch x frame stride (x plane stride) of one format"""
    rng = np.random.default_rng(1000 + 17 * fmt + seed)
    for w in WIDTHS:
        for h in HEIGHTS:
            for n in BATCHES:
                for pe in PITCH_EXTRA:
                    for fp in FRAME_PAD:
                        for pp in (PLANE_PAD if fmt == PLANAR else (0,)):
                            yield Case(fmt, w, h, n, pe, fp, pp, rng)


def all_triples():
    """256 RGB frames of 256 x 256: every (R, G, B) exactly once"""
    r, g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return Case(RGB8, 256, 256, 256, chans=[r, g, b])
