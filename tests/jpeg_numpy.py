"""JPEG reconstruction stated in numpy float64, and the small baseline encoder that writes the streams it is held to
(tests/test_jpeg_statement_host.py, tests/test_gpu_jpeg_statement.py, tests/golden/make_jpegs.py).  Helpers only.

The encoder takes the quantised coefficients themselves, so a test knows every coefficient of a stream it made and needs
no entropy decoder.  The statement is the inverse DCT through the 8x8 cosine matrix (planes_exact), the upsampling rule
per output pixel (upsample), the JFIF colour equations (rgb) and frames_cases.luma_numpy; rgb_bounds is its interval form
for planes that are only known to within a margin."""
import os
import struct

import numpy as np

from frames_cases import luma_numpy

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]


# ---- a minimal baseline encoder: any sampling factors, 8- or 16-bit tables, flat Huffman codes ------------------------
class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        """the low `length` bits of code, most significant first; a zero byte is stuffed behind every 0xFF"""
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        while self.n:
            self.put(1, 1)
        return bytes(self.out)


def category(v):
    return 0 if v == 0 else int(abs(int(v))).bit_length()


def magnitude_bits(v, s):
    return v if v >= 0 else v + (1 << s) - 1


# Flat codes: DC categories 0..11 as 4-bit codes, AC symbols EOB, ZRL and every (run, size 1..15) as 8-bit codes.  Sizes up to
# 15 reach the whole int16 range that extreme.jpg needs (the Annex K tables stop at 10).  The DC table stops at category 11:
# successive DC values of a component may differ by at most 2047.
DC_SYMS = list(range(12))
AC_SYMS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 16)]
DC_CODE = {s: (i, 4) for i, s in enumerate(DC_SYMS)}
AC_CODE = {s: (i, 8) for i, s in enumerate(AC_SYMS)}


def segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def encode(w, h, comps, coefs, qtabs):
    """comps: [(h, v, tq)]; coefs[k]: int array [bh, bw, 64] (quantised, natural order) covering whole MCUs; qtabs: {tq: 64
    values in natural order}."""
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    if len(comps) == 1:
        hmax = vmax = 1
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    for tq, tab in sorted(qtabs.items()):
        pq = 1 if max(tab) > 255 else 0
        vals = [tab[ZIGZAG[i]] for i in range(64)]
        out += segment(0xDB, bytes([(pq << 4) | tq]) + (struct.pack(">64H", *vals) if pq else bytes(vals)))
    sof = struct.pack(">BHHB", 8, h, w, len(comps))
    for i, (ch, cv, tq) in enumerate(comps):
        sof += bytes([i + 1, (ch << 4) | cv, tq])
    out += segment(0xC0, sof)
    for tc, syms, length in ((0, DC_SYMS, 4), (1, AC_SYMS, 8)):
        counts = [0] * 16
        counts[length - 1] = len(syms)
        out += segment(0xC4, bytes([tc << 4]) + bytes(counts) + bytes(syms))
    sos = bytes([len(comps)]) + b"".join(bytes([i + 1, 0x00]) for i in range(len(comps))) + bytes([0, 63, 0])
    out += segment(0xDA, sos)
    bits = Bits()
    pred = [0] * len(comps)
    for my in range(mcuy):
        for mx in range(mcux):
            for k, (ch, cv, _) in enumerate(comps):
                if len(comps) == 1:
                    ch = cv = 1
                for vv in range(cv):
                    for hh in range(ch):
                        blk = coefs[k][my * cv + vv, mx * ch + hh].tolist()
                        diff = blk[0] - pred[k]
                        pred[k] = blk[0]
                        s = category(diff)
                        bits.put(*DC_CODE[s])
                        bits.put(magnitude_bits(diff, s), s)
                        run = 0
                        for i in range(1, 64):
                            v = blk[ZIGZAG[i]]
                            if v == 0:
                                run += 1
                                continue
                            while run > 15:
                                bits.put(*AC_CODE[0xF0])
                                run -= 16
                            s = category(v)
                            bits.put(*AC_CODE[(run << 4) | s])
                            bits.put(magnitude_bits(v, s), s)
                            run = 0
                        if run:
                            bits.put(*AC_CODE[0x00])
    out += bits.flush() + b"\xff\xd9"
    return bytes(out)


def dct_matrix():
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    m[0] /= np.sqrt(2)
    return m


# ---- the frame's geometry ---------------------------------------------------------------------------------------------
def layout(w, h, factors):
    """(hmax, vmax, [(bw, bh, cw, ch)]): per component the block grid of the stream (whole MCUs) and the samples that
    belong to the picture, ceil(w * h_c / hmax) x ceil(h * v_c / vmax).  One component: a gray stream, factors ignored."""
    if len(factors) == 1:
        factors = [(1, 1)]
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return hmax, vmax, [(mcux * fh, mcuy * fv, -(-w * fh // hmax), -(-h * fv // vmax)) for fh, fv in factors]


# ---- the statement ----------------------------------------------------------------------------------------------------
def planes_exact(coefs, q):
    """The f64 inverse DCT of the dequantised blocks [bh, bw, 64] through the cosine matrix, plus 128, unrounded, as a plane
    [bh * 8, bw * 8]."""
    bh, bw, _ = coefs.shape
    D = dct_matrix()
    dq = (np.asarray(coefs, np.float64) * np.asarray(q, np.float64)).reshape(bh, bw, 8, 8)
    x = np.einsum("ui,abuv,vj->abij", D, dq, D)
    return x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8) + 128.0


def rounded(x):
    """ref: the plane a decoder with an exact transform gives"""
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int64)


def block_sums(coefs, q):
    """sum |coef * q| of every block, spread over the block's 8x8 samples: [bh * 8, bw * 8]"""
    s = np.abs(np.asarray(coefs, np.float64) * np.asarray(q, np.float64)).sum(axis=2)
    return np.repeat(np.repeat(s, 8, axis=0), 8, axis=1)


# The deliberate mistakes of the teeth tests: each changes one word of the upsampling rule.
MISTAKES = ("h2v1_round_1", "far_row_other_side", "neighbour_i_plus_1", "copy_fractional")


def sample(p, cw, ch, fh, fv, hmax, vmax, x, y, mistakes=()):
    """The value of component plane p (integers; cw x ch of them belong to the picture) at output pixel (x, y)."""
    if (fh, fv) == (hmax, vmax):
        return int(p[y, x])
    if "copy_fractional" in mistakes and hmax // fh == 1 and vmax // fv == 1:
        return int(p[y, x]) if y < p.shape[0] and x < p.shape[1] else 0
    if hmax == 2 * fh and vmax in (fv, 2 * fv):
        # triangle filter: three parts of the sample the pixel lies in, one part of the next one on the pixel's side
        i = x // 2
        j = i + 1 if x % 2 else i - 1
        if "neighbour_i_plus_1" in mistakes:
            j = i + 1
        end = j < 0 or j >= cw
        if vmax == fv:
            if end:
                return int(p[y, i])
            return (3 * int(p[y, i]) + int(p[y, j]) + (1 if "h2v1_round_1" in mistakes else 2)) >> 2
        yn = y // 2
        below = bool(y % 2) != ("far_row_other_side" in mistakes)
        yf = min(yn + 1, ch - 1) if below else max(yn - 1, 0)
        ti = 3 * int(p[yn, i]) + int(p[yf, i])
        if end:
            return (ti + 2) >> 2
        tj = 3 * int(p[yn, j]) + int(p[yf, j])
        return (3 * ti + tj + 8) >> 4
    return int(p[min(y * fv // vmax, ch - 1), min(x * fh // hmax, cw - 1)])


def upsample(plane, cw, ch, factor, hmax, vmax, w, h, mistakes=()):
    """The component at the frame's resolution, [h, w] integers."""
    out = np.empty((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            out[y, x] = sample(plane, cw, ch, factor[0], factor[1], hmax, vmax, x, y, mistakes)
    return out


TIE = 2.0 ** -10


def _channels(Y, Cb, Cr):
    Y, cb, cr = np.asarray(Y, np.float64), np.asarray(Cb, np.float64) - 128.0, np.asarray(Cr, np.float64) - 128.0
    return Y + 1.402 * cr, Y - 0.34414 * cb - 0.71414 * cr, Y + 1.772 * cb


def _round_u8(v):
    v = np.stack(v, axis=-1)
    t = v + 0.5
    return np.clip(np.floor(t), 0, 255).astype(np.int64), np.abs(t - np.round(t)) < TIE


def rgb(Y, Cb, Cr):
    """The JFIF equations in f64 on full-resolution components: ([h, w, 3] values, [h, w, 3] mask of the values within
    2^-10 of a rounding tie, which the f32 form may round the other way).  Only G can come that close: the products of R
    and B are multiples of 0.002."""
    return _round_u8(_channels(Y, Cb, Cr))


def frame_rgb(planes, w, h, factors, mistakes=()):
    """rgb of the upsampled integer planes of a colour frame"""
    hmax, vmax, geo = layout(w, h, factors)
    up = [upsample(p, g[2], g[3], f, hmax, vmax, w, h, mistakes) for p, g, f in zip(planes, geo, factors)]
    return rgb(*up)


def luma(px):
    return luma_numpy(px[..., 0], px[..., 1], px[..., 2])


def rgb_bounds(lo, hi, w, h, factors):
    """The interval form: planes known to lie in [lo[k], hi[k]] (integers in 0..255) give (rgb_lo, rgb_hi, luma_lo,
    luma_hi).  upsample has only positive weights, so it is monotone; each channel's equation takes the end of every
    term that its sign asks for; luma_numpy is monotone in R, G and B.  Treating the channels as independent is valid,
    only slightly wide.  A value within 2^-10 of a tie gives way by one level on that side."""
    hmax, vmax, geo = layout(w, h, factors)
    ul = [upsample(p, g[2], g[3], f, hmax, vmax, w, h) for p, g, f in zip(lo, geo, factors)]
    uh = [upsample(p, g[2], g[3], f, hmax, vmax, w, h) for p, g, f in zip(hi, geo, factors)]
    r0, _, b0 = _channels(ul[0], ul[1], ul[2])
    r1, _, b1 = _channels(uh[0], uh[1], uh[2])
    _, g0, _ = _channels(ul[0], uh[1], uh[2])
    _, g1, _ = _channels(uh[0], ul[1], ul[2])
    v0, t0 = _round_u8((r0, g0, b0))
    v1, t1 = _round_u8((r1, g1, b1))
    v0 = np.clip(v0 - t0, 0, 255)
    v1 = np.clip(v1 + t1, 0, 255)
    return v0, v1, luma(v0), luma(v1)


def within_one(ref):
    """[ref - 1, ref + 1] clipped to 0..255: a plane from a transform that meets the IEEE 1180 peak error"""
    return [np.clip(p - 1, 0, 255) for p in ref], [np.clip(p + 1, 0, 255) for p in ref]


def assert_exact(s, px, lum, what):
    """Stream s decoded to RGB px (None: not looked at) and luma lum: px equal to the statement except at masked ties, which
    are excused by +-1 in that channel in at most 0.1 % of the values; lum the luma of px, or, without px, the luma of the
    statement's RGB under the same rule.  Returns how many values were excused."""
    want, tie = frame_rgb(s.ref, s.w, s.h, s.factors)
    if px is not None:
        d = np.abs(px.astype(np.int64) - want)
        bad = d > tie
        assert not bad.any(), (what, int(bad.sum()), int(d.max()), np.argwhere(bad)[0])
        assert np.array_equal(lum, luma(px)), what
    else:
        bad = (lum < luma(np.clip(want - tie, 0, 255))) | (lum > luma(np.clip(want + tie, 0, 255)))
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0])
        d = lum != luma(want)
    assert (d > 0).sum() <= 0.001 * d.size, (what, int((d > 0).sum()))
    return int((d > 0).sum())


def assert_inside(bounds, s, px, lum, what):
    """RGB px (None: not looked at) and luma lum of stream s inside rgb_bounds of the plane intervals `bounds`"""
    lo, hi, llo, lhi = rgb_bounds(bounds[0], bounds[1], s.w, s.h, s.factors)
    if px is not None:
        bad = (px < lo) | (px > hi)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0])
    bad = (lum < llo) | (lum > lhi)
    assert not bad.any(), (what, "luma", int(bad.sum()), np.argwhere(bad)[0])
    return lo, hi


# ---- streams shared by the host and the device tests ------------------------------------------------------------------
FACTOR_SETS = [
    ((1, 1), (1, 1), (1, 1)),
    ((2, 1), (1, 1), (1, 1)),
    ((2, 2), (1, 1), (1, 1)),
    ((1, 2), (1, 1), (1, 1)),
    ((4, 1), (1, 1), (1, 1)),
    ((4, 2), (2, 2), (1, 1)),
    ((1, 1), (2, 2), (2, 2)),  # luma subsampled
    ((2, 2), (2, 1), (1, 2)),  # mixed
    ((3, 1), (2, 1), (1, 1)),  # the fractional ones: a factor that does not divide the maximum
    ((1, 3), (1, 2), (1, 1)),
    ((4, 1), (3, 1), (1, 1)),
    ((3, 2), (2, 1), (1, 1)),
]
FRACTIONAL = FACTOR_SETS[8:]
EXACT_Q = [8] + [3] * 63


def factors_id(factors):
    return "-".join(f"{a}x{b}" for a, b in factors)


class Stream:
    """One stream a test made: its bytes, and the planes its coefficients state."""

    def __init__(self, w, h, factors, coefs, qtabs, tq=None):
        self.w, self.h, self.factors = w, h, [tuple(f) for f in factors]
        self.coefs = coefs
        self.tq = list(tq) if tq is not None else [0] * len(factors)
        self.q = [np.asarray(qtabs[t], np.int64) for t in self.tq]
        self.data = encode(w, h, [(f[0], f[1], t) for f, t in zip(self.factors, self.tq)], coefs, qtabs)
        self.exact = [planes_exact(c, q) for c, q in zip(coefs, self.q)]
        self.ref = [rounded(x) for x in self.exact]

    @classmethod
    def of(cls, w, h, comps, coefs, qtabs):
        """from the arguments of encode"""
        return cls(w, h, [c[:2] for c in comps], coefs, qtabs, [c[2] for c in comps])

    def write(self, directory, name):
        self.path = os.path.join(str(directory), name)
        with open(self.path, "wb") as f:
            f.write(self.data)
        return self.path

    def margin_bounds(self, eps):
        """Plane intervals from a transform whose value before the clamp is within m = 0.5 + eps * sum |coef * q| (over the
        block) of exact: [clip(exact - m), clip(exact + m)].  It follows that |got - clip(exact)| <= m, and that a sample
        whose exact value lies beyond 0..255 by more than m is saturated on the right side."""
        lo, hi = [], []
        for x, c, q in zip(self.exact, self.coefs, self.q):
            m = 0.5 + eps * block_sums(c, q)
            lo.append(np.clip(np.ceil(x - m), 0, 255).astype(np.int64))
            hi.append(np.clip(np.floor(x + m), 0, 255).astype(np.int64))
        return lo, hi


def colour_stream(tier, factors, w, h, seed):
    """A colour frame with the DC of every block drawn in +-110 at q[0] = 8, so that the planes are the integers dc + 128 per
    block, which the integer transform gives exactly (tier "exact"); plus six AC coefficients per block in +-40 at q = 3
    (tier "textured"), where the planes are known to +-1."""
    rng = np.random.default_rng(seed)
    _, _, geo = layout(w, h, factors)
    coefs = []
    for bw, bh, _, _ in geo:
        c = np.zeros((bh, bw, 64), np.int64)
        c[..., 0] = rng.integers(-110, 111, (bh, bw))
        if tier == "textured":
            for by in range(bh):
                for bx in range(bw):
                    c[by, bx, rng.choice(np.arange(1, 64), size=6, replace=False)] = rng.integers(-40, 41, 6)
        coefs.append(c)
    return Stream(w, h, factors, coefs, {0: EXACT_Q})


def gray_stream(w, h, coefs, q):
    return Stream(w, h, [(1, 1)], [np.asarray(coefs, np.int64)], {0: [int(v) for v in q]})


def accuracy_coefs(lo, hi, sign, nblocks, seed):
    """IEEE 1180 style: the rounded f64 forward DCT of random 8x8 blocks with samples in lo..hi, times sign: [n, 64]"""
    rng = np.random.default_rng(seed)
    px = sign * rng.integers(lo, hi + 1, (nblocks, 8, 8)).astype(np.float64)
    D = dct_matrix()
    return np.round(np.einsum("ui,nij,vj->nuv", D, px, D)).astype(np.int64).reshape(nblocks, 64)


ACCURACY_RANGES = [(-128, 127), (-5, 5), (-100, 100)]
# the limits of IEEE 1180-1990 for an 8x8 inverse transform
PEAK, PMSE, OMSE, PME, OME = 1, 0.06, 0.02, 0.015, 0.0015


def accuracy_figures(got, s):
    """(peak, worst per-position mse, overall mse, worst per-position |mean|, overall |mean|) against ref, and the peak
    against the unrounded value clipped to 0..255, of a gray frame whose blocks tile it exactly"""
    e = (got.astype(np.int64) - s.ref[0]).astype(np.float64)
    bh, bw = e.shape[0] // 8, e.shape[1] // 8
    pos = e.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    unr = np.abs(got - np.clip(s.exact[0], 0, 255)).max()
    return (np.abs(e).max(), (pos ** 2).mean(axis=0).max(), (pos ** 2).mean(), np.abs(pos.mean(axis=0)).max(),
            abs(pos.mean()), unr)


def assert_accuracy(fig, what):
    peak, pmse, omse, pme, ome, unr = fig
    print(f"{what}: peak {peak:g} pmse {pmse:.4f} omse {omse:.4f} pme {pme:.4f} ome {ome:.5f} unrounded {unr:.3f}")
    assert peak <= PEAK and pmse <= PMSE and omse <= OMSE and pme <= PME and ome <= OME and unr < 1, (what, fig)


BASIS_A = 300


def shortcut_blocks():
    """[n, 64] at q = 1: each of the 64 coefficients alone at +A and -A; blocks with coefficients only in row 0 (every column
    takes the DC shortcut of the column pass) and only in column 0; a DC plus one coefficient at (r >= 1, c), so that
    exactly one column takes the full path; the all-zero block."""
    rng = np.random.default_rng(64)
    out = []
    for k in range(64):
        for a in (BASIS_A, -BASIS_A):
            b = np.zeros(64, np.int64)
            b[k] = a
            out.append(b)
    for _ in range(16):
        b = np.zeros((8, 8), np.int64)
        b[0, :] = rng.integers(-60, 61, 8)
        out.append(b.reshape(64))
    for _ in range(16):
        b = np.zeros((8, 8), np.int64)
        b[:, 0] = rng.integers(-60, 61, 8)
        out.append(b.reshape(64))
    for r in range(1, 8):
        for c in range(8):
            b = np.zeros((8, 8), np.int64)
            b[0, 0] = rng.integers(-200, 201)
            b[r, c] = rng.choice([-1, 1]) * rng.integers(100, 301)
            out.append(b.reshape(64))
    out.append(np.zeros(64, np.int64))
    return np.stack(out)


EPS = 2.0 ** -13
Q8 = [255] * 64
Q16 = [65535 - i for i in range(64)]


def large_coefs(top, nblocks, seed, dense):
    """[n, 64]: a small DC (the flat DC table's reach), and 12 or all 63 AC coefficients of magnitude t/2 .. t; t is top in
    every other block, and in the rest drawn per block evenly in the logarithm over 1 .. top, so that samples stay inside
    0..255 at every scale"""
    rng = np.random.default_rng(seed)
    c = np.zeros((nblocks, 64), np.int64)
    c[:, 0] = rng.integers(-16, 17, nblocks)
    for b in range(nblocks):
        idx = np.arange(1, 64) if dense[b] else rng.choice(np.arange(1, 64), size=12, replace=False)
        t = top if b % 2 else int(np.exp(rng.uniform(0, np.log(top))))
        c[b, idx] = rng.choice([-1, 1], size=len(idx)) * rng.integers((t + 1) // 2, t + 1, size=len(idx))
    return c


def strip(blocks, q):
    """n blocks [n, 64] as a gray stream one block high"""
    return gray_stream(8 * len(blocks), 8, np.asarray(blocks).reshape(1, len(blocks), 64), q)


def measured_eps(got, s):
    """The smallest eps at which a gray frame lies inside margin_bounds(eps): the max of (err - 0.5) / sum |coef * q|, where
    err is |got - exact|, counted on one side only where got is 0 or 255 (the clamp hides the other)."""
    x = s.exact[0][:s.h, :s.w]
    g = got.astype(np.float64)
    err = np.where(g == 0, x - g, np.where(g == 255, g - x, np.abs(g - x)))
    return float(((err - 0.5) / np.maximum(block_sums(s.coefs[0], s.q[0])[:s.h, :s.w], 1.0)).max())


def assert_margin(got, s, what):
    """a gray frame inside margin_bounds(EPS)"""
    lo, hi = s.margin_bounds(EPS)
    bad = (got < lo[0][:s.h, :s.w]) | (got > hi[0][:s.h, :s.w])
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0])
