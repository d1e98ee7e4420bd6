"""CPU test of the set prologue of k_detector_march (csrc/akz_march.hip, det_set_cell -- the function the kernel itself decodes
its workgroup index with -- through akz_debug_detector_set_cells): no GPU."""
import ctypes as C

# (half width, images, [(w, h) per entry, largest first])
SETS = [
    (2, 32, [(1920, 1080)]),
    (2, 3, [(97, 75)]),                                          # a set of one with fewer than eight cells
    (2, 32, [(1920, 1080), (960, 540)]),
    (3, 2, [(500, 130), (250, 65)]),
    (2, 32, [(1920, 1080), (1920, 1080), (960, 540), (960, 540)]),
    (2, 3, [(964, 68), (482, 34), (241, 17), (120, 16)]),        # one band per level; the last entries have 3 cells
    (1, 1, [(3840, 2160), (1920, 1080), (97, 75), (24, 18)]),    # very unequal; the last entry is a single cell
    (4, 5, [(481, 270), (480, 135), (241, 68), (33, 40)]),
]


def test_detector_set_cells_cover_every_entry_once(amd):
    """Every (image, band, strip) of every entry of a planned set is decoded by exactly one workgroup, padding workgroups
    decode to no work, every entry's share of an XCD (workgroup index & 7) is one contiguous range of the entry's cells, and
    every XCD walks the entries in the order given."""
    lib = amd.lib()
    for S, n, levels in SETS:
        ne = len(levels)
        ws = (C.c_uint32 * ne)(*[w for w, _ in levels])
        hs = (C.c_uint32 * ne)(*[h for _, h in levels])
        grids = (C.c_int32 * (3 * ne))()
        nwg = C.c_uint32()
        assert lib.akz_debug_detector_set_cells(S, ws, hs, ne, n, None, 0, grids, C.byref(nwg)) == 0
        total = nwg.value
        assert total % 8 == 0 and total > 0
        cells = (C.c_int32 * (4 * total))()
        assert lib.akz_debug_detector_set_cells(S, ws, hs, ne, n, cells, total, grids, C.byref(nwg)) == 0
        assert nwg.value == total
        want = 0
        for e, (w, h) in enumerate(levels):
            strips, bands, band_rows = grids[3 * e], grids[3 * e + 1], grids[3 * e + 2]
            assert strips == (w + 479) // 480 and bands >= 1 and band_rows >= 1
            assert (bands - 1) * band_rows < h - 2 * S <= bands * band_rows, (levels, e)  # the bands tile the interior rows
            want += (n * strips * bands + 7) // 8 * 8
        assert total == want, (levels, total, want)
        seen = [dict() for _ in range(ne)]
        per_xcd = [[[] for _ in range(8)] for _ in range(ne)]
        order = [[] for _ in range(8)]
        padding = 0
        for i in range(total):
            e, img, band, strip = cells[4 * i:4 * i + 4]
            if e < 0:
                assert (e, img, band, strip) == (-1, -1, -1, -1)
                padding += 1
                continue
            strips, bands = grids[3 * e], grids[3 * e + 1]
            assert 0 <= e < ne and 0 <= img < n and 0 <= band < bands and 0 <= strip < strips, (levels, i)
            key = (img, band, strip)
            assert key not in seen[e], (levels, i, e, key)
            seen[e][key] = i
            per_xcd[e][i & 7].append((img * bands + band) * strips + strip)
            order[i & 7].append(e)
        for e in range(ne):
            cnt = n * grids[3 * e] * grids[3 * e + 1]
            assert len(seen[e]) == cnt, (levels, e, len(seen[e]), cnt)
            at = 0
            for x in range(8):  # XCD x: the cells [at, at + k) of the entry, in ascending order
                got = per_xcd[e][x]
                assert got == list(range(at, at + len(got))), (levels, e, x)
                assert len(got) <= (cnt + 7) // 8
                at += len(got)
            assert at == cnt
        assert padding == total - sum(len(s) for s in seen)
        for x in range(8):
            assert order[x] == sorted(order[x]), (levels, x)


def test_detector_set_of_one_plans_as_a_lone_level(amd):
    """A set of one level is cut as a one-level launch always was: enough bands for three workgroups per compute unit (256
    of them where no device answers), none shorter than 40 interior rows -- 24 for four strip columns or fewer."""
    lib = amd.lib()
    grids = (C.c_int32 * 3)()
    nwg = C.c_uint32()
    for S in (1, 2, 3, 4):
        for w, h, n in ((1920, 1080, 32), (960, 540, 32), (3840, 2160, 8), (481, 135, 6), (1920, 1080, 1), (640, 480, 2)):
            ws, hs = (C.c_uint32 * 1)(w), (C.c_uint32 * 1)(h)
            assert lib.akz_debug_detector_set_cells(S, ws, hs, 1, n, None, 0, grids, C.byref(nwg)) == 0
            cols, rows = n * ((w + 479) // 480), h - 2 * S
            nb = max(1, min(-(-768 // cols), max(1, rows // (24 if cols <= 4 else 40))))
            band_rows = -(-rows // nb)
            assert (grids[0], grids[1], grids[2]) == ((w + 479) // 480, -(-rows // band_rows), band_rows), (S, w, h, n)
            assert nwg.value == (n * grids[0] * grids[1] + 7) // 8 * 8
