"""The JPEG fixtures of tests/golden/jpeg (tests/golden/make_jpegs.py) and the host side of device reconstruction: the set
covers every sampling and stream feature the device path must reproduce (parsed here from the SOF, SOS, DQT and DRI
markers), the host decoder accepts every file, and the new entry points are exported and declared."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")


def markers(path):
    """{sof: (marker, w, h, [(h, v)]), sos: count, dri: interval, dqt: [(pq, values)]}"""
    d = open(path, "rb").read()
    assert d[:2] == b"\xff\xd8"
    info = {"sos": 0, "dri": 0, "dqt": []}
    p = 2
    while p + 4 <= len(d):
        if d[p] != 0xFF or d[p + 1] in (0x00, 0xFF) or 0xD0 <= d[p + 1] <= 0xD7:
            p += 1
            continue
        m = d[p + 1]
        if m == 0xD9:
            break
        ln = (d[p + 2] << 8) | d[p + 3]
        body = d[p + 4:p + 2 + ln]
        if m in (0xC0, 0xC1, 0xC2):
            h, w, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            info["sof"] = (m, w, h, [(body[6 + 3 * i + 1] >> 4, body[6 + 3 * i + 1] & 15) for i in range(nc)])
        elif m == 0xDA:
            info["sos"] += 1
        elif m == 0xDD:
            info["dri"] = (body[0] << 8) | body[1]
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq = body[q] >> 4
                n = 128 if pq else 64
                raw = body[q + 1:q + 1 + n]
                vals = [(raw[2 * i] << 8) | raw[2 * i + 1] for i in range(64)] if pq else list(raw)
                info["dqt"].append((pq, vals))
                q += 1 + n
        p += 2 + ln
    return info


def fixtures():
    files = sorted(glob.glob(os.path.join(JPEG_DIR, "*.jpg")))
    assert files
    return {os.path.basename(f): markers(f) for f in files}


def test_fixture_set_covers_the_reconstruction_branches():
    fx = fixtures()
    samplings = set()
    for name, m in fx.items():
        _, w, h, f = m["sof"]
        if len(f) == 1:
            samplings.add("gray")
            continue
        (yh, yv), rest = f[0], f[1:]
        assert rest == [(1, 1), (1, 1)] or name.startswith("s321"), name
        samplings.add({(1, 1): "444", (2, 1): "422", (2, 2): "420", (1, 2): "440", (4, 1): "411", (3, 1): "321"}[(yh, yv)])
    assert {"gray", "444", "422", "420", "440", "411"} <= samplings, samplings
    assert any(m["sof"][0] == 0xC2 and m["sof"][3][0] == (2, 2) and m["sos"] > 1 for m in fx.values())  # progressive 4:2:0
    assert any(m["dri"] for m in fx.values())  # restart intervals
    assert any(pq == 0 and all(v == 1 for v in vals) for m in fx.values() for pq, vals in m["dqt"])  # quality 100
    sizes = {(m["sof"][1], m["sof"][2]) for m in fx.values()}
    assert {(1, 1), (2, 2), (17, 9)} <= sizes, sizes
    assert any(w > 16 and h > 16 for w, h in sizes)  # larger than one MCU
    # a chroma plane one sample wide: ceil(w * h_c / hmax) == 1
    assert any(len(m["sof"][3]) == 3 and -(-m["sof"][1] * 1 // max(f[0] for f in m["sof"][3])) == 1 for m in fx.values())
    ext = fx["extreme.jpg"]
    assert any(pq == 1 and min(vals) > 65000 for pq, vals in ext["dqt"])
    assert sum(os.path.getsize(os.path.join(JPEG_DIR, n)) for n in fx) < 300_000


def test_host_decoder_accepts_every_fixture(amd):
    for name, m in fixtures().items():
        luma = amd.load_image_luma(os.path.join(JPEG_DIR, name))
        assert luma.shape == (m["sof"][2], m["sof"][1]), name


def test_new_symbols_exported_and_declared(amd):
    L = amd.lib()
    hdr = open(os.path.join(ROOT, "include", "akaze_hip.h")).read()
    for s in ("akz_image_load_luma_device", "akz_extract_features_files"):
        assert re.search(rf"\b{s}\s*\(", hdr), s
        assert hasattr(L, s) and s in L._declared, s
    assert {6: "k_jpeg_idct", 7: "k_jpeg_luma"}.items() <= amd.KERNEL_ROW_KINDS.items()
