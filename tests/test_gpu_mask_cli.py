"""extract_features -m/--mask: the tool's masked extraction against the Python masked call on the same pixels, and its refusal of
a mask of another size."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "akaze-rust_amd", "bin", "extract_features")
IMG0 = os.path.join(ROOT, "tests", "golden", "1.jpg")


def test_cli_mask_equals_python(ctx, amd, tmp_path):
    luma = amd.load_image_luma(IMG0)
    h, w = luma.shape
    mask = np.zeros((h, w), np.uint8)
    mask[:, :w // 2] = 255
    mask_path, out = str(tmp_path / "left.png"), str(tmp_path / "f.cbor")
    amd.save_png(mask_path, mask)
    assert np.array_equal(amd.load_image_luma(mask_path), mask)
    p = subprocess.run([BIN, IMG0, out, "-m", mask_path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    kp, desc = amd.deserialize_features_from_file(out)
    want = ctx.extract_features_masked(luma, mask, keep_all_planes=False)
    plain = ctx.extract_features_file(IMG0, keep_all_planes=False)
    assert 100 < len(kp) < plain.counts()[1]
    assert kp.tobytes() == want.keypoints().tobytes() and np.array_equal(desc, want.descriptors())
    want.close()
    plain.close()


def test_cli_mask_of_another_size(amd, tmp_path):
    mask_path = str(tmp_path / "small.png")
    amd.save_png(mask_path, np.full((100, 120), 255, np.uint8))
    p = subprocess.run([BIN, IMG0, str(tmp_path / "f.cbor"), "--mask", mask_path], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "120 x 100" in p.stderr and "2016 x 1512" in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "f.cbor"))
