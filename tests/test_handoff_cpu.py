"""The CV_32F hand-off on the host: the oracle's orc_stage_f32 equals the independent numpy restatement (tests/handoff_ref.py)
on the whole value set -- every u / 255, every rounding tie and its ulp neighbours, negatives, values above 1, a denormal, and
products an int cannot hold -- for 1 and 3 channels, tight and with a padded row stride."""
import numpy as np
import pytest

import handoff_ref as HR
import oracle_lib as O

W, H = 163, 123   # w % 4 == 3; handoff_ref.value_image checks that every value meets every column position mod 4


def oracle_stage(img, pad_floats):
    """orc_stage_f32 on a buffer whose rows are pad_floats floats longer than the image's (the padding holds NaN's neighbour in
    spirit: 1e10, which no output may pick up)"""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    buf = np.full((h, w * ch + pad_floats), 1e10, np.float32)
    buf[:, :w * ch] = img.reshape(h, w * ch)
    out = np.full((h, w + 3), 0xEE, np.uint8)
    O.lib().orc_stage_f32(buf.ctypes.data, w, h, buf.strides[0], ch, out.ctypes.data, w + 3)
    assert np.all(out[:, w:] == 0xEE)
    return out[:, :w].copy()


def test_tie_inputs_are_ties_of_both_parities():
    t = HR.tie_inputs()
    assert t.dtype == np.float32 and len(t) == 255
    p = t * np.float32(255)
    assert np.array_equal(p, np.arange(255, dtype=np.float32) + np.float32(0.5))
    got = HR.stage_f32(t[None, :])[0]
    assert got[0] == 0 and got[1] == 2 and got[2] == 2 and got[253] == 254 and got[254] == 254   # half to even, by hand
    assert np.all(got % 2 == 0)
    assert np.all(np.abs(t.astype(np.float64) * 255 - (np.arange(255) + 0.5)) < 1e-4)


def test_reference_on_values_computed_by_hand():
    """0.5 -> 127.5 -> 128; 1.7 -> 433.5 -> 255; -0.3 -> 0; the out-of-range rule; BGR (10, 200, 90) -> 145"""
    x = np.array([[0.5, 1.7, -0.3, -0.0, 8.4e6, 8.5e6, 1e10, -1e10, np.inf, -np.inf, np.nan, 1.0, 1.0000001]], np.float32)
    assert HR.stage_f32(x).tolist() == [[128, 255, 0, 0, 255, 0, 0, 0, 0, 0, 0, 255, 255]]
    bgr = (np.array([[[10, 200, 90]]], np.float32) / np.float32(255))
    assert HR.stage_f32(bgr).tolist() == [[(10 * 1868 + 200 * 9617 + 90 * 4899 + 8192) >> 14]]
    u = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(HR.stage_f32(u[None, :])[0], np.arange(256))


@pytest.mark.parametrize("pad", [0, 5], ids=["tight", "padded"])
@pytest.mark.parametrize("ch", [1, 3])
def test_oracle_stage_f32_equals_numpy_restatement(ch, pad):
    img = HR.value_image(W, H, ch)
    want = HR.stage_f32(img)
    got = oracle_stage(img, pad)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d pixels differ, first at row %d col %d (input %r): %d vs %d" % (
        len(bad), bad[0][0], bad[0][1], img[tuple(bad[0])], got[tuple(bad[0])], want[tuple(bad[0])])
    if pad == 0:
        assert np.array_equal(O.stage_f32(img), want)
    if ch == 1:
        assert len(np.unique(want)) == 256
