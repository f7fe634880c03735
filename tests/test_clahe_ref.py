"""tests/clahe_ref.py (the NumPy restatement of CLAHE that the GPU tests compare against) pinned on cases worked
out by hand, and the library's CLAHE probe declared.  CPU only.

Every case is a (piecewise) constant image, so each tile's histogram has one or two bins and the LUT entry
follows from counting: with `clip` the clip limit, a tile of area A whose only value is v has clipped = A - clip,
batch = clipped // 256 = 0, residual = clipped, step = 256 // residual, and
    cumsum[v] = #{multiples of step in [0, v]} + clip          (as long as v // step < residual)
    lut[v] = rint(float32(cumsum[v]) * float32(255 / A)).
Interpolating between equal LUT entries L gives L * xa1 + L * xa, which is within a few float32 ulps of L and
rounds back to L, so the output is constant wherever the four LUTs agree."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_constant_64x64_by_hand():
    """64 x 64 of value 100: no extension, tiles 8 x 8, A = 64, clip = (int)(10 * 64 / 256) = 2; clipped = 62,
    batch 0, residual 62, step = 256 // 62 = 4: bins 0, 4, ..., 244 gain one.  cumsum[100] = 26 (multiples of 4 in
    [0, 100]) + 2 = 28; lut = rint(28 * 255 / 64) = rint(111.5625) = 112."""
    from clahe_ref import clahe_luts, clahe_ref
    img = np.full((64, 64), 100, dtype=np.uint8)
    luts, info = clahe_luts(img)
    assert (info["tw"], info["th"], info["clip"]) == (8, 8, 2)
    assert set(info["clipped"]) == {62} and set(info["residual"]) == {62} and set(info["step"]) == {4}
    assert np.all(luts[:, :, 100] == 112)
    # below the value only the redistributed ones count: cumsum[99] = 25 -> rint(99.609) = 100
    assert np.all(luts[:, :, 99] == 100)
    assert np.all(clahe_ref(img) == 112)


def test_width_not_multiple_of_8_by_hand():
    """w = 60, h = 64: the width gains 8 - 60 % 8 = 4 columns and the height, though it divides, a whole 8 rows:
    72 x 64 -> tiles tw = 8, th = 9, A = 72, clip = (int)(720 / 256) = 2.  A constant tile: clipped = residual =
    70, step = 256 // 70 = 3.  Value 50: cumsum = 17 (0, 3, ..., 48) + 2 = 19, lut = rint(19 * 255 / 72) =
    rint(67.29) = 67.  Value 100: cumsum = 34 + 2 = 36 and float32(255 / 72) * 36 = 127.5000029 rounds to the
    float32 127.5 (spacing 2^-17 there): a tie, which rint takes to the even 128."""
    from clahe_ref import clahe_luts, clahe_ref
    img = np.full((64, 60), 50, dtype=np.uint8)
    _, info = clahe_luts(img)
    assert (info["tw"], info["th"], info["clip"]) == (8, 9, 2)
    assert set(info["residual"]) == {70} and set(info["step"]) == {3}
    out = clahe_ref(img)
    assert out.shape == (64, 60) and np.all(out == 67)
    assert np.float32(36) * (np.float32(255) / np.float32(72)) == np.float32(127.5)
    assert np.all(clahe_ref(np.full((64, 60), 100, dtype=np.uint8)) == 128)


def test_only_height_not_multiple_of_8_by_hand():
    """w = 64, h = 60: the height gains 4 rows and the width the full 8 columns: 72 x 64 -> tw = 9, th = 8, A = 72,
    clip 2.  Value 50 everywhere but columns 62 and 63, which hold 200.  Tile column 7 is x in [63, 71]: column 63
    and the reflect-101 columns 62, 61, ..., 55, so 2 columns of 200 and 7 of 50; tile column 6 is x in [54, 62]:
    one column of 200.  Both: clipped = (56 - 2) + (16 - 2) = 68 resp. (64 - 2) + (8 - 2) = 68, step = 256 // 68 =
    3, cumsum[200] = 67 (0, 3, ..., 198) + 2 + 2 = 71 -> rint(71 * 255 / 72) = rint(251.46) = 251, and cumsum[50]
    = 17 + 2 = 19 -> 67.  The other tile columns are constant 50: lut[50] = 67 as in the case above.  Columns 62
    and 63 interpolate between tile columns 6 and 7 only (their centres are at x = 58 and 67), so they come out
    251 and the rest 67.  Without the full pad (tw = 8, A = 64) value 50 would map to 60."""
    from clahe_ref import clahe_luts, clahe_ref
    img = np.full((60, 64), 50, dtype=np.uint8)
    img[:, 62:] = 200
    luts, info = clahe_luts(img)
    assert (info["tw"], info["th"], info["clip"]) == (9, 8, 2)
    clipped = np.array(info["clipped"]).reshape(8, 8)
    assert np.all(clipped[:, :6] == 70) and np.all(clipped[:, 6:] == 68)
    assert np.all(np.array(info["step"]) == 3)
    assert np.all(luts[:, 6:, 200] == 251) and np.all(luts[:, :, 50] == 67)
    out = clahe_ref(img)
    assert out.shape == (60, 64)
    assert np.all(out[:, 62:] == 251) and np.all(out[:, :62] == 67)


def test_clamp_regions_and_weights():
    """The first half tile keeps the weight it had before the clamp: x = 0 at tw = 8 gives txf = -0.5, floor -1,
    xa = 0.5 with both indices 0; the last half tile has both indices 7."""
    from clahe_ref import _axis
    i1, i2, a, a1, raw = _axis(64, 8)
    assert (i1[0], i2[0], raw[0]) == (0, 0, -1) and a[0] == np.float32(0.5) and a1[0] == np.float32(0.5)
    assert (i1[4], i2[4]) == (0, 1) and a[4] == 0.0
    assert (i1[63], i2[63]) == (7, 7) and a[63] == np.float32(0.375)


def test_native_declares_clahe_probe():
    from uvio_amd import _native as N
    assert "uvio_hp_debug_clahe" in N.EXPORTED
    assert hasattr(N.load(), "uvio_hp_debug_clahe")
