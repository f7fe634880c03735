"""NumPy restatement of cv::createCLAHE(10.0, Size(8, 8))->apply() on CV_8UC1 (TrackKLT.cpp:56-67's CLAHE
path), the reference of tests/test_clahe_ref.py and tests/test_gpu_clahe.py.

It follows OpenCV 4.x modules/imgproc/src/clahe.cpp as DESIGN.md §4 restates it (OpenCV itself is not a
dependency of this project, so parity with OpenCV's own build rests on that restatement):

  * LUT source: the image, or (when either side is no multiple of 8) the image extended on the right by
    8 - w % 8 columns and at the bottom by 8 - h % 8 rows with reflect-101 borders; a side that divides still
    gains a whole 8.  Tile size tw x th = extended size / 8.
  * clip = max((int)(10.0 * tw * th / 256), 1) (double, truncated).
  * per tile: histogram, clip, the clipped mass spread as batch = clipped // 256 to every bin and the residual
    one each to bins 0, step, 2 step, ... (step = max(256 // residual, 1)) while residual lasts; inclusive
    prefix sum; lut = saturate(rint(float32(cumsum) * (255.0f / float32(area)))).
  * per pixel: float32 bilinear interpolation between the LUTs of the four nearest tile centres, the weights
    taken before the tile indices are clamped, every product and sum rounded on its own (no fused operation),
    rint (ties to even), saturate.
"""
import numpy as np

TILES = 8
CLIP_LIMIT = 10.0


def _extend(img):
    h, w = img.shape
    if w % TILES == 0 and h % TILES == 0:
        return img
    return np.pad(img, ((0, TILES - h % TILES), (0, TILES - w % TILES)), mode="reflect")


def clahe_luts(img):
    """(luts[8, 8, 256] uint8, info): info holds tw, th, clip and per tile (row-major lists of 64) clipped,
    residual and step (step 0 where residual is 0)."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype == np.uint8 and min(img.shape) > TILES
    src = _extend(img)
    th, tw = src.shape[0] // TILES, src.shape[1] // TILES
    area = tw * th
    clip = max(int(CLIP_LIMIT * area / 256), 1)
    scale = np.float32(255.0) / np.float32(area)
    luts = np.zeros((TILES, TILES, 256), dtype=np.uint8)
    info = {"tw": tw, "th": th, "clip": clip, "clipped": [], "residual": [], "step": []}
    for ty in range(TILES):
        for tx in range(TILES):
            tile = src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
            clipped = int(np.maximum(hist - clip, 0).sum())
            hist = np.minimum(hist, clip)
            batch = clipped // 256
            residual = clipped - 256 * batch
            hist += batch
            step = 0
            if residual != 0:
                step = max(256 // residual, 1)
                i, r = 0, residual
                while i < 256 and r > 0:
                    hist[i] += 1
                    i += step
                    r -= 1
            cum = np.cumsum(hist).astype(np.float32)
            luts[ty, tx] = np.clip(np.rint(cum * scale), 0, 255).astype(np.uint8)
            info["clipped"].append(clipped)
            info["residual"].append(residual)
            info["step"].append(step)
    return luts, info


def _axis(n, tile):
    """per coordinate: first / second tile index (clamped) and the float32 weights of the second / first"""
    inv = np.float32(1.0) / np.float32(tile)
    f = np.arange(n, dtype=np.float32) * inv - np.float32(0.5)
    i1 = np.floor(f).astype(np.int32)
    a = f - i1.astype(np.float32)
    a1 = np.float32(1.0) - a
    assert f.dtype == a.dtype == a1.dtype == np.float32
    return np.maximum(i1, 0), np.minimum(i1 + 1, TILES - 1), a, a1, i1


def clahe_ref(img, return_info=False):
    img = np.asarray(img)
    luts, info = clahe_luts(img)
    h, w = img.shape
    tx1, tx2, xa, xa1, rx = _axis(w, info["tw"])
    ty1, ty2, ya, ya1, ry = _axis(h, info["th"])
    v = img.astype(np.intp)
    y1, y2 = ty1[:, None], ty2[:, None]
    x1, x2 = tx1[None, :], tx2[None, :]
    l11 = luts[y1, x1, v].astype(np.float32)
    l12 = luts[y1, x2, v].astype(np.float32)
    l21 = luts[y2, x1, v].astype(np.float32)
    l22 = luts[y2, x2, v].astype(np.float32)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = l11 * xa1 + l12 * xa
    bot = l21 * xa1 + l22 * xa
    res = top * ya1 + bot * ya
    assert res.dtype == np.float32
    out = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    if return_info:
        # the clamp region of every coordinate: 0 below the first tile centre (unclamped index -1), 2 past the
        # last one (second index clamped), 1 between
        info["region_x"] = np.where(rx < 0, 0, np.where(rx + 1 > TILES - 1, 2, 1))
        info["region_y"] = np.where(ry < 0, 0, np.where(ry + 1 > TILES - 1, 2, 1))
        return out, info
    return out
