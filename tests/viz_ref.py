"""Sequential numpy restatement of the image products' rendering rules ("Image products").

A painter's loop: the primitives of TrackBase::display_history (TrackBase.cpp:119-228) are drawn one after the other
in the reference's order and a later pixel simply overwrites an earlier one.  Written from TrackBase.cpp and the
rules, not from the kernels; it takes the inputs of ``uvio_amd.draw_tracks`` / ``uvio_amd.loop_depth``.
"""
import numpy as np

SAT = 1 << 20  # rounded coordinates saturate here (cvRound is undefined beyond int)
MAXTRACKS = 50


def cv_round(v):
    """cvRound of a float32: round half to even."""
    v = np.float32(v)
    if np.isnan(v):
        return -SAT
    return int(min(max(np.rint(np.float64(v)), -SAT), SAT))


def _clamp(c):
    return min(255, max(0, int(c)))


class Painter:
    """One camera's w x h view of the canvas: every write is clipped to it."""

    def __init__(self, canvas, x_off, w, h):
        self.c, self.x_off, self.w, self.h = canvas, x_off, w, h

    def put(self, x, y, col):
        if 0 <= x < self.w and 0 <= y < self.h:
            self.c[y, self.x_off + x] = col

    def disc(self, cx, cy, r, col):
        # the midpoint circle's spans: r = 1 the plus, r = 2 rows +-2 with |dx| <= 1 and rows |dy| <= 1 with |dx| <= 2
        spans = {1: {-1: 0, 0: 1, 1: 0}, 2: {-2: 1, -1: 2, 0: 2, 1: 2, 2: 1}}[r]
        for dy, half in spans.items():
            for dx in range(-half, half + 1):
                self.put(cx + dx, cy + dy, col)

    def segment(self, x0, y0, x1, y1, col):
        dx, dy = x1 - x0, y1 - y0
        ax, ay = abs(dx), abs(dy)
        n = max(ax, ay)
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        if n == 0:
            self.put(x0, y0, col)
            return
        # every step 0..n of the rule, each pixel clipped on its own (one colour: the order within a segment is moot)
        i = np.arange(n + 1, dtype=np.int64)
        if ax >= ay:
            x, y = x0 + sx * i, y0 + sy * ((2 * i * ay + n) // (2 * n))
        else:
            x, y = x0 + sx * ((2 * i * ax + n) // (2 * n)), y0 + sy * i
        ok = (x >= 0) & (x < self.w) & (y >= 0) & (y < self.h)
        self.c[y[ok], self.x_off + x[ok]] = col

    def rectangle(self, x0, y0, x1, y1, col):
        for x in range(x0, x1 + 1):
            self.put(x, y0, col)
            self.put(x, y1, col)
        for y in range(y0, y1 + 1):
            self.put(x0, y, col)
            self.put(x1, y, col)

    def fill(self, x0, y0, x1, y1, col):
        xa, xb = max(x0, 0), min(x1, self.w - 1)
        ya, yb = max(y0, 0), min(y1, self.h - 1)
        if xa <= xb and ya <= yb:
            self.c[ya:yb + 1, self.x_off + xa:self.x_off + xb + 1] = col


def history_colour(size, z, stereo, c1=(255, 255, 0), c2=(255, 255, 255)):
    """TrackBase.cpp:193-196 with (r1, g1, b1) = c1, (r2, g2, b2) = c2; Scalar(a, b, c) -> channels 0, 1, 2."""
    r1, g1, b1 = c1
    r2, g2, b2 = c2
    a = (b2 if stereo else r2) - int(1.0 * (b1 if stereo else r1) / size * z)
    b = (r2 if stereo else g2) - int(1.0 * (r1 if stereo else g1) / size * z)
    c = (g2 if stereo else b2) - int(1.0 * (g1 if stereo else b1) / size * z)
    return (_clamp(a), _clamp(b), _clamp(c))


def history_steps(size):
    """the z values display_history draws for a history of `size` entries"""
    out = []
    z = size - 1
    while z > 0:
        if size - z > MAXTRACKS:
            break
        out.append(z)
        z -= 1
    return out


def mask_tint(p):
    """addWeighted(mask, 0.1, img, 1.0, 0) on channel 2 under a set mask pixel: p + 25.5 rounded half to even"""
    p = int(p)
    return min(255, p + 25 + (1 if p % 2 == 0 else 0))


def draw_tracks(images, tracks, masks=None):
    ncam = len(images)
    max_w = max(im.shape[1] for im in images)
    max_h = max(im.shape[0] for im in images)
    small = min(max_w, max_h) < 400
    r, half = (1, 3) if small else (2, 5)
    canvas = np.zeros((max_h, ncam * max_w, 3), dtype=np.uint8)
    for k, im in enumerate(images):
        h, w = im.shape
        x_off = k * max_w
        canvas[:h, x_off:x_off + w, :] = np.asarray(im, dtype=np.uint8)[:, :, None]
        pa = Painter(canvas, x_off, w, h)
        for t in tracks[k]:
            if t["highlighted"]:
                u, v, hs = np.float32(t["u"]), np.float32(t["v"]), np.float32(half)
                green = (0, 255, 0)
                pa.rectangle(cv_round(u - hs), cv_round(v - hs), cv_round(u + hs), cv_round(v + hs), green)
                pa.disc(cv_round(u), cv_round(v), r, green)
            hist = np.asarray(t["hist"], dtype=np.float32).reshape(-1, 2)
            size = len(hist)
            if size == 0 or t["to_delete"]:
                continue
            for z in history_steps(size):
                col = history_colour(size, z, t["n_cams"] > 1)
                x, y = cv_round(hist[z, 0]), cv_round(hist[z, 1])
                pa.disc(x, y, r, col)
                if z + 1 < size:
                    pa.segment(x, y, cv_round(hist[z + 1, 0]), cv_round(hist[z + 1, 1]), col)
        m = None if masks is None else masks[k]
        if m is not None:
            sel = np.asarray(m)[:h, :w] > 127
            ch2 = canvas[:h, x_off:x_off + w, 2]
            ch2[sel] = np.array([mask_tint(p) for p in range(256)], dtype=np.uint8)[ch2[sel]]
    return canvas


def depth_colour(d):
    """ROS1Visualizer.cpp:977-990 in float32"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        idp = f(1.0) / f(d)
        chans = []
        for base in (0.0, 1.0, 2.0):
            x = (f(base) - idp) * f(255) / f(1.0)
            if x < 0:
                x = -x
            c = 0 if np.isnan(x) or x < 0 else (255 if x > 255 else int(x))
            chans.append(255 - c)
    return tuple(chans)


def loop_depth(img, ids, uvd):
    """ROS1Visualizer.cpp:950-996 for the tracks (ids, (u, v, depth)) in ascending id -> (depth u16, viz u8 x 3)"""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    depth = np.zeros((h, w), dtype=np.uint16)
    viz = np.repeat(img[:, :, None], 3, axis=2).copy()
    pa = Painter(viz, 0, w, h)
    dw = 4.0
    uvd = np.asarray(uvd, dtype=np.float64).reshape(-1, 3)
    for k in np.argsort(np.asarray(ids, dtype=np.uint64), kind="stable"):
        u, v, d = (float(x) for x in uvd[k])
        if u < dw or u > w - dw or v < dw or v > h - dw or np.isnan(u) or np.isnan(v):
            continue
        m = 1000 * d
        depth[int(v), int(u)] = (int(m) if np.isfinite(m) and abs(m) < 9.0e18 else 0) & 0xFFFF
        pa.fill(int(u - dw), int(v - dw), int(u + dw), int(v + dw), depth_colour(d))
    return depth, viz
