"""A deterministic textured scene and the image-shape case table of the KLT front-end's shape tests
(tests/test_track_shapes_ref.py on the CPU, tests/test_gpu_track_shapes.py on the device).  NumPy only.

Frames are crops of one canvas (blurred random rectangles plus noise) under a moving offset, frame i at offset
(2 i, i): the detector finds corners, LK has a motion to recover and tracks leave through the image borders.
Both sides of every comparison read the same options and the comparison is bit for bit, so the camera
intrinsics stay EuRoC's whatever the image size: the geometry need not be physical.
"""
import numpy as np

N_FRAMES = 6
WIN = 15  # the LK window: buildOpticalFlowPyramid stops once the next level's side would be <= WIN
MAX_LEVEL = 5


def canvas(w, h, seed, pad=24):
    rng = np.random.default_rng(seed)
    W, H = w + 2 * pad, h + 2 * pad
    img = np.full((H, W), 110.0)
    for _ in range(max(12, W * H // 600)):
        x, y = rng.integers(0, W), rng.integers(0, H)
        a, b = rng.integers(5, 22), rng.integers(5, 22)
        img[y:y + b, x:x + a] = rng.integers(20, 236)
    k = np.array([1, 2, 1]) / 4.0
    img = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, img)
    img = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, img)
    img += rng.normal(0, 1.5, img.shape)
    return img.clip(0, 255).astype(np.uint8)


def frames(w, h, seed, n, pad=24):
    """frame i: the canvas cropped at offset (2 i, i)"""
    c = canvas(w, h, seed, pad)
    return [np.ascontiguousarray(c[i % (2 * pad):i % (2 * pad) + h, (2 * i) % (2 * pad):(2 * i) % (2 * pad) + w])
            for i in range(n)]


def depth_rule(w, h):
    """number of pyramid levels: level 0, then halving ((side + 1) // 2) until the next side would be <= WIN"""
    d = 1
    while d <= MAX_LEVEL:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        d += 1
    return d


def _mask_o(w, h):
    m = np.zeros((h, w), dtype=np.uint8)
    m[:, :61] = 255
    m[90:, 130:] = 255
    return m


class Case:
    def __init__(self, name, cams, depth, reaches, mask=None, seeds=None, separate=False, **over):
        self.name = name
        self.separate = separate  # every camera is a mono run of its own (its own managers, seed 7)
        self.cams = cams        # tracked (w, h) per camera; with downsample_cameras the raw frames are 2w x 2h
        self.depth = depth      # pyramid levels per camera, as the oracle reports them
        self.reaches = reaches
        self.over = over        # option overrides on top of num_cameras / use_stereo / init_max_features
        self.mask = mask        # (w, h) -> mask of camera 0, or None
        stereo = bool(over.get("use_stereo", 0))
        # a mono camera and each camera of an independent rig: seed 7 + k; both cameras of a stereo pair: seed 7
        self.seeds = seeds if seeds is not None else [7 if stereo else 7 + k for k in range(len(cams))]

    def parts(self):
        """the runs of this case: itself, or one mono case per camera"""
        if not self.separate:
            return [self]
        return [Case("%s%d" % (self.name, k), [self.cams[k]], [self.depth[k]], self.reaches, **self.over)
                for k in range(len(self.cams))]

    @property
    def cam_ids(self):
        return list(range(len(self.cams)))

    @property
    def downsample(self):
        return bool(self.over.get("downsample_cameras", 0))

    @property
    def method(self):
        return self.over.get("histogram_method", 1)

    def options(self, yaml, **extra):
        import uvio_amd as U
        over = {"num_cameras": len(self.cams), "use_stereo": 0, "init_max_features": 120}
        over.update(self.over)
        over.update(extra)
        opts = U.load_options(yaml, **over)
        for k, (w, h) in enumerate(self.cams):
            opts.cams[k].width = w
            opts.cams[k].height = h
        return opts

    def oracle_options(self, yaml):
        """The oracle equalizes only for histogram_method 1, so for CLAHE (2) it runs method 0 and is fed
        clahe_ref(frame) (oracle_images), as tests/test_gpu_clahe.py pairs them."""
        return self.options(yaml, histogram_method=0) if self.method == 2 else self.options(yaml)

    def oracle_images(self, imgs):
        if self.method != 2:
            return imgs
        from clahe_ref import clahe_ref
        assert not self.downsample
        return [clahe_ref(im) for im in imgs]

    def raw_frames(self):
        """[frame][camera] -> the u8 image fed for that camera (2w x 2h with downsample_cameras)"""
        f = 2 if self.downsample else 1
        per_cam = [frames(f * w, f * h, s, N_FRAMES) for (w, h), s in zip(self.cams, self.seeds)]
        return [[per_cam[k][i] for k in range(len(self.cams))] for i in range(N_FRAMES)]

    def masks(self):
        """the masks argument of a feed (None: no camera is masked); a mask has the size of the fed image"""
        if self.mask is None:
            return None
        f = 2 if self.downsample else 1
        return [self.mask(f * self.cams[0][0], f * self.cams[0][1])] + [None] * (len(self.cams) - 1)

    @staticmethod
    def time(i):
        return 1.0 + 0.05 * i


CASES = [
    Case("A", [(67, 45)], [2], "w % 4 == 3: scalar level-0 stores, a 3-pixel last tile column; w h % 16 == 7; "
         "the histogram memset path over several frames; 13 x 9 cells"),
    Case("B", [(64, 48)], [2], "exactly one level-0 tile wide"),
    Case("C", [(130, 98)], [3], "w % 4 == 2; level 2 = 33 x 25 (second 32-wide tile one pixel wide); no level 3"),
    Case("D", [(131, 97)], [3], "both sides odd at levels 0 and 2"),
    Case("E", [(193, 127)], [4], "3 x 64 + 1 and 8 x 16 - 1; levels 97 x 64, 49 x 32, 25 x 16"),
    Case("F", [(253, 161)], [4], "levels 127 x 81, 64 x 41, 32 x 21"),
    Case("G", [(322, 242)], [5], "levels 161 x 121, 81 x 61, 41 x 31, 21 x 16: the l = 4 launch alone"),
    Case("H", [(515, 389)], [5], "partial tiles on both axes, several tiles inside"),
    Case("I", [(513, 511)], [6], "top level 17 x 16: smaller than LK's staged tile"),
    Case("J", [(90, 30)], [1], "level 0 only; single-level LK", grid_x=3, grid_y=2),
    Case("K", [(31, 31)], [2], "6 x 6 cells: no corner can exist; zero tracks, pyramids still equal"),
    Case("L", [(131, 97)], [3], "the identity LUT", histogram_method=0),
    Case("M", [(131, 97), (67, 45)], [3, 2], "CLAHE level 0 on small images: two mono runs",
         separate=True, histogram_method=2),
    Case("N", [(97, 65)], [3], "k_decimate_multi to odd halves (raw 194 x 130)", downsample_cameras=1),
    Case("O", [(193, 127)], [4], "mask grid at sizes that do not divide", mask=_mask_o),
    Case("P", [(131, 97), (131, 97)], [3, 3], "stereo LK at odd sizes", use_stereo=1),
    Case("Q", [(193, 127), (130, 98)], [4, 3], "two sizes and two depths in one pair and one launch", use_stereo=1),
    Case("R", [(193, 127), (67, 45), (322, 242), (131, 97)], [4, 2, 5, 3],
         "the mixed batch: grids from the maximum, per-camera exits, a depth-2 camera's histogram cleared by the "
         "others' l = 2 launch, shmax past a small camera's cells"),
    Case("S", [(161, 121), (161, 121)], [4, 4], "decimation and stereo together (raw 322 x 242)",
         downsample_cameras=1, use_stereo=1),
]
BY_NAME = {c.name: c for c in CASES}
# smallest images first: the order the device tests run in
ORDER = sorted(CASES, key=lambda c: sum(w * h for w, h in c.cams))
