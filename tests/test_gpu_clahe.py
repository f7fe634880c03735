"""GPU parity of histogram_method CLAHE (k_clahe_lut + the CLAHE mode of the level-0 pyramid kernel) against
tests/clahe_ref.py, the NumPy restatement of cv::createCLAHE(10.0, Size(8, 8))->apply().

The oracle (oracle/) equalizes only for histogram_method 1 and copies otherwise, so the pipeline tests pair the
device running histogram_method 2 on the raw frames with the oracle running histogram_method 0 on
clahe_ref(frame): everything downstream of the equalization is then checked by the oracle as usual.

Tolerances: none.  The tile LUTs are integer work up to one float32 product per entry, and the interpolation
is a fixed sequence of individually rounded float32 operations, which the reference repeats: the probe, the
pyramids and the tracks are bit-exact; the lock-step estimator on top keeps tests/test_gpu_parity.py's bounds.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = [(64, 48), (67, 45), (64, 45), (40, 40)]  # (w, h); 40 x 40: 10 * 25 / 256 < 1, the clip limit forced to 1


def _mix(w, h, seed):
    """a saturated block, a smooth ramp and noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (xx * 200.0 / w + yy * 40.0 / h + rng.normal(0.0, 6.0, (h, w))).clip(0, 255)
    img[h // 3:h // 3 + h // 4, w // 2:w // 2 + w // 3] = 255
    img[:h // 5, :w // 4] = rng.integers(0, 256, (h // 5, w // 4))
    return img.astype(np.uint8)


def _setup(euroc_yaml, n_frames, **over):
    import uvio_amd as U
    from uvio_amd.render import SceneRenderer
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, **over)
    s = SimStream(opts, duration=n_frames / opts.track_frequency + 1.2, seed=5, spawn=10)
    return opts, s, SceneRenderer(opts, device="cuda")


def _variant(opts, **fields):
    """a copy of the options with some fields changed"""
    o = type(opts).from_buffer_copy(opts)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def _frames(s, r, cams, n):
    for i in range(n):
        yield i, s.cam_t[i], [r.render(k, *s.camera_pose(i, k), frame_seed=i).cpu().numpy() for k in cams]


def test_probe_bit_exact(euroc_yaml):
    import uvio_amd as U
    from clahe_ref import clahe_ref
    opts, s, r = _setup(euroc_yaml, 2)
    real = r.render(0, *s.camera_pose(0, 0), frame_seed=0).cpu().numpy()
    assert real.shape == (480, 752) and real.dtype == np.uint8
    # the rendered frame spreads every tile's histogram under the clip limit (220 of 5640 pixels), so it alone
    # never clips: the same frame under-exposed (values / 4) with a saturated lamp is the further real-size input
    dark = (real // 4).astype(np.uint8)
    dark[100:300, 200:500] = 255
    inputs = [_mix(w, h, 11 + k) for k, (w, h) in enumerate(SMALL)] + [real, dark]
    refs = [clahe_ref(img, return_info=True) for img in inputs]
    # the inputs reach every branch of the LUT redistribution and every clamp region of the interpolation
    tiles = [(c, res, st) for _, info in refs for c, res, st in zip(info["clipped"], info["residual"], info["step"])]
    assert any(c > 0 and res != 0 for c, res, st in tiles)
    assert any(c >= 256 and res != 0 for c, res, st in tiles), "no tile with batch > 0"
    assert any(st == 1 for c, res, st in tiles), "no tile with residual > 128"
    assert any(st > 1 for c, res, st in tiles)
    assert any(c == 0 for c, res, st in tiles), "no tile left unclipped"
    assert refs[3][1]["clip"] == 1 and refs[3][1]["tw"] * refs[3][1]["th"] == 25
    # corner, edge and interior clamp regions (3 per axis).  Where the extension puts the last tile centre past
    # the image (67 and 45: centres at 67.5 and 45) the far regions do not exist, so the nine are asked of the
    # inputs together and of each input whose sides divide by 8
    seen = set()
    for (_, info), img in zip(refs, inputs):
        regions = {(int(ry), int(rx)) for ry in info["region_y"] for rx in info["region_x"]}
        if img.shape[0] % 8 == 0 and img.shape[1] % 8 == 0:
            assert len(regions) == 9, (img.shape, regions)
        seen |= regions
    assert len(seen) == 9
    for (ref, info), img in zip(refs, inputs):
        got = U.clahe(img)
        diff = int(np.count_nonzero(got != ref))
        print("clahe probe %dx%d: tile %dx%d clip %d, %d pixels differ" %
              (img.shape[1], img.shape[0], info["tw"], info["th"], info["clip"], diff))
        assert got.shape == ref.shape and got.dtype == np.uint8
        assert np.array_equal(got, ref), (img.shape, diff)
    # a row stride larger than the width (a view into a wider buffer) reads the same pixels
    wide = np.zeros((45, 80), dtype=np.uint8)
    wide[:, :67] = inputs[1]
    assert np.array_equal(U.clahe(wide[:, :67]), refs[1][0])


def test_pyramid_bit_exact(euroc_yaml):
    import uvio_amd as U
    from clahe_ref import clahe_ref
    from oracle import oracle as O
    opts, s, r = _setup(euroc_yaml, 4, histogram_method=2)
    g, o = U.VioManager(opts), O.OracleManager(_variant(opts, histogram_method=0))
    for i, t, imgs in _frames(s, r, [0, 1], 2):
        g.feed_measurement_camera(t, [0, 1], imgs, allow_uninit=True)
        o.feed_measurement_camera(t, [0, 1], [clahe_ref(im) for im in imgs], allow_uninit=True)
        for c in (0, 1):
            for level in range(5):
                ig, dg = g.get_pyramid(c, level)
                io, do = o.get_pyramid(c, level)
                assert ig.shape == io.shape
                assert np.array_equal(ig, io), (i, c, level)
                assert np.array_equal(dg, do), (i, c, level)


def test_tracks_bit_exact(euroc_yaml):
    """12 stereo frames: same ids, same uv as the oracle on the reference's equalized frames."""
    import uvio_amd as U
    from clahe_ref import clahe_ref
    from oracle import oracle as O
    from test_gpu_track import _compare_tracks
    opts, s, r = _setup(euroc_yaml, 13, init_max_features=200, histogram_method=2)
    g, o = U.VioManager(opts), O.OracleManager(_variant(opts, histogram_method=0))
    n_dev = bad = n_oracle = 0
    for i, t, imgs in _frames(s, r, [0, 1], 12):
        g.feed_measurement_camera(t, [0, 1], imgs, allow_uninit=True)
        o.feed_measurement_camera(t, [0, 1], [clahe_ref(im) for im in imgs], allow_uninit=True)
        n, b = _compare_tracks(g, o, [0, 1])
        n_oracle += n
        bad += b
        n_dev += sum(len(g.get_tracks(c)[0]) for c in (0, 1))
    print("tracks over 12 frames: device %d, oracle %d, mismatched %d" % (n_dev, n_oracle, bad))
    # the oracle's own count is the floor: an empty or starved device tracker cannot pass
    assert n_oracle > 12 * 2 * 50  # the scene keeps the tracker busy
    assert n_dev >= n_oracle, (n_dev, n_oracle)
    assert bad == 0, (bad, n_oracle)


def test_tracks_bit_exact_downsampled(euroc_yaml):
    """downsample_cameras: CLAHE runs on the pyrDown'ed image.  The reference input is clahe_ref of the oracle's
    own pyrDown'ed frame: a first oracle (method 0, downsampling) is fed the raw frame and its level 0 read
    back; a second oracle (method 0, no downsampling: the configured cameras are the halved ones already) gets
    clahe_ref of it."""
    import uvio_amd as U
    from clahe_ref import clahe_ref
    from oracle import oracle as O
    from test_gpu_track import _compare_tracks
    opts, s, r = _setup(euroc_yaml, 5, init_max_features=200, histogram_method=2, downsample_cameras=1)
    # the rendered frames are the raw (configured-size) camera images; the manager tracks at half that size
    g = U.VioManager(opts)
    o_down = O.OracleManager(_variant(opts, histogram_method=0))
    o = O.OracleManager(_variant(opts, histogram_method=0, downsample_cameras=0))
    n_dev = bad = n_oracle = 0
    for i, t, imgs in _frames(s, r, [0, 1], 4):
        g.feed_measurement_camera(t, [0, 1], imgs, allow_uninit=True)
        o_down.feed_measurement_camera(t, [0, 1], imgs, allow_uninit=True)
        halves = [o_down.get_pyramid(c, 0)[0] for c in (0, 1)]
        assert halves[0].shape == (opts.cams[0].height, opts.cams[0].width)
        o.feed_measurement_camera(t, [0, 1], [clahe_ref(hf) for hf in halves], allow_uninit=True)
        for c in (0, 1):
            assert np.array_equal(g.get_pyramid(c, 0)[0], o.get_pyramid(c, 0)[0]), (i, c)
        n, b = _compare_tracks(g, o, [0, 1])
        n_oracle += n
        bad += b
        n_dev += sum(len(g.get_tracks(c)[0]) for c in (0, 1))
    print("downsampled tracks over 4 frames: device %d, oracle %d, mismatched %d" % (n_dev, n_oracle, bad))
    assert n_oracle > 4 * 2 * 50
    assert n_dev >= n_oracle, (n_dev, n_oracle)
    assert bad == 0, (bad, n_oracle)


class _ClaheFedOracle:
    """the oracle with histogram_method 0 behind a feed that equalizes the frames with clahe_ref first"""

    def __init__(self, opts):
        from oracle import oracle as O
        self._o = O.OracleManager(_variant(opts, histogram_method=0))

    def feed_measurement_camera(self, t, cams, imgs, **kw):
        from clahe_ref import clahe_ref
        return self._o.feed_measurement_camera(t, cams, [clahe_ref(im) for im in imgs], **kw)

    def __getattr__(self, name):
        return getattr(self._o, name)


def test_lockstep_short(euroc_yaml):
    """6 frames with the estimator on (track -> propagate -> update), tests/test_gpu_parity.py's lock-step: the
    oracle adopts the device's state before every frame, and x / P agree to 1e-10 after it."""
    import test_gpu_parity as P
    import uvio_amd as U
    from test_gpu_track import _compare_tracks
    opts, s, r = _setup(euroc_yaml, 6, init_max_features=200, max_msckf_in_update=200, histogram_method=2)
    g, o = U.VioManager(opts), _ClaheFedOracle(opts)
    steps = P.Steps()
    bad = [0]

    def before(nf, t):
        o.set_state(g.get_state_vector()[0], g.get_fej_vector(), g.get_cov())

    def before_feed(m):
        if m is o:
            o.set_steer(g.debug_frame_feats())

    def after(nf, t):
        bad[0] += _compare_tracks(g, o, [0, 1])[1]
        steps.append((P._snap(g), P._snap(o)))

    s.run([g, o], n_frames=6, before_frame=before, before_feed=before_feed, on_frame=after, renderer=r)
    steps.steer = o.steer_log()
    g.close()
    assert len(steps) == 6 and bad[0] == 0
    worst = P._check_lockstep(steps)
    print("clahe lock-step worst", worst)
    assert worst["x"] < 1e-10 and worst["P"] < 1e-10


def test_clahe_rejects_bad_args(euroc_yaml):
    import ctypes as C
    import uvio_amd as U
    from uvio_amd import _native as N
    lib = N.load()
    img = np.zeros((16, 16), dtype=np.uint8)
    out = np.zeros((16, 16), dtype=np.uint8)
    bp = C.POINTER(C.c_uint8)
    pi, po = img.ctypes.data_as(bp), out.ctypes.data_as(bp)
    assert lib.uvio_hp_debug_clahe(None, 16, 16, 16, po) == N.E_ARG
    assert lib.uvio_hp_debug_clahe(pi, 16, 16, 16, None) == N.E_ARG
    assert lib.uvio_hp_debug_clahe(pi, 16, 16, 15, po) == N.E_ARG  # stride < w
    assert lib.uvio_hp_debug_clahe(pi, 8, 16, 16, po) == N.E_ARG   # a side below 9
    assert lib.uvio_hp_debug_clahe(pi, 16, 8, 16, po) == N.E_ARG
    assert lib.uvio_hp_debug_clahe(pi, 9, 9, 16, po) == 0          # the smallest image
    with pytest.raises(ValueError):
        U.clahe(np.zeros((16, 16), dtype=np.float32))
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.clahe(np.zeros((8, 32), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="E_CONFIG"):
        U.VioManager(U.load_options(euroc_yaml, histogram_method=3))
    with pytest.raises(RuntimeError, match="E_CONFIG"):
        U.VioManager(U.load_options(euroc_yaml, histogram_method=-1))
