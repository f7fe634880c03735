"""The image products on the device (kernels_viz.hip + engine_viz.cpp) against the sequential reference renderer
tests/viz_ref.py.  Tolerances: none -- the renderer is integer work and every comparison is byte for byte.

  * uvio_hp_debug_draw_tracks (the getter's kernels on caller-given inputs) on tiny inputs that reach every rule:
    history lengths around the cap, both draw orders of overlapping tracks, points outside / on every border and
    corner, half-integer coordinates, the highlight box, to_delete, a mask, two cameras of different sizes with
    strided rows, the not-small radii, and 400 x 50 random steps that overdraw most pixels many times (twice: the
    same bytes).
  * uvio_hp_get_track_image in estimator runs on rendered images at the small shapes of tests/shape_scene.py (mono E,
    the stereo pair Q of two sizes, E with O's kind of mask), with SLAM landmarks and marginalized clones.  The
    reference renderer is fed through public getters only.  Every frame is compared (so the first, the last and
    the one before the first marginalization are).
  * uvio_hp_get_track_history against the test's own per-frame record of uvio_hp_get_tracks.
  * uvio_hp_get_loop_depth against the restatement on the stereo run's last frame and on a hand-made case.
  * a run that calls the getters after every frame ends in the same state bytes as one that never does.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import viz_ref as R  # noqa: E402
from shape_scene import BY_NAME  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUROC = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")


def _track(hist, ident=1, n_cams=1, highlighted=0, to_delete=0, at=None):
    hist = np.asarray(hist, dtype=np.float32).reshape(-1, 2)
    u, v = at if at is not None else ((hist[-1, 0], hist[-1, 1]) if len(hist) else (0.0, 0.0))
    return {"id": ident, "u": float(u), "v": float(v), "highlighted": highlighted, "n_cams": n_cams,
            "to_delete": to_delete, "hist": hist}


def _image(rng, w, h, pad=0):
    """a random u8 image; with pad, a view of a wider buffer (row stride w + pad)"""
    buf = rng.integers(0, 256, (h, w + pad), dtype=np.uint8)
    return buf[:, :w]


def _same(images, tracks, masks=None):
    import uvio_amd as U
    got = U.draw_tracks(images, tracks, masks)
    want = R.draw_tracks(images, tracks, masks)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=2))
    assert len(bad[0]) == 0, (len(bad[0]), [(int(x), int(y), got[y, x].tolist(), want[y, x].tolist())
                                            for y, x in list(zip(*bad))[:5]])
    return got


def _walk(rng, n, w, h, step=3.0, start=None):
    p = np.array(start if start is not None else (rng.uniform(2, w - 2), rng.uniform(2, h - 2)))
    out = []
    for _ in range(n):
        out.append(p.copy())
        p = p + rng.uniform(-step, step, 2)
    return np.array(out, dtype=np.float32)


# ---------------------------------------------------------------- uvio_hp_debug_draw_tracks, one 31 x 31 camera
def test_no_tracks_is_the_gray_image():
    rng = np.random.default_rng(1)
    img = _image(rng, 31, 31)
    out = _same([img], [[]])
    assert (out == img[:, :, None]).all()


@pytest.mark.parametrize("size", [1, 2, 51, 52, 60])
def test_history_lengths(size):
    rng = np.random.default_rng(10 + size)
    img = _image(rng, 31, 31)
    hist = np.stack([np.linspace(1, 29, size), 15 + 10 * np.sin(np.arange(size) / 3.0)], axis=1)
    out = _same([img], [[_track(hist)]])
    assert (out != img[:, :, None]).any() == (size > 1)


def test_overlapping_tracks_in_both_orders():
    rng = np.random.default_rng(2)
    img = _image(rng, 31, 31)
    a = _track([(2, 14), (9, 16), (16, 15), (22, 15), (28, 16)], ident=1, n_cams=1)
    b = _track([(15, 2), (16, 9), (15, 15), (16, 22), (15, 28)], ident=2, n_cams=2)
    ab, ba = _same([img], [[a, b]]), _same([img], [[b, a]])
    assert (ab != ba).any()


def test_points_outside_and_on_every_border_and_corner():
    rng = np.random.default_rng(3)
    img = _image(rng, 31, 31)
    w = h = 31
    corners = [(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1), (0, 0)]
    borders = [(15, 0), (w - 1, 15), (15, h - 1), (0, 15), (15, 0)]
    outside = [(-7, -3), (40, 5), (36, 44), (-20, 50), (15, -9), (15.2, 70), (-1, -1), (31, 31), (1e9, -1e9)]
    far = [(-3000, 12), (3000, 14), (10, -2500), (12, 2600)]  # long segments that cross the whole image
    tracks = [_track(corners, 1), _track(borders, 2, n_cams=2), _track(outside, 3), _track(far, 4),
              _track([(5, 5), (float("nan"), 3), (9, 9)], 5),
              _track([(-4, 8), (-2, 9)], 6, highlighted=1), _track([(29, 29), (30, 30)], 7, highlighted=1)]
    _same([img], [tracks])


def test_half_integer_coordinates_round_to_even():
    rng = np.random.default_rng(4)
    img = _image(rng, 31, 31)
    hist = [(0.5, 0.5), (1.5, 2.5), (2.5, 1.5), (3.5, 4.5), (10.5, 7.5), (11.5, 20.5), (20.5, 21.5)]
    _same([img], [[_track(hist), _track([(3, 3), (6.5, 5.5)], 2, highlighted=1)]])


def test_highlighted_and_to_delete_tracks():
    rng = np.random.default_rng(5)
    img = _image(rng, 31, 31)
    hist = _walk(rng, 8, 31, 31)
    out = _same([img], [[_track(hist, highlighted=1), _track(_walk(rng, 8, 31, 31), 2, to_delete=1),
                         _track(_walk(rng, 5, 31, 31), 3, to_delete=1, highlighted=1), _track([], 4, highlighted=1,
                                                                                             at=(12.0, 3.5))]])
    assert ((out == (0, 255, 0)).all(axis=2)).sum() >= 3 * 20


def test_mask_over_half_the_image():
    rng = np.random.default_rng(6)
    img = _image(rng, 31, 31)
    img[0, :6] = (0, 1, 229, 230, 254, 255)
    mask = np.zeros((31, 31), dtype=np.uint8)
    mask[:, :16] = 255
    mask[5, :] = 128
    mask[6, :] = 127
    out = _same([img], [[_track(_walk(rng, 20, 31, 31)), _track(_walk(rng, 20, 31, 31), 2, n_cams=2)]], [mask])
    assert out.shape == (31, 31, 3)
    # without tracks: 127 is not set, 128 is; a masked pixel differs from the gray value in channel 2 only
    plain = _same([img], [[]], [mask])
    assert (plain[6, 16:] == img[6, 16:, None]).all() and (plain[5, :, :2] == img[5, :, None]).all()
    assert (plain[5, :, 2] != img[5, :]).sum() >= 25
    assert plain[0, :6, 2].tolist() == [26, 26, 254, 255, 255, 255]


def test_two_cameras_of_different_sizes_and_strides():
    rng = np.random.default_rng(7)
    a, b = _image(rng, 90, 30, pad=13), _image(rng, 31, 33, pad=5)
    assert a.strides[0] == 103 and b.strides[0] == 36
    ta = [_track(_walk(rng, 30, 90, 30, 6.0), i, n_cams=1 + i % 2, highlighted=i % 3 == 0) for i in range(6)]
    # camera 1's tracks run past its own 31 x 33 image into where its 90-wide cell is padding
    tb = [_track(_walk(rng, 30, 60, 40, 6.0, start=(28, 28)), 10 + i, highlighted=1) for i in range(6)]
    mask_b = np.zeros((33, 31), dtype=np.uint8)
    mask_b[20:, :] = 200
    out = _same([a, b], [ta, tb], [None, mask_b])
    assert out.shape == (33, 180, 3)
    assert (out[30:, :90] == 0).all() and (out[:, 90 + 31:] == 0).all()


def test_not_small_radii_and_half_sides():
    rng = np.random.default_rng(8)
    img = _image(rng, 416, 400)
    tracks = [_track(_walk(rng, 12, 416, 400, 9.0), i, n_cams=1 + i % 2, highlighted=i % 2) for i in range(12)]
    tracks.append(_track([(0, 0), (415, 399), (415, 0), (0, 399)], 99, highlighted=1))
    _same([img], [tracks])


def test_400_tracks_of_50_steps_overdrawn_and_repeatable():
    import uvio_amd as U
    rng = np.random.default_rng(9)
    img = _image(rng, 64, 48)
    tracks = [_track(np.stack([rng.uniform(-3, 67, 51), rng.uniform(-3, 51, 51)], axis=1), i, n_cams=1 + i % 2,
                     highlighted=i % 7 == 0) for i in range(400)]
    first = _same([img], [tracks])
    again = U.draw_tracks([img], [tracks])
    assert first.tobytes() == again.tobytes()


def test_stage_times_are_reported():
    """the five device stage times (uploads, base, primitives, compose, copy out) of the stand-alone entry and of a
    handle's own call (uvio_hp_debug_track_image_times): what tools/viz_times.py reads"""
    import uvio_amd as U
    rng = np.random.default_rng(12)
    img = _image(rng, 64, 48)
    tracks = [_track(_walk(rng, 20, 64, 48), i) for i in range(20)]
    out, ms = U.draw_tracks([img], [tracks], stage_ms=True)
    assert np.array_equal(out, R.draw_tracks([img], [tracks]))
    assert ms.shape == (5,) and np.all(np.isfinite(ms)) and np.all(ms >= 0) and ms[1:4].min() > 0
    case = BY_NAME["A"]
    g = U.VioManager(case.options(EUROC))
    frames = case.raw_frames()
    for i in range(2):
        g.feed_measurement_camera(case.time(i), case.cam_ids, frames[i], allow_uninit=True)
    assert not g.track_image_times(on=True).any()   # nothing timed yet
    first, _ = g.get_track_image()
    ms = g.track_image_times(on=False)
    assert np.all(np.isfinite(ms)) and np.all(ms >= 0) and ms[1:4].min() > 0
    again, _ = g.get_track_image()                   # untimed: the same image, the times left as they were
    assert np.array_equal(first, again) and np.array_equal(g.track_image_times(on=False), ms)
    g.close()


# ---------------------------------------------------------------- uvio_hp_get_track_image in a run
N_RUN = 22
MAX_CLONES = 6


def _run_options(case, **extra):
    """The shape case's cameras with intrinsics scaled to its image width (the rendered room then fills the small
    image with corners), a short clone window and SLAM landmarks."""
    opts = case.options(EUROC, max_clone_size=MAX_CLONES, max_slam_features=12, max_slam_in_update=6, dt_slam_delay=0.2,
                        max_msckf_in_update=40, num_pts=60, init_max_features=60, grid_x=5, grid_y=4, min_px_dist=6,
                        try_zupt=0, **extra)
    for k, (w, h) in enumerate(case.cams):
        s = w / 752.0
        for j in range(4):
            opts.cams[k].intrinsics[j] *= s
    return opts


class _Feeder:
    """what SimStream.run drives: the manager, with the case's masks added to every camera feed"""

    def __init__(self, g, masks):
        self.g, self.masks = g, masks

    def __getattr__(self, name):
        return getattr(self.g, name)

    def feed_measurement_camera(self, t, cams, imgs, allow_uninit=False):
        return self.g.feed_measurement_camera(t, cams, imgs, masks=self.masks, allow_uninit=allow_uninit)


def _subsequence_ending_in_last(hist, rec):
    if len(hist) == 0 or not np.array_equal(hist[-1], rec[-1]):
        return False
    j = 0
    for p in hist:
        while j < len(rec) and not np.array_equal(rec[j], p):
            j += 1
        if j == len(rec):
            return False
        j += 1
    return True


def _ref_inputs(g, cams, masks, slam_ids):
    """the reference renderer's inputs through public getters only"""
    images, tracks = [], []
    for k in cams:
        images.append(g.get_pyramid(k, 0)[0])
        ids, uv = g.get_tracks(k)
        tr = []
        for i, fid in enumerate(ids):
            hist, n_cams, to_delete = g.get_track_history(k, fid)
            tr.append({"id": int(fid), "u": float(uv[i, 0]), "v": float(uv[i, 1]), "highlighted": int(fid) in slam_ids,
                       "n_cams": n_cams, "to_delete": to_delete, "hist": hist})
        tracks.append(tr)
    return images, tracks, masks


def _run(case, masks=None, use_getters=True, n_frames=N_RUN, **extra):
    """One estimator run on rendered images; with use_getters every frame's track image (host and device variant)
    is compared with the reference renderer and the histories with the record.  Returns a summary."""
    import uvio_amd as U
    from uvio_amd.render import SceneRenderer
    from uvio_amd.sim import SimStream
    opts = _run_options(case, **extra)
    cams = case.cam_ids
    sim = SimStream(opts, duration=n_frames / opts.track_frequency + 1.2, seed=5, spawn=4)
    g = U.VioManager(opts)
    out = {"frames": 0, "slam": 0, "marg": 0, "drawn": 0, "highlighted": 0, "consumed": 0, "stereo": 0}
    record = {k: {} for k in cams}  # camera -> feature id -> [uv per frame it was tracked in]
    state = {"marg": False, "full": False}
    if use_getters:
        img0, ov0 = g.get_track_image()
        assert img0.shape == (0, 0, 3)  # before the first feed: the reference's empty cv::Mat

    def on_frame(nf, t):
        out["frames"] = nf
        # a frame that starts with a full window marginalizes its oldest clone
        if state["full"]:
            state["marg"] = True
        state["full"] = len(g.get_clone_times()) >= MAX_CLONES
        if not use_getters:
            return
        # The record: every later frame's get_tracks.  The first feed only detects (TrackKLT.cpp:110-127 returns
        # before database->update_feature), so its points are in pts_last but not in the database
        for k in cams:
            ids, uv = g.get_tracks(k)
            for i, fid in enumerate(ids):
                if nf > 1:
                    record[k].setdefault(int(fid), []).append(uv[i].copy())
        slam_ids = set(g.get_features_slam())
        used = {int(i) for i in g.debug_frame_feats()[1]}  # the features of this frame's updater calls
        images, tracks, mk = _ref_inputs(g, cams, masks, slam_ids)
        for k, tr in zip(cams, tracks):
            assert nf > 1 or len(tr) > 0
            for t_ in tr:
                rec = np.array(record[k].get(t_["id"], []), dtype=np.float32).reshape(-1, 2)
                if nf == 1:
                    assert len(t_["hist"]) == 0 and t_["n_cams"] == 0
                elif not state["marg"]:
                    assert np.array_equal(t_["hist"], rec), (nf, k, t_["id"], len(t_["hist"]), len(rec))
                elif t_["n_cams"] == 0:
                    # unknown to the database although tracked: only a feature that an updater of this very frame
                    # consumed (to_delete, UpdaterMSCKF.cpp:262, UpdaterSLAM.cpp:235, 456, then the database's
                    # cleanup) -- the tracker enters it again at the next feed.  The reference draws such a track
                    # as its highlight box alone
                    assert len(t_["hist"]) == 0 and t_["id"] in used, (nf, k, t_["id"])
                    out["consumed"] += 1
                else:
                    assert _subsequence_ending_in_last(t_["hist"], rec), (nf, k, t_["id"], len(t_["hist"]), len(rec))
                out["stereo"] += t_["n_cams"] > 1
        want = R.draw_tracks(images, tracks, mk)
        got, overlay = g.get_track_image()
        assert overlay == 0
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got, want), (nf, int((got != want).any(axis=2).sum()))
        dev, ov_dev = g.get_track_image(device=True)
        assert ov_dev == 0 and dev.cpu().numpy().tobytes() == got.tobytes(), nf
        gray = np.concatenate([np.pad(im, ((0, got.shape[0] - im.shape[0]), (0, got.shape[1] // len(cams) - im.shape[1])))
                               for im in images], axis=1)
        out["drawn"] += int((got != gray[:, :, None]).any(axis=2).sum())
        out["highlighted"] += sum(t_["highlighted"] for tr in tracks for t_ in tr)
        out["slam"] = max(out["slam"], len(slam_ids))
        out["marg"] += state["marg"]
        t_d, depth, viz = g.get_loop_depth()
        if nf == n_frames:
            out["last"] = (images, g.get_active_tracks(), t_d, depth, viz)

    sim.run(_Feeder(g, masks), n_frames=n_frames, on_frame=on_frame, renderer=SceneRenderer(opts, device="cuda"))
    out["x"], out["P"] = g.get_state_vector()[0], g.get_cov()
    g.close()
    return out


def _check_run(out):
    assert out["frames"] == N_RUN
    assert out["drawn"] > 2000, out["drawn"]          # tracks were drawn
    assert out["slam"] > 0 and out["highlighted"] > 0, (out["slam"], out["highlighted"])  # landmarks exist
    assert out["marg"] >= 5, out["marg"]              # frames after clones were marginalized


@pytest.fixture(scope="module")
def mono_run():
    return _run(BY_NAME["E"])


def test_track_image_mono_run(mono_run):
    _check_run(mono_run)


def test_track_image_stereo_run_and_loop_depth():
    out = _run(BY_NAME["Q"])
    _check_run(out)
    assert out["stereo"] > 0  # the stereo colours were used
    images, (t_act, _, uvd), t_d, depth, viz = out["last"]
    assert t_d == t_act and len(uvd) > 0
    ids = sorted(uvd)
    want_depth, want_viz = R.loop_depth(images[0], ids, [uvd[i] for i in ids])
    assert np.array_equal(depth, want_depth) and np.array_equal(viz, want_viz)
    assert np.count_nonzero(depth) > 0 and (viz != images[0][:, :, None]).any()


def test_track_image_masked_run():
    case = BY_NAME["E"]
    w, h = case.cams[0]
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[:, :40] = 255
    mask[100:, 150:] = 255
    out = _run(case, masks=[mask])
    _check_run(out)


def test_feed_is_unchanged_by_the_getters(mono_run):
    quiet = _run(BY_NAME["E"], use_getters=False)
    assert quiet["x"].tobytes() == mono_run["x"].tobytes()
    assert quiet["P"].tobytes() == mono_run["P"].tobytes()


def test_size_query_capacity_and_overlay_before_initialization():
    import ctypes as C
    import uvio_amd as U
    from uvio_amd import _native as N
    case = BY_NAME["A"]
    g = U.VioManager(case.options(EUROC))
    lib = N.load()
    w, h, ov = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    buf = np.zeros(3 * 67 * 45, dtype=np.uint8)
    bp = C.POINTER(C.c_uint8)
    # before the first feed: 0 x 0, nothing written, "init"
    assert lib.uvio_hp_get_track_image(g._h, buf.ctypes.data_as(bp), buf.size, C.byref(w), C.byref(h), C.byref(ov)) == 0
    assert (w.value, h.value, ov.value) == (0, 0, 1) and not buf.any()
    frames = case.raw_frames()
    for i in range(2):
        g.feed_measurement_camera(case.time(i), case.cam_ids, frames[i], allow_uninit=True)
    assert lib.uvio_hp_get_track_image(g._h, None, 0, C.byref(w), C.byref(h), C.byref(ov)) == 0
    assert (w.value, h.value, ov.value) == (67, 45, 1)
    assert lib.uvio_hp_get_track_image(g._h, buf.ctypes.data_as(bp), buf.size - 1, C.byref(w), C.byref(h),
                                       C.byref(ov)) == N.E_CAPACITY
    assert (w.value, h.value) == (67, 45) and not buf.any()
    img, overlay = g.get_track_image()
    assert overlay == 1 and img.shape == (45, 67, 3)
    slam = set(g.get_features_slam())
    assert np.array_equal(img, R.draw_tracks(*_ref_inputs(g, case.cam_ids, None, slam)))
    # an unknown feature has no history
    hist, n_cams, to_delete = g.get_track_history(0, 10 ** 9)
    assert len(hist) == 0 and n_cams == 0 and to_delete == 0
    g.close()


def test_overlay_on_a_zero_velocity_update_frame():
    """the shipped iros_2023_uvio ZUPT settings on a platform that rests first (the scene of
    tests/test_gpu_zupt_retri.py::test_zupt_iros_config_disparity_images)"""
    import uvio_amd as U
    from uvio_amd.render import SceneRenderer
    from uvio_amd.sim import SimStream
    opts = U.load_options(os.path.join(ROOT, "configs", "iros_2023_uvio", "estimator_config.yaml"),
                          init_max_features=150, use_uwb=0)
    n = 30
    sim = SimStream(opts, duration=n / opts.track_frequency + 1.2, seed=5, spawn=4, static_for=1.0)
    g = U.VioManager(opts)
    seen = []

    def on_frame(nf, t):
        z = g.get_timing()["zupt"]
        if not seen or seen[-1][0] != z:  # the first frame and every change of the flag
            img, overlay = g.get_track_image()
            assert overlay == (2 if z else 0), (nf, z, overlay)
            assert img.shape[2] == 3 and img.size > 0
            seen.append((z, nf))

    sim.run(g, n_frames=n, on_frame=on_frame, renderer=SceneRenderer(opts, device="cuda"))
    g.close()
    assert {z for z, _ in seen} == {0, 1}, seen


# ---------------------------------------------------------------- uvio_hp_get_loop_depth, a hand-made case
def test_loop_depth_overlap_and_border_limits():
    import uvio_amd as U
    rng = np.random.default_rng(11)
    img = _image(rng, 24, 20, pad=3)
    w, h, dw = 24, 20, 4
    ids = [7, 3, 5, 9, 11, 13, 15, 17, 19, 2]
    uvd = [(10.9, 8.2, 2.0), (12.0, 9.0, 0.5),      # overlapping squares: id 7 is drawn over id 3
           (dw, h - dw, 1.0), (w - dw, dw, 70.0),   # on the limits (inside): lower u, upper v; upper u, lower v
           (dw - 1e-9, 10, 1.0), (w - dw + 1e-9, 10, 1.0), (10, dw - 1e-9, 1.0), (10, h - dw + 1e-9, 1.0),  # just outside
           (15.5, 12.5, 0.3), (8.0, 14.0, 1e-3)]
    depth, viz = U.loop_depth(img, ids, uvd)
    want_depth, want_viz = R.loop_depth(img, ids, uvd)
    assert np.array_equal(depth, want_depth) and np.array_equal(viz, want_viz)
    assert np.count_nonzero(depth) == 6
    assert tuple(viz[6, 9]) == R.depth_colour(2.0)  # inside the squares of ids 3 and 7 only: 7 is drawn later
