"""The sequential reference renderer of the image products (tests/viz_ref.py) against hand-written pixel sets: the
rendering rules of DESIGN.md section 4 ("Image products") one by one.  Also: the ctypes mirror declares the new
entry points, and the C++ facade's image-product part compiles and behaves without a GPU."""
import os
import re
import subprocess

import numpy as np

import viz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["uvio_hp_get_track_image", "uvio_hp_get_track_image_device", "uvio_hp_get_track_history",
               "uvio_hp_get_loop_depth", "uvio_hp_debug_draw_tracks", "uvio_hp_debug_loop_depth",
               "uvio_hp_debug_track_image_times"]


def _pixels(draw, w=8, h=8, x_off=0):
    """the set of (x, y) a primitive paints on a blank w x h view"""
    canvas = np.zeros((h, x_off + w, 3), dtype=np.uint8)
    draw(R.Painter(canvas, x_off, w, h))
    ys, xs = np.nonzero(canvas.any(axis=2))
    return {(int(x) - x_off, int(y)) for x, y in zip(xs, ys)}


WHITE = (255, 255, 255)


def test_cv_round_is_half_to_even():
    assert [R.cv_round(v) for v in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, 2.4999, 2.5001)] == [0, 2, 2, 4, 0, -2, 2, 3]


def test_cv_round_saturates_where_cvround_is_undefined():
    # DESIGN.md's rule: a NaN and anything beyond +-2^20 saturate there
    assert R.cv_round(1e9) == 1 << 20 and R.cv_round(-1e9) == -(1 << 20)
    assert R.cv_round(float("inf")) == 1 << 20 and R.cv_round(float("nan")) == -(1 << 20)
    assert R.cv_round(1048575.5) == 1 << 20 and R.cv_round(1048574.5) == 1048574


def test_disc_radius_1_is_the_plus():
    assert _pixels(lambda p: p.disc(3, 4, 1, WHITE)) == {(3, 3), (2, 4), (3, 4), (4, 4), (3, 5)}


def test_disc_radius_2_is_21_pixels():
    want = {(3 + dx, 3 + dy) for dy in (-2, 2) for dx in (-1, 0, 1)}
    want |= {(3 + dx, 3 + dy) for dy in (-1, 0, 1) for dx in (-2, -1, 0, 1, 2)}
    got = _pixels(lambda p: p.disc(3, 3, 2, WHITE))
    assert got == want and len(got) == 21


def test_disc_is_clipped_to_the_view():
    assert _pixels(lambda p: p.disc(0, 0, 1, WHITE)) == {(0, 0), (1, 0), (0, 1)}
    assert _pixels(lambda p: p.disc(7, 7, 2, WHITE), 8, 8) == {(5, 7), (6, 7), (7, 7), (5, 6), (6, 6), (7, 6), (6, 5),
                                                              (7, 5)}


def test_segments():
    assert _pixels(lambda p: p.segment(0, 0, 3, 1, WHITE)) == {(0, 0), (1, 0), (2, 1), (3, 1)}
    assert _pixels(lambda p: p.segment(0, 0, 1, 3, WHITE)) == {(0, 0), (0, 1), (1, 2), (1, 3)}
    assert _pixels(lambda p: p.segment(2, 2, 2, 2, WHITE)) == {(2, 2)}
    # a tie (the minor step falls exactly half way) goes with the direction of travel: a segment and its reverse
    # differ there
    assert _pixels(lambda p: p.segment(0, 0, 2, 1, WHITE)) == {(0, 0), (1, 1), (2, 1)}
    assert _pixels(lambda p: p.segment(2, 1, 0, 0, WHITE)) == {(2, 1), (1, 0), (0, 0)}
    # without a tie they are the same pixels
    assert _pixels(lambda p: p.segment(3, 1, 0, 0, WHITE)) == {(0, 0), (1, 0), (2, 1), (3, 1)}
    # diagonal, and negative directions on both axes
    assert _pixels(lambda p: p.segment(4, 4, 1, 1, WHITE)) == {(4, 4), (3, 3), (2, 2), (1, 1)}
    assert _pixels(lambda p: p.segment(5, 1, 1, 3, WHITE)) == {(5, 1), (4, 2), (3, 2), (2, 3), (1, 3)}


def test_segment_leaving_the_view_keeps_its_inside_pixels():
    # the walk over all steps of the unclipped segment, clipped per pixel, is what the clipped walk must give
    def all_steps(x0, y0, x1, y1, w, h):
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        sx, sy = np.sign(dx), np.sign(dy)
        out = set()
        for i in range(n + 1):
            if abs(dx) >= abs(dy):
                x, y = x0 + sx * i, y0 + sy * ((2 * i * abs(dy) + n) // (2 * n))
            else:
                x, y = x0 + sx * ((2 * i * abs(dx) + n) // (2 * n)), y0 + sy * i
            if 0 <= x < w and 0 <= y < h:
                out.add((int(x), int(y)))
        return out

    for seg in [(-5, 2, 12, 6), (12, 6, -5, 2), (3, -9, 5, 20), (5, 20, 3, -9), (-4, -4, -1, -1), (20, 3, 9, 3),
                (-3, 30, 30, -3), (7, 0, 7, 9), (-1, 5, -1, 6)]:
        assert _pixels(lambda p: p.segment(*seg, WHITE)) == all_steps(*seg, 8, 8), seg


def test_rectangle_clipped_by_the_image_corner():
    got = _pixels(lambda p: p.rectangle(-2, -2, 3, 3, WHITE), 6, 6)
    assert got == {(x, 3) for x in range(4)} | {(3, y) for y in range(4)}
    # the four one-pixel edges, nothing inside
    got = _pixels(lambda p: p.rectangle(1, 1, 4, 3, WHITE), 6, 6)
    assert got == {(x, y) for x in range(1, 5) for y in (1, 3)} | {(x, 2) for x in (1, 4)}


def test_fading_colour_at_size_3():
    assert R.history_colour(3, 2, False) == (85, 85, 255)
    assert R.history_colour(3, 1, False) == (170, 170, 255)
    assert R.history_colour(3, 2, True) == (255, 85, 85)
    assert R.history_colour(3, 1, True) == (255, 170, 170)
    # the truncation of TrackBase.cpp:194 ((int) of 255.0 / 7 * 3 = 109.28...)
    assert R.history_colour(7, 3, False) == (146, 146, 255)


def test_history_cap():
    assert R.history_steps(1) == []
    assert R.history_steps(2) == [1]
    assert R.history_steps(50) == list(range(49, 0, -1))
    assert R.history_steps(51) == list(range(50, 0, -1))
    assert R.history_steps(52) == list(range(51, 1, -1))
    assert R.history_steps(60) == list(range(59, 9, -1))


def _track(hist, ident=1, n_cams=1, highlighted=0, to_delete=0):
    hist = np.asarray(hist, dtype=np.float32).reshape(-1, 2)
    return {"id": ident, "u": float(hist[-1, 0]) if len(hist) else 0.0, "v": float(hist[-1, 1]) if len(hist) else 0.0,
            "highlighted": highlighted, "n_cams": n_cams, "to_delete": to_delete, "hist": hist}


def test_history_never_draws_the_oldest_point_and_stops_at_the_cap():
    img = np.zeros((9, 3 * 62 + 2), dtype=np.uint8)
    for size, first_drawn in ((2, 1), (51, 1), (52, 2), (60, 10)):
        hist = [(1 + 3 * k, 4) for k in range(size)]  # discs 3 apart: their pluses do not touch
        out = R.draw_tracks([img], [[_track(hist)]])
        drawn = [k for k in range(size) if out[4, 1 + 3 * k].any()]
        assert drawn == list(range(first_drawn, size)), size
        # the segment first_drawn -> first_drawn + 1 is there, nothing left of the first drawn disc
        assert not out[:, :3 * first_drawn].any()
        if size > first_drawn + 1:
            assert out[4, 3 * first_drawn + 2].any() and out[4, 3 * first_drawn + 3].any()


def test_to_delete_and_empty_histories_draw_nothing_but_the_highlight():
    img = np.full((31, 31), 9, dtype=np.uint8)
    hist = [(5, 5), (10, 10), (15, 12)]
    base = np.repeat(img[:, :, None], 3, axis=2)
    assert (R.draw_tracks([img], [[_track(hist, to_delete=1)]]) == base).all()
    assert (R.draw_tracks([img], [[_track([])]]) == base).all()
    out = R.draw_tracks([img], [[_track(hist, to_delete=1, highlighted=1)]])
    ys, xs = np.nonzero((out != base).any(axis=2))
    got = {(int(x), int(y)) for x, y in zip(xs, ys)}
    box = {(x, y) for x in range(12, 19) for y in (9, 15)} | {(x, y) for x in (12, 18) for y in range(9, 16)}
    assert got == box | {(15, 11), (14, 12), (15, 12), (16, 12), (15, 13)}
    assert all(tuple(out[y, x]) == (0, 255, 0) for x, y in got)


def test_overwrite_order_of_two_crossing_tracks():
    img = np.zeros((31, 31), dtype=np.uint8)
    a = _track([(2, 15), (4, 15), (28, 15)], ident=1, n_cams=1)   # horizontal, mono colours
    b = _track([(15, 1), (15, 3), (15, 29)], ident=2, n_cams=2)   # vertical, stereo colours
    ab = R.draw_tracks([img], [[a, b]])
    ba = R.draw_tracks([img], [[b, a]])
    # where they cross, the later track's segment is on top (the segment 1 -> 2 has z = 1's colour, 255 - 85 = 170;
    # z = 2, the newest point, has a disc only)
    assert tuple(ab[15, 15]) == (255, 170, 170)
    assert tuple(ba[15, 15]) == (170, 170, 255)
    # within a track the older step is drawn later: the z = 1 segment ends on the z = 2 disc's centre
    assert tuple(ab[15, 28]) == (170, 170, 255) and tuple(ab[14, 28]) == (85, 85, 255)
    assert (ab != ba).any(axis=2).sum() == 1


def test_mask_tint():
    assert [R.mask_tint(p) for p in (0, 1, 229, 230, 254, 255)] == [26, 26, 254, 255, 255, 255]
    img = np.array([[0, 1, 229, 230, 254, 255]] * 2, dtype=np.uint8)
    mask = np.array([[255] * 6, [127] * 6], dtype=np.uint8)  # set means > 127
    out = R.draw_tracks([img], [[]], [mask])
    assert out[0, :, 2].tolist() == [26, 26, 254, 255, 255, 255]
    assert out[1, :, 2].tolist() == img[1].tolist()
    assert (out[:, :, :2] == img[:, :, None]).all()


def test_canvas_of_two_cameras_pads_with_black_and_clips_to_each_camera():
    a = np.full((30, 90), 50, dtype=np.uint8)
    b = np.full((33, 31), 60, dtype=np.uint8)
    # a highlighted track at camera 1's right border: its box would reach into the padding of its 90-wide cell
    t = _track([(29, 10), (30, 31)], highlighted=1)
    t["u"], t["v"] = 30.0, 31.0
    out = R.draw_tracks([a, b], [[], [t]])
    assert out.shape == (33, 180, 3)
    assert (out[:30, :90] == 50).all() and (out[30:, :90] == 0).all()
    assert (out[:, 90 + 31:] == 0).all()
    assert tuple(out[28, 90 + 27]) == (0, 255, 0)


def test_depth_products():
    img = np.full((20, 24), 100, dtype=np.uint8)
    ids = [7, 3, 5, 9, 11]
    uvd = [(10.9, 8.2, 2.0),    # id 7, drawn after id 3 and 5
           (12.0, 9.0, 0.5),    # id 3
           (4.0, 16.0, 1.0),    # id 5: on the lower limits u = dw, v = h - dw
           (20.1, 10.0, 1.0),   # id 9: u > w - dw, skipped
           (20.0, 4.0, 70.0)]   # id 11: on the upper limit u = w - dw, v = dw; 70000 wraps in 16 bits
    depth, viz = R.loop_depth(img, ids, uvd)
    want = np.zeros((20, 24), dtype=np.uint16)
    want[8, 10], want[9, 12], want[16, 4], want[4, 20] = 2000, 500, 1000, 70000 - 65536
    assert (depth == want).all()
    assert R.depth_colour(2.0) == (255 - 127, 255 - 127, 0)
    assert R.depth_colour(0.5) == (0, 0, 255)
    assert R.depth_colour(1.0) == (0, 255, 0)
    # id 7's square (6..14, 4..12) lies over id 3's (8..16, 5..13)
    assert tuple(viz[9, 12]) == R.depth_colour(2.0) and tuple(viz[13, 12]) == R.depth_colour(0.5)
    assert tuple(viz[12, 15]) == R.depth_colour(0.5) and tuple(viz[12, 14]) == R.depth_colour(2.0)
    # the square at the right limit is clipped by the image: columns 16..23 of 16..24
    assert tuple(viz[0, 23]) == R.depth_colour(70.0) and tuple(viz[8, 16]) == R.depth_colour(70.0)
    assert tuple(viz[9, 17]) == (100, 100, 100)
    assert tuple(viz[19, 0]) == R.depth_colour(1.0) and tuple(viz[11, 5]) == (100, 100, 100)


def test_ctypes_mirror_declares_the_new_symbols():
    from uvio_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "uvio_hp.h")).read()
    declared = set(re.findall(r"\b(uvio_hp_[a-z0-9_]+)\s*\(", hdr))
    sigs = {"uvio_hp_" + s[0]: s for s in N.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in sigs and name in N.EXPORTED, name
    lib = N.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).argtypes == sigs[name][2]
    # the struct the draw call takes has the header's layout: u64, 2 floats, 5 ints
    assert N.VizTrack.hist_n.offset == 32 and C_sizeof(N.VizTrack) == 40


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_cpp_facade_viz_compiles_checks_arguments_and_fails_loudly_without_gpu(tmp_path):
    import torch
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_viz_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_viz_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    cfg = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
    # the no-device behaviour: hide the devices of a GPU host from the program
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "draw args ok" in r.stdout and "depth ok" in r.stdout and "code -3" in r.stdout
