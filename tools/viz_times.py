"""What the track-history image costs at the cfg3 shape ("Image products"), and the host
alternative beside it, on the same data.

A cfg3 run (bench.py's workload: two 512 x 512 cameras, 400 tracks each, 20 clones) of FRAMES frames on rendered
images; after its last frame

  * uvio_hp_get_track_image is called WARM + N times with the event timing on (uvio_hp_debug_track_image_times): the
    device milliseconds of the uploads, the base, primitive and compose kernels and the copy out, and the wall time of
    the whole call (the walk over the tracks and the database, the table build and the final host copy included);
  * the host alternative: uvio_hp_get_pyramid level 0 for both cameras plus the same drawing in C++ on the host
    (tools/viz_host.cpp, compiled here with g++ -O2), WARM + N times, wall time.  Its inputs besides the images (the
    tracks and their histories) are fetched once through the public getters before the loop and not counted: an
    adapter would have to keep them itself.  Its canvas must equal the device's, byte for byte.

Then the upper end, which no run reaches (the database holds a track only as far back as the oldest clone): 400
synthetic tracks per camera with full 50-step histories, through uvio_hp_debug_draw_tracks and the host drawing.

Medians; min and max beside them.

    python tools/viz_times.py [N] [WARM] [FRAMES]
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_lib():
    out = os.path.join(ROOT, "build", "libviz_host.so")
    src = os.path.join(ROOT, "tools", "viz_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                               "-o", out])
    return C.CDLL(out)


def stats(name, v):
    v = np.asarray(v)
    print("  %-34s %8.4f  (min %.4f max %.4f)" % (name, np.median(v), v.min(), v.max()))
    return float(np.median(v))


def main():
    import bench
    import uvio_amd as U
    from uvio_amd import _native as N
    from uvio_amd.render import SceneRenderer
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    opts = bench.workload_options(U, "cfg3")
    sim = bench.make_stream(opts, frames + 2, seed=5, workload="cfg3")
    g = U.VioManager(opts)
    sim.run(g, n_frames=frames, renderer=SceneRenderer(opts, device="cuda"))
    lib = N.load()
    bp, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    cams = list(range(opts.num_cameras))

    # ---- the getter ----
    w, h, ov = C.c_int(), C.c_int(), C.c_int()
    assert lib.uvio_hp_get_track_image(g._h, None, 0, C.byref(w), C.byref(h), C.byref(ov)) == 0
    canvas = np.zeros((h.value, w.value, 3), dtype=np.uint8)
    g.track_image_times(on=True)
    ms, wall = [], []
    for i in range(warm + n):
        t0 = time.perf_counter()
        rc = lib.uvio_hp_get_track_image(g._h, canvas.ctypes.data_as(bp), canvas.size, C.byref(w), C.byref(h), C.byref(ov))
        t1 = time.perf_counter()
        assert rc == 0
        if i >= warm:
            ms.append(g.track_image_times(on=True))
            wall.append(1e3 * (t1 - t0))
    ms = np.array(ms)

    # ---- the host alternative's inputs, through public getters ----
    slam = set(g.get_features_slam())
    tracks, uv, counts, off = [], [], [], 0
    for k in cams:
        ids, pts = g.get_tracks(k)
        counts.append(len(ids))
        for i, fid in enumerate(ids):
            hist, n_cams, to_delete = g.get_track_history(k, fid)
            tracks.append(N.VizTrack(int(fid), float(pts[i, 0]), float(pts[i, 1]), int(int(fid) in slam), n_cams, to_delete,
                                     off, len(hist)))
            uv.append(hist)
            off += len(hist)
    lens = np.array([len(x) for x in uv])
    uv = np.ascontiguousarray(np.concatenate(uv), dtype=np.float32)
    arr = (N.VizTrack * len(tracks))(*tracks)
    cw, ch = w.value // len(cams), h.value
    imgs = [np.zeros((ch, cw), dtype=np.uint8) for _ in cams]
    img_p = (bp * len(cams))(*[im.ctypes.data_as(bp) for im in imgs])
    ws = np.array([cw] * len(cams), dtype=np.int32)
    hs = np.array([ch] * len(cams), dtype=np.int32)
    cnt = np.array(counts, dtype=np.int32)
    host = host_lib()
    host_canvas = np.zeros_like(canvas)
    pw, ph = C.c_int(), C.c_int()
    t_pyr, t_draw = [], []
    for i in range(warm + n):
        t0 = time.perf_counter()
        for k in cams:
            rc = lib.uvio_hp_get_pyramid(g._h, k, 0, C.byref(pw), C.byref(ph), imgs[k].ctypes.data_as(bp), None,
                                         imgs[k].size)
            assert rc == 0 and (pw.value, ph.value) == (cw, ch)
        t1 = time.perf_counter()
        host.viz_host_draw(len(cams), img_p, ws.ctypes.data_as(ip), hs.ctypes.data_as(ip), ws.ctypes.data_as(ip), None,
                           cnt.ctypes.data_as(ip), arr, uv.ctypes.data_as(C.POINTER(C.c_float)),
                           host_canvas.ctypes.data_as(bp))
        t2 = time.perf_counter()
        if i >= warm:
            t_pyr.append(1e3 * (t1 - t0))
            t_draw.append(1e3 * (t2 - t1))
    same = bool(np.array_equal(canvas, host_canvas))

    print("cfg3 run of %d frames: canvas %d x %d, tracks per camera %s, history steps per track mean %.1f max %d, "
          "%d SLAM landmarks; median of %d calls after %d (ms)" % (frames, w.value, h.value, counts, lens.mean(),
                                                                  lens.max(), len(slam), n, warm))
    print("uvio_hp_get_track_image, device stages (HIP events):")
    for j, name in enumerate(["uploads", "base", "primitives", "compose", "copy out"]):
        stats(name, ms[:, j])
    stats("sum of the stages", ms.sum(axis=1))
    stats("whole call, wall", wall)
    print("host alternative:")
    stats("uvio_hp_get_pyramid, both cameras", t_pyr)
    stats("drawing on the host (C++)", t_draw)
    stats("both, wall", np.array(t_pyr) + np.array(t_draw))
    print("host canvas equals the device canvas: %s" % same)
    g.close()
    return (0 if same else 1) + synthetic(U, N, host, n, warm)


def synthetic(U, N, host, n, warm, ncam=2, w=512, h=512, ntracks=400, steps=51, seed=3):
    """The upper end: every track with a full 50-step history (a run's database holds a track only as far back as
    its oldest clone), every tenth highlighted, through uvio_hp_debug_draw_tracks (the getter's renderer; the
    stand-alone entry's own allocations and image upload are outside the five stages) and the host drawing."""
    rng = np.random.default_rng(seed)
    images, tracks = [], []
    for k in range(ncam):
        images.append(rng.integers(0, 256, (h, w), dtype=np.uint8))
        cam = []
        for i in range(ntracks):
            p = np.cumsum(np.vstack([rng.uniform(20, [w - 20, h - 20]), rng.normal(0, 3.0, (steps - 1, 2))]), axis=0)
            cam.append({"id": i, "u": float(p[-1, 0]), "v": float(p[-1, 1]), "highlighted": int(i % 10 == 0),
                        "n_cams": ncam, "to_delete": 0, "hist": p.astype(np.float32)})
        tracks.append(cam)
    ms = []
    for i in range(warm + n):
        canvas, m = U.draw_tracks(images, tracks, stage_ms=True)
        if i >= warm:
            ms.append(m)
    ms = np.array(ms)
    bp, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    flat = [t for cam in tracks for t in cam]
    arr = (N.VizTrack * len(flat))(*[N.VizTrack(t["id"], t["u"], t["v"], t["highlighted"], t["n_cams"], 0, i * steps, steps)
                                     for i, t in enumerate(flat)])
    uv = np.ascontiguousarray(np.concatenate([t["hist"] for t in flat]), dtype=np.float32)
    img_p = (bp * ncam)(*[im.ctypes.data_as(bp) for im in images])
    ws, hs = np.array([w] * ncam, dtype=np.int32), np.array([h] * ncam, dtype=np.int32)
    cnt = np.array([ntracks] * ncam, dtype=np.int32)
    host_canvas = np.zeros_like(canvas)
    t_draw = []
    for i in range(warm + n):
        t0 = time.perf_counter()
        host.viz_host_draw(ncam, img_p, ws.ctypes.data_as(ip), hs.ctypes.data_as(ip), ws.ctypes.data_as(ip), None,
                           cnt.ctypes.data_as(ip), arr, uv.ctypes.data_as(C.POINTER(C.c_float)),
                           host_canvas.ctypes.data_as(bp))
        if i >= warm:
            t_draw.append(1e3 * (time.perf_counter() - t0))
    same = bool(np.array_equal(canvas, host_canvas))
    print("synthetic, %d x %d x %d, %d tracks x %d steps per camera; median of %d calls after %d (ms)" %
          (ncam, w, h, ntracks, steps - 1, n, warm))
    print("uvio_hp_debug_draw_tracks, device stages (HIP events):")
    for j, name in enumerate(["uploads", "base", "primitives", "compose", "copy out"]):
        stats(name, ms[:, j])
    stats("sum of the stages", ms.sum(axis=1))
    print("host alternative (images already on the host):")
    stats("drawing on the host (C++)", t_draw)
    print("host canvas equals the device canvas: %s" % same)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
