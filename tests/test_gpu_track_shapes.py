"""The KLT front-end (kernels_track.hip + engine_track.cpp) against the oracle's TrackKLT restatement at image
shapes the other device tests never feed: sides that are no multiple of 4, 8 or the 64 x 16 / 32 x 8 tiles, odd
sides at every level, pyramids of 1, 2, 3, 4, 5 and 6 levels, levels narrower than a tile or than LK's staged
window, FAST cells with a remainder strip or too small for a ring, cameras of different sizes and depths in one
launch (independent and as a stereo pair), CLAHE / decimation / masks at such sizes, and images handed over in
device memory, packed and as a strided, misaligned view.  The cases and what each reaches: tests/shape_scene.py.

Tolerances: none.  As tests/test_gpu_track.py states, the front-end is integer and individually rounded float
work in the oracle's operation order, so after every one of the 6 frames of a case
  * both sides report the same number of pyramid levels, and asking either for level `depth` fails with E_STATE;
  * every level's image and Scharr derivatives are bit-exact (frames after the first are where a stale histogram
    or a stale pyramid slot would show);
  * every camera's track ids and uv are bit-exact (_compare_tracks of tests/test_gpu_track.py: 0 mismatches).
The one exception tests/test_gpu_track.py allows for, an acos / cos ulp flipping a RANSAC inlier, was not
observed in any case: no seed was changed.

The oracle's own track totals over the 6 frames (per camera), the floor under every case here, are pinned at
>= half of these by tests/test_track_shapes_ref.py on the CPU, which also pins the oracle's pyramids at these
shapes against the NumPy definitions:

    A 77    B 77    C 354   D 321   E 431   F 480   G 575   H 599   I 595   J 106   K 0   L 132
    M 303 / 52 (two mono runs)   N 192   O 234   P 241 / 222   Q 301 / 236
    R 220 / 86 / 254 / 170       S 281 / 266

Case K (31 x 31, 6 x 6 cells) holds zero tracks on both sides after every frame; its pyramids are still compared.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

from shape_scene import BY_NAME, ORDER  # noqa: E402


def _depth(m, cam, expect):
    """levels 0 .. expect - 1 exist, level `expect` fails with E_STATE"""
    for level in range(expect):
        m.get_pyramid(cam, level)
    with pytest.raises(RuntimeError, match="E_STATE"):
        m.get_pyramid(cam, expect)


def _compare_pyramids(g, o, part, where):
    for k in part.cam_ids:
        for level in range(part.depth[k]):
            ig, dg = g.get_pyramid(k, level)
            io, do = o.get_pyramid(k, level)
            assert ig.shape == io.shape, (where, k, level, ig.shape, io.shape)
            assert np.array_equal(ig, io), (where, k, level, "image", int(np.count_nonzero(ig != io)))
            assert np.array_equal(dg, do), (where, k, level, "derivatives", int(np.count_nonzero(dg != do)))


def _device_images(imgs, strided):
    """the frames as uint8 CUDA tensors: packed, or views buf[:, 5:5 + w] of (h, w + 13) buffers (row stride !=
    width, base pointer 5 bytes past the buffer's alignment)"""
    import torch
    out = []
    for im in imgs:
        h, w = im.shape
        if not strided:
            t = torch.from_numpy(im).cuda()
            assert t.stride(0) == w and t.data_ptr() % 16 == 0
        else:
            buf = torch.full((h, w + 13), 255, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            t = buf[:, 5:5 + w]
            t.copy_(torch.from_numpy(im))
            assert t.stride(0) == w + 13 and t.data_ptr() % 16 == 5
        out.append(t)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ORDER, ids=lambda c: c.name)
def test_shape_case(euroc_yaml, case):
    import uvio_amd as U
    from oracle import oracle as O
    from test_gpu_track import _compare_tracks
    for part in case.parts():
        g, o = U.VioManager(part.options(euroc_yaml)), O.OracleManager(part.oracle_options(euroc_yaml))
        masks = part.masks()
        total = np.zeros(len(part.cams), dtype=int)
        for i, imgs in enumerate(part.raw_frames()):
            g.feed_measurement_camera(part.time(i), part.cam_ids, imgs, masks=masks, allow_uninit=True)
            o.feed_measurement_camera(part.time(i), part.cam_ids, part.oracle_images(imgs), masks=masks,
                                      allow_uninit=True)
            for k in part.cam_ids:
                _depth(g, k, part.depth[k])
                _depth(o, k, part.depth[k])
            _compare_pyramids(g, o, part, (part.name, i))
            n, bad = _compare_tracks(g, o, part.cam_ids)
            assert bad == 0, (part.name, i, bad, n)
            for k in part.cam_ids:
                ng, no = len(g.get_tracks(k)[0]), len(o.get_tracks(k)[0])
                assert ng == no, (part.name, i, k, ng, no)
                total[k] += no
        print("case %s: oracle track totals %s, all equal on the device" % (part.name, total.tolist()))
        if case.name == "K":
            assert total.tolist() == [0]
        else:
            assert np.all(total > 0), total  # the floors proper: tests/test_track_shapes_ref.py
        g.close()


@pytest.mark.parametrize("name", ["A", "E", "N", "R"])
def test_device_fed_images(euroc_yaml, name):
    """feed_measurement_camera_device: the same frames through (a) the host feed, (b) packed uint8 CUDA tensors
    (the 16-byte histogram path and its tail) and (c) strided, misaligned views (the byte histogram path, the
    level-0 row stride, for N the decimation's source stride).  All three are bit-identical in pyramids and
    tracks and equal the oracle."""
    import uvio_amd as U
    from oracle import oracle as O
    from test_gpu_track import _compare_tracks
    case = BY_NAME[name]
    assert not case.separate and case.masks() is None
    o = O.OracleManager(case.oracle_options(euroc_yaml))
    gs = {feed: U.VioManager(case.options(euroc_yaml)) for feed in ("host", "packed", "strided")}
    total = 0
    for i, imgs in enumerate(case.raw_frames()):
        t = case.time(i)
        o.feed_measurement_camera(t, case.cam_ids, case.oracle_images(imgs), allow_uninit=True)
        gs["host"].feed_measurement_camera(t, case.cam_ids, imgs, allow_uninit=True)
        for feed in ("packed", "strided"):
            dev = _device_images(imgs, feed == "strided")
            gs[feed].feed_measurement_camera_device(t, case.cam_ids, dev, allow_uninit=True)
        for feed, g in gs.items():
            _compare_pyramids(g, o, case, (name, feed, i))
            n, bad = _compare_tracks(g, o, case.cam_ids)
            assert bad == 0, (name, feed, i, bad, n)
            total += n
        for k in case.cam_ids:  # and directly against each other
            ia, ua = gs["host"].get_tracks(k)
            for feed in ("packed", "strided"):
                ib, ub = gs[feed].get_tracks(k)
                assert np.array_equal(ia, ib) and np.array_equal(ua, ub), (name, feed, i, k)
    assert total > 0
    for g in gs.values():
        g.close()
