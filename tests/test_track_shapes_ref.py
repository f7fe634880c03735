"""The oracle's TrackKLT restatement (oracle/src/tracker*.cpp) on its own at the image shapes of
tests/shape_scene.py, before the device is held to it at those shapes (tests/test_gpu_track_shapes.py).  CPU only.

  * Every case, frame, camera and level: the oracle manager's pyramid (image and Scharr derivatives) equals
    the chain of the NumPy definitions of tests/test_oracle_tracker.py: _np_equalize (or the identity, or
    clahe_ref), _np_pyr_down per level, _np_scharr; with downsample_cameras one _np_pyr_down of the raw frame
    comes first.  Bit-exact: all of it is integer work.
  * The number of levels equals the rule (level 0, then halve until the next side would be <= 15) and the
    case table's column; asking for level `depth` raises.
  * Floors on the oracle's own track counts, so that no device case can pass on a starved tracker.  Totals
    over the 6 frames per camera, measured with shape_scene's generator when this test was written:

        A 77    B 77    C 354   D 321   E 431   F 480   G 575   H 599   I 595   J 106   K 0   L 132
        M 303 / 52 (two mono runs)   N 192   O 234   P 241 / 222   Q 301 / 236
        R 220 / 86 / 254 / 170       S 281 / 266

    Each total must stay >= half of that; K is exactly 0 (6 x 6 cells hold no FAST ring).  B and M's 67 x 45
    camera drop to zero tracks on some frames (B: frame 4; M: frames 1 and 5).
  * Every camera of every case but K keeps at least one track from one frame into the next, so LK and RANSAC
    are compared on the device.  No case needed another seed for it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from shape_scene import CASES, N_FRAMES, depth_rule  # noqa: E402

MEASURED = {"A": [77], "B": [77], "C": [354], "D": [321], "E": [431], "F": [480], "G": [575], "H": [599],
            "I": [595], "J": [106], "K": [0], "L": [132], "M": [303, 52], "N": [192], "O": [234],
            "P": [241, 222], "Q": [301, 236], "R": [220, 86, 254, 170], "S": [281, 266]}

_RUNS = {}


def _chain(case, raw):
    """[(img, der)] per level of one camera's frame, from the NumPy definitions"""
    from clahe_ref import clahe_ref
    from test_oracle_tracker import _np_equalize, _np_pyr_down, _np_scharr
    img = _np_pyr_down(raw) if case.downsample else raw
    img = {0: lambda a: a, 1: _np_equalize, 2: clahe_ref}[case.method](img)
    out = []
    for _ in range(depth_rule(img.shape[1], img.shape[0])):
        out.append((img, _np_scharr(img)))
        img = _np_pyr_down(img)
    return out


def _run(case, yaml):
    """one oracle run per case (every part of it), shared by the tests below"""
    if case.name in _RUNS:
        return _RUNS[case.name]
    from oracle import oracle as O
    rec = {"pyr_bad": [], "depth": [], "past_end": [], "counts": [], "survive": []}
    for part in case.parts():
        o = O.OracleManager(part.oracle_options(yaml))
        prev = [set() for _ in part.cams]
        survive = [False] * len(part.cams)
        counts = np.zeros((N_FRAMES, len(part.cams)), dtype=int)
        for i, imgs in enumerate(part.raw_frames()):
            o.feed_measurement_camera(part.time(i), part.cam_ids, part.oracle_images(imgs), masks=part.masks(),
                                      allow_uninit=True)
            for k in part.cam_ids:
                ref = _chain(part, imgs[k])
                for level, (img, der) in enumerate(ref):
                    io, do = o.get_pyramid(k, level)
                    if not (io.shape == img.shape and np.array_equal(io, img) and np.array_equal(do, der)):
                        rec["pyr_bad"].append((part.name, i, k, level))
                ids = set(int(x) for x in o.get_tracks(k)[0])
                counts[i, k] = len(ids)
                survive[k] |= bool(i and ids & prev[k])
                prev[k] = ids
                if i == N_FRAMES - 1:
                    rec["depth"].append(len(ref))
                    try:
                        o.get_pyramid(k, len(ref))
                        rec["past_end"].append(False)
                    except RuntimeError as e:
                        rec["past_end"].append("E_STATE" in str(e))
        rec["counts"].append(counts)
        rec["survive"] += survive
    rec["totals"] = [int(t) for c in rec["counts"] for t in c.sum(axis=0)]
    _RUNS[case.name] = rec
    return rec


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_pyramid_equals_numpy_chain(euroc_yaml, case):
    rec = _run(case, euroc_yaml)
    assert rec["pyr_bad"] == []


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_depth_follows_the_rule(euroc_yaml, case):
    rec = _run(case, euroc_yaml)
    assert [depth_rule(w, h) for w, h in case.cams] == case.depth
    assert rec["depth"] == case.depth  # every level below `depth` was read back for the chain comparison
    assert all(rec["past_end"]), "get_pyramid(level = depth) must raise E_STATE"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_track_floors(euroc_yaml, case):
    rec = _run(case, euroc_yaml)
    print("case %s: totals %s (measured %s), per frame %s" %
          (case.name, rec["totals"], MEASURED[case.name], [c.tolist() for c in rec["counts"]]))
    if case.name == "K":
        assert rec["totals"] == [0]
        return
    assert len(rec["totals"]) == len(MEASURED[case.name])
    for got, measured in zip(rec["totals"], MEASURED[case.name]):
        assert 2 * got >= measured, (rec["totals"], MEASURED[case.name])
    assert all(rec["survive"]), rec["survive"]
