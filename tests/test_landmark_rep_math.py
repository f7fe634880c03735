"""The six landmark representations' conversions (uvio_amd/csrc/landmark_rep.h, the one statement shared by the
host mean, k_feature's landmark read and the retriangulation) against a numpy statement of
ov_type::Landmark::get_xyz / set_from_xyz (Landmark.cpp:26-137), and the option loader's six names.  CPU only.

Bounds: 1e-14 relative (max abs difference / max abs value) for the round trip and for the comparison with
numpy.  The spherical representations recover phi with acos, whose error for a point at angle phi off the z axis
is eps / sin(phi): the round trip's relative error is about 1.1e-16 / tan(phi).  The points of the main table are
therefore drawn at least 0.05 rad off the axis (2.2e-15), which keeps the whole bound for every representation;
test_round_trip_near_the_optical_axis covers the cone that leaves out, with the bound that follows from acos.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["GLOBAL_3D", "GLOBAL_FULL_INVERSE_DEPTH", "ANCHORED_3D", "ANCHORED_FULL_INVERSE_DEPTH",
         "ANCHORED_MSCKF_INVERSE_DEPTH", "ANCHORED_INVERSE_DEPTH_SINGLE"]
TOL = 1e-14


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def np_set_from_xyz(rep, p):
    """Landmark::set_from_xyz (Landmark.cpp:65-137): (value, bearing); the bearing only for rep 5"""
    if rep in (0, 2):
        return p.copy(), None
    if rep in (1, 3):
        rho = 1 / np.linalg.norm(p)
        return np.array([np.arctan2(p[1], p[0]), np.arccos(rho * p[2]), rho]), None
    if rep == 4:
        return np.array([p[0] / p[2], p[1] / p[2], 1 / p[2]]), None
    return np.array([1.0 / p[2]]), (1.0 / p[2]) * p


def np_get_xyz(rep, val, fej, uvn0, getfej):
    """Landmark::get_xyz (Landmark.cpp:26-63); reps 4 and 5 ignore getfej"""
    p = fej if getfej else val
    if rep in (0, 2):
        return p.copy()
    if rep in (1, 3):
        return np.array([(1 / p[2]) * np.cos(p[0]) * np.sin(p[1]), (1 / p[2]) * np.sin(p[0]) * np.sin(p[1]),
                         (1 / p[2]) * np.cos(p[1])])
    if rep == 4:
        return np.array([(1 / val[2]) * val[0], (1 / val[2]) * val[1], 1 / val[2]])
    return (1.0 / val[0]) * uvn0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("lmrep")
    out = str(d / "landmark_rep_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "uvio_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "landmark_rep_check.cpp"), "-o", out])
    return out


def _convert(exe, pts, fej):
    """every representation on the given points (and first-estimate points), through the C++ header"""
    lines = []
    for rep in range(6):
        for p, q in zip(pts, fej):
            lines.append("%d %s" % (rep, " ".join("%.17g" % v for v in np.concatenate([p, q]))))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60)
    rows = np.array([[float(v) for v in ln.split()] for ln in out.stdout.strip().split("\n")])
    assert rows.shape == (6 * len(pts), 20)
    return rows.reshape(6, len(pts), 20)


@pytest.fixture(scope="module")
def table(exe):
    """the same 200 points (and nearby first-estimate points) for every representation"""
    rng = np.random.default_rng(11)
    pts = []
    while len(pts) < 200:
        p = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0.5, 12.0)])
        if np.hypot(p[0], p[1]) / p[2] > np.tan(0.05):
            pts.append(p)
    pts = np.array(pts)
    fej = pts + rng.uniform(-0.05, 0.05, pts.shape)
    return pts, fej, _convert(exe, pts, fej)


def test_round_trip_near_the_optical_axis(exe):
    """Points from 1e-6 to 0.05 rad off the z axis, and on it.  The representations without acos keep 1e-14.  The
    spherical ones recover phi = acos(c), c = rho z rounded to eps / 2 = 1.1e-16 relative: d phi <= 1.1e-16 /
    sin(phi), a transverse error of |p| d phi.  Near the axis acos(1 - eps/2 steps) resolves phi only to
    sqrt(eps) = 1.5e-8 rad, which caps the error: relative to |p| it is at most min(1.1e-16 / tan(phi), 1.5e-8),
    asserted with a factor 4 for the other roundings, plus the 1e-14 of the points off the axis."""
    rng = np.random.default_rng(12)
    phi = np.concatenate([[0.0], np.exp(rng.uniform(np.log(1e-6), np.log(0.05), 99))])
    th = rng.uniform(-np.pi, np.pi, phi.size)
    r = rng.uniform(0.5, 12.0, phi.size)
    pts = np.stack([r * np.sin(phi) * np.cos(th), r * np.sin(phi) * np.sin(th), r * np.cos(phi)], axis=1)
    rows = _convert(exe, pts, pts)
    for rep in range(6):
        for k, p in enumerate(pts):
            bound = TOL
            if rep in (1, 3):
                ph = np.arctan2(np.hypot(p[0], p[1]), p[2])
                bound += 4 * min(1.1e-16 / np.tan(ph), 1.5e-8) if ph > 0 else 4 * 1.5e-8
            assert _rel(rows[rep, k, 12:15], p) < bound, (rep, k, rows[rep, k, 12:15], p, bound)


@pytest.mark.parametrize("rep", range(6))
def test_round_trip_and_numpy_statement(table, rep):
    pts, fejp, rows = table
    size = 1 if rep == 5 else 3
    for k, (p, pf) in enumerate(zip(pts, fejp)):
        r = rows[rep, k]
        val, fej, uvn0, uvn0f, xyz, xyzf = (r[3 * i:3 * i + 3] for i in range(6))
        assert int(r[18]) == size and int(r[19]) == (1 if rep >= 2 else 0)
        # from_xyz -> xyz returns the point
        assert _rel(xyz, p) < TOL, (rep, k, xyz, p)
        # the numpy statement: stored value, bearing and both reads
        nv, nb = np_set_from_xyz(rep, p)
        nf, nbf = np_set_from_xyz(rep, pf)
        assert _rel(val[:size], nv) < TOL and _rel(fej[:size], nf) < TOL
        assert _rel(xyz, np_get_xyz(rep, nv, nf, nb, False)) < TOL
        assert _rel(xyzf, np_get_xyz(rep, nv, nf, nb, True)) < TOL
        if rep in (4, 5):  # the reference's quirk: the first estimate is never read
            assert np.array_equal(xyzf, xyz)
        else:
            assert _rel(xyzf, pf) < TOL and not np.array_equal(xyzf, xyz)


def test_single_inverse_depth_stores_rho_and_bearing(table):
    """rep 5 as oracle/src/state.cpp:61-69: the value is 1 / z alone, the bearing p / z lies beside it (the
    first estimate's in its own slot), and the two unused value slots stay untouched"""
    pts, fejp, rows = table
    for k, (p, pf) in enumerate(zip(pts, fejp)):
        r = rows[5, k]
        assert r[0] == 1.0 / p[2] and r[1] == 0.0 and r[2] == 0.0
        assert r[3] == 1.0 / pf[2] and r[4] == 0.0 and r[5] == 0.0
        assert np.array_equal(r[6:9], (1.0 / p[2]) * p)
        assert np.array_equal(r[9:12], (1.0 / pf[2]) * pf)
        assert abs(r[8] - 1.0) < 4e-16


def _config_with(tmp_path, key, name):
    src = os.path.join(ROOT, "configs", "euroc_mav")
    dst = tmp_path / ("cfg_%s_%s" % (key, name))
    shutil.copytree(src, dst)
    path = dst / "estimator_config.yaml"
    lines = []
    for ln in path.read_text().split("\n"):
        if ln.startswith(key + ":"):
            ln = '%s: "%s"' % (key, name)
        lines.append(ln)
    path.write_text("\n".join(lines))
    return str(path)


@pytest.mark.parametrize("key", ["feat_rep_msckf", "feat_rep_slam"])
def test_options_load_maps_the_six_names(tmp_path, key):
    import uvio_amd as U
    for rep, name in enumerate(NAMES):
        o = U.load_options(_config_with(tmp_path, key, name))
        assert getattr(o, key) == rep, (key, name)
    with pytest.raises(RuntimeError, match="E_CONFIG"):
        U.load_options(_config_with(tmp_path, key, "ANCHORED_4D"))
