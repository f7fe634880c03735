"""The MSCKF batch of the device (k_feature in mode 0, k_gemm_HPg / k_gemm_HPg_tiled, k_chi2<S> / k_chi2_S2, then the
direct or the Gram + information-form update) at the sizes at which it changes path, against the extended-precision
reference tests/feat_ref.py.  One msckf_update call per case on a generated state (tests/feat_setup.py): no stream, the
sizes are the ones feat_ref.CASES computes from the dispatch rules.

Every case asserts: the device's statuses are the designed ones and, with used / to_delete, the oracle's (which has
no status 2: it reports a failed refinement as 1); p_FinG within 1e-9 m of the oracle's; P+ exactly symmetric; the
suite's bounds against the oracle (chi2 1e-11 relative to max(chi2, 1), state and P 1e-10 in max norm); and, for the
chi2 of every feature, for P+ (ekf_ref.scaled_err) and for dx (ekf_ref.scaled_dx_err),
    e_dev <= RATIO * max(e_orc, FLOOR)
with the reference evaluated at the device's own p_FinG for e_dev and at the oracle's for e_orc, so neither a
triangulation difference nor an oracle error is charged to the device.  dx is the device's own, read with
debug_last_msckf_dx: the updated state, stored in double precision, cannot show it (the rounding of a stored focal
length of 458 px is 5.8e-10 of its prior deviation of 1e-5).  The oracle's msckf_update returns no dx; its e_orc is the
larger of its update arithmetic on the reference's stacked rows (feat_setup.oracle_dx) and of its own x+ taken
component by component beyond that storage rounding (feat_setup.x_err_floored), and the device's x+ is held to the
same bound in that metric.  An all-rejected batch leaves P and the state
bit-identical; a mixed batch equals the reference over the accepted rows only, which is what shows that the gate zeroed
the others.  A feature of which a float cast of the reference (at the device's p_FinG) lies within 1e-6 ulp of a
rounding midpoint may round either way: at most one per case, printed.

What the cases reach (feat_ref.dispatch_of; rows = the batch's stacked rows, n its state columns):
  k_chi2<1> up to 63 projected rows of the largest feature (33 measurements), k_chi2<2> from 65 (34)
      -- kernels_chi2.hip chi2_instance: smax = (R + 1 + 63) / 64
  S in k_chi2's LDS while chi2_lds_bytes(R, n) <= kMaxDynLds: at n = 120 up to R = 61 (32 measurements); k_chi2_S2
      forms it in global memory from R = 63 -- kernels_chi2.hip launch_chi2_batch
  k_gemm_HPg below 4096 stacked rows, k_gemm_HPg_tiled<false> from there -- launch_chi2_batch
  direct update for rows <= n (and <= 255), Gram + information form above -- engine_chain.cpp enqueue_update
  sequential batch build below 256 features, chunked from 256 when the host pool has more than one thread
      (UVIO_HP_THREADS, default min(16, hardware threads); the cases of 256 and 257 features assert it)
      -- engine_update.cpp add_features_to_batch
  (per case: features, largest feature's measurements, stacked rows, state columns, T GEMM, gate, where S is formed,
  update, batch build)
  mono-one2-fej1-rep0       feats   1 max  2 rows    1 n  12 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-one3-fej1-rep0       feats   1 max  3 rows    3 n  18 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-rows=n-fej1-rep0     feats   4 max  6 rows   36 n  36 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-rows=n+1-fej1-rep0   feats   5 max  6 rows   37 n  36 k_gemm_HPg       k_chi2<1> LDS       information sequential
  mono-rejected-fej1-rep0   feats   2 max  6 rows   14 n  36 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-mixed-fej1-rep0      feats   6 max  6 rows   38 n  36 k_gemm_HPg       k_chi2<1> LDS       information sequential
  mono-one2-fej0-rep4       feats   1 max  2 rows    1 n  12 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-one3-fej0-rep4       feats   1 max  3 rows    3 n  18 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-rows=n-fej0-rep4     feats   4 max  6 rows   36 n  36 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-rows=n+1-fej0-rep4   feats   5 max  6 rows   37 n  36 k_gemm_HPg       k_chi2<1> LDS       information sequential
  mono-rejected-fej0-rep4   feats   2 max  6 rows   14 n  36 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  mono-mixed-fej0-rep4      feats   6 max  6 rows   38 n  36 k_gemm_HPg       k_chi2<1> LDS       information sequential
  stereo-one9-fej1-rep0     feats   1 max  9 rows   15 n  82 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-one10-fej1-rep0    feats   1 max 10 rows   17 n  88 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-sizes-fej1-rep0    feats   5 max 22 rows   77 n  94 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-mixed-fej1-rep0    feats   7 max 22 rows  101 n  94 k_gemm_HPg       k_chi2<1> LDS       information sequential
  stereo-one9-fej0-rep0     feats   1 max  9 rows   15 n  82 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-one10-fej0-rep0    feats   1 max 10 rows   17 n  88 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-sizes-fej0-rep0    feats   5 max 22 rows   77 n  94 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-mixed-fej0-rep0    feats   7 max 22 rows  101 n  94 k_gemm_HPg       k_chi2<1> LDS       information sequential
  stereo-one9-fej1-rep4     feats   1 max  9 rows   15 n  82 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-one10-fej1-rep4    feats   1 max 10 rows   17 n  88 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-sizes-fej1-rep4    feats   5 max 22 rows   77 n  94 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-mixed-fej1-rep4    feats   7 max 22 rows  101 n  94 k_gemm_HPg       k_chi2<1> LDS       information sequential
  stereo-rejected-fej1-rep0 feats   3 max 11 rows   29 n  94 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  stereo-n255-fej1-rep0     feats 255 max  4 rows  765 n  58 k_gemm_HPg       k_chi2<1> LDS       information sequential
  stereo-n256-fej1-rep0     feats 256 max  4 rows  766 n  58 k_gemm_HPg       k_chi2<1> LDS       information chunked
  stereo-n257-fej1-rep0     feats 257 max  4 rows  769 n  58 k_gemm_HPg       k_chi2<1> LDS       information chunked
  quad-one32-fej1-rep0      feats   1 max 32 rows   61 n 120 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  quad-one33-fej1-rep0      feats   1 max 33 rows   63 n 120 k_gemm_HPg       k_chi2<1> k_chi2_S2 direct      sequential
  quad-one34-fej1-rep0      feats   1 max 34 rows   65 n 120 k_gemm_HPg       k_chi2<2> k_chi2_S2 direct      sequential
  quad-one64-fej1-rep0      feats   1 max 64 rows  125 n 120 k_gemm_HPg       k_chi2<2> k_chi2_S2 information sequential
  quad-one64-fej1-rep4      feats   1 max 64 rows  125 n 120 k_gemm_HPg       k_chi2<2> k_chi2_S2 information sequential
  quad-one32-fej0-rep4      feats   1 max 32 rows   61 n 120 k_gemm_HPg       k_chi2<1> LDS       direct      sequential
  quad-rows4095-fej1-rep0   feats  33 max 64 rows 4095 n 120 k_gemm_HPg       k_chi2<2> k_chi2_S2 information sequential
  quad-rows4125-fej1-rep0   feats  33 max 64 rows 4125 n 120 k_gemm_HPg_tiled k_chi2<2> k_chi2_S2 information sequential
  quad-mixed-fej1-rep0      feats   6 max 64 rows  296 n 120 k_gemm_HPg       k_chi2<2> k_chi2_S2 information sequential
Not reachable from msckf_update and so not here: k_chi2<3> and k_chi2<4> (a feature has at most 125 rows), k_chi2_S
(k_chi2_S2 serves up to 128 rows), k_gemm_HPg_tiled<true> (the engine always passes the gather buffer).

RATIO = 16: 4 x the worst measured ratio, rounded up to a power of two.  Measured on MI355X over the cases:
    chi2  1.49  stereo-mixed-fej1-rep4   (device 5.3e-15, oracle 9.7e-16 of max(chi2, 1))
    P+    2.16  stereo-mixed-fej1-rep4   (device 1.2e-14, oracle 5.3e-15)
    dx    1.70  stereo-n256-fej1-rep0    (device 2.3e-14, oracle 1.4e-14)
The device forms the left nullspace with three Householder reflections where the oracle uses Givens rotations, and
multiplies by explicit inverses of the factors' diagonal blocks where the oracle solves: a small constant over the
oracle in some cases, below it in most (of the 34 cases with an update, ratio under 1 in 33 for P+ and in 31 for dx).
Largest device errors: chi2 5.3e-15; P+ 3.4e-14 (quad-rows4095, 4095 stacked rows; the oracle, which compresses that
stack with Givens rotations, 4.8e-13); dx 3.5e-14 (quad-rows4125; oracle 5.3e-14); x+ beyond its storage rounding
2.6e-14.  In max norm against the oracle: p_FinG 5.3e-13 m, chi2 6.3e-15, P 1.8e-12, x 1.5e-16 at most.

One device manager and one oracle are alive at a time: a (setup, do_fej, representation) needs its own options, so the
pair of the previous one is closed when the next is made (the cases are grouped by it).

Capacity: 65 measurements in one feature, a batch whose k_feature LDS need (feature_lds_bytes of the batch's largest
measurement count and widest Jacobian, taken separately) exceeds its grant, each E_CAPACITY with covariance and state
untouched and the handle usable afterwards.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as R  # noqa: E402
import feat_ref as F  # noqa: E402
from test_gpu_ekf_paths import FLOOR  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_EXTENDED, reason=R.REASON)]

RATIO = 16.0
MIDPOINT = 1e-6
_cache = {}


def _close_pairs():
    for _, g, o, _ in _cache.values():
        g.close()
        o.close()
    _cache.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_managers():
    yield
    _close_pairs()


def _pool_threads():
    """the host pool's size as pool.h takes it"""
    e = os.environ.get("UVIO_HP_THREADS")
    return max(1, int(e)) if e else min(16, os.cpu_count() or 1)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def pair_of(key):
    """(options, device manager, oracle manager, generated state) of a (setup, fej, rep)"""
    if key not in _cache:
        _close_pairs()
        import feat_setup as S
        import uvio_amd as U
        from oracle import oracle as O
        opts = S.options(*key)
        g, o = U.VioManager(opts), O.OracleManager(opts)
        times = S.to_clones([g, o], opts, key[0])
        xg, mg = g.get_state_vector()
        xo, mo = o.get_state_vector()
        assert np.array_equal(mg, mo)
        _cache[key] = (opts, g, o, S.generated_state(o, opts, times))
    return _cache[key]


def run_both(key, c):
    """the case on the device and on the oracle, each from the generated snapshot"""
    import feat_setup as S
    opts, g, o, st = pair_of(key)
    feats = F.make_case(st, c, S.undistort_of(opts), opts)
    meas = F.as_measurements(st, feats)
    S.adopt(g, st)
    S.adopt(o, st)
    rg, ro = g.msckf_update(meas), o.msckf_update(meas)
    return opts, g, o, st, feats, rg, ro


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_msckf_case(c):
    import feat_setup as S
    opts, g, o, st, feats, rg, ro = run_both((c["setup"], c["fej"], c["rep"]), c)
    want = [F.STATUS[f.kind] for f in feats]
    assert len(feats) < F.K_CHUNKED_BUILD or _pool_threads() > 1, "the chunked batch build needs a host pool"
    ids_o, pG_o, st_o, c2_o = o.debug_last_msckf()
    by = {int(i): k for k, i in enumerate(ids_o)}  # (the oracle's list grows over its calls: the last entry of an id)
    assert [r["status"] for r in rg] == want
    assert [int(st_o[by[f.fid]]) for f in feats] == [1 if w == 2 else w for w in want]
    assert [(r["used"], r["to_delete"]) for r in rg] == [(r["used"], r["to_delete"]) for r in ro]
    Pg, xg = g.get_cov(), g.get_state_vector()[0]
    Po, xo = o.get_cov(), o.get_state_vector()[0]
    assert np.array_equal(Pg, Pg.T)
    if not any(w == 0 for w in want):
        assert "rejected" in c["id"] and all(r["status"] != 0 for r in rg)
        assert np.array_equal(Pg, st.P) and np.array_equal(xg, st.val)
        return
    # the suite's bounds against the oracle
    dp = max([float(np.max(np.abs(r["p_FinG"] - pG_o[by[f.fid]]))) for r, f, w in zip(rg, feats, want) if w in (0, 3)])
    dc = max([abs(r["chi2"] - c2_o[by[f.fid]]) / max(abs(c2_o[by[f.fid]]), 1.0) for r, f, w in zip(rg, feats, want)
              if w in (0, 3)])
    mP, mx = _rel(Pg, Po), _rel(xg, xo)
    assert dp < 1e-9 and dc < 1e-11 and mP < 1e-10 and mx < 1e-10, (dp, dc, mP, mx)
    # against the reference, each at its own landmark positions
    s2 = opts.msckf_sigma_pix ** 2
    p_o, acc = S.positions(st, feats, ids_o, pG_o, st_o)
    p_g = [None if r["status"] in (1, 2) else np.array(r["p_FinG"]) for r in rg]
    ref_o = F.evaluate(st, feats, p_o, acc, c["rep"], bool(c["fej"]), s2)
    same = all((a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))
               for a, b in zip(p_g, p_o))
    ref_g = ref_o if same else F.evaluate(st, feats, p_g, acc, c["rep"], bool(c["fej"]), s2)
    near = [feats[j].fid for j, d in ref_g.casts.items() if d < MIDPOINT]
    if near:
        print("MSCKFPATH %s: a float cast within %g ulp of a midpoint in features %s" % (c["id"], MIDPOINT, near))
    assert len(near) <= 1
    worst_c = (0.0, 0.0, 0.0)
    for j in ref_g.chi2:
        if feats[j].fid in near:
            continue
        cg, cr = rg[j]["chi2"], float(ref_g.chi2[j])
        co, cro = c2_o[by[feats[j].fid]], float(ref_o.chi2[j])
        e_dev = float(abs(R.LD(cg) - ref_g.chi2[j]) / max(cr, 1.0))
        e_orc = float(abs(R.LD(co) - ref_o.chi2[j]) / max(cro, 1.0))
        worst_c = max(worst_c, (e_dev / max(e_orc, FLOOR), e_dev, e_orc))
        assert e_dev <= RATIO * max(e_orc, FLOOR), (feats[j].fid, cg, cr, e_dev, e_orc)
    eP, eP_o = R.scaled_err(Pg, ref_g.P_plus, st.P), R.scaled_err(Po, ref_o.P_plus, st.P)
    # dx: the device's own (debug_last_msckf_dx).  The oracle's msckf_update returns none: its yardstick is the larger
    # of its update arithmetic on the reference's rows (feat_setup.oracle_dx) and of its own x+, component by
    # component beyond what storing x+ in double precision costs (feat_setup.x_err_floored)
    dxg = g.debug_last_msckf_dx()
    assert dxg.shape == (st.N,)
    ed = R.scaled_dx_err(dxg, ref_g.dx, st.P)
    ed_o, ex_o = R.scaled_dx_err(S.oracle_dx(st, ref_o, s2), ref_o.dx, st.P), S.x_err_floored(xo, ref_o.x_plus, st)
    ex = S.x_err_floored(xg, ref_g.x_plus, st)  # the state moved by that dx
    print("MSCKFPATH %s chi2 dev %.2e orc %.2e ratio %.2f | P+ dev %.2e orc %.2e ratio %.2f | dx dev %.2e orc %.2e "
          "(x+ %.2e) ratio %.2f | x+ dev %.2e | maxnorm p %.1e chi2 %.1e P %.1e x %.1e same_p %d" %
          (c["id"], worst_c[1], worst_c[2], worst_c[0], eP, eP_o, eP / max(eP_o, FLOOR), ed, ed_o, ex_o,
           ed / max(ed_o, ex_o, FLOOR), ex, dp, dc, mP, mx, same))
    if near:
        return  # (that feature's rows may differ by a float ulp of a pixel: the update is compared by the bounds above)
    assert eP <= RATIO * max(eP_o, FLOOR), (eP, eP_o)
    assert ed <= RATIO * max(ed_o, ex_o, FLOOR), (ed, ed_o, ex_o)
    assert ex <= RATIO * max(ed_o, ex_o, FLOOR), (ex, ed_o, ex_o)


def test_global_3d_against_full_inverse_depth():
    """GLOBAL_3D and GLOBAL_FULL_INVERSE_DEPTH (rep 1) differ in H_f by an invertible 3 x 3 factor: the same left
    nullspace, so chi2, P+ and x+ agree.  No reference here: the device's two results against each other, with the
    oracle's two results against each other as the yardstick."""
    import feat_setup as S
    c = F.REP01_CASE
    out = {}
    for rep in (0, 1):
        opts, g, o, st, feats, rg, ro = run_both((c["setup"], c["fej"], rep), c)
        assert [r["status"] for r in rg] == [0] * len(feats)
        ids, _, _, c2 = o.debug_last_msckf()
        last = {int(i): float(v) for i, v in zip(ids, c2)}
        out[rep] = (st, rg, g.get_cov(), g.debug_last_msckf_dx(), o.get_cov(), o.get_state_vector()[0],
                    np.array([last[f.fid] for f in feats]))
    st, rg0, Pg0, dg0, Po0, xo0, co0 = out[0]
    _, rg1, Pg1, dg1, Po1, xo1, co1 = out[1]
    assert np.array_equal(st.P, out[1][0].P) and np.array_equal(st.val, out[1][0].val)
    ec = max(abs(a["chi2"] - b["chi2"]) / max(a["chi2"], 1.0) for a, b in zip(rg0, rg1))
    ec_o = float(np.max(np.abs(co0 - co1) / np.maximum(co0, 1.0)))
    eP, eP_o = R.scaled_err(Pg0, Pg1, st.P), R.scaled_err(Po0, Po1, st.P)
    # the device's two dx against each other; the oracle has only its two x+, beyond their storage rounding
    ex, ex_o = R.scaled_dx_err(dg0, dg1, st.P), S.x_err_floored(xo0, xo1, st)
    print("MSCKFPATH rep0-rep1 chi2 dev %.2e orc %.2e | P+ dev %.2e orc %.2e | dx dev %.2e, x+ orc %.2e" %
          (ec, ec_o, eP, eP_o, ex, ex_o))
    assert ec <= RATIO * max(ec_o, FLOOR) and eP <= RATIO * max(eP_o, FLOOR) and ex <= RATIO * max(ex_o, FLOOR)


# ---- capacity ----
def _synthetic(fid, vw, times):
    """a feature over the (clone, camera) pairs vw with made-up pixels: a refusal comes before anything reads them"""
    return (fid, [(c, times[i], 300.0 + 2.0 * k, 200.0 + 1.0 * k, 0.01 * (k % 7), -0.01 * (k % 5))
                  for k, (i, c) in enumerate(vw)])


def _capacity_manager(setup, clones, **more):
    """a device manager of the setup's cameras with `clones` clones 0.1 s apart, on a generated state"""
    import feat_setup as S
    import uvio_amd as U
    opts = S.options(setup, 1, 0, max_clone_size=clones, **more)
    g = U.VioManager(opts)
    times = S.to_clones([g], opts, [0.1 * (k + 1) for k in range(clones)])
    st = S.generated_state(g, opts, times)
    S.adopt(g, st)
    return opts, g, st, times


def _refused_then_usable(opts, g, st, batch, match):
    import feat_setup as S
    with pytest.raises(RuntimeError, match=match):
        g.msckf_update(batch)
    assert np.array_equal(g.get_cov(), st.P) and np.array_equal(g.get_state_vector()[0], st.val)
    assert np.array_equal(g.get_fej_vector(), st.fej)
    K = len(st.clone_times)
    ok = F._ok_views(st, 6, np.random.default_rng(9), S.undistort_of(opts), 7, opts.msckf_sigma_pix ** 2, 0, True,
                     vw=[(K - 6 + k, 0) for k in range(6)])
    r = g.msckf_update(F.as_measurements(st, [ok]))
    assert r[0]["status"] == 0
    P = g.get_cov()
    assert np.array_equal(P, P.T) and not np.array_equal(P, st.P)


def test_capacity_measurements_and_feature_lds():
    """four cameras, extrinsics calibrated, 30 clones"""
    opts, g, st, times = _capacity_manager("quad", 30)
    cap = F.K_MAX_MEAS_PER_FEAT
    # 65 measurements in one feature (17 clones x 4 cameras, one dropped ... 65 kept)
    vw = [(i, c) for i in range(17) for c in range(4)][:cap + 1]
    _refused_then_usable(opts, g, st, [_synthetic(1, vw, times)], "E_CAPACITY")
    # 64 measurements over few columns (16 clones x 4 cameras: 96 + 24) beside a wide feature (25 clones of camera 0:
    # 150 + 6 columns).  Each fits k_feature's LDS alone; the launch is sized by the batch's largest measurement
    # count and its widest Jacobian taken separately
    few = [(i, c) for i in range(16) for c in range(4)]
    wide = [(i, 0) for i in range(25)]
    nf_few, nf_wide = 6 * 16 + 6 * 4, 6 * 25 + 6
    assert len(few) == cap
    assert F.feature_lds_bytes(len(few), nf_few) <= F.K_FEATURE_LDS
    assert F.feature_lds_bytes(len(wide), nf_wide) <= F.K_FEATURE_LDS
    assert F.feature_lds_bytes(len(few), nf_wide) > F.K_FEATURE_LDS
    st.P, st.val = g.get_cov(), g.get_state_vector()[0]  # (the state after the valid update above)
    _refused_then_usable(opts, g, st, [_synthetic(1, few, times), _synthetic(2, wide, times)], "E_CAPACITY.*LDS")
    g.close()


def test_capacity_wide_feature_on_a_calibrated_stereo_state():
    """a 60-measurement feature on a 30-clone stereo state with extrinsic and intrinsic calibration: 180 + 28 Jacobian
    columns, about 200 KB of k_feature's LDS.  An ordinary caller-built input: E_CAPACITY, not E_INTERNAL (which
    would stop the handle)."""
    opts, g, st, times = _capacity_manager("stereo", 30)
    vw = [(i, c) for i in range(30) for c in range(2)]
    assert F.feature_lds_bytes(len(vw), 6 * 30 + 14 * 2) > F.K_FEATURE_LDS
    _refused_then_usable(opts, g, st, [_synthetic(1, vw, times)], "E_CAPACITY.*LDS")
    g.close()
