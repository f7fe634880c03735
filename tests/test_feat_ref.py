"""tests/feat_ref.py (the extended-precision restatement of the MSCKF feature batch and its case generator) against
the oracle, on the CPU.

  * Jacobians: res, H_f and H_x of the reference against probe_feature_jacobian on every setup, with and without FEJ,
    GLOBAL_3D and ANCHORED_MSCKF_INVERSE_DEPTH.  res is bit-equal (every float cast of the reference is further than
    1e-6 ulp from a rounding midpoint, which is asserted); H within JAC_TOL of the extended value.
  * every case of feat_ref.CASES: the oracle's msckf_update gives the designed statuses (the oracle reports a failed
    refinement as 1, like a failed triangulation; that the status-2 features fail in the refinement and not before
    is shown with probe_triangulate); chi2 sits a factor 2 on the designed side of its threshold, the linear
    triangulation's condition number, depth and baseline ratio a factor 2 inside (or, for the rejected features,
    outside) theirs; the oracle's P+ and dx agree with the reference evaluated at the oracle's own landmark
    positions, in the metrics that see small-variance blocks, within RATIO x what the reference's own float64 run
    loses (the second yardstick); no accepted batch moves a state component by more than 0.1.  The oracle's
    msckf_update returns no dx: dx is its update (compression, EKFUpdate) of the reference's stacked rows
    (feat_setup.oracle_dx), and its own x+ is held component by component beyond what storing x+ in double precision
    costs (feat_setup.x_err_floored; one maximum over all components would make the rounding of a stored 458 px
    focal length, 5.8e-10 of its prior deviation, the yardstick of every component).
  * injected errors: the reference with the clone position block's sign flipped, or linearized at the other of the
    two estimates, fails that comparison by orders of magnitude.

JAC_TOL = 1e-13 of the largest entry: about 50 operations per entry in double precision, 50 x 2^-53 = 6e-15, and a
factor 16 for the cancellation in the (x, y) / z^2 terms.  Measured: 9e-16 at most, the float64 run of the reference
the same.
RATIO = 1024: the oracle compresses a tall stack with Givens rotations (m - n rotations per column, errors growing
with the row count) before a plain update, the float64 yardstick updates directly.  Measured here, worst over
the cases: P+ 134 (quad-rows4095: oracle 4.8e-13, float64 1.8e-15), next 14 (quad-rows4125); dx 1.8
(stereo-mixed-fej1-rep4), largest oracle dx error 5.3e-14 (quad-rows4125; float64 5.8e-14); x+ beyond its storage
rounding 2.7e-14 at most.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as R  # noqa: E402
import feat_ref as F  # noqa: E402

pytestmark = pytest.mark.skipif(not R.HAVE_EXTENDED, reason=R.REASON)

JAC_TOL = 1e-13
RATIO = 1024.0
FLOOR = 16 * 2.0 ** -52
MIDPOINT = 1e-6
_cache = {}


def setup_of(key):
    """(options, oracle manager at K clones, generated state) of a (setup, fej, rep)"""
    if key not in _cache:
        import feat_setup as S
        from oracle import oracle as O
        opts = S.options(*key)
        o = O.OracleManager(opts)
        times = S.to_clones([o], opts, key[0])
        _cache[key] = (opts, o, S.generated_state(o, opts, times))
    return _cache[key]


def test_chi2_quantiles():
    from oracle import oracle as O
    for dof in list(range(1, 130)) + [499]:
        assert abs(F.chi2_95(dof) - O.chi2_quantile95(dof)) < 1e-9 * O.chi2_quantile95(dof), dof


def test_dispatch_coverage():
    """the case list reaches every path the issue names, by the restated rules"""
    d = [F.dispatch_of(c) for c in F.CASES]
    for key, want in (("chi2", {"k_chi2<1>", "k_chi2<2>"}), ("S", {"LDS", "k_chi2_S2"}),
                      ("gemm", {"k_gemm_HPg", "k_gemm_HPg_tiled"}), ("update", {"direct", "information"}),
                      ("build", {"sequential", "chunked"})):
        assert set(x[key] for x in d) == want, key
    rows = sorted(set(F.rows_of(m) for c in F.CASES for _, m in c["feats"]))
    assert {1, 3, 15, 17, 61, 63, 65, 125} <= set(rows)
    assert any(x["rows"] == x["n"] for x in d) and any(x["rows"] == x["n"] + 1 for x in d)
    assert any(x["rows"] == F.K_TILED_ROWS - 1 for x in d)
    assert sorted(set(len(c["feats"]) for c in F.CASES) & {255, 256, 257}) == [255, 256, 257]


JAC_KEYS = sorted(set((c["setup"], c["fej"]) for c in F.CASES))


@pytest.mark.parametrize("rep", [0, 4])
@pytest.mark.parametrize("setup,fej", JAC_KEYS)
def test_jacobian_matches_probe(setup, fej, rep):
    import feat_setup as S
    opts, o, st = setup_of((setup, fej, next(c["rep"] for c in F.CASES if (c["setup"], c["fej"]) == (setup, fej))))
    S.adopt(o, st)
    K, C = len(st.clone_times), len(st.cams)
    rng = np.random.default_rng(5 + rep)
    f = F._ok_views(st, min(K * C, 12), rng, S.undistort_of(opts), 1, 1.0, rep, bool(fej))
    t = F.triangulate_linear(st, f, np.float64)
    ac, ai = t.anchor
    order = F.reference_rows(f)
    if rep == 0:
        lam, kw = np.array(t.p_FinG), {}
    else:
        pA = np.array(t.p_FinA)
        lam = np.array([pA[0] / pA[2], pA[1] / pA[2], 1 / pA[2]])
        kw = dict(anchor_cam=ac, anchor_time=st.clone_times[ai])
    res, Hf, Hx, blocks = o.probe_feature_jacobian(rep, f.cam, [st.clone_times[i] for i in f.clone], f.uv, f.uvn, lam,
                                                   **kw)
    cols = np.concatenate([np.arange(c, c + s) for c, s in blocks])
    rows = np.concatenate([[2 * j, 2 * j + 1] for j in order])

    def run(dt, inject=None):
        if rep == 0:
            return F.feature_jacobian(st, f, 0, bool(fej), p_FinG=lam, dt=dt, inject=inject)
        pA = np.array([lam[0] / lam[2], lam[1] / lam[2], 1 / lam[2]])  # Landmark::get_xyz, in double like the probe
        return F.feature_jacobian(st, f, 4, bool(fej), p_FinA=pA, anchor=(ac, ai), dt=dt, inject=inject)

    def miss(lin):
        assert sorted(lin.cols) == sorted(cols)
        at = {int(c): k for k, c in enumerate(lin.cols)}
        H = lin.H_x[rows][:, [at[int(c)] for c in cols]]
        return (float(np.max(np.abs(H - Hx)) / np.max(np.abs(H))),
                float(np.max(np.abs(lin.H_f[rows] - Hf)) / np.max(np.abs(lin.H_f))))

    ld, f64 = run(R.LD), run(np.float64)
    assert ld.casts.dist >= MIDPOINT, ld.casts.dist
    assert np.array_equal(ld.res[rows].astype(np.float64), res)
    ex, ef = miss(ld)
    print("JAC %s fej%d rep%d: H_x %.2e H_f %.2e (float64 run %.2e %.2e) cast distance %.2e" %
          ((setup, fej, rep, ex, ef) + miss(f64) + (ld.casts.dist,)))
    assert ex <= JAC_TOL and ef <= JAC_TOL
    # the same comparison must fail for a wrong Jacobian
    bad = miss(run(R.LD, "clone_pos_sign"))
    assert bad[0] > 1e-2, bad
    if fej:
        bad = miss(run(R.LD, "swap_fej"))
        assert bad[0] > 1e3 * JAC_TOL and bad[1] > 1e3 * JAC_TOL, bad


def run_case(c):
    """the oracle's msckf_update on the case and the reference at the oracle's landmark positions"""
    import feat_setup as S
    opts, o, st = setup_of((c["setup"], c["fej"], c["rep"]))
    feats = F.make_case(st, c, S.undistort_of(opts), opts)
    S.adopt(o, st)
    out = o.msckf_update(F.as_measurements(st, feats))
    ids, pG, status, chi2 = o.debug_last_msckf()
    return opts, o, st, feats, out, ids, pG, status, chi2


@pytest.mark.parametrize("c", F.CASES, ids=F.case_id)
def test_case_against_oracle(c):
    import feat_setup as S
    from oracle import oracle as O
    opts, o, st, feats, out, ids, pG, status, chi2 = run_case(c)
    by = {int(i): k for k, i in enumerate(ids)}
    want = [F.STATUS[f.kind] for f in feats]
    got = [int(status[by[f.fid]]) for f in feats]
    assert got == [1 if w == 2 else w for w in want], (want, got)  # (the oracle has no status 2)
    assert [r["used"] for r in out] == [w == 0 for w in want] and all(r["to_delete"] for r in out)
    assert any(w == 0 for w in want) or "rejected" in c["id"]
    # the triangulation's margins
    for f, w in zip(feats, want):
        t = F.triangulate_linear(st, f)
        if w == 1:
            assert t.cond >= 2 * opts.fi_max_cond_number, t.cond
            continue
        assert t.cond <= opts.fi_max_cond_number / 2 and 2 * opts.fi_min_dist <= t.depth <= opts.fi_max_dist / 2, t
        ts = [st.clone_times[i] for i in f.clone]
        if w == 2:  # passes the linear stage, fails the refinement with a depth beyond twice fi_max_dist
            assert o.probe_triangulate(f.cam, ts, f.uv, f.uvn, refine=False)[0]
            ok, _, pA, _, _ = o.probe_triangulate(f.cam, ts, f.uv, f.uvn, refine=True)
            assert not ok and pA[2] >= 2 * opts.fi_max_dist, (ok, pA)
        else:
            assert t.ratio <= opts.fi_max_baseline / 2, t.ratio
            ok, _, pA, _, _ = o.probe_triangulate(f.cam, ts, f.uv, f.uvn, refine=True)
            assert ok and 2 * opts.fi_min_dist <= pA[2] <= opts.fi_max_dist / 2, pA
    # the gate's margins
    for f, w in zip(feats, want):
        if w in (0, 3):
            k = by[f.fid]
            thr = opts.msckf_chi2_multipler * O.chi2_quantile95(F.rows_of(len(f.cam)))
            assert (chi2[k] <= thr / 2) if w == 0 else (chi2[k] >= 2 * thr), (f.fid, w, chi2[k], thr)
    s2 = opts.msckf_sigma_pix ** 2
    p, acc = S.positions(st, feats, ids, pG, status)
    ld = F.evaluate(st, feats, p, acc, c["rep"], bool(c["fej"]), s2)
    assert min(ld.casts.values(), default=1.0) >= MIDPOINT, ld.casts
    for j in ld.chi2:
        k = by[feats[j].fid]
        assert abs(float(ld.chi2[j]) - chi2[k]) <= 1e-11 * max(abs(chi2[k]), 1.0), (j, float(ld.chi2[j]), chi2[k])
    Po, xo = o.get_cov(), o.get_state_vector()[0]
    if not acc:
        assert np.array_equal(Po, st.P) and np.array_equal(xo, st.val)
        return
    d = F.evaluate(st, feats, p, acc, c["rep"], bool(c["fej"]), s2, dt=np.float64)
    assert float(np.max(np.abs(ld.dx))) <= 0.1
    eP, eP64 = R.scaled_err(Po, ld.P_plus, st.P), R.scaled_err(d.P_plus, ld.P_plus, st.P)
    ed, ed64 = R.scaled_dx_err(S.oracle_dx(st, ld, s2), ld.dx, st.P), R.scaled_dx_err(d.dx, ld.dx, st.P)
    ex, ex64 = S.x_err_floored(xo, ld.x_plus, st), S.x_err_floored(d.x_plus, ld.x_plus, st)
    print("FEATREF %s P+ oracle %.2e float64 %.2e ratio %.1f  dx oracle %.2e float64 %.2e ratio %.1f  x+ oracle %.2e "
          "float64 %.2e  max|dx| %.1e" %
          (c["id"], eP, eP64, eP / max(eP64, FLOOR), ed, ed64, ed / max(ed64, FLOOR), ex, ex64,
           float(np.max(np.abs(ld.dx)))))
    assert eP <= RATIO * max(eP64, FLOOR), (eP, eP64)
    assert ed <= RATIO * max(ed64, FLOOR), (ed, ed64)
    # the oracle's own x+ (its msckf_update returns no dx), component by component beyond its storage rounding
    assert ex <= RATIO * max(ed64, ex64, FLOOR), (ex, ex64, ed64)


@pytest.mark.parametrize("cid,inject", [("mono-mixed-fej1-rep0", "clone_pos_sign"),
                                        ("mono-mixed-fej1-rep0", "swap_fej"),
                                        ("stereo-sizes-fej1-rep4", "clone_pos_sign"),
                                        ("stereo-sizes-fej1-rep4", "swap_fej")])
def test_injected_error_fails_the_comparison(cid, inject):
    """a test that cannot fail is of no use: the wrong reference misses the oracle by far more than the bound"""
    import feat_setup as S
    c = next(x for x in F.CASES if x["id"] == cid)
    opts, o, st, feats, out, ids, pG, status, chi2 = run_case(c)
    s2 = opts.msckf_sigma_pix ** 2
    p, acc = S.positions(st, feats, ids, pG, status)
    ld = F.evaluate(st, feats, p, acc, c["rep"], bool(c["fej"]), s2)
    d = F.evaluate(st, feats, p, acc, c["rep"], bool(c["fej"]), s2, dt=np.float64)
    bad = F.evaluate(st, feats, p, acc, c["rep"], bool(c["fej"]), s2, inject=inject)
    Po, xo = o.get_cov(), o.get_state_vector()[0]
    bound_P = RATIO * max(R.scaled_err(d.P_plus, ld.P_plus, st.P), FLOOR)
    bound_x = RATIO * max(R.scaled_dx_err(d.dx, ld.dx, st.P), S.x_err_floored(d.x_plus, ld.x_plus, st), FLOOR)
    eP, ex = R.scaled_err(Po, bad.P_plus, st.P), S.x_err_floored(xo, bad.x_plus, st)
    print("INJECT %s %s: P+ %.2e (bound %.2e) x+ %.2e (bound %.2e)" % (cid, inject, eP, bound_P, ex, bound_x))
    assert eP > 1e3 * bound_P and ex > 1e3 * bound_x
    k = next(j for j in bad.chi2 if j in acc)
    kk = {int(i): n for n, i in enumerate(ids)}[feats[k].fid]
    assert abs(float(bad.chi2[k]) - chi2[kk]) > 1e-6 * max(abs(chi2[kk]), 1.0)
