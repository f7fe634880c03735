// IMU-rate odometry: Propagator::fast_state_propagate (Propagator.cpp:140-267) on plain arrays.  Host-only, no
// Engine members: the cache (state time, IMU value, 15 x 15 IMU marginal, time offset, IMU intrinsics), one
// interval's step (corrected mean measurements, F, G, Qd, F P F^T + Qd, the mean) and the output stage.  The
// engine owns a Cache and decides when it is replaced from the filter state (engine_odom.cpp); a stand-alone
// program can compile this header with imu_math.h alone (tests/cpp/fast_prop_check.cpp).
//
// Error-state order of the 15 x 15 (IMU.h): theta (0), p (3), v (6), b_g (9), b_a (12).
#pragma once
#include <cstring>
#include <vector>

#include "imu_math.h"

namespace uvhp {
namespace fastprop {

// the IMU intrinsic matrices the reference forms on every call (Propagator.cpp:167-172)
struct Calib {
  double Dw[9], Da[9], Tg[9], R_acc[9], R_gyro[9];
};
inline void make_calib(int imu_model, const double *dw, const double *da, const double *tg, const double *q_acc,
                       const double *q_gyro, Calib *c) {
  Dm(imu_model, dw, c->Dw);
  Dm(imu_model, da, c->Da);
  TgM(tg, c->Tg);
  quat_2_Rot(q_acc, c->R_acc);
  quat_2_Rot(q_gyro, c->R_gyro);
}

// NoiseManager's squared sigmas (Propagator.h:44) and the gravity magnitude
struct Noise {
  double sigma_w_2, sigma_a_2, sigma_wb_2, sigma_ab_2, gravity_mag;
};

// cache_state_time / cache_state_est / cache_state_covariance / cache_t_off (Propagator.h:449-453)
struct Cache {
  double t = 0;
  double est[16] = {0};   // q_GtoI (4) p (3) v (3) b_g (3) b_a (3)
  double cov[225] = {0};  // row-major 15 x 15
  double t_off = 0;
  Calib calib{};
};

// a_hat = R_ACCtoIMU Da (am - b_a), w_hat = R_GYROtoIMU Dw (wm - b_g - Tg a_hat)  (Propagator.cpp:184-190)
inline void corrected(const Cache &c, const ImuSample &s, double *a_hat, double *w_hat) {
  const double *bg = c.est + 10, *ba = c.est + 13;
  double RaDa[9], RwDw[9], d[3], Ta[3];
  m3_mul(c.calib.R_acc, c.calib.Da, RaDa);
  for (int k = 0; k < 3; k++) d[k] = s.am[k] - ba[k];
  m3_vec(RaDa, d, a_hat);
  m3_vec(c.calib.Tg, a_hat, Ta);
  m3_mul(c.calib.R_gyro, c.calib.Dw, RwDw);
  for (int k = 0; k < 3; k++) d[k] = s.wm[k] - bg[k] - Ta[k];
  m3_vec(RwDw, d, w_hat);
}

// One interval's F (15 x 15) and Qd (15 x 15) at the cache's current estimate (Propagator.cpp:193-230), from the
// averaged corrected measurements.  Outputs row-major.
inline void interval_F_Qd(const Cache &c, const Noise &n, const double *a_hat, const double *w_hat, double dt, double *F,
                          double *Qd) {
  double R[9], Rexp[9], J[9], RJ[9], mw[3], pw[3];
  quat_2_Rot(c.est, R);
  for (int k = 0; k < 3; k++) mw[k] = -w_hat[k] * dt, pw[k] = w_hat[k] * dt;
  exp_so3(mw, Rexp);
  Jl_so3(pw, J);  // Jr_so3(-w dt) = Jl_so3(w dt)
  m3_mul(Rexp, J, RJ);
  double adt[3] = {a_hat[0] * dt, a_hat[1] * dt, a_hat[2] * dt}, adt2[3] = {a_hat[0] * dt * dt, a_hat[1] * dt * dt,
                                                                            a_hat[2] * dt * dt};
  double S1[9], S2[9], RtS1[9], RtS2[9];
  skew(adt, S1);
  skew(adt2, S2);
  m3_mul_at(R, S1, RtS1);
  m3_mul_at(R, S2, RtS2);
  std::memset(F, 0, sizeof(double) * 225);
  double G[15 * 12];
  std::memset(G, 0, sizeof(G));
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double Rt = R[3 * j + i], I = (i == j) ? 1.0 : 0.0;
      F[(0 + i) * 15 + 0 + j] = Rexp[3 * i + j];
      F[(0 + i) * 15 + 9 + j] = -RJ[3 * i + j] * dt;
      F[(9 + i) * 15 + 9 + j] = I;
      F[(6 + i) * 15 + 0 + j] = -RtS1[3 * i + j];
      F[(6 + i) * 15 + 6 + j] = I;
      F[(6 + i) * 15 + 12 + j] = -Rt * dt;
      F[(12 + i) * 15 + 12 + j] = I;
      F[(3 + i) * 15 + 0 + j] = -0.5 * RtS2[3 * i + j];
      F[(3 + i) * 15 + 6 + j] = I * dt;
      F[(3 + i) * 15 + 12 + j] = -0.5 * Rt * dt * dt;
      F[(3 + i) * 15 + 3 + j] = I;
      G[(0 + i) * 12 + 0 + j] = -RJ[3 * i + j] * dt;
      G[(6 + i) * 12 + 3 + j] = -Rt * dt;
      G[(3 + i) * 12 + 3 + j] = -0.5 * Rt * dt * dt;
      G[(9 + i) * 12 + 6 + j] = I;
      G[(12 + i) * 12 + 9 + j] = I;
    }
  // Qd = G Qc G^T, symmetrized (Propagator.cpp:223-230); Qc is diagonal
  double qc[12];
  for (int k = 0; k < 3; k++) {
    qc[k] = n.sigma_w_2 / dt;
    qc[3 + k] = n.sigma_a_2 / dt;
    qc[6 + k] = n.sigma_wb_2 * dt;
    qc[9 + k] = n.sigma_ab_2 * dt;
  }
  double Q[225];
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = 0;
      for (int k = 0; k < 12; k++) s += G[i * 12 + k] * qc[k] * G[j * 12 + k];
      Q[i * 15 + j] = s;
    }
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) Qd[i * 15 + j] = 0.5 * (Q[i * 15 + j] + Q[j * 15 + i]);
}

// The mean of one interval (Propagator.cpp:233-236): zero-order quaternion, constant acceleration
inline void interval_mean(Cache &c, const Noise &n, const double *a_hat, const double *w_hat, double dt) {
  double R[9], Rexp[9], Rn[9], mw[3], Rta[3];
  quat_2_Rot(c.est, R);
  for (int k = 0; k < 3; k++) mw[k] = -w_hat[k] * dt;
  exp_so3(mw, Rexp);
  m3_mul(Rexp, R, Rn);
  m3t_vec(R, a_hat, Rta);
  const double g[3] = {0, 0, n.gravity_mag};
  double *p = c.est + 4, *v = c.est + 7;
  for (int k = 0; k < 3; k++) {
    p[k] = p[k] + v[k] * dt + 0.5 * Rta[k] * dt * dt - 0.5 * g[k] * dt * dt;
    v[k] = v[k] + Rta[k] * dt - g[k] * dt;
  }
  rot_2_quat(Rn, c.est);
}

// One interval of the loop at Propagator.cpp:176-237
inline void step(Cache &c, const Noise &n, const ImuSample &minus, const ImuSample &plus) {
  const double dt = plus.t - minus.t;
  double a1[3], a2[3], w1[3], w2[3], a_hat[3], w_hat[3];
  corrected(c, minus, a1, w1);
  corrected(c, plus, a2, w2);
  for (int k = 0; k < 3; k++) a_hat[k] = 0.5 * (a1[k] + a2[k]), w_hat[k] = 0.5 * (w1[k] + w2[k]);
  double F[225], Qd[225], FP[225], Pn[225];
  interval_F_Qd(c, n, a_hat, w_hat, dt, F, Qd);
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = 0;
      for (int k = 0; k < 15; k++) s += F[i * 15 + k] * c.cov[k * 15 + j];
      FP[i * 15 + j] = s;
    }
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = 0;
      for (int k = 0; k < 15; k++) s += FP[i * 15 + k] * F[j * 15 + k];
      Pn[i * 15 + j] = s + Qd[i * 15 + j];
    }
  std::memcpy(c.cov, Pn, sizeof(Pn));
  interval_mean(c, n, a_hat, w_hat, dt);
}

// The output stage (Propagator.cpp:244-265): state_plus = [q_GtoI, p_IinG, v_IinI, w_IinI]; the 12 x 12 is the
// (theta, p, v) block with v rotated into the local frame, and sigma_w^2 / dt of the last interval for w
inline void output(const Cache &c, const Noise &n, const ImuSample &last, double dt_last, double *state_plus,
                   double *cov12) {
  double Rq[9], a[3], w[3];
  quat_2_Rot(c.est, Rq);
  for (int k = 0; k < 13; k++) state_plus[k] = 0;
  for (int k = 0; k < 7; k++) state_plus[k] = c.est[k];
  m3_vec(Rq, c.est + 7, state_plus + 7);
  corrected(c, last, a, w);
  for (int k = 0; k < 3; k++) state_plus[10 + k] = w[k];
  // Phi P Phi^T with Phi = I but Phi(6:9, 6:9) = R(q): rows, then columns 6..8 of the leading 9 x 9
  double T[81], U[81];
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++) {
      if (i < 6) {
        T[i * 9 + j] = c.cov[i * 15 + j];
      } else {
        double s = 0;
        for (int k = 0; k < 3; k++) s += Rq[3 * (i - 6) + k] * c.cov[(6 + k) * 15 + j];
        T[i * 9 + j] = s;
      }
    }
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++) {
      if (j < 6) {
        U[i * 9 + j] = T[i * 9 + j];
      } else {
        double s = 0;
        for (int k = 0; k < 3; k++) s += T[i * 9 + 6 + k] * Rq[3 * (j - 6) + k];
        U[i * 9 + j] = s;
      }
    }
  for (int k = 0; k < 144; k++) cov12[k] = 0;
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++) cov12[i * 12 + j] = U[i * 9 + j];
  for (int k = 0; k < 3; k++) cov12[(9 + k) * 12 + 9 + k] = n.sigma_w_2 / dt_last;
}

// Propagator::fast_state_propagate on a valid cache and the IMU buffer: false (nothing written, the cache as it
// was) with fewer than two selected readings; otherwise the cache is left at the query time with a zero time
// offset, so successive queries chain (Propagator.cpp:239-242)
inline bool query(Cache &c, const Noise &n, const std::vector<ImuSample> &imu, double t, double *state_plus,
                  double *cov12) {
  const double time0 = c.t + c.t_off, time1 = t + c.t_off;
  const std::vector<ImuSample> prop = select_imu(imu, time0, time1);
  if (prop.size() < 2) return false;
  for (size_t i = 0; i + 1 < prop.size(); i++) step(c, n, prop[i], prop[i + 1]);
  c.t = time1;
  c.t_off = 0.0;
  output(c, n, prop.back(), prop.back().t - prop[prop.size() - 2].t, state_plus, cov12);
  return true;
}

}  // namespace fastprop
}  // namespace uvhp
