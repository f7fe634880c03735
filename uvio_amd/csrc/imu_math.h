// Host-only IMU helpers shared by the propagator (engine_prop.cpp) and the IMU-rate odometry (fast_prop.h):
// the IMU sample, Propagator::select_imu_readings, the SO(3) exponential and left Jacobian, and the IMU
// intrinsic matrices.  Plain arrays, no Engine members: a stand-alone program can compile this header.
#pragma once
#include <cmath>
#include <vector>

#include "hp_math.h"

namespace uvhp {

struct ImuSample {
  double t, wm[3], am[3];
};

inline void eye3(double *I) {
  for (int i = 0; i < 9; i++) I[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

// exp_so3 (quat_ops.h:231)
inline void exp_so3(const double *w, double *R) {
  double th = norm3(w), A, B;
  if (th < 1e-7) {
    A = 1;
    B = 0.5;
  } else {
    A = sin(th) / th;
    B = (1 - cos(th)) / (th * th);
  }
  if (th == 0) {
    eye3(R);
    return;
  }
  double S[9], S2[9];
  skew(w, S);
  m3_mul(S, S, S2);
  for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + A * S[i] + B * S2[i];
}
// Jl_so3 (quat_ops.h:515); Jr_so3(w) = Jl_so3(-w) (quat_ops.h:537)
inline void Jl_so3(const double *w, double *J) {
  double th = norm3(w);
  if (th < 1e-6) {
    eye3(J);
    return;
  }
  double a[3] = {w[0] / th, w[1] / th, w[2] / th}, S[9];
  skew(a, S);
  double c1 = sin(th) / th, c2 = 1 - sin(th) / th, c3 = (1 - cos(th)) / th;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) J[3 * i + j] = ((i == j) ? c1 : 0.0) + c2 * a[i] * a[j] + c3 * S[3 * i + j];
}

// State::Dm / State::Tg (State.h:92-111)
inline void Dm(int model, const double *v, double *D) {
  for (int i = 0; i < 9; i++) D[i] = 0;
  if (model == 0) {
    D[0] = v[0];
    D[3] = v[1]; D[4] = v[3];
    D[6] = v[2]; D[7] = v[4]; D[8] = v[5];
  } else {
    D[0] = v[0]; D[1] = v[1]; D[2] = v[3];
    D[4] = v[2]; D[5] = v[4];
    D[8] = v[5];
  }
}
inline void TgM(const double *v, double *T) {
  T[0] = v[0]; T[1] = v[3]; T[2] = v[6];
  T[3] = v[1]; T[4] = v[4]; T[5] = v[7];
  T[6] = v[2]; T[7] = v[5]; T[8] = v[8];
}

// Propagator::select_imu_readings (Propagator.cpp:269-393) on a given buffer
inline std::vector<ImuSample> select_imu(const std::vector<ImuSample> &imu, double time0, double time1) {
  auto interp = [](const ImuSample &a, const ImuSample &b, double t) {
    double lambda = (t - a.t) / (b.t - a.t);
    ImuSample d;
    d.t = t;
    for (int k = 0; k < 3; k++) {
      d.am[k] = (1 - lambda) * a.am[k] + lambda * b.am[k];
      d.wm[k] = (1 - lambda) * a.wm[k] + lambda * b.wm[k];
    }
    return d;
  };
  std::vector<ImuSample> prop;
  if (imu.empty()) return prop;
  for (size_t i = 0; i < imu.size() - 1; i++) {
    if (imu[i + 1].t > time0 && imu[i].t < time0) {
      prop.push_back(interp(imu[i], imu[i + 1], time0));
      continue;
    }
    if (imu[i].t >= time0 && imu[i + 1].t <= time1) {
      prop.push_back(imu[i]);
      continue;
    }
    if (imu[i + 1].t > time1) {
      if (imu[i].t > time1 && i == 0) {
        break;
      } else if (imu[i].t > time1) {
        prop.push_back(interp(imu[i - 1], imu[i], time1));
      } else {
        prop.push_back(imu[i]);
      }
      if (prop.back().t != time1) prop.push_back(interp(imu[i], imu[i + 1], time1));
      break;
    }
  }
  if (prop.empty()) return prop;
  if (prop.back().t != time1) prop.push_back(interp(imu[imu.size() - 2], imu[imu.size() - 1], time1));
  for (size_t i = 0; i + 1 < prop.size(); i++)
    if (std::abs(prop[i + 1].t - prop[i].t) < 1e-12) {
      prop.erase(prop.begin() + i);
      i--;
    }
  return prop;
}

}  // namespace uvhp
