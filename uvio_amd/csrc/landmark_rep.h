// The landmark representations' two conversions (ov_type::Landmark::get_xyz / set_from_xyz, Landmark.cpp:26-137;
// representation ids of LandmarkRepresentation.h:38), stated once for the host mean (Var::xyz / set_xyz), the
// device's landmark read (k_feature mode 1) and the retriangulation.  Part of hp_math.h; includable on its own by a
// plain C++ compiler (tests/test_landmark_rep_math.py).
#pragma once
#include <cmath>

#ifndef HPD
#define HPD inline
#define UVHP_LANDMARK_REP_OWN_HPD
#endif

namespace uvhp {

enum LandmarkRep {
  REP_GLOBAL_3D = 0,
  REP_GLOBAL_FULL_INVERSE_DEPTH = 1,
  REP_ANCHORED_3D = 2,
  REP_ANCHORED_FULL_INVERSE_DEPTH = 3,
  REP_ANCHORED_MSCKF_INVERSE_DEPTH = 4,
  REP_ANCHORED_INVERSE_DEPTH_SINGLE = 5,
};

// LandmarkRepresentation::is_relative_representation (LandmarkRepresentation.h:97-101)
HPD bool landmark_rep_relative(int rep) { return rep == 2 || rep == 3 || rep == 4 || rep == 5; }
// Landmark's state size: the single inverse depth keeps its bearing beside the state (Landmark.h:67-70)
HPD int landmark_rep_size(int rep) { return rep == 5 ? 1 : 3; }

// get_xyz(getfej): val / fej are the landmark's value and first estimate (3 doubles; 1 for rep 5), uvn0 / uvn0_fej
// rep 5's anchor bearing.  Reference quirks, kept: reps 4 and 5 ignore getfej (Landmark.cpp:47-60).
HPD void landmark_get_xyz(int rep, const double *val, const double *fej, const double *uvn0, bool getfej, double *o) {
  const double *p = getfej ? fej : val;
  switch (rep) {
    case 0:
    case 2:
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
      break;
    case 1:
    case 3:
      o[0] = (1 / p[2]) * cos(p[0]) * sin(p[1]);
      o[1] = (1 / p[2]) * sin(p[0]) * sin(p[1]);
      o[2] = (1 / p[2]) * cos(p[1]);
      break;
    case 4:
      o[0] = (1 / val[2]) * val[0];
      o[1] = (1 / val[2]) * val[1];
      o[2] = 1 / val[2];
      break;
    case 5:
      o[0] = (1.0 / val[0]) * uvn0[0];
      o[1] = (1.0 / val[0]) * uvn0[1];
      o[2] = (1.0 / val[0]) * uvn0[2];
      break;
    default:
      o[0] = o[1] = o[2] = 0;
  }
}

// set_from_xyz: d receives the value (or the first estimate); for rep 5 uvn0 (the value's or the first estimate's
// bearing, as the caller chose d) receives p / z.  uvn0 may be null for the other representations.
HPD void landmark_set_from_xyz(int rep, const double *p, double *d, double *uvn0) {
  switch (rep) {
    case 0:
    case 2:
      d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
      break;
    case 1:
    case 3: {
      const double g_rho = 1 / sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
      const double g_phi = acos(g_rho * p[2]);
      const double g_theta = atan2(p[1], p[0]);
      d[0] = g_theta; d[1] = g_phi; d[2] = g_rho;
      break;
    }
    case 4:
      d[0] = p[0] / p[2];
      d[1] = p[1] / p[2];
      d[2] = 1 / p[2];
      break;
    case 5:
      d[0] = 1.0 / p[2];
      uvn0[0] = (1.0 / p[2]) * p[0];
      uvn0[1] = (1.0 / p[2]) * p[1];
      uvn0[2] = (1.0 / p[2]) * p[2];
      break;
    default:
      break;
  }
}

}  // namespace uvhp

#ifdef UVHP_LANDMARK_REP_OWN_HPD
#undef HPD
#undef UVHP_LANDMARK_REP_OWN_HPD
#endif
