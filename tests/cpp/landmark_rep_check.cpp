// Driver of tests/test_landmark_rep_math.py: the shared landmark conversions (uvio_amd/csrc/landmark_rep.h) on
// the points of stdin.  Input lines "rep x y z xf yf zf" (a point and the point of the first estimate); output per
// line: val(3) fej(3) uvn0(3) uvn0_fej(3) xyz(false)(3) xyz(true)(3) size relative, in %.17g.
#include <cstdio>

#include "landmark_rep.h"

int main() {
  int rep;
  double p[3], pf[3];
  while (std::scanf("%d %lf %lf %lf %lf %lf %lf", &rep, p, p + 1, p + 2, pf, pf + 1, pf + 2) == 7) {
    double val[3] = {0, 0, 0}, fej[3] = {0, 0, 0}, uvn0[3] = {0, 0, 0}, uvn0_fej[3] = {0, 0, 0}, o[3], of[3];
    uvhp::landmark_set_from_xyz(rep, p, val, uvn0);
    uvhp::landmark_set_from_xyz(rep, pf, fej, uvn0_fej);
    uvhp::landmark_get_xyz(rep, val, fej, uvn0, false, o);
    uvhp::landmark_get_xyz(rep, val, fej, uvn0, true, of);
    const double *all[6] = {val, fej, uvn0, uvn0_fej, o, of};
    for (auto *a : all) std::printf("%.17g %.17g %.17g ", a[0], a[1], a[2]);
    std::printf("%d %d\n", uvhp::landmark_rep_size(rep), uvhp::landmark_rep_relative(rep) ? 1 : 0);
  }
  return 0;
}
