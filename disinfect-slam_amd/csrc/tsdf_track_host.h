// tsdf_track_host.h -- the host side of one tracking iteration (tsdf_track; DESIGN.md "Pose
// tracking"): the 6 x 6 Cholesky solve of the normal equations, Rodrigues' formula and the pose
// update, all in double. Plain C++17 with no HIP types: host/tests/track_solve_main.cc includes it.
#pragma once

#include <cmath>

namespace track_host {

// A x = rhs for the symmetric A whose upper triangle (row-major, i <= j) is up21. False when a
// Cholesky pivot is <= 0 or not finite (A is not positive definite, or holds a NaN); x is then untouched.
inline bool solve_spd6(const double* up21, const double* rhs, double* x) {
  double L[6][6] = {};
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) L[j][i] = up21[k++];  // the lower triangle, overwritten by the factor
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
    for (int p = 0; p < j; ++p) d -= L[j][p] * L[j][p];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double s = std::sqrt(d);
    L[j][j] = s;
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
      for (int p = 0; p < j; ++p) v -= L[i][p] * L[j][p];
      L[i][j] = v / s;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = rhs[i];
    for (int p = 0; p < i; ++p) v -= L[i][p] * y[p];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int p = i + 1; p < 6; ++p) v -= L[p][i] * x[p];
    x[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

// R = exp([w]x) (row-major), Rodrigues: I + a K + b K^2 with a = sin t / t, b = (1 - cos t) / t^2,
// t = |w|; below t = 1e-4 their Taylor series (the closed forms cancel there)
inline void so3_exp(const double* w, double* R) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double t = std::sqrt(t2);
  double a, b;
  if (t < 1e-4) {
    a = 1.0 - t2 / 6.0 + t2 * t2 / 120.0;
    b = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
  } else {
    a = std::sin(t) / t;
    b = (1.0 - std::cos(t)) / t2;
  }
  const double x = w[0], y = w[1], z = w[2];
  R[0] = 1.0 - b * (y * y + z * z);
  R[1] = -a * z + b * x * y;
  R[2] = a * y + b * x * z;
  R[3] = a * z + b * x * y;
  R[4] = 1.0 - b * (x * x + z * z);
  R[5] = -a * x + b * y * z;
  R[6] = -a * y + b * x * z;
  R[7] = a * x + b * y * z;
  R[8] = 1.0 - b * (x * x + y * y);
}

// world_T_cam (R_wc row-major, p_wc) of the float pose cam_T_world (q = x, y, z, w; t)
inline void pose_to_world(const float* q, const float* t, double* R_wc, double* p_wc) {
  double x = q[0], y = q[1], z = q[2], w = q[3];
  const double n = std::sqrt(x * x + y * y + z * z + w * w);
  x /= n, y /= n, z /= n, w /= n;
  // R_cw of the unit quaternion; R_wc is its transpose
  const double Rcw[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                         2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R_wc[3 * i + j] = Rcw[3 * j + i];
  for (int i = 0; i < 3; ++i) p_wc[i] = -(R_wc[3 * i] * t[0] + R_wc[3 * i + 1] * t[1] + R_wc[3 * i + 2] * t[2]);
}

// the update of one iteration, xi = (omega, t): R_wc <- exp([omega]x) R_wc, p_wc <- exp([omega]x) p_wc + t
inline void apply_twist(const double* xi, double* R_wc, double* p_wc) {
  double E[9], R[9], p[3];
  so3_exp(xi, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = E[3 * i] * R_wc[j] + E[3 * i + 1] * R_wc[3 + j] + E[3 * i + 2] * R_wc[6 + j];
    p[i] = E[3 * i] * p_wc[0] + E[3 * i + 1] * p_wc[1] + E[3 * i + 2] * p_wc[2] + xi[3 + i];
  }
  for (int i = 0; i < 9; ++i) R_wc[i] = R[i];
  for (int i = 0; i < 3; ++i) p_wc[i] = p[i];
}

// cam_T_world of world_T_cam rounded to floats: the unit quaternion of R_cw = R_wc^T (the branch of
// its largest component, normalised in double, w >= 0) and t = -R_cw p_wc
inline void world_to_pose(const double* R_wc, const double* p_wc, float* q, float* t) {
  double m[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[i][j] = R_wc[3 * j + i];
  double x, y, z, w;
  const double tr = m[0][0] + m[1][1] + m[2][2];
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(1.0 + tr);
    w = 0.25 * s, x = (m[2][1] - m[1][2]) / s, y = (m[0][2] - m[2][0]) / s, z = (m[1][0] - m[0][1]) / s;
  } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
    const double s = 2.0 * std::sqrt(1.0 + m[0][0] - m[1][1] - m[2][2]);
    w = (m[2][1] - m[1][2]) / s, x = 0.25 * s, y = (m[0][1] + m[1][0]) / s, z = (m[0][2] + m[2][0]) / s;
  } else if (m[1][1] > m[2][2]) {
    const double s = 2.0 * std::sqrt(1.0 + m[1][1] - m[0][0] - m[2][2]);
    w = (m[0][2] - m[2][0]) / s, x = (m[0][1] + m[1][0]) / s, y = 0.25 * s, z = (m[1][2] + m[2][1]) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + m[2][2] - m[0][0] - m[1][1]);
    w = (m[1][0] - m[0][1]) / s, x = (m[0][2] + m[2][0]) / s, y = (m[1][2] + m[2][1]) / s, z = 0.25 * s;
  }
  double n = std::sqrt(x * x + y * y + z * z + w * w);
  if (w < 0.0) n = -n;
  q[0] = (float)(x / n), q[1] = (float)(y / n), q[2] = (float)(z / n), q[3] = (float)(w / n);
  for (int i = 0; i < 3; ++i) t[i] = (float)(-(m[i][0] * p_wc[0] + m[i][1] * p_wc[1] + m[i][2] * p_wc[2]));
}

}  // namespace track_host
