// plane_solve.h — the point-to-plane step from its normal equations (include/icp_hip.h
// icp_plane_sums), host only, header only (exported as icp_plane_solve; built alone under the
// sanitizers by `make plane_asan`).
//
// Minimise sum (r + J.x)^2 over x = (w, t'): A x = -g with A = sum J J^T, g = sum J r. The unknowns
// have different units (radians about the origin, metres), so A is scaled to a unit diagonal,
// M = D^-1/2 A D^-1/2, and M is factored by Cholesky. A pivot (the diagonal of M's LDL^T, L_jj^2)
// of at most 2^-26 = sqrt(eps) means the solution keeps fewer than half its digits: the solve
// refuses (a guard, not a tuned value) and the caller takes the point-to-point step instead.
// The step maps x -> R (x - c) + c + t' with R the Rodrigues rotation of w and c the sums' origin.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/icp_hip.h"

namespace icp {

constexpr double kPlanePivotMin = 0x1p-26;

// Solves A x = -g. Returns false (x untouched) when a diagonal entry is not positive or a pivot of
// the scaled matrix is at most kPlanePivotMin.
inline bool plane_solve_system(const double A[36], const double g[6], double x[6]) {
  double sc[6];
  for (int i = 0; i < 6; i++) {
    if (!(A[6 * i + i] > 0.0)) return false;
    sc[i] = 1.0 / std::sqrt(A[6 * i + i]);
  }
  double L[6][6] = {};
  for (int j = 0; j < 6; j++) {
    double piv = 1.0;  // M_jj
    for (int k = 0; k < j; k++) piv -= L[j][k] * L[j][k];
    if (!(piv > kPlanePivotMin)) return false;
    L[j][j] = std::sqrt(piv);
    for (int i = j + 1; i < 6; i++) {
      double v = (A[6 * i + j] * sc[i]) * sc[j];
      for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {  // L y = -D^-1/2 g
    double v = -(g[i] * sc[i]);
    for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {  // L^T z = y
    double v = y[i];
    for (int k = i + 1; k < 6; k++) v -= L[k][i] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; i++) x[i] = y[i] * sc[i];
  return true;
}

// R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2, K the cross-product matrix of w, t = |w|; the
// second coefficient as 2 sin^2(t / 2) / t^2 (no cancellation at small angles).
inline void rodrigues(const double w[3], double R[9]) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double t = std::sqrt(t2);
  double a = 1.0, b = 0.5;
  if (t > 0x1p-100) {
    a = std::sin(t) / t;
    const double h = std::sin(0.5 * t);
    b = 2.0 * (h * h) / t2;
  }
  const double x = w[0], y = w[1], z = w[2];
  R[0] = 1.0 - b * (y * y + z * z);
  R[1] = b * (x * y) - a * z;
  R[2] = b * (x * z) + a * y;
  R[3] = b * (x * y) + a * z;
  R[4] = 1.0 - b * (x * x + z * z);
  R[5] = b * (y * z) - a * x;
  R[6] = b * (x * z) - a * y;
  R[7] = b * (y * z) + a * x;
  R[8] = 1.0 - b * (x * x + y * y);
}

// icp_plane_solve (include/icp_hip.h).
inline void plane_solve(const icp_plane_sums* s, double T[16], int32_t* ok) {
  if (ok) *ok = 0;
  if (!s || !T || s->n < 6) return;
  double x[6];
  if (!plane_solve_system(s->A, s->g, x)) return;
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(x[i])) return;
  double R[9];
  rodrigues(x, R);
  const double* c = s->origin;
  for (int r = 0; r < 3; r++) {
    const double Rc = (R[3 * r] * c[0] + R[3 * r + 1] * c[1]) + R[3 * r + 2] * c[2];
    for (int k = 0; k < 3; k++) T[4 * r + k] = R[3 * r + k];
    T[4 * r + 3] = (x[3 + r] + c[r]) - Rc;
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
  if (ok) *ok = 1;
}

}  // namespace icp
