// The fp64 pose arithmetic that the Gauss-Newton loops share (mvsn_tsdf_align.hip, mvsn_cloud_register.hip; DESIGN.md
// section 17): the rotation of an update and the solve of the 6 x 6 normal equations from the sums.  The including file
// turns contraction off: every step here is one fp64 operation.
#pragma once

namespace mvsn {

// exp([w]x) by Rodrigues, the small-angle series below |w|^2 = 1e-8 (the next terms are below 1e-17 of the kept ones)
__device__ inline void align_rotation(const double *w, double *Rd) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double a, b;
  if (t2 < 1e-8) {
    a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0);
    b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0);
  } else {
    const double t = sqrt(t2);
    a = sin(t) / t;
    b = (1.0 - cos(t)) / t2;
  }
  // I + a [w]x + b [w]x^2, [w]x^2 = w w^T - |w|^2 I
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rd[i * 3 + j] = b * (w[i] * w[j]) + (i == j ? 1.0 - b * t2 : 0.0);
  Rd[1] -= a * w[2], Rd[2] += a * w[1];
  Rd[3] += a * w[2], Rd[5] -= a * w[0];
  Rd[6] -= a * w[1], Rd[7] += a * w[0];
}

// The solve from the sums s (30: the 21 of H's upper triangle row-major, the 6 of b, sum w, sum w r^2, count):
// delta = -H^-1 b (v, then omega) through the Cholesky factor of H scaled to a unit diagonal, handed to
// `apply(const double *delta) -> int` whose value is returned (the update of the pose, 0); or, with apply not called,
// the status that stops the loop (1: count < min_count; 2: a diagonal entry that is not a positive finite number, a
// pivot of the scaled matrix below min_pivot, or a delta that is not finite).  (A callable and not an output array: the
// caller's update then sits where it sat when the solve was written out in the caller, branch for branch.)
template <class Apply>
__device__ inline int pose_solve(const double *s, double min_count, double min_pivot, Apply &&apply) {
  if (!(s[29] >= min_count)) return 1;
  double M[6][6], sc[6], y[6];
  {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++m) M[i][j] = M[j][i] = s[m];
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    ok = ok && M[i][i] > 0.0 && M[i][i] <= 1.7976931348623157e308;
    sc[i] = 1.0 / sqrt(M[i][i]);
  }
  if (!ok) return 2;
  // the Cholesky factor L (in the lower triangle of M) of S H S; the pivot of column j is L_jj^2 before its root
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double p = (M[j][j] * sc[j]) * sc[j];
#pragma unroll
    for (int k = 0; k < j; ++k) p = p - M[j][k] * M[j][k];
    ok = ok && p >= min_pivot;                                      // (a NaN fails)
    const double l = sqrt(p);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double e = (M[j][i] * sc[i]) * sc[j];                         // (the upper triangle still holds H)
#pragma unroll
      for (int k = 0; k < j; ++k) e = e - M[i][k] * M[j][k];
      M[i][j] = e / l;
    }
    M[j][j] = l;
  }
  if (!ok) return 2;
  // (S H S) y = -S b: L z = -S b, L^T y = z; delta = S y
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double e = -(s[21 + i] * sc[i]);
#pragma unroll
    for (int k = 0; k < i; ++k) e = e - M[i][k] * y[k];
    y[i] = e / M[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double e = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) e = e - M[k][i] * y[k];
    y[i] = e / M[i][i];
  }
  double delta[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) delta[i] = y[i] * sc[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && fabs(delta[i]) <= 1.7976931348623157e308;
  if (!ok) return 2;
  return apply(delta);
}

}  // namespace mvsn
