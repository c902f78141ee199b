// Normals of a bare cloud (see include/mvsn_hip.h: mvsn_cloud_normals; the semantics are DESIGN.md section 21): for
// every query point the principal axes of the covariance of the support points within the radius (PCA), on an index
// that mvsn_cloud_index_build made.  The neighbourhood is section 14's query (mvsn_cloud.h: cloud_visit, the visitor
// form of the walk).
//
//   cloud_normals_kernel   one thread per query point.  Per accepted neighbour the three fp32 differences of the walk
//                          are scaled by inv (one fp32 multiply each) and quantised to integers of 2^-20 cells (rintf:
//                          ties to even, |u| < 2^21); the count, the three sums of u_a and the six sums of u_a u_b are
//                          exact 64-bit integers, so the order of a cell's records (which depends on the order in which
//                          the scatter's atomics arrived) reaches no output.  Then, in the same thread and in fp64: the
//                          covariance, CN_SWEEPS cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2), a sort of the
//                          three eigenpairs, the gap test, the sign rule, and one rounding of every output to fp32.
// One launch, no workspace of its own, no atomics, nothing waits on another thread, every loop bounded: every output is
// a bitwise-reproducible function of the inputs and does not depend on the order of the support's rows.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add: every step of section 21
// is one operation.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"

namespace mvsn {

constexpr int CN_SWEEPS = 6;
constexpr long CN_MAX_NEIGHBOURS = 1L << 20;            // each product is below 2^42: the sums cannot overflow up to here
constexpr float CN_QUANTUM = 0x1p20f;                   // integers of 2^-20 cells

// One Jacobi rotation in the plane (p, q) of a symmetric 3x3, r the third index: app, aqq, apq the plane's entries, arp
// and arq the third row's; vp, vq the two columns of the eigenvector matrix.  Only + - * / and sqrt.
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *vp,
                                              double *vq) {
  if (apq == 0.0) return;                                 // nothing to annihilate (and no 0 / 0 below)
  const double theta = (aqq - app) / (2.0 * apq);       // +-inf where apq vanishes against the difference: t = 0
  const double mag = (theta < 0.0 ? -theta : theta) + sqrt(theta * theta + 1.0);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / mag;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double tau = t * apq;
  app = app - tau;
  aqq = aqq + tau;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double kp = vp[k], kq = vq[k];
    vp[k] = c * kp - s * kq;
    vq[k] = s * kp + c * kq;
  }
}

// (lambda a, column a) and (lambda b, column b) in ascending order; equal values keep their places
__device__ __forceinline__ void eigen_order(double &la, double &lb, double *va, double *vb) {
  const bool swap = lb < la;
  const double l = la;
  la = swap ? lb : la;
  lb = swap ? l : lb;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = va[k];
    va[k] = swap ? vb[k] : va[k];
    vb[k] = swap ? v : vb[k];
  }
}

__global__ __launch_bounds__(CL_THREADS) void cloud_normals_kernel(
    const float *__restrict__ query, long nq, const float *__restrict__ viewpoint, long viewpoint_rows, float h, float inv,
    float r2, long min_neighbours, double min_gap, const unsigned long long *__restrict__ keys,
    const int *__restrict__ pop, const int *__restrict__ start, const floatx4 *__restrict__ records, size_t slots, long n,
    float *__restrict__ normals, float *__restrict__ eigenvalues, int *__restrict__ count) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= nq) return;
  const float qx = query[(size_t)i * 3], qy = query[(size_t)i * 3 + 1], qz = query[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};

  // the sums are unsigned so that a neighbourhood past the limit wraps instead of overflowing; each product is formed
  // from two ints as a signed 64-bit number and is exact
  int within = 0;
  unsigned long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
  cloud_visit(qx, qy, qz, inv, r2, ix, records, n,
              [&](float dx, float dy, float dz, float, const floatx4 &) {
                const int ux = (int)rintf((dx * inv) * CN_QUANTUM);
                const int uy = (int)rintf((dy * inv) * CN_QUANTUM);
                const int uz = (int)rintf((dz * inv) * CN_QUANTUM);
                ++within;
                sx += (unsigned long long)(int64_t)ux, sy += (unsigned long long)(int64_t)uy;
                sz += (unsigned long long)(int64_t)uz;
                sxx += (unsigned long long)((int64_t)ux * ux);
                sxy += (unsigned long long)((int64_t)ux * uy);
                sxz += (unsigned long long)((int64_t)ux * uz);
                syy += (unsigned long long)((int64_t)uy * uy);
                syz += (unsigned long long)((int64_t)uy * uz);
                szz += (unsigned long long)((int64_t)uz * uz);
              });
  count[i] = within;

  double lam[3] = {0.0, 0.0, 0.0}, nrm[3] = {0.0, 0.0, 0.0};
  if (within >= 1 && (long)within <= CN_MAX_NEIGHBOURS) {
    const double cnt = (double)within;
    const double mx = (double)(int64_t)sx / cnt, my = (double)(int64_t)sy / cnt, mz = (double)(int64_t)sz / cnt;
    double a00 = (double)(int64_t)sxx / cnt - mx * mx, a01 = (double)(int64_t)sxy / cnt - mx * my;
    double a02 = (double)(int64_t)sxz / cnt - mx * mz, a11 = (double)(int64_t)syy / cnt - my * my;
    double a12 = (double)(int64_t)syz / cnt - my * mz, a22 = (double)(int64_t)szz / cnt - mz * mz;
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};   // the columns of V
#pragma unroll 1
    for (int sweep = 0; sweep < CN_SWEEPS; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);   // (0,1), third index 2
      jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);   // (0,2), third index 1
      jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);   // (1,2), third index 0
    }
    eigen_order(a00, a11, v0, v1);
    eigen_order(a11, a22, v1, v2);
    eigen_order(a00, a11, v0, v1);
    const double unit = (double)h * 0x1p-20;
    const double scale = unit * unit;
    lam[0] = a00 * scale, lam[1] = a11 * scale, lam[2] = a22 * scale;
    const bool defined = (long)within >= min_neighbours && !(a11 - a00 <= min_gap * a22);
    if (defined) {
      // the canonical sign: the component of largest magnitude is positive, ties to the lowest axis
      const double m0 = v0[0] < 0.0 ? -v0[0] : v0[0], m1 = v0[1] < 0.0 ? -v0[1] : v0[1], m2 = v0[2] < 0.0 ? -v0[2] : v0[2];
      const double lead = (m0 >= m1 && m0 >= m2) ? v0[0] : (m1 >= m2 ? v0[1] : v0[2]);
      bool flip = lead < 0.0;
      if (viewpoint_rows > 0) {
        const float *vp = viewpoint + (viewpoint_rows == 1 ? (size_t)0 : (size_t)i * 3);
        const float wx = vp[0], wy = vp[1], wz = vp[2];
        if (isfinite(wx) && isfinite(wy) && isfinite(wz)) {
          const double ex = (double)wx - (double)qx, ey = (double)wy - (double)qy, ez = (double)wz - (double)qz;
          const double dot = (v0[0] * ex + v0[1] * ey) + v0[2] * ez;
          if (dot != 0.0) flip = dot < 0.0;                 // dot == 0: the canonical sign stays
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) nrm[k] = flip ? -v0[k] : v0[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) normals[(size_t)i * 3 + k] = (float)nrm[k];
  if (eigenvalues) {
#pragma unroll
    for (int k = 0; k < 3; ++k) eigenvalues[(size_t)i * 3 + k] = (float)lam[k];
  }
}

}  // namespace mvsn

extern "C" int mvsn_cloud_normals(const float *query, long nq, const float *viewpoint, long viewpoint_rows, float cell,
                                  float inv_cell, float r2, long min_neighbours, double min_gap,
                                  const void *index_workspace, size_t index_workspace_bytes, long n_target,
                                  float *normals, float *eigenvalues, int *count, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_normals";
  MVSN_REQUIRE(query && normals && count, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(nq > 0 && n_target > 0, MVSN_E_BADARG, "%s: %ld queries against %ld points", who, nq, n_target);
  MVSN_REQUIRE((viewpoint == nullptr) == (viewpoint_rows == 0) &&
                   (viewpoint_rows == 0 || viewpoint_rows == 1 || viewpoint_rows == nq),
               MVSN_E_BADARG, "%s: %ld viewpoint rows (0 without a viewpoint, 1, or one per query)", who, viewpoint_rows);
  MVSN_REQUIRE(cell > 0.0f && cell <= 3.0e38f && inv_cell > 0.0f && inv_cell <= 3.0e38f && r2 > 0.0f && r2 <= 3.0e38f,
               MVSN_E_BADARG, "%s: cell size %g, its inverse %g or squared radius %g is not a positive finite number", who,
               (double)cell, (double)inv_cell, (double)r2);
  MVSN_REQUIRE(min_neighbours >= 3, MVSN_E_BADARG, "%s: min_neighbours %ld (at least 3)", who, min_neighbours);
  MVSN_REQUIRE(min_gap >= 0.0 && min_gap < 1.0, MVSN_E_BADARG, "%s: min_gap %g (inside [0, 1))", who, min_gap);
  MVSN_REQUIRE(nq <= 0x7fffffffL && n_target <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld queries against %ld points (at most 2^31 - 1 each)", who, nq, n_target);
  CloudLayout l;
  if (int e = cloud_index_check(who, "index workspace", index_workspace, index_workspace_bytes, n_target, &l)) return e;
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, l, &records);
  hipLaunchKernelGGL(cloud_normals_kernel, dim3((unsigned)((nq + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0,
                     (hipStream_t)stream, query, nq, viewpoint, viewpoint_rows, cell, inv_cell, r2, min_neighbours, min_gap,
                     ix.keys, ix.pop, ix.start, records, ix.slots, n_target, normals, eigenvalues, count);
  return check_launch("mvsn_cloud_normals: normals");
}
