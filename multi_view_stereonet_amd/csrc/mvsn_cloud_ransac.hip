// RANSAC over point correspondences: the rigid pose with the most inliers (see include/mvsn_hip.h: mvsn_cloud_ransac; the
// semantics and every step are DESIGN.md section 23).
//
//   cloud_ransac_kernel         one thread per hypothesis h.  Three draws by integer operations alone (the splitmix64
//                               finaliser of seed + (3h + j + 1) 0x9E3779B97F4A7C15, taken to [0, C) by the high half of a
//                               32 x 32-bit multiply), the rejection tests, the pose from two orthonormal frames, then the
//                               walk over all C correspondences: their six floats are staged through LDS in tiles of 256
//                               (a correspondence outside either cloud is staged as NaN and is never dereferenced), every
//                               lane reads the same LDS word at a time, and the inlier count is an integer.  The winner is
//                               max over (count << 32 | 0xffffffff - h) by a 64-bit integer atomicMax: most inliers, ties to
//                               the lowest hypothesis, whatever the order of arrival.  No float is reduced.
//   cloud_ransac_finish_kernel  one workgroup: the number of usable correspondences, the winner's pose again (the same
//                               function, the same bits), T, its fp64 copy, (hypothesis, inliers, status) and the inlier
//                               mask.  Nothing is read on the host between the two launches.
// fp64 throughout, only + - x / sqrt and compares.  Contraction is off for the whole file and nothing here is written as a
// fused multiply-add: every step of section 23 is one operation.
#pragma clang fp contract(off)
#include "mvsn_common.h"

namespace mvsn {

constexpr int CR_THREADS = 256;
constexpr long CR_MAX_HYPOTHESES = 1L << 24;
constexpr size_t CR_WORKSPACE_BYTES = 256;                 // the key word, and room to stay 256-byte granular

struct RansacPose {
  double R[9], t[3];
};

__device__ __forceinline__ unsigned ransac_draw(unsigned long long seed, unsigned long long h, int j, unsigned c) {
  unsigned long long z = seed + (3ull * h + (unsigned long long)j + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (unsigned)(((z >> 32) * (unsigned long long)c) >> 32);
}

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the frame (e1, e2, e3) of three points, as rows of F; false where the triangle is degenerate:
// |a x b|^2 <= 2^-40 |a|^2 |b|^2 (a comparison that a NaN fails to pass: the triangle is then refused too)
__device__ __forceinline__ bool ransac_frame(const double (*p)[3], double (*F)[3]) {
  double a[3], b[3], n[3];
  for (int k = 0; k < 3; ++k) a[k] = p[1][k] - p[0][k], b[k] = p[2][k] - p[0][k];
  const double aa = dot3(a, a), bb = dot3(b, b);
  const double la = sqrt(aa);
  for (int k = 0; k < 3; ++k) F[0][k] = a[k] / la;
  cross3(F[0], b, n);
  double c[3];
  cross3(a, b, c);
  const double cc = dot3(c, c);
  if (!(cc > 0x1p-40 * (aa * bb))) return false;
  const double ln = sqrt(dot3(n, n));
  for (int k = 0; k < 3; ++k) F[2][k] = n[k] / ln;
  cross3(F[2], F[0], F[1]);
  return true;
}

// Hypothesis h: its draws, the rejection tests and the pose.  false where it is rejected.
__device__ __forceinline__ bool ransac_hypothesis(const float *__restrict__ source, long ns, const float *__restrict__ target,
                                                  long nt, const int64_t *__restrict__ corr, unsigned c, double es2,
                                                  unsigned long long seed, unsigned long long h, RansacPose &pose) {
  unsigned d[3];
  for (int j = 0; j < 3; ++j) d[j] = ransac_draw(seed, h, j, c);
  if (d[0] == d[1] || d[0] == d[2] || d[1] == d[2]) return false;
  double s[3][3], t[3][3];
  bool finite = true;
  for (int j = 0; j < 3; ++j) {
    const int64_t a = corr[(size_t)d[j] * 2], b = corr[(size_t)d[j] * 2 + 1];
    if (a < 0 || a >= (int64_t)ns || b < 0 || b >= (int64_t)nt) return false;
    for (int k = 0; k < 3; ++k) {
      const float x = source[(size_t)a * 3 + k], y = target[(size_t)b * 3 + k];
      finite = finite && isfinite(x) && isfinite(y);
      s[j][k] = (double)x, t[j][k] = (double)y;
    }
  }
  if (!finite) return false;
  for (int u = 0; u < 3; ++u)
    for (int v = u + 1; v < 3; ++v) {
      double es[3], et[3];
      for (int k = 0; k < 3; ++k) es[k] = s[v][k] - s[u][k], et[k] = t[v][k] - t[u][k];
      const double ls = dot3(es, es), lt = dot3(et, et);
      const double lo = ls < lt ? ls : lt, hi = ls < lt ? lt : ls;
      if (lo < es2 * hi) return false;
    }
  double Fs[3][3], Ft[3][3];
  if (!ransac_frame(s, Fs) || !ransac_frame(t, Ft)) return false;
  bool ok = true;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double r = (Ft[0][i] * Fs[0][j] + Ft[1][i] * Fs[1][j]) + Ft[2][i] * Fs[2][j];
      pose.R[i * 3 + j] = r;
      ok = ok && isfinite(r);
    }
  double cs[3], ct[3];
  for (int k = 0; k < 3; ++k) cs[k] = ((s[0][k] + s[1][k]) + s[2][k]) / 3.0, ct[k] = ((t[0][k] + t[1][k]) + t[2][k]) / 3.0;
  for (int i = 0; i < 3; ++i) {
    pose.t[i] = ct[i] - dot3(pose.R + i * 3, cs);
    ok = ok && isfinite(pose.t[i]);
  }
  return ok;                                               // (a pose that overflowed is rejected)
}

// the six floats of correspondence j, NaN where it takes no part (a row outside either cloud, never dereferenced)
__device__ __forceinline__ void ransac_stage(const float *__restrict__ source, long ns, const float *__restrict__ target,
                                             long nt, const int64_t *__restrict__ corr, long j, float *six) {
  const int64_t a = corr[(size_t)j * 2], b = corr[(size_t)j * 2 + 1];
  const bool inside = a >= 0 && a < (int64_t)ns && b >= 0 && b < (int64_t)nt;
  for (int k = 0; k < 3; ++k) {
    six[k] = inside ? source[(size_t)a * 3 + k] : (float)NAN;
    six[3 + k] = inside ? target[(size_t)b * 3 + k] : (float)NAN;
  }
}

__device__ __forceinline__ bool ransac_inlier(const RansacPose &pose, const float *six, double r2) {
  const double s[3] = {(double)six[0], (double)six[1], (double)six[2]};
  double e[3];
  for (int i = 0; i < 3; ++i) e[i] = (dot3(pose.R + i * 3, s) + pose.t[i]) - (double)six[3 + i];
  return dot3(e, e) <= r2;                                 // (a NaN compares false)
}

__global__ __launch_bounds__(CR_THREADS) void cloud_ransac_kernel(const float *__restrict__ source, long ns,
                                                                  const float *__restrict__ target, long nt,
                                                                  const int64_t *__restrict__ corr, long c, float r2,
                                                                  double edge_similarity, long hypotheses,
                                                                  unsigned long long seed, unsigned long long *key_word) {
  __shared__ float tile[CR_THREADS * 6];
  const long h = (long)blockIdx.x * CR_THREADS + threadIdx.x;
  RansacPose pose;
  const bool ok = h < hypotheses && ransac_hypothesis(source, ns, target, nt, corr, (unsigned)c, edge_similarity * edge_similarity,
                                                      seed, (unsigned long long)h, pose);
  const double r2d = (double)r2;
  unsigned count = 0;
#pragma unroll 1
  for (long base = 0; base < c; base += CR_THREADS) {
    const int rows = (int)min((long)CR_THREADS, c - base);
    __syncthreads();                                      // (the tile may still be read from the pass before)
    if ((int)threadIdx.x < rows) ransac_stage(source, ns, target, nt, corr, base + threadIdx.x, tile + threadIdx.x * 6);
    __syncthreads();
    if (ok) {
#pragma unroll 1
      for (int r = 0; r < rows; ++r) count += ransac_inlier(pose, tile + r * 6, r2d) ? 1u : 0u;
    }
  }
  if (ok) atomicMax(key_word, ((unsigned long long)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)h));
}

__global__ __launch_bounds__(CR_THREADS) void cloud_ransac_finish_kernel(const float *__restrict__ source, long ns,
                                                                         const float *__restrict__ target, long nt,
                                                                         const int64_t *__restrict__ corr, long c, float r2,
                                                                         double edge_similarity, unsigned long long seed,
                                                                         const unsigned long long *key_word,
                                                                         float *__restrict__ T, double *__restrict__ T64,
                                                                         int64_t *__restrict__ best,
                                                                         unsigned char *__restrict__ inlier) {
  __shared__ int usable;
  if (threadIdx.x == 0) usable = 0;
  __syncthreads();
  const unsigned long long key = *key_word;
  const unsigned long long h = (unsigned long long)(0xffffffffu - (unsigned)(key & 0xffffffffull));
  RansacPose pose;
  const bool ok = key != 0ull && ransac_hypothesis(source, ns, target, nt, corr, (unsigned)c, edge_similarity * edge_similarity,
                                                   seed, h, pose);
  const double r2d = (double)r2;
  int mine = 0;
  for (long j = threadIdx.x; j < c; j += CR_THREADS) {
    float six[6];
    ransac_stage(source, ns, target, nt, corr, j, six);
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && isfinite(six[k]);
    mine += finite ? 1 : 0;
    inlier[j] = (ok && ransac_inlier(pose, six, r2d)) ? 1 : 0;
  }
  atomicAdd(&usable, mine);                                // (an integer sum: the order does not reach it)
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const double v = !ok ? (i == j ? 1.0 : 0.0) : i == 3 ? (j == 3 ? 1.0 : 0.0) : j == 3 ? pose.t[i] : pose.R[i * 3 + j];
      T64[i * 4 + j] = v;
      T[i * 4 + j] = (float)v;
    }
  best[0] = ok ? (int64_t)h : (int64_t)-1;
  best[1] = ok ? (int64_t)(key >> 32) : (int64_t)0;
  best[2] = ok ? 0 : usable < 3 ? 1 : 2;
}

}  // namespace mvsn

extern "C" size_t mvsn_cloud_ransac_workspace_bytes() { return mvsn::CR_WORKSPACE_BYTES; }

extern "C" int mvsn_cloud_ransac(const float *source, long ns, const float *target, long nt, const int64_t *correspondences,
                                 long c, float r2, double edge_similarity, long hypotheses, unsigned long long seed,
                                 void *workspace, size_t workspace_bytes, float *T, double *T64, int64_t *best,
                                 unsigned char *inlier, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_ransac";
  MVSN_REQUIRE(source && target && correspondences && T && T64 && best && inlier, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(ns > 0 && nt > 0 && c > 0, MVSN_E_BADARG, "%s: %ld correspondences between %ld and %ld points", who, c, ns, nt);
  MVSN_REQUIRE(r2 > 0.0f && r2 <= 3.0e38f, MVSN_E_BADARG, "%s: squared radius %g is not a positive finite number", who,
               (double)r2);
  MVSN_REQUIRE(edge_similarity > 0.0 && edge_similarity <= 1.0, MVSN_E_BADARG, "%s: edge_similarity = %g (inside (0, 1])", who,
               edge_similarity);
  MVSN_REQUIRE(hypotheses >= 1, MVSN_E_BADARG, "%s: hypotheses = %ld (1 to 2^24)", who, hypotheses);
  MVSN_REQUIRE(hypotheses <= CR_MAX_HYPOTHESES, MVSN_E_TOOLARGE, "%s: hypotheses = %ld (1 to 2^24)", who, hypotheses);
  MVSN_REQUIRE(ns <= 0x7fffffffL && nt <= 0x7fffffffL && c <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld correspondences between %ld and %ld points (at most 2^31 - 1 each)", who, c, ns, nt);
  MVSN_REQUIRE(workspace && workspace_bytes >= CR_WORKSPACE_BYTES, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed",
               who, workspace_bytes, CR_WORKSPACE_BYTES);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "%s: workspace not 16-byte aligned", who);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long *key = (unsigned long long *)workspace;
  if (hipError_t e = hipMemsetAsync(key, 0, sizeof(unsigned long long), st)) {   // (a memset node on the stream, no host write)
    (void)hipGetLastError();
    set_error("%s: clearing the key word: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(cloud_ransac_kernel, dim3((unsigned)((hypotheses + CR_THREADS - 1) / CR_THREADS)), dim3(CR_THREADS), 0, st,
                     source, ns, target, nt, correspondences, c, r2, edge_similarity, hypotheses, seed, key);
  if (int e = check_launch("mvsn_cloud_ransac: hypotheses")) return e;
  hipLaunchKernelGGL(cloud_ransac_finish_kernel, dim3(1), dim3(CR_THREADS), 0, st, source, ns, target, nt, correspondences, c, r2,
                     edge_similarity, seed, (const unsigned long long *)key, T, T64, best, inlier);
  return check_launch("mvsn_cloud_ransac: finish");
}
