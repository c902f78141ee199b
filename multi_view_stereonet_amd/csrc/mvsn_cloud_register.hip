// Registration of one cloud to another (see include/mvsn_hip.h: mvsn_cloud_register, mvsn_cloud_register_system; the
// semantics are DESIGN.md section 20): Gauss-Newton on the point-to-plane or the point-to-point residual between a moved
// source point and its nearest target point.  The match is section 14's query (mvsn_cloud.h) on an index that
// mvsn_cloud_index_build made; the solve and the rotation are section 17's (mvsn_pose.h).
//
//   cloud_register_accumulate_kernel<PLANE, MATCHES>
//        a workgroup of 256 threads owns CR_BLOCK_POINTS = 1024 consecutive source rows at a time, in four passes of 256
//        (thread t of pass p has row base + 256 p + t: coalesced); above CR_MAX_BLOCKS = 1024 workgroups the grid stays
//        there and workgroup g goes on to the blocks g + 1024, g + 2048, ...  Thread 0 rounds the fp64 pose to its twelve
//        fp32 numbers in LDS.  Per point: the transform, the grid walk, the differences to the matched row, the normal
//        of that row (plane mode), the residual and its Jacobian in fp32, and 30 fp64 sums.  The wave adds them by an xor
//        tree, the four waves are added in index order through LDS, and the workgroup stores one record of 30 doubles.
//   cloud_register_solve_kernel
//        one workgroup of 64 threads: thread i < 30 adds term i of the records in index order; thread 0 writes the
//        history row and, when asked to, solves and applies the update to the fp64 pose in the workspace.  The last
//        launch only reduces: it writes the normal matrix and the fp32 pose.
// iterations + 1 pairs of launches; a launch boundary is the only ordering between workgroups.  No atomics, nothing
// waits on another workgroup: the order of every sum is fixed by the number of source points, so the outputs are bitwise
// reproducible.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add: every step of section 20
// is one operation.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"
#include "mvsn_pose.h"

namespace mvsn {

constexpr int CR_THREADS = 256;
constexpr int CR_PASSES = 4;
constexpr long CR_BLOCK_POINTS = (long)CR_THREADS * CR_PASSES;   // source rows of a workgroup per block
constexpr long CR_MAX_BLOCKS = 1024;                    // workgroups at most: 4 per compute unit of 256, 240 KiB of records
constexpr int CR_TERMS = 30;                            // 21 of H (upper triangle, row-major), 6 of b, sum w, sum w r^2, count
constexpr int CR_SOLVE_THREADS = 64;
constexpr int CR_POSE = 12;                             // doubles of the pose in the workspace: R row-major, then t
constexpr int CR_MAX_ITERATIONS = 1000;
constexpr float CR_FLT_MAX = 3.4028234e38f;

// the pose as 12 doubles: the workspace's, or (before the first update) the float32 values of T
__device__ inline void register_pose(const float *T, const double *pose, double *P) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) P[a * 3 + b] = pose ? pose[a * 3 + b] : (double)T[a * 4 + b];
    P[9 + a] = pose ? pose[9 + a] : (double)T[a * 4 + 3];
  }
}

// one residual row: H += (w J) J^T, b += (w J) r
__device__ __forceinline__ void register_row(double *acc, double wd, const float *J, float r) {
  const double rd = (double)r;
  int m = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wJ = wd * (double)J[i];
#pragma unroll
    for (int j = i; j < 6; ++j, ++m) acc[m] = acc[m] + wJ * (double)J[j];
    acc[21 + i] = acc[21 + i] + wJ * rd;
  }
}

template <bool PLANE, bool MATCHES>
__global__ __launch_bounds__(CR_THREADS) void cloud_register_accumulate_kernel(
    const float *__restrict__ source, long n, const float *__restrict__ weights, const float *__restrict__ target,
    const float *__restrict__ normals, long n_target, float inv, float r2, const unsigned long long *__restrict__ keys,
    const int *__restrict__ pop, const int *__restrict__ start, const floatx4 *__restrict__ records, size_t slots,
    const float *__restrict__ T, const double *__restrict__ pose, const float *__restrict__ centre, long blocks,
    double *__restrict__ sums, int64_t *__restrict__ index, float *__restrict__ residual) {
  __shared__ float spose[CR_POSE + 3];
  __shared__ double swave[CR_THREADS / 64][CR_TERMS];
  if (threadIdx.x == 0) {
    double P[CR_POSE];
    register_pose(T, pose, P);
#pragma unroll
    for (int i = 0; i < CR_POSE; ++i) spose[i] = (float)P[i];       // each number rounded once
#pragma unroll
    for (int a = 0; a < 3; ++a) spose[CR_POSE + a] = centre[a];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const CloudIndex ix = {keys, pop, start, slots};
  float R[9], t[3], c[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = spose[i];
#pragma unroll
  for (int a = 0; a < 3; ++a) t[a] = spose[9 + a], c[a] = spose[CR_POSE + a];

  double acc[CR_TERMS];
#pragma unroll
  for (int i = 0; i < CR_TERMS; ++i) acc[i] = 0.0;
  int count = 0;

#pragma unroll 1
  for (long block = blockIdx.x; block < blocks; block += gridDim.x) {
#pragma unroll 1
    for (int pass = 0; pass < CR_PASSES; ++pass) {
      const long i = block * CR_BLOCK_POINTS + (long)pass * CR_THREADS + threadIdx.x;
      if (i >= n) continue;                                         // (no barrier inside the loops)
      const float x = source[(size_t)i * 3], y = source[(size_t)i * 3 + 1], z = source[(size_t)i * 3 + 2];
      const float w = weights ? weights[i] : 1.0f;
      float p[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) p[a] = ((R[a * 3] * x + R[a * 3 + 1] * y) + R[a * 3 + 2] * z) + t[a];
      bool takes = fabsf(x) <= CR_FLT_MAX && fabsf(y) <= CR_FLT_MAX && fabsf(z) <= CR_FLT_MAX && fabsf(p[0]) <= CR_FLT_MAX &&
                   fabsf(p[1]) <= CR_FLT_MAX && fabsf(p[2]) <= CR_FLT_MAX && w > 0.0f && w <= CR_FLT_MAX;   // (a NaN fails)
      long row = -1;
      float res = NAN;
      if (takes) {
        unsigned long long best = ~0ull;
        int within = 0;
        cloud_walk(p[0], p[1], p[2], inv, r2, ix, records, n_target, best, within);
        const long j = (long)(unsigned)(best & 0xffffffffull);
        takes = best != ~0ull && j < n_target;                      // (a built index holds rows below n_target only)
        if (takes) {
          const float *tp = target + (size_t)j * 3;
          const float d[3] = {p[0] - tp[0], p[1] - tp[1], p[2] - tp[2]};   // the differences the walk formed
          const float q[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
          const double wd = (double)w;
          if (PLANE) {
            const float *np = normals + (size_t)j * 3;
            const float nv[3] = {np[0], np[1], np[2]};
            takes = fabsf(nv[0]) <= CR_FLT_MAX && fabsf(nv[1]) <= CR_FLT_MAX && fabsf(nv[2]) <= CR_FLT_MAX;
            if (takes) {
              const float r = (d[0] * nv[0] + d[1] * nv[1]) + d[2] * nv[2];
              const float J[6] = {nv[0], nv[1], nv[2], q[1] * nv[2] - q[2] * nv[1], q[2] * nv[0] - q[0] * nv[2],
                                  q[0] * nv[1] - q[1] * nv[0]};
              register_row(acc, wd, J, r);
              const double rd = (double)r;
              acc[28] = acc[28] + (wd * rd) * rd;
              res = r;
            }
          } else {
            // J_a = (e_a, q x e_a): q x e_x = (0, q_z, -q_y), q x e_y = (-q_z, 0, q_x), q x e_z = (q_y, -q_x, 0)
            const float Jx[6] = {1.0f, 0.0f, 0.0f, 0.0f, q[2], -q[1]};
            const float Jy[6] = {0.0f, 1.0f, 0.0f, -q[2], 0.0f, q[0]};
            const float Jz[6] = {0.0f, 0.0f, 1.0f, q[1], -q[0], 0.0f};
            register_row(acc, wd, Jx, d[0]);
            register_row(acc, wd, Jy, d[1]);
            register_row(acc, wd, Jz, d[2]);
            const float d2 = __uint_as_float((unsigned)(best >> 32));
            acc[28] = acc[28] + wd * (double)d2;
            res = d2;
          }
          if (takes) {
            acc[27] = acc[27] + wd;
            ++count;
            row = j;
          }
        }
      }
      if (MATCHES) index[i] = (int64_t)row, residual[i] = res;
    }
  }
  acc[29] = (double)count;

  // the wave's sum: an xor tree, every lane ends with the same bits (a + b = b + a)
#pragma unroll
  for (int i = 0; i < CR_TERMS; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[i] = acc[i] + __shfl_xor(acc[i], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < CR_TERMS; ++i) swave[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < CR_TERMS) {                                     // the waves in index order
    const int i = threadIdx.x;
    sums[(size_t)blockIdx.x * CR_TERMS + i] = ((swave[0][i] + swave[1][i]) + swave[2][i]) + swave[3][i];
  }
}

// The update from the sums s: 0 and the new pose in P, or the status that stops the run with P untouched.
// R <- Rd R, t <- Rd (t - c) + c + v about the fp32 centre c.
__device__ inline int register_update(const double *s, double min_points, double min_pivot, const float *centre,
                                      double *P) {
  return pose_solve(s, min_points, min_pivot, [&](const double *delta) {
    double Rd[9], N[CR_POSE];
    align_rotation(delta + 3, Rd);
    const double cw[3] = {(double)centre[0], (double)centre[1], (double)centre[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) N[a * 3 + b] = (Rd[a * 3] * P[b] + Rd[a * 3 + 1] * P[3 + b]) + Rd[a * 3 + 2] * P[6 + b];
      N[9 + a] = (((Rd[a * 3] * (P[9] - cw[0]) + Rd[a * 3 + 1] * (P[10] - cw[1])) + Rd[a * 3 + 2] * (P[11] - cw[2])) + cw[a]) +
                 delta[a];
    }
#pragma unroll
    for (int i = 0; i < CR_POSE; ++i) P[i] = N[i];
    return 0;
  });
}

// One workgroup.  `pose_in` null: the pose is the float32 T (before the first update).  `update`: solve and write the new
// pose to pose_out (the old one when the run is stopped); without it the launch only reduces.  Outputs that are null are
// not written.  `status` is read unless `first` (then it is 0) and written with `update`.
__global__ __launch_bounds__(CR_SOLVE_THREADS) void cloud_register_solve_kernel(
    const double *__restrict__ sums, int n_records, const float *__restrict__ T, const double *pose_in, double *pose_out,
    const float *__restrict__ centre, int first, int update, double min_points, double min_pivot, int *status,
    double *__restrict__ history, int history_row, double *__restrict__ information, double *__restrict__ rhs,
    float *__restrict__ T_out) {
  __shared__ double ssum[CR_TERMS];
  if (threadIdx.x < CR_TERMS) {
    const double *p = sums + threadIdx.x;
    double sum = 0.0;
    int g = 0;
    for (; g + 8 <= n_records; g += 8) {                            // eight loads in flight; the adds in index order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(g + k) * CR_TERMS];
#pragma unroll
      for (int k = 0; k < 8; ++k) sum = sum + v[k];
    }
    for (; g < n_records; ++g) sum = sum + p[(size_t)g * CR_TERMS];
    ssum[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[CR_TERMS];
#pragma unroll
  for (int i = 0; i < CR_TERMS; ++i) s[i] = ssum[i];
  if (history) {
    double *h = history + (size_t)history_row * 3;
    h[0] = s[29], h[1] = s[27], h[2] = s[28];
  }
  if (information) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++m) information[i * 6 + j] = information[j * 6 + i] = s[m];
  }
  if (rhs) {
#pragma unroll
    for (int i = 0; i < 6; ++i) rhs[i] = s[21 + i];
  }
  double P[CR_POSE];
  register_pose(T, pose_in, P);
  if (first && !update && status) status[0] = 0;                    // no iteration asked for: the run did them all
  if (update) {
    int st = first ? 0 : status[0];
    if (st == 0) st = register_update(s, min_points, min_pivot, centre, P);
    status[0] = st;
#pragma unroll
    for (int i = 0; i < CR_POSE; ++i) pose_out[i] = P[i];
  }
  if (T_out) {                                                      // each number rounded once; the bottom row is T's
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) T_out[a * 4 + b] = (float)P[a * 3 + b];
      T_out[a * 4 + 3] = (float)P[9 + a];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) T_out[12 + b] = T[12 + b];
  }
}

struct RegisterPlan {
  long blocks;                                                      // blocks of CR_BLOCK_POINTS source rows
  long groups;                                                      // workgroups, and records
  size_t pose_bytes, record_bytes;
};

inline RegisterPlan register_plan(long n) {
  RegisterPlan p;
  p.blocks = (n + CR_BLOCK_POINTS - 1) / CR_BLOCK_POINTS;
  p.groups = p.blocks < CR_MAX_BLOCKS ? p.blocks : CR_MAX_BLOCKS;
  p.pose_bytes = align256(sizeof(double) * CR_POSE);
  p.record_bytes = align256(sizeof(double) * CR_TERMS * (size_t)p.groups);
  return p;
}

struct RegisterArgs {
  const float *source;
  long n;
  const float *weights, *target, *normals;
  long n_target;
  float inv, r2;
  const void *index_ws;
  size_t index_bytes;
  const float *T, *centre;
  void *workspace;
  size_t workspace_bytes;
};

// the checks both entries share; 0 or the error code
inline int register_check(const char *who, const RegisterArgs &a) {
  MVSN_REQUIRE(a.source && a.target && a.T && a.centre, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(a.n > 0 && a.n_target > 0, MVSN_E_BADARG, "%s: %ld source points against %ld target points", who, a.n,
               a.n_target);
  MVSN_REQUIRE(a.n <= 0x7fffffffL && a.n_target <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld source points against %ld target points (at most 2^31 - 1 each)", who, a.n, a.n_target);
  MVSN_REQUIRE(a.inv > 0.0f && a.inv <= 3.0e38f && a.r2 > 0.0f && a.r2 <= 3.0e38f, MVSN_E_BADARG,
               "%s: inverse cell size %g or squared radius %g is not a positive finite number", who, (double)a.inv,
               (double)a.r2);
  const CloudLayout l = cloud_layout(a.n_target);
  MVSN_REQUIRE(a.index_ws && a.index_bytes >= l.bytes, MVSN_E_WORKSPACE, "%s: index workspace of %zu bytes, %zu needed", who,
               a.index_bytes, l.bytes);
  const RegisterPlan p = register_plan(a.n);
  const size_t need = p.pose_bytes + p.record_bytes;
  MVSN_REQUIRE(a.workspace && a.workspace_bytes >= need, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               a.workspace_bytes, need);
  MVSN_REQUIRE(((uintptr_t)a.index_ws & 15) == 0 && ((uintptr_t)a.workspace & 15) == 0, MVSN_E_BADARG,
               "%s: workspace not 16-byte aligned", who);
  return 0;
}

template <bool PLANE, bool MATCHES>
inline void register_launch(const RegisterArgs &a, const RegisterPlan &p, const double *pose, double *sums,
                            int64_t *index, float *residual, hipStream_t st) {
  const floatx4 *records;
  const CloudIndex ix = cloud_index(a.index_ws, cloud_layout(a.n_target), &records);
  hipLaunchKernelGGL((cloud_register_accumulate_kernel<PLANE, MATCHES>), dim3((unsigned)p.groups), dim3(CR_THREADS), 0, st,
                     a.source, a.n, a.weights, a.target, a.normals, a.n_target, a.inv, a.r2, ix.keys, ix.pop, ix.start,
                     records, ix.slots, a.T, pose, a.centre, p.blocks, sums, index, residual);
}

inline int register_accumulate(const RegisterArgs &a, const RegisterPlan &p, const double *pose, double *sums,
                               int64_t *index, float *residual, hipStream_t st, const char *what) {
  const bool matches = index != nullptr;
  if (a.normals) {
    if (matches) register_launch<true, true>(a, p, pose, sums, index, residual, st);
    else register_launch<true, false>(a, p, pose, sums, index, residual, st);
  } else {
    if (matches) register_launch<false, true>(a, p, pose, sums, index, residual, st);
    else register_launch<false, false>(a, p, pose, sums, index, residual, st);
  }
  return check_launch(what);
}

}  // namespace mvsn

extern "C" size_t mvsn_cloud_register_workspace_bytes(long n_source) {
  using namespace mvsn;
  if (n_source <= 0 || n_source > 0x7fffffffL) return 0;
  const RegisterPlan p = register_plan(n_source);
  return p.pose_bytes + p.record_bytes;
}

extern "C" int mvsn_cloud_register_system(const float *source, long n_source, const float *weights, const float *target,
                                          const float *target_normals, long n_target, float inv_cell, float r2,
                                          const void *index_workspace, size_t index_workspace_bytes, const float *T,
                                          const float *centre, void *workspace, size_t workspace_bytes, double *H,
                                          double *b, double *sums, int64_t *index, float *residual,
                                          mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_register_system";
  const RegisterArgs a = {source, n_source, weights, target, target_normals, n_target, inv_cell, r2, index_workspace,
                          index_workspace_bytes, T, centre, workspace, workspace_bytes};
  MVSN_REQUIRE(H && b && sums, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE((index == nullptr) == (residual == nullptr), MVSN_E_BADARG, "%s: index and residual go together", who);
  if (int e = register_check(who, a)) return e;
  const RegisterPlan p = register_plan(n_source);
  double *records = (double *)((char *)workspace + p.pose_bytes);
  const hipStream_t st = (hipStream_t)stream;
  if (int e = register_accumulate(a, p, nullptr, records, index, residual, st, "mvsn_cloud_register_system: accumulate"))
    return e;
  hipLaunchKernelGGL(cloud_register_solve_kernel, dim3(1), dim3(CR_SOLVE_THREADS), 0, st, (const double *)records,
                     (int)p.groups, T, (const double *)nullptr, (double *)nullptr, centre, 1, 0, 0.0, 0.0, (int *)nullptr,
                     sums, 0, H, b, (float *)nullptr);
  return check_launch("mvsn_cloud_register_system: reduce");
}

extern "C" int mvsn_cloud_register(const float *source, long n_source, const float *weights, const float *target,
                                   const float *target_normals, long n_target, float inv_cell, float r2,
                                   const void *index_workspace, size_t index_workspace_bytes, const float *T_init,
                                   const float *centre, int iterations, long min_points, double min_pivot,
                                   void *workspace, size_t workspace_bytes, float *T_out, double *history, int *status,
                                   double *information, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_register";
  const RegisterArgs a = {source, n_source, weights, target, target_normals, n_target, inv_cell, r2, index_workspace,
                          index_workspace_bytes, T_init, centre, workspace, workspace_bytes};
  MVSN_REQUIRE(T_out && history && status && information, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(iterations >= 0 && iterations <= CR_MAX_ITERATIONS, MVSN_E_BADARG, "%s: %d iterations (0 to 1000)", who,
               iterations);
  MVSN_REQUIRE(min_points >= 1, MVSN_E_BADARG, "%s: min_points %ld (at least 1)", who, min_points);
  MVSN_REQUIRE(min_pivot > 0.0 && min_pivot < 1.0, MVSN_E_BADARG, "%s: min_pivot %g (inside (0, 1))", who, min_pivot);
  if (int e = register_check(who, a)) return e;
  const RegisterPlan p = register_plan(n_source);
  double *pose = (double *)workspace;
  double *records = (double *)((char *)workspace + p.pose_bytes);
  const hipStream_t st = (hipStream_t)stream;
  for (int it = 0; it <= iterations; ++it) {
    const double *cur = it == 0 ? nullptr : pose;                   // before the first update: the float32 T_init
    if (int e = register_accumulate(a, p, cur, records, nullptr, nullptr, st, "mvsn_cloud_register: accumulate")) return e;
    const bool last = it == iterations;
    hipLaunchKernelGGL(cloud_register_solve_kernel, dim3(1), dim3(CR_SOLVE_THREADS), 0, st, (const double *)records,
                       (int)p.groups, T_init, cur, pose, centre, it == 0 ? 1 : 0, last ? 0 : 1, (double)min_points,
                       min_pivot, status, history, it, last ? information : (double *)nullptr, (double *)nullptr,
                       last ? T_out : (float *)nullptr);
    if (int e = check_launch("mvsn_cloud_register: solve")) return e;
  }
  return 0;
}
