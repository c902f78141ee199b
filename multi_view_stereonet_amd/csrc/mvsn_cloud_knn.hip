// The k nearest neighbours between two clouds, and the statistics behind the statistical outlier filter (see
// include/mvsn_hip.h: mvsn_cloud_knn, mvsn_cloud_mean_stats; the semantics are DESIGN.md section 22).  The candidates of
// a query are section 14's (mvsn_cloud.h: cloud_visit, the visitor form of the walk) on an index that
// mvsn_cloud_index_build made.
//
//   cloud_knn_kernel<CAP>  one thread per query point, CAP = 8, 16, 32 or 64 the least capacity >= k.  The thread keeps
//                          CAP 64-bit keys (d2 bits << 32 | row) in ascending order in registers: the first CAP - k are
//                          the sentinel 0, which no insertion moves (every compare is strict), the last k start at ~0
//                          (nothing), so the k-th least key so far is always key[CAP - 1].  A candidate costs one 64-bit
//                          compare against it; one that makes the list replaces key[CAP - 1] and sinks through CAP - 1
//                          compare-exchanges, fully unrolled: every list index is a compile-time constant and the list
//                          never leaves the registers (no scratch).  The least k of a set do not depend on the order
//                          in which its members arrive, and keys of different rows differ: the order of a cell's
//                          records (which depends on the order in which the scatter's atomics arrived) reaches no
//                          output.  Then the stores (slot s is key[CAP - k + s]) and, in fp64 and in slot order, the
//                          mean of the k distances.
//   cloud_mean_sum_kernel<SECOND>
//                          a workgroup of 256 threads owns 1024 consecutive rows at a time, in four passes of 256; above
//                          1024 workgroups the grid stays there and workgroup g goes on to the blocks g + 1024, ...  Per
//                          row that is not NaN: the count and the sum of m (first pass) or the sum of (m - mu)^2 (second).
//                          The wave adds by an xor tree, the four waves are added in index order through LDS, and the
//                          workgroup stores one record.
//   cloud_mean_final_kernel<SECOND>
//                          one workgroup: the records in index order; (count, mu) to the workspace, then (count, mu,
//                          sigma) to the output.
// No atomics, nothing waits on another workgroup, every loop bounded: every output is a bitwise-reproducible function of
// the inputs.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add: every step of section 22
// is one operation.
#pragma clang fp contract(off)
#include "mvsn_cloud.h"

namespace mvsn {

constexpr int CK_MAX_K = 64;
constexpr int CS_THREADS = 256;
constexpr int CS_PASSES = 4;
constexpr long CS_BLOCK_ROWS = (long)CS_THREADS * CS_PASSES;
constexpr long CS_MAX_BLOCKS = 1024;
constexpr int CS_FINAL_THREADS = 64;

template <int CAP>
__global__ __launch_bounds__(CL_THREADS) void cloud_knn_kernel(
    const float *__restrict__ query, long nq, int k, int exclude_self, float inv, float r2,
    const unsigned long long *__restrict__ keys, const int *__restrict__ pop, const int *__restrict__ start,
    const floatx4 *__restrict__ records, size_t slots, long n, float *__restrict__ dist2, int64_t *__restrict__ index,
    int *__restrict__ within, double *__restrict__ mean) {
  const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= nq) return;
  const float qx = query[(size_t)i * 3], qy = query[(size_t)i * 3 + 1], qz = query[(size_t)i * 3 + 2];
  const CloudIndex ix = {keys, pop, start, slots};
  const int pad = CAP - k;                                // sentinels in front of the list
  const unsigned self = exclude_self ? (unsigned)i : 0xffffffffu;   // (rows are below 2^31: ~0 is nobody's)

  unsigned long long key[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) key[j] = j < pad ? 0ull : ~0ull;
  int count = 0;
  cloud_visit(qx, qy, qz, inv, r2, ix, records, n,
              [&](float, float, float, float d2, const floatx4 &r) {
                const unsigned row = __float_as_uint(r[3]);
                if (row == self) return;
                ++count;
                const unsigned long long cand = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)row;
                if (cand < key[CAP - 1]) {
                  key[CAP - 1] = cand;
#pragma unroll
                  for (int j = CAP - 1; j > 0; --j) {
                    const unsigned long long hi = key[j], lo = key[j - 1];
                    const bool swap = hi < lo;              // (strict: a sentinel, or an equal key, stays where it is)
                    key[j] = swap ? lo : hi;
                    key[j - 1] = swap ? hi : lo;
                  }
                }
              });
  within[i] = count;

  float *od = dist2 + (size_t)i * (size_t)k;
  int64_t *oi = index + (size_t)i * (size_t)k;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const int s = j - pad;
    if (s >= 0) {
      const bool any = key[j] != ~0ull;
      const float d2 = any ? __uint_as_float((unsigned)(key[j] >> 32)) : __builtin_inff();
      od[s] = d2;
      oi[s] = any ? (int64_t)(unsigned)(key[j] & 0xffffffffull) : (int64_t)-1;
      if (mean) sum = sum + sqrt((double)d2);
    }
  }
  if (mean) mean[i] = count >= k ? sum / (double)k : (double)NAN;
}

// the sum of v over the workgroup in a fixed order: an xor tree in the wave (every lane ends with the same bits), then
// the waves in index order; thread 0 has it
__device__ __forceinline__ double mean_block_sum(double v, double *swave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  __syncthreads();                                        // (swave may still be read from the call before)
  if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((swave[0] + swave[1]) + swave[2]) + swave[3];
}

// SECOND false: record (count, sum m).  SECOND true: record sum (m - mu)^2 with mu = head[1].
template <bool SECOND>
__global__ __launch_bounds__(CS_THREADS) void cloud_mean_sum_kernel(const double *__restrict__ m, long n, long blocks,
                                                                    const double *__restrict__ head,
                                                                    double *__restrict__ rec) {
  __shared__ double swave[CS_THREADS / 64];
  const double mu = SECOND ? head[1] : 0.0;
  double acc = 0.0, cnt = 0.0;
#pragma unroll 1
  for (long block = blockIdx.x; block < blocks; block += gridDim.x) {
#pragma unroll 1
    for (int pass = 0; pass < CS_PASSES; ++pass) {
      const long i = block * CS_BLOCK_ROWS + (long)pass * CS_THREADS + threadIdx.x;
      if (i >= n) continue;                                 // (no barrier inside the loops)
      const double v = m[i];
      if (v != v) continue;
      if (SECOND) {
        const double d = v - mu;
        acc = acc + d * d;
      } else {
        acc = acc + v;
        cnt = cnt + 1.0;
      }
    }
  }
  const double total = mean_block_sum(acc, swave);
  if (SECOND) {
    if (threadIdx.x == 0) rec[blockIdx.x] = total;
  } else {
    const double count = mean_block_sum(cnt, swave);
    if (threadIdx.x == 0) rec[(size_t)blockIdx.x * 2] = count, rec[(size_t)blockIdx.x * 2 + 1] = total;
  }
}

// One workgroup; thread 0 adds the records in index order.  SECOND false: head = (count, mu).  SECOND true: stats =
// (count, mu, sigma) from head and the records of the second pass.
template <bool SECOND>
__global__ __launch_bounds__(CS_FINAL_THREADS) void cloud_mean_final_kernel(const double *__restrict__ rec, int n_records,
                                                                            double *head, double *__restrict__ stats) {
  if (threadIdx.x != 0) return;
  if (SECOND) {
    double s = 0.0;
    for (int g = 0; g < n_records; ++g) s = s + rec[g];
    const double count = head[0];
    stats[0] = count;
    stats[1] = head[1];
    stats[2] = count < 2.0 ? 0.0 : sqrt(s / (count - 1.0));
  } else {
    double count = 0.0, s = 0.0;
    for (int g = 0; g < n_records; ++g) count = count + rec[(size_t)g * 2], s = s + rec[(size_t)g * 2 + 1];
    head[0] = count;
    head[1] = count < 1.0 ? (double)NAN : s / count;
  }
}

struct MeanLayout {
  size_t head, first, second, bytes;
  long blocks, groups;
};

inline MeanLayout mean_layout(long n) {
  MeanLayout l;
  l.blocks = (n + CS_BLOCK_ROWS - 1) / CS_BLOCK_ROWS;
  l.groups = l.blocks < CS_MAX_BLOCKS ? l.blocks : CS_MAX_BLOCKS;
  l.head = 0;
  l.first = align256(l.head + 2 * sizeof(double));
  l.second = align256(l.first + 2 * sizeof(double) * (size_t)l.groups);
  l.bytes = align256(l.second + sizeof(double) * (size_t)l.groups);
  return l;
}

template <int CAP>
static void launch_knn(const float *query, long nq, int k, int exclude_self, float inv, float r2, const CloudIndex &ix,
                       const floatx4 *records, long n_target, float *dist2, int64_t *index, int *within, double *mean,
                       hipStream_t st) {
  hipLaunchKernelGGL(cloud_knn_kernel<CAP>, dim3((unsigned)((nq + CL_THREADS - 1) / CL_THREADS)), dim3(CL_THREADS), 0, st,
                     query, nq, k, exclude_self, inv, r2, ix.keys, ix.pop, ix.start, records, ix.slots, n_target, dist2, index,
                     within, mean);
}

}  // namespace mvsn

extern "C" int mvsn_cloud_knn(const float *query, long nq, int k, int exclude_self, float cell, float inv_cell, float r2,
                              const void *index_workspace, size_t index_workspace_bytes, long n_target, float *dist2,
                              int64_t *index, int *within, double *mean, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_knn";
  MVSN_REQUIRE(query && dist2 && index && within, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(nq > 0 && n_target > 0, MVSN_E_BADARG, "%s: %ld queries against %ld points", who, nq, n_target);
  MVSN_REQUIRE(k >= 1 && k <= CK_MAX_K, MVSN_E_BADARG, "%s: k = %d (1 to %d)", who, k, CK_MAX_K);
  MVSN_REQUIRE(cell > 0.0f && cell <= 3.0e38f && inv_cell > 0.0f && inv_cell <= 3.0e38f && r2 > 0.0f && r2 <= 3.0e38f,
               MVSN_E_BADARG, "%s: cell size %g, its inverse %g or squared radius %g is not a positive finite number", who,
               (double)cell, (double)inv_cell, (double)r2);
  MVSN_REQUIRE(nq <= 0x7fffffffL && n_target <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld queries against %ld points (at most 2^31 - 1 each)", who, nq, n_target);
  CloudLayout l;
  if (int e = cloud_index_check(who, "index workspace", index_workspace, index_workspace_bytes, n_target, &l)) return e;
  const floatx4 *records;
  const CloudIndex ix = cloud_index(index_workspace, l, &records);
  const hipStream_t st = (hipStream_t)stream;
  const int self = exclude_self ? 1 : 0;
  if (k <= 8)
    launch_knn<8>(query, nq, k, self, inv_cell, r2, ix, records, n_target, dist2, index, within, mean, st);
  else if (k <= 16)
    launch_knn<16>(query, nq, k, self, inv_cell, r2, ix, records, n_target, dist2, index, within, mean, st);
  else if (k <= 32)
    launch_knn<32>(query, nq, k, self, inv_cell, r2, ix, records, n_target, dist2, index, within, mean, st);
  else
    launch_knn<64>(query, nq, k, self, inv_cell, r2, ix, records, n_target, dist2, index, within, mean, st);
  return check_launch("mvsn_cloud_knn: knn");
}

extern "C" size_t mvsn_cloud_mean_stats_workspace_bytes(long n) {
  if (n <= 0 || n > 0x7fffffffL) return 0;
  return mvsn::mean_layout(n).bytes;
}

extern "C" int mvsn_cloud_mean_stats(const double *mean, long n, void *workspace, size_t workspace_bytes, double *stats,
                                     mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_mean_stats";
  MVSN_REQUIRE(mean && stats, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(n > 0, MVSN_E_BADARG, "%s: %ld rows", who, n);
  MVSN_REQUIRE(n <= 0x7fffffffL, MVSN_E_TOOLARGE, "%s: %ld rows (at most 2^31 - 1)", who, n);
  const MeanLayout l = mean_layout(n);
  MVSN_REQUIRE(workspace && workspace_bytes >= l.bytes, MVSN_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               workspace_bytes, l.bytes);
  MVSN_REQUIRE(((uintptr_t)workspace & 15) == 0, MVSN_E_BADARG, "%s: workspace not 16-byte aligned", who);
  char *ws = (char *)workspace;
  double *head = (double *)(ws + l.head), *first = (double *)(ws + l.first), *second = (double *)(ws + l.second);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)l.groups), one(1);
  hipLaunchKernelGGL(cloud_mean_sum_kernel<false>, grid, dim3(CS_THREADS), 0, st, mean, n, l.blocks,
                     (const double *)nullptr, first);
  if (int e = check_launch("mvsn_cloud_mean_stats: sums")) return e;
  hipLaunchKernelGGL(cloud_mean_final_kernel<false>, one, dim3(CS_FINAL_THREADS), 0, st, (const double *)first,
                     (int)l.groups, head, (double *)nullptr);
  if (int e = check_launch("mvsn_cloud_mean_stats: mean")) return e;
  hipLaunchKernelGGL(cloud_mean_sum_kernel<true>, grid, dim3(CS_THREADS), 0, st, mean, n, l.blocks, (const double *)head,
                     second);
  if (int e = check_launch("mvsn_cloud_mean_stats: squares")) return e;
  hipLaunchKernelGGL(cloud_mean_final_kernel<true>, one, dim3(CS_FINAL_THREADS), 0, st, (const double *)second,
                     (int)l.groups, head, stats);
  return check_launch("mvsn_cloud_mean_stats: deviation");
}
