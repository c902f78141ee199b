// Nearest neighbours in descriptor space (see include/mvsn_hip.h: mvsn_cloud_feature_nearest, mvsn_cloud_feature_mutual;
// the semantics are DESIGN.md section 23).
//
//   feature_nearest_kernel  a workgroup of eight waves owns 64 query rows, lane l of every wave query l with its 33
//                           values in registers (10^4 queries are 160 workgroups: one wave each would leave most of
//                           the chip idle).  The target rows go through LDS in tiles of 256 rows (33 KiB), staged with
//                           coalesced loads; the flag "this row takes part" (all 33 values finite, one of them not
//                           zero) is formed once per staged row (a stride of 33 words, no bank conflict).  Wave w takes
//                           rows w, w + 8, ... of the tile; in its distance loop every lane reads the same LDS
//                           word at a time, which broadcasts.  d2 = sum_b (q_b - t_b)^2 from b = 0 upwards, one fp32
//                           operation per step.  The thread keeps the two least 64-bit keys (d2 bits << 32 | row): the
//                           least is the nearest with ties to the lowest row, as cloud_walk packs it; the second serves
//                           a ratio test.  The eight waves' pairs are merged through LDS at the end.  The least two of a
//                           set of distinct keys do not depend on the order in which its members are seen.
//   feature_mutual_kernel   mutual[i] = back[index[i]] == i.
// No atomics, nothing waits on another workgroup: every output is a bitwise-reproducible function of the inputs.
//
// Contraction is off for the whole file and nothing here is written as a fused multiply-add.
#pragma clang fp contract(off)
#include "mvsn_common.h"

namespace mvsn {

constexpr int FM_DIM = 33;
constexpr int FM_QUERIES = 64;                            // query rows of a workgroup: one per lane
constexpr int FM_WAVES = 8;                               // each takes every eighth row of a tile for the same 64 queries
constexpr int FM_THREADS = FM_QUERIES * FM_WAVES;
constexpr int FM_TILE = 256;
constexpr int FM_MUTUAL_THREADS = 256;

__global__ __launch_bounds__(FM_THREADS) void feature_nearest_kernel(const float *__restrict__ query, long nq,
                                                                     const float *__restrict__ target, long nt,
                                                                     int64_t *__restrict__ index, float *__restrict__ dist2,
                                                                     float *__restrict__ second_dist2) {
  __shared__ float tile[FM_TILE * FM_DIM];
  __shared__ int live[FM_TILE];
  __shared__ unsigned long long merge[FM_WAVES][FM_QUERIES][2];
  const int tid = threadIdx.x, lane = tid & (FM_QUERIES - 1), wave = tid / FM_QUERIES;
  const long i = (long)blockIdx.x * FM_QUERIES + lane;
  const bool has = i < nq;

  float q[FM_DIM];
  bool finite = true, any = false;
#pragma unroll
  for (int b = 0; b < FM_DIM; ++b) {
    q[b] = has ? query[(size_t)i * FM_DIM + b] : 0.0f;
    finite = finite && isfinite(q[b]);
    any = any || q[b] != 0.0f;
  }
  const bool part = has && finite && any;

  unsigned long long best = ~0ull, second = ~0ull;
#pragma unroll 1
  for (long base = 0; base < nt; base += FM_TILE) {
    const int rows = (int)min((long)FM_TILE, nt - base);
    __syncthreads();                                      // (the tile may still be read from the pass before)
    for (int e = tid; e < rows * FM_DIM; e += FM_THREADS) tile[e] = target[(size_t)base * FM_DIM + e];
    __syncthreads();
    for (int r = tid; r < rows; r += FM_THREADS) {
      bool f = true, a = false;
#pragma unroll
      for (int b = 0; b < FM_DIM; ++b) {
        const float v = tile[r * FM_DIM + b];
        f = f && isfinite(v);
        a = a || v != 0.0f;
      }
      live[r] = f && a;
    }
    __syncthreads();
    if (part) {
#pragma unroll 1
      for (int r = wave; r < rows; r += FM_WAVES) {
        if (!live[r]) continue;                            // (uniform: every lane of the wave reads the same word)
        const float *t = tile + r * FM_DIM;
        float acc = 0.0f;
#pragma unroll
        for (int b = 0; b < FM_DIM; ++b) {
          const float d = q[b] - t[b];
          acc = acc + d * d;
        }
        const unsigned long long key =
            ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned long long)(unsigned)(base + r);
        if (key < best) {
          second = best;
          best = key;
        } else if (key < second) {
          second = key;
        }
      }
    }
  }
  // the two least keys of the eight waves' pairs: keys of different rows differ, so the order of the merge reaches nothing
  merge[wave][lane][0] = best, merge[wave][lane][1] = second;
  __syncthreads();
  if (wave != 0 || !has) return;
#pragma unroll
  for (int w = 1; w < FM_WAVES; ++w)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned long long key = merge[w][lane][k];
      if (key < best) {
        second = best;
        best = key;
      } else if (key < second) {
        second = key;
      }
    }
  index[i] = best != ~0ull ? (int64_t)(unsigned)(best & 0xffffffffull) : (int64_t)-1;
  dist2[i] = best != ~0ull ? __uint_as_float((unsigned)(best >> 32)) : __builtin_inff();
  second_dist2[i] = second != ~0ull ? __uint_as_float((unsigned)(second >> 32)) : __builtin_inff();
}

__global__ __launch_bounds__(FM_MUTUAL_THREADS) void feature_mutual_kernel(const int64_t *__restrict__ index, long nq,
                                                                           const int64_t *__restrict__ back, long nt,
                                                                           unsigned char *__restrict__ mutual) {
  const long i = (long)blockIdx.x * FM_MUTUAL_THREADS + threadIdx.x;
  if (i >= nq) return;
  const int64_t j = index[i];
  mutual[i] = (j >= 0 && j < (int64_t)nt && back[j] == (int64_t)i) ? 1 : 0;   // (a row outside the target is nobody's)
}

}  // namespace mvsn

extern "C" int mvsn_cloud_feature_nearest(const float *query, long nq, const float *target, long nt, int dim,
                                          int64_t *index, float *dist2, float *second_dist2, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_feature_nearest";
  MVSN_REQUIRE(query && target && index && dist2 && second_dist2, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(nq > 0 && nt > 0, MVSN_E_BADARG, "%s: %ld query rows against %ld target rows", who, nq, nt);
  MVSN_REQUIRE(dim == FM_DIM, MVSN_E_BADARG, "%s: dim = %d (only %d, the FPFH descriptor, is built)", who, dim, FM_DIM);
  MVSN_REQUIRE(nq <= 0x7fffffffL && nt <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld query rows against %ld target rows (at most 2^31 - 1 each)", who, nq, nt);
  hipLaunchKernelGGL(feature_nearest_kernel, dim3((unsigned)((nq + FM_QUERIES - 1) / FM_QUERIES)), dim3(FM_THREADS), 0,
                     (hipStream_t)stream, query, nq, target, nt, index, dist2, second_dist2);
  return check_launch("mvsn_cloud_feature_nearest: nearest");
}

extern "C" int mvsn_cloud_feature_mutual(const int64_t *index, long nq, const int64_t *back, long nt,
                                         unsigned char *mutual, mvsn_stream_t stream) {
  using namespace mvsn;
  const char *who = "mvsn_cloud_feature_mutual";
  MVSN_REQUIRE(index && back && mutual, MVSN_E_BADARG, "%s: null pointer", who);
  MVSN_REQUIRE(nq > 0 && nt > 0, MVSN_E_BADARG, "%s: %ld query rows against %ld target rows", who, nq, nt);
  MVSN_REQUIRE(nq <= 0x7fffffffL && nt <= 0x7fffffffL, MVSN_E_TOOLARGE,
               "%s: %ld query rows against %ld target rows (at most 2^31 - 1 each)", who, nq, nt);
  hipLaunchKernelGGL(feature_mutual_kernel, dim3((unsigned)((nq + FM_MUTUAL_THREADS - 1) / FM_MUTUAL_THREADS)),
                     dim3(FM_MUTUAL_THREADS), 0,
                     (hipStream_t)stream, index, nq, back, nt, mutual);
  return check_launch("mvsn_cloud_feature_mutual: mutual");
}
