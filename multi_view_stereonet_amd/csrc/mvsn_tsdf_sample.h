// The sample of the dense TSDF volume that the ray-cast (mvsn_tsdf_raycast.hip) and the alignment
// (mvsn_tsdf_align.hip, section 17) share: the plane d = sdf_sum / weight, the 8 corners of a cell, the trilinear
// interpolant and its analytic gradient, and the limits both entries check.  Every file that includes this has
// contraction off: each fused multiply-add is written as fmaf, every other step is one fp32 operation.
#pragma once
#include <math.h>

#include "mvsn_common.h"
#include "mvsn_geom.h"

namespace mvsn {

constexpr int TR_THREADS = 256;
constexpr int TR_VOX = 4;                               // voxels per thread of the values pass: one 16-byte access
constexpr float TR_FLT_MAX = 3.4028234e38f;
constexpr int TR_MAX_EXTENT = 1 << 24;                  // rows, cols, dims and k up to here: every index is an exact fp32

// Defined in mvsn_tsdf_raycast.hip: the plane d = sdf_sum / weight (one IEEE division, the quotient the mesh extraction
// classifies by) with a NaN where weight < min_weight; launch ceil(ceil(n / TR_VOX) / TR_THREADS) workgroups.
__global__ __launch_bounds__(TR_THREADS) void tsdf_values_kernel(const float *__restrict__ sdf_sum,
                                                                 const float *__restrict__ weight, long n,
                                                                 float min_weight, float *__restrict__ d);

// the 8 values of the cell whose lowest corner is at `at`: v[c], c = dx + 2 dy + 4 dz (the compiler fetches each
// x-adjacent pair with one 8-byte load: four loads per cell)
__device__ __forceinline__ void cell_load(const float *__restrict__ p, long at, long nx, long nxy, float *v) {
  v[0] = p[at], v[1] = p[at + 1], v[2] = p[at + nx], v[3] = p[at + nx + 1];
  v[4] = p[at + nxy], v[5] = p[at + nxy + 1], v[6] = p[at + nxy + nx], v[7] = p[at + nxy + nx + 1];
}

__device__ __forceinline__ float lerp(float fr, float lo, float hi) { return fmaf(fr, hi - lo, lo); }

// the trilinear interpolant: along x, then y, then z
__device__ __forceinline__ float trilinear(const float *v, float fx, float fy, float fz) {
  const float x00 = lerp(fx, v[0], v[1]), x10 = lerp(fx, v[2], v[3]);
  const float x01 = lerp(fx, v[4], v[5]), x11 = lerp(fx, v[6], v[7]);
  return lerp(fz, lerp(fy, x00, x10), lerp(fy, x01, x11));
}

// the gradient of the trilinear interpolant: per axis the bilinear interpolant of the four differences along it
__device__ __forceinline__ void trilinear_gradient(const float *v, float fx, float fy, float fz, float *grad) {
  grad[0] = lerp(fz, lerp(fy, v[1] - v[0], v[3] - v[2]), lerp(fy, v[5] - v[4], v[7] - v[6]));
  grad[1] = lerp(fz, lerp(fx, v[2] - v[0], v[3] - v[1]), lerp(fx, v[6] - v[4], v[7] - v[5]));
  grad[2] = lerp(fy, lerp(fx, v[4] - v[0], v[5] - v[1]), lerp(fx, v[6] - v[2], v[7] - v[3]));
}

inline bool raycast_dims_ok(int nx, int ny, int nz) {
  return nx > 0 && ny > 0 && nz > 0 && nx <= TR_MAX_EXTENT && ny <= TR_MAX_EXTENT && nz <= TR_MAX_EXTENT &&
         (long)nx * ny <= 0x7fffffffL && (long)nx * ny * nz <= 0x7fffffffL;
}

inline bool raycast_positive(float x) { return x > 0.0f && x <= TR_FLT_MAX; }

}  // namespace mvsn
