// The pinhole camera that the TSDF integration (mvsn_tsdf.hip) and the cloud render
// (mvsn_cloud_render.hip, section 25) project with: one 3x4 per view, staged in LDS by the kernels that use it.
#pragma once
#include "mvsn_geom.h"

namespace mvsn {

constexpr int TS_CAM = 12;                              // floats per camera: P = K T^-1 (3x4), row 2 = T^-1's (z)

// P = K T^-1 of one view, fp64, rounded once; K's bottom row is taken to be (0,0,1), so row 2 is T^-1's own.  Every
// step is one correctly rounded operation: contraction is off inside, whatever the file that includes it is compiled
// with.
__device__ inline void tsdf_camera(const float *K, const float *T, float *out) {
#pragma clang fp contract(off)
  double Ai[9], Ti[12];
  inv3_d(T, Ai);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int n = 0; n < 3; ++n) Ti[m * 4 + n] = Ai[m * 3 + n];
    Ti[m * 4 + 3] = -(Ai[m * 3 + 0] * (double)T[3] + Ai[m * 3 + 1] * (double)T[7] + Ai[m * 3 + 2] * (double)T[11]);
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    out[0 + n] = (float)(((double)K[0] * Ti[n] + (double)K[1] * Ti[4 + n]) + (double)K[2] * Ti[8 + n]);
    out[4 + n] = (float)(((double)K[4] * Ti[n] + (double)K[5] * Ti[4 + n]) + (double)K[6] * Ti[8 + n]);
    out[8 + n] = (float)Ti[8 + n];
  }
}

}  // namespace mvsn
