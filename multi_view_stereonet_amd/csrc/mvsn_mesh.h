// What the mesh kernels share (DESIGN.md sections 18 and 26 to 29: mvsn_mesh.hip, mvsn_mesh_sample.hip,
// mvsn_mesh_nearest.hip, mvsn_mesh_render.hip, mvsn_mesh_simplify.hip, mvsn_mesh_edges.hip, mvsn_mesh_smooth.hip): the
// largest mesh, the one test that decides whether a face takes part, the load of its vertices, the rotation that makes
// a face's bits independent of the corner it starts with, the fp64 cross product, and the interpolation of vertex normals
// and colours at barycentric weights.
//
// Taking part, stated once: a face whose three rows lie in [0, m) takes part in the integer entries (components, edges,
// the simplifier's face set); in every other entry its nine coordinates must be finite as well.  A face that takes no
// part is skipped, and nothing beyond its own row of `faces` is dereferenced.
// NOT here, on purpose: smooth_ends (mvsn_mesh_smooth.hip) loads an edge, not a face, and nearest_face_box
// (mvsn_mesh_nearest.hip) interleaves the vertex load with its box arithmetic; both keep their loads.
#pragma once
#include "mvsn_common.h"

namespace mvsn {

constexpr long MESH_MAX_ROWS = 0x7fffffffL;             // vertices, faces, samples, queries: a row is an int32

// The three rows of face i as they stand in the int64 tensor; false when one lies outside [0, m).  The compare is on
// the 64-bit value: a row of 2^40 has a valid low word, so a caller narrows to int or long only after a true result.
__device__ __forceinline__ bool face_rows(const int64_t *__restrict__ faces, long i, long m, int64_t *r) {
  r[0] = faces[i * 3], r[1] = faces[i * 3 + 1], r[2] = faces[i * 3 + 2];
  return r[0] >= 0 && r[0] < m && r[1] >= 0 && r[1] < m && r[2] >= 0 && r[2] < m;
}

// The lowest of three rows rotated to the front: the winding stays, and what is computed from `row` does not depend
// on which corner the face happens to start with.  A tie goes to the earlier corner (a face with two equal rows has a
// cross product of exactly zero whichever way it is turned).  The simplifier's canonical triple of three DISTINCT
// cluster ids is the same function on int: without a tie, <= and < agree.
template <class I>
__device__ __forceinline__ void face_lead(const I *in, I *row) {
  const bool lead0 = in[0] <= in[1] && in[0] <= in[2], lead1 = !lead0 && in[1] <= in[2];
  row[0] = lead0 ? in[0] : lead1 ? in[1] : in[2];
  row[1] = lead0 ? in[1] : lead1 ? in[2] : in[0];
  row[2] = lead0 ? in[2] : lead1 ? in[0] : in[1];
}

// p[j][k] = coordinate k of vertex r[j], as float or widened to double (exact); false when one is not finite.  The rows
// are inside [0, m): face_rows said so.
template <class T>
__device__ __forceinline__ bool face_points(const float *__restrict__ vertices, const int64_t *r, T (*p)[3]) {
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = vertices[r[j] * 3 + k];
      finite = finite && isfinite(x);
      p[j][k] = (T)x;
    }
  return finite;
}

// face_rows, then face_points: whether face i takes part in an entry that reads its vertices
template <class T>
__device__ __forceinline__ bool face_load(const float *__restrict__ vertices, long m, const int64_t *__restrict__ faces,
                                          long i, int64_t *r, T (*p)[3]) {
  return face_rows(faces, i, m, r) && face_points(vertices, r, p);
}

// c = (p1 - p0) x (p2 - p0) in fp64, every step one correctly rounded operation: contraction is off inside, whatever
// the file that includes it is compiled with.
__device__ __forceinline__ void face_cross(const double (*p)[3], double *c) {
#pragma clang fp contract(off)
  const double ab[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
  const double ac[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
  c[0] = ab[1] * ac[2] - ab[2] * ac[1];
  c[1] = ab[2] * ac[0] - ab[0] * ac[2];
  c[2] = ab[0] * ac[1] - ab[1] * ac[0];
}

// the weighted sum of the three vertex normals in fp64, left to right, divided by its length; (0,0,0) where the length is
// 0 or not finite, and where !ok (nothing is dereferenced then).  A sample writes `out` as a row, a pixel as planes.
__device__ __forceinline__ void face_normal(const float *__restrict__ normals, const int64_t *r, const double *w, bool ok,
                                            float *out) {
#pragma clang fp contract(off)
  double s[3] = {0.0, 0.0, 0.0};
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      s[k] = (w[0] * (double)normals[r[0] * 3 + k] + w[1] * (double)normals[r[1] * 3 + k]) +
             w[2] * (double)normals[r[2] * 3 + k];
  }
  const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  const bool defined = ok && len > 0.0 && isfinite(len);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = defined ? (float)(s[k] / len) : 0.0f;
}

// the weighted sum of the three vertex colours, floor(x + 0.5), clamped to 0..255; (0,0,0) where !ok
__device__ __forceinline__ void face_color(const uint8_t *__restrict__ colors, const int64_t *r, const double *w, bool ok,
                                           uint8_t *out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double x = 0.0;
    if (ok)
      x = (w[0] * (double)colors[r[0] * 3 + k] + w[1] * (double)colors[r[1] * 3 + k]) + w[2] * (double)colors[r[2] * 3 + k];
    const double y = floor(x + 0.5);
    out[k] = (uint8_t)(y > 0.0 ? (y < 255.0 ? y : 255.0) : 0.0);
  }
}

}  // namespace mvsn
