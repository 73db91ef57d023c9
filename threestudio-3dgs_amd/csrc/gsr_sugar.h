// gsr_sugar.h — what the SuGaR geometry stages share (gsr_mesh.hip, gsr_dynamic.hip, gsr_arap.hip): the barycentric
// table, the face normal and its adjoint, the rows of an incidence table and the fp64 wave sums of vectors.
#pragma once

#include "../../include/gsr.h"
#include "gsr_math.h"
#include "gsr_wave.h"

namespace gsr {

// bary (G, 3) as a kernel argument
struct FaceBary {
  float w[GSR_MESH_MAX_G][3];
};
static inline FaceBary face_bary(int G, const float* bary) {  // (host memory: it travels in the kernel arguments)
  FaceBary b{};
  for (int g = 0; g < G; ++g)
    for (int k = 0; k < 3; ++k) b.w[g][k] = bary[3 * g + k];
  return b;
}

// k is an index into n entries
GSR_HD bool in_range(int k, long long n) { return (unsigned)k < (unsigned)n; }

// the corners of face f; false when one is outside [0, V): the caller then dereferences nothing of the face
GSR_HD bool face_corners(const int* faces, int V, int f, int (&i)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) i[c] = faces[3 * (size_t)f + c];
  return in_range(i[0], V) && in_range(i[1], V) && in_range(i[2], V);
}

// c = (p1 - p0) x (p2 - p0);  n = normalize(c, 1e-6);  R0 = normalize(n, 1e-12): the unit normal, 0 for a degenerate
// face
struct FaceNormal {
  D3 c, n, R0;
};
GSR_HD FaceNormal face_normal(D3 p0, D3 p1, D3 p2) {
  FaceNormal f;
  f.c = cross(p1 - p0, p2 - p0);
  f.n = normalize(f.c, 1e-6);
  f.R0 = normalize(f.n, 1e-12);
  return f;
}
// adds to g0, g1, g2 the gradients to the corners, given the gradient gR0 to R0
GSR_HD void face_normal_grad(const FaceNormal& f, D3 p0, D3 p1, D3 p2, D3 gR0, D3& g0, D3& g1, D3& g2) {
  const D3 gc = normalize_grad(normalize_grad(gR0, f.n, 1e-12), f.c, 1e-6);
  const D3 e1 = p1 - p0, e2 = p2 - p0;
  const D3 ge1 = cross(e2, gc), ge2 = cross(gc, e1);
  g1 = g1 + ge1;
  g2 = g2 + ge2;
  g0 = g0 - (ge1 + ge2);
}

// Row i of an incidence table over n entries (offsets: one more than rows): [b, e) clamped to [0, n].  The walkers
// skip an entry that is not in_range(entry, n).
GSR_HD void row_range(const int* offsets, int i, long long n, long long& b, long long& e) {
  b = offsets[i], e = offsets[i + 1];
  b = b < 0 ? 0 : b;
  e = e > n ? n : e;
}

__device__ __forceinline__ D3 wave_sum_d3(D3 a) {
  return d3(wave_sum_f64(a.x), wave_sum_f64(a.y), wave_sum_f64(a.z));
}
__device__ __forceinline__ Q4 wave_sum_q4(Q4 a) { return q4(wave_sum_d3(a.v), wave_sum_f64(a.w)); }

}  // namespace gsr
