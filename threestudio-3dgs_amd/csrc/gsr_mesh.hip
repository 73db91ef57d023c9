// gsr_mesh.hip — the geometry of mesh-bound SuGaR Gaussians, forward and backward (include/gsr.h gsr_sugar_mesh_*;
// replaces SuGaRModel.points / .scaling / .quaternions / .get_gs_normals of geometry/sugar.py:449-536, their (F, 3, 3)
// vertex gather, the pytorch3d face normals, matrix_to_quaternion and the index_put scatter of the autograd backward).
//
// Gaussian f G + g belongs to face f with corners p0, p1, p2 (normalize(v, eps) = v / max(|v|, eps)):
//     c = (p1 - p0) x (p2 - p0);  n = normalize(c, 1e-6);  R0 = normalize(n, 1e-12)        (face_normal, gsr_sugar.h)
//     b1 = normalize(p0 - p1, 1e-12);  b2 = normalize(R0 x b1, 1e-12)
//     z = normalize(complex, 1e-12);  R1 = z0 b1 + z1 b2;  R2 = -z1 b1 + z0 b2;  q = matrix_to_quaternion([R0|R1|R2])
//     xyz = sum_k bary[g][k] p_k;  scaling = (thickness, exp(log_scales));  rotation = normalize(q, 1e-12)
//     normals = R0
// Precision: everything is evaluated in fp64 from the fp32 inputs, the per-face frame, the per-Gaussian part and the
// gradient arithmetic alike, and every output is rounded to fp32 once.  (The kernels are bound by their 52 bytes of
// output per Gaussian and the matching gradient reads; the fp64 arithmetic is a few hundred operations per Gaussian.)
// The corner rows of the backward are fp32 (one rounding each); the per-vertex sum adds them in fp64 and rounds once.
//
// Kernels:
//   k_mesh_forward  one lane per Gaussian: the lanes of a face read the same three vertices (one request), every
//                   lane rebuilds the frame and stores its own 13 floats, so a wave's stores cover a contiguous range
//                   of each output.  Nothing is kept for the backward.
//   k_mesh_face     one lane per face: rebuilds the frame once, walks the face's Gaussians in ascending g (writing
//                   dL/dcomplex and dL/dlog_scales), sums their gradients to the frame and to the corners in that
//                   order, carries the sum through the frame and stores three corner rows (36 bytes per face).
//   k_mesh_vertex   one lane per vertex: adds its incident corner rows in corner_order (its row of the incidence
//                   table: row_range, gsr_sugar.h), from 0, writes dL/dverts.
// No atomics: every sum's order is fixed by the input.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

struct MeshFrame : FaceNormal {
  D3 p0, p1, p2;
  D3 d, b1, m, b2;
};

// the face's corners; false (nothing dereferenced) when an index is outside [0, V)
__device__ __forceinline__ bool mesh_corners(const MeshCall& a, int f, MeshFrame& fr) {
  int i[3];
  if (!face_corners(a.faces, a.V, f, i)) return false;
  fr.p0 = load3(a.verts + 3 * (size_t)i[0]);
  fr.p1 = load3(a.verts + 3 * (size_t)i[1]);
  fr.p2 = load3(a.verts + 3 * (size_t)i[2]);
  return true;
}

__device__ __forceinline__ void mesh_frame(MeshFrame& fr) {
  static_cast<FaceNormal&>(fr) = face_normal(fr.p0, fr.p1, fr.p2);
  fr.d = fr.p0 - fr.p1;
  fr.b1 = normalize(fr.d, 1e-12);
  fr.m = cross(fr.R0, fr.b1);
  fr.b2 = normalize(fr.m, 1e-12);
}

// matrix_to_quaternion's chosen row before its division, for M = [R0 | R1 | R2] (m_ij = row i of column j):
// t[i] the four trace combinations, `best` the index of the largest max(t, 0) (lowest on ties; the square root is
// monotone, so this is a largest a_i), a = sqrt of it, row = the candidate row (its own entry = a^2).
struct MeshQuat {
  int best;
  double a, den;  // den = 2 max(a, 0.1)
  double row[4];
};
__device__ __forceinline__ MeshQuat mesh_quat(D3 R0, D3 R1, D3 R2) {
  const double m00 = R0.x, m10 = R0.y, m20 = R0.z, m01 = R1.x, m11 = R1.y, m21 = R1.z, m02 = R2.x, m12 = R2.y,
               m22 = R2.z;
  const double t0 = fmax(1.0 + m00 + m11 + m22, 0.0), t1 = fmax(1.0 + m00 - m11 - m22, 0.0),
               t2 = fmax(1.0 - m00 + m11 - m22, 0.0), t3 = fmax(1.0 - m00 - m11 + m22, 0.0);
  MeshQuat q;
  q.best = 0;
  double t = t0;
  if (t1 > t) t = t1, q.best = 1;
  if (t2 > t) t = t2, q.best = 2;
  if (t3 > t) t = t3, q.best = 3;
  q.a = sqrt(t);
  q.den = 2.0 * fmax(q.a, 0.1);
  const double a2 = q.a * q.a;
  if (q.best == 0)
    q.row[0] = a2, q.row[1] = m21 - m12, q.row[2] = m02 - m20, q.row[3] = m10 - m01;
  else if (q.best == 1)
    q.row[0] = m21 - m12, q.row[1] = a2, q.row[2] = m10 + m01, q.row[3] = m02 + m20;
  else if (q.best == 2)
    q.row[0] = m02 - m20, q.row[1] = m10 + m01, q.row[2] = a2, q.row[3] = m12 + m21;
  else
    q.row[0] = m10 - m01, q.row[1] = m20 + m02, q.row[2] = m21 + m12, q.row[3] = a2;
  return q;
}

__global__ __launch_bounds__(256) void k_mesh_forward(MeshCall a, FaceBary bary, float thickness,
                                                      float* __restrict__ xyz, float* __restrict__ scaling,
                                                      float4* __restrict__ rotation, float* __restrict__ normals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.F * a.G) return;
  const int f = (int)(i / a.G), g = (int)(i % a.G);
  MeshFrame fr;
  if (!mesh_corners(a, f, fr)) {  // a face entry out of range: zeros
    const D3 zero = d3(0.0, 0.0, 0.0);
    store3(xyz + 3 * i, zero);
    store3(scaling + 3 * i, zero);
    store3(normals + 3 * i, zero);
    rotation[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  mesh_frame(fr);
  const float2 zc = ((const float2*)a.cplx)[i];
  const float2 ls = ((const float2*)a.log_scales)[i];
  const double w0 = (double)bary.w[g][0], w1 = (double)bary.w[g][1], w2 = (double)bary.w[g][2];
  store3(xyz + 3 * i, w0 * fr.p0 + w1 * fr.p1 + w2 * fr.p2);
  scaling[3 * i] = thickness;
  scaling[3 * i + 1] = (float)exp((double)ls.x);
  scaling[3 * i + 2] = (float)exp((double)ls.y);
  store3(normals + 3 * i, fr.R0);
  const double zx = (double)zc.x, zy = (double)zc.y;
  const double zinv = 1.0 / fmax(sqrt(fma(zy, zy, zx * zx)), 1e-12);
  const double u0 = zx * zinv, u1 = zy * zinv;
  const MeshQuat q = mesh_quat(fr.R0, u0 * fr.b1 + u1 * fr.b2, u0 * fr.b2 - u1 * fr.b1);
  double r[4];
  double nn = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r[k] = q.row[k] / q.den;
    nn = fma(r[k], r[k], nn);
  }
  const double qinv = 1.0 / fmax(sqrt(nn), 1e-12);
  rotation[i] = make_float4((float)(r[0] * qinv), (float)(r[1] * qinv), (float)(r[2] * qinv), (float)(r[3] * qinv));
}

struct MeshGrads {
  const float *g_xyz, *g_scaling, *g_rotation, *g_normals;  // any may be null (zero)
};

__global__ __launch_bounds__(256) void k_mesh_face(MeshCall a, FaceBary bary, MeshGrads up,
                                                   float2* __restrict__ dcplx, float2* __restrict__ dlog_scales,
                                                   float* __restrict__ rows) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  float* row = rows + 9 * (size_t)f;
  MeshFrame fr;
  if (!mesh_corners(a, f, fr)) {  // a face entry out of range: zero gradients
    for (int g = 0; g < a.G; ++g) {
      dcplx[(size_t)f * a.G + g] = make_float2(0.0f, 0.0f);
      dlog_scales[(size_t)f * a.G + g] = make_float2(0.0f, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) row[k] = 0.0f;
    return;
  }
  mesh_frame(fr);
  const D3 zero = d3(0.0, 0.0, 0.0);
  D3 gR0 = zero, gb1 = zero, gb2 = zero, gp0 = zero, gp1 = zero, gp2 = zero;
  for (int g = 0; g < a.G; ++g) {  // the face's Gaussians in ascending g
    const size_t i = (size_t)f * a.G + g;
    const float2 ls = ((const float2*)a.log_scales)[i];
    float2 dls = make_float2(0.0f, 0.0f);
    if (up.g_scaling != nullptr) {
      dls.x = (float)((double)up.g_scaling[3 * i + 1] * exp((double)ls.x));
      dls.y = (float)((double)up.g_scaling[3 * i + 2] * exp((double)ls.y));
    }
    dlog_scales[i] = dls;
    if (up.g_xyz != nullptr) {
      const D3 gx = load3(up.g_xyz + 3 * i);
      gp0 = gp0 + (double)bary.w[g][0] * gx;
      gp1 = gp1 + (double)bary.w[g][1] * gx;
      gp2 = gp2 + (double)bary.w[g][2] * gx;
    }
    if (up.g_normals != nullptr) gR0 = gR0 + load3(up.g_normals + 3 * i);
    float2 dz = make_float2(0.0f, 0.0f);
    if (up.g_rotation != nullptr) {
      const float2 zc = ((const float2*)a.cplx)[i];
      const double zx = (double)zc.x, zy = (double)zc.y;
      const double zlen = sqrt(fma(zy, zy, zx * zx));
      const double zinv = 1.0 / fmax(zlen, 1e-12);
      const double u0 = zx * zinv, u1 = zy * zinv;
      const MeshQuat q = mesh_quat(fr.R0, u0 * fr.b1 + u1 * fr.b2, u0 * fr.b2 - u1 * fr.b1);
      const float4 gq4 = ((const float4*)up.g_rotation)[i];
      const double gq[4] = {(double)gq4.x, (double)gq4.y, (double)gq4.z, (double)gq4.w};
      // rotation = r / max(|r|, 1e-12), r = row / den
      double r[4], nn = 0.0, rg = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r[k] = q.row[k] / q.den;
        nn = fma(r[k], r[k], nn);
        rg = fma(r[k], gq[k], rg);
      }
      const double rlen = sqrt(nn);
      double gr[4];
      if (rlen >= 1e-12) {
#pragma unroll
        for (int k = 0; k < 4; ++k) gr[k] = (gq[k] - r[k] * rg / nn) / rlen;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) gr[k] = gq[k] * 1e12;
      }
      // r = row / den: the gradients to the row and to den; den = 2 max(a, 0.1), row[best] = a^2 = t (t > 0)
      double grow[4], gden = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        grow[k] = gr[k] / q.den;
        gden = fma(-gr[k], r[k] / q.den, gden);
      }
      double gt = 0.0;  // to the chosen trace combination (sqrt_pos: no gradient at t <= 0)
      if (q.a > 0.0) gt = grow[q.best] + (q.a >= 0.1 ? gden / q.a : 0.0);
      // to the matrix entries: column 0 = R0, column 1 = R1, column 2 = R2
      double g00, g11, g22, g21 = 0.0, g12 = 0.0, g02 = 0.0, g20 = 0.0, g10 = 0.0, g01 = 0.0;
      if (q.best == 0) {
        g00 = gt, g11 = gt, g22 = gt;
        g21 = grow[1], g12 = -grow[1], g02 = grow[2], g20 = -grow[2], g10 = grow[3], g01 = -grow[3];
      } else if (q.best == 1) {
        g00 = gt, g11 = -gt, g22 = -gt;
        g21 = grow[0], g12 = -grow[0], g10 = grow[2], g01 = grow[2], g02 = grow[3], g20 = grow[3];
      } else if (q.best == 2) {
        g00 = -gt, g11 = gt, g22 = -gt;
        g02 = grow[0], g20 = -grow[0], g10 = grow[1], g01 = grow[1], g12 = grow[3], g21 = grow[3];
      } else {
        g00 = -gt, g11 = -gt, g22 = gt;
        g10 = grow[0], g01 = -grow[0], g20 = grow[1], g02 = grow[1], g21 = grow[2], g12 = grow[2];
      }
      gR0 = gR0 + d3(g00, g10, g20);
      const D3 gR1 = d3(g01, g11, g21), gR2 = d3(g02, g12, g22);
      // R1 = u0 b1 + u1 b2, R2 = u0 b2 - u1 b1
      gb1 = gb1 + (u0 * gR1 - u1 * gR2);
      gb2 = gb2 + (u1 * gR1 + u0 * gR2);
      const double gu0 = dot(gR1, fr.b1) + dot(gR2, fr.b2), gu1 = dot(gR1, fr.b2) - dot(gR2, fr.b1);
      if (zlen >= 1e-12) {
        const double ug = u0 * gu0 + u1 * gu1;
        dz = make_float2((float)((gu0 - u0 * ug) * zinv), (float)((gu1 - u1 * ug) * zinv));
      } else {
        dz = make_float2((float)(gu0 * 1e12), (float)(gu1 * 1e12));
      }
    }
    dcplx[i] = dz;
  }
  // through the frame: b2 = normalize(m), m = R0 x b1, b1 = normalize(d), d = p0 - p1, then the normal's chain
  const D3 gm = normalize_grad(gb2, fr.m, 1e-12);
  gR0 = gR0 + cross(fr.b1, gm);
  gb1 = gb1 + cross(gm, fr.R0);
  const D3 gd = normalize_grad(gb1, fr.d, 1e-12);
  gp0 = gp0 + gd;
  gp1 = gp1 - gd;
  face_normal_grad(fr, fr.p0, fr.p1, fr.p2, gR0, gp0, gp1, gp2);
  store3(row, gp0);
  store3(row + 3, gp1);
  store3(row + 6, gp2);
}

__global__ __launch_bounds__(256) void k_mesh_vertex(int V, int F, const int* __restrict__ corner_order,
                                                     const int* __restrict__ vert_offsets,
                                                     const float* __restrict__ rows, float* __restrict__ dverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const long long n = 3ll * F;
  long long b, e;
  row_range(vert_offsets, v, n, b, e);
  D3 s = d3(0.0, 0.0, 0.0);
  for (long long i = b; i < e; ++i) {
    const int co = corner_order[i];
    if (!in_range(co, n)) continue;  // not a corner: skipped
    s = s + load3(rows + 3 * (size_t)co);
  }
  store3(dverts + 3 * (size_t)v, s);
}

size_t mesh_workspace_bytes(int F, int V) {
  (void)V;
  return align_up(sizeof(float) * 9 * (size_t)(F > 0 ? F : 1), 256);
}

void launch_mesh_forward(const MeshCall& c, const float* bary, float thickness, float* xyz, float* scaling,
                         float* rotation, float* normals, hipStream_t stream) {
  const long long N = (long long)c.F * c.G;
  hipLaunchKernelGGL(k_mesh_forward, dim3(div_up(N, 256)), dim3(256), 0, stream, c, face_bary(c.G, bary), thickness,
                     xyz, scaling, (float4*)rotation, normals);
}

void launch_mesh_backward(const MeshCall& c, const float* bary, const int* corner_order, const int* vert_offsets,
                          const float* g_xyz, const float* g_scaling, const float* g_rotation, const float* g_normals,
                          float* dverts, float* dcplx, float* dlog_scales, void* workspace, hipStream_t stream) {
  float* rows = (float*)workspace;
  hipLaunchKernelGGL(k_mesh_face, dim3(div_up(c.F, 256)), dim3(256), 0, stream, c, face_bary(c.G, bary),
                     MeshGrads{g_xyz, g_scaling, g_rotation, g_normals}, (float2*)dcplx, (float2*)dlog_scales, rows);
  if (c.V > 0)
    hipLaunchKernelGGL(k_mesh_vertex, dim3(div_up(c.V, 256)), dim3(256), 0, stream, c.V, c.F, corner_order,
                       vert_offsets, rows, dverts);
}

}  // namespace gsr
