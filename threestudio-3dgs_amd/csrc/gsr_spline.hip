// gsr_spline.hip — the B-spline of the timed node (or vertex) attributes of dynamic SuGaR, forward and backward
// (include/gsr.h gsr_sugar_spline_*; replaces Spline.forward of geometry/spline_utils.py:195-332 as
// DynamicSuGaRModel.get_timed_dg_attributes calls it: the gather of degree + 1 knots per point and timestamp, pypose's
// Inv @, Log, Exp and cumprod for the rotation, the bvv outer products and sums for the translation and the scale, and
// the index_put scatter of their autograd backward).  The formulas are in the header.
//
// Segment choice: fp32, in the reference's operation order (clamp, subtract, a correctly rounded divide, floor), so
// that the knots a timestamp reads are the reference's.  Everything after it is fp64 from the fp32 inputs, every output
// and gradient rounded to fp32 once; the gradient rows that pass between the two kernels of the backward are fp64.
//
// T timestamps, P points, D = degree, knots frame-major (n_knots, P, C):
//   k_spline_forward  one lane per (t, p), p fastest: D + 1 knot rows of each attribute (coalesced over p), the chain,
//                     three stores.
//   k_spline_rows     (backward) one lane per (t, p): recomputes the chain, writes the gradient rows to its D + 1
//                     knots: rows[t][j][c][p], c = 0..2 xyz, 3..6 rotation (xyzw), 7..9 scale.
//   k_spline_knots    one lane per (knot, p): walks t = 0 .. T-1 in ascending order and adds the rows of the timestamps
//                     whose segment covers the knot, from 0; a knot no timestamp covers gets exactly 0.
// No atomics: every sum's order is fixed by the input.  The bodies are host-callable functions of an item index.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

#define GSR_SPLINE_ROW 10  // doubles per (t, p, knot of the segment): dL/dxyz (3), dL/drot (4, xyzw), dL/dscale (3)

// the first knot of timestamp t's segment, clamped to [0, n_knots - degree - 1], and the position u in it
struct SplineSeg {
  int i;
  double u;
};
GSR_HD SplineSeg spline_segment(const SplineCall& a, int t) {
  const float ts = fminf(fmaxf(a.timestamps[t], a.lo), a.hi);
#ifdef __HIP_DEVICE_COMPILE__
  const float nt = __fdiv_rn(ts - a.start, a.interval);
#else
  const float nt = (ts - a.start) / a.interval;
#endif
  // (a timestamp within the bounds is far from the int range: the clamp only keeps the conversion defined)
  const int fl = (int)fminf(fmaxf(floorf(nt), -1073741824.0f), 1073741824.0f);
  SplineSeg s;
  s.u = (double)(nt - (float)fl);
  const int i = a.degree == 3 ? fl - 1 : fl, last = a.n_knots - a.degree - 1;
  s.i = i < 0 ? 0 : (i > last ? last : i);
  return s;
}

// the weights of the D + 1 knots (xyz, scale) and, for the cubic, of the three rotation increments
template <int D>
struct SplineCoef {
  double c[D + 1], b[3];
};
template <int D>
GSR_HD SplineCoef<D> spline_coef(double u) {
  SplineCoef<D> k;
  if constexpr (D == 3) {
    const double uu = u * u, uuu = uu * u, s = 1.0 / 6.0;
    k.c[0] = s - 0.5 * u + 0.5 * uu - s * uuu;
    k.c[1] = 4.0 * s - uu + 0.5 * uuu;
    k.c[2] = s + 0.5 * u + 0.5 * uu - 0.5 * uuu;
    k.c[3] = s * uuu;
    k.b[0] = 5.0 * s + 0.5 * u - 0.5 * uu + s * uuu;
    k.b[1] = s + 0.5 * u + 0.5 * uu - 2.0 * s * uuu;
    k.b[2] = s * uuu;
  } else {
    k.c[0] = 1.0 - u;
    k.c[1] = u;
    k.b[0] = k.b[1] = k.b[2] = 0.0;
  }
  return k;
}

template <int D>
GSR_HD D3 spline_mix(const SplineCoef<D>& k, const float* knots, size_t first, size_t P) {
  D3 s = k.c[0] * load3(knots + 3 * first);
#pragma unroll
  for (int j = 1; j <= D; ++j) s = s + k.c[j] * load3(knots + 3 * (first + j * P));
  return s;
}

// The rotation chain.  Cubic: r_j = Log(conj(q_j) (x) q_j+1), E_j = Exp(b_j r_j), q = q_0 (x) E_0 (x) E_1 (x) E_2.
// Linear: q = Exp((1 - u) Log(q_0) + u Log(q_1)).
template <int D>
GSR_HD Q4 spline_rot(const SplineCoef<D>& k, const Q4* q) {
  if constexpr (D == 3) {
    Q4 r = q[0];
#pragma unroll
    for (int j = 0; j < D; ++j) r = qmul(r, qexp(k.b[j] * qlog(qmul(conj(q[j]), q[j + 1]))));
    return r;
  } else {
    return qexp(k.c[0] * qlog(q[0]) + k.c[1] * qlog(q[1]));
  }
}

// the gradients gq[0 .. D] to the knots, given the gradient g to the result
template <int D>
GSR_HD void spline_rot_grad(const SplineCoef<D>& k, const Q4* q, Q4 g, Q4* gq) {
  if constexpr (D == 3) {
    Q4 d[3], A[3];  // d_j = conj(q_j) (x) q_j+1;  A_j = q_0 (x) E_0 .. E_j-1: the product before E_j
    D3 phi[3];
    A[0] = q[0];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      d[j] = qmul(conj(q[j]), q[j + 1]);
      phi[j] = k.b[j] * qlog(d[j]);
      if (j + 1 < D) A[j + 1] = qmul(A[j], qexp(phi[j]));
    }
#pragma unroll
    for (int j = 0; j <= D; ++j) gq[j] = qzero();
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {  // g: the gradient to A_j (x) E_j
      const Q4 gd = qlog_grad(d[j], k.b[j] * qexp_grad(phi[j], qmul_grad_b(A[j], g)));
      gq[j] = gq[j] + conj(qmul_grad_a(gd, q[j + 1]));
      gq[j + 1] = gq[j + 1] + qmul_grad_b(conj(q[j]), gd);
      g = qmul_grad_a(g, qexp(phi[j]));
    }
    gq[0] = gq[0] + g;
  } else {
    const D3 gphi = qexp_grad(k.c[0] * qlog(q[0]) + k.c[1] * qlog(q[1]), g);
    gq[0] = qlog_grad(q[0], k.c[0] * gphi);
    gq[1] = qlog_grad(q[1], k.c[1] * gphi);
  }
}

template <int D>
GSR_HD void spline_point_forward(const SplineCall& a, long long idx, float* xyz, float* rot, float* scale) {
  const int t = (int)(idx / a.P), p = (int)(idx % a.P);  // idx = t P + p
  const SplineSeg s = spline_segment(a, t);
  const SplineCoef<D> k = spline_coef<D>(s.u);
  const size_t P = (size_t)a.P, first = (size_t)s.i * P + p;
  store3(xyz + 3 * idx, spline_mix<D>(k, a.knots_xyz, first, P));
  Q4 q[D + 1];
#pragma unroll
  for (int j = 0; j <= D; ++j) q[j] = load_xyzw(a.knots_rot + 4 * (first + j * P));
  store4(rot + 4 * idx, spline_rot<D>(k, q));
  if (scale != nullptr) store3(scale + 3 * idx, spline_mix<D>(k, a.knots_scale, first, P));
}

// g_xyz, g_rot, g_scale: the upstream gradients or null (zero: that part of the rows is neither written nor read)
struct SplineGrads {
  const float *g_xyz, *g_rot, *g_scale;
};

// element c of the row of (t, knot j of the segment, p)
GSR_HD size_t spline_row(int D, size_t P, int t, int j, int c, int p) {
  return (((size_t)t * (D + 1) + j) * GSR_SPLINE_ROW + c) * P + p;
}

template <int D>
GSR_HD void spline_point_backward(const SplineCall& a, const SplineGrads& up, long long idx, double* rows) {
  const int t = (int)(idx / a.P), p = (int)(idx % a.P);
  const SplineSeg s = spline_segment(a, t);
  const SplineCoef<D> k = spline_coef<D>(s.u);
  const size_t P = (size_t)a.P, first = (size_t)s.i * P + p;
  if (up.g_xyz != nullptr) {
    const D3 g = load3(up.g_xyz + 3 * idx);
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      rows[spline_row(D, P, t, j, 0, p)] = k.c[j] * g.x;
      rows[spline_row(D, P, t, j, 1, p)] = k.c[j] * g.y;
      rows[spline_row(D, P, t, j, 2, p)] = k.c[j] * g.z;
    }
  }
  if (up.g_rot != nullptr) {
    Q4 q[D + 1], gq[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) q[j] = load_xyzw(a.knots_rot + 4 * (first + j * P));
    spline_rot_grad<D>(k, q, load_xyzw(up.g_rot + 4 * idx), gq);
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      rows[spline_row(D, P, t, j, 3, p)] = gq[j].v.x;
      rows[spline_row(D, P, t, j, 4, p)] = gq[j].v.y;
      rows[spline_row(D, P, t, j, 5, p)] = gq[j].v.z;
      rows[spline_row(D, P, t, j, 6, p)] = gq[j].w;
    }
  }
  if (up.g_scale != nullptr) {
    const D3 g = load3(up.g_scale + 3 * idx);
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      rows[spline_row(D, P, t, j, 7, p)] = k.c[j] * g.x;
      rows[spline_row(D, P, t, j, 8, p)] = k.c[j] * g.y;
      rows[spline_row(D, P, t, j, 9, p)] = k.c[j] * g.z;
    }
  }
}

GSR_HD void spline_knot_backward(const SplineCall& a, const SplineGrads& up, long long idx, const double* rows,
                                 float* dxyz, float* drot, float* dscale) {
  const int knot = (int)(idx / a.P), p = (int)(idx % a.P);  // idx = knot P + p
  const int D = a.degree;
  const size_t P = (size_t)a.P;
  D3 sx = d3(0.0, 0.0, 0.0), ss = sx;
  Q4 sq = qzero();
  for (int t = 0; t < a.T; ++t) {  // the timestamps in ascending t
    const int j = knot - spline_segment(a, t).i;
    if (j < 0 || j > D) continue;  // the segment does not cover the knot
    if (up.g_xyz != nullptr)
      sx = sx + d3(rows[spline_row(D, P, t, j, 0, p)], rows[spline_row(D, P, t, j, 1, p)],
                   rows[spline_row(D, P, t, j, 2, p)]);
    if (up.g_rot != nullptr)
      sq = sq + q4(d3(rows[spline_row(D, P, t, j, 3, p)], rows[spline_row(D, P, t, j, 4, p)],
                      rows[spline_row(D, P, t, j, 5, p)]),
                   rows[spline_row(D, P, t, j, 6, p)]);
    if (up.g_scale != nullptr)
      ss = ss + d3(rows[spline_row(D, P, t, j, 7, p)], rows[spline_row(D, P, t, j, 8, p)],
                   rows[spline_row(D, P, t, j, 9, p)]);
  }
  store3(dxyz + 3 * idx, sx);
  store4(drot + 4 * idx, sq);
  if (dscale != nullptr) store3(dscale + 3 * idx, ss);
}

template <int D>
__global__ __launch_bounds__(256) void k_spline_forward(SplineCall a, float* __restrict__ xyz, float* __restrict__ rot,
                                                        float* __restrict__ scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.P) spline_point_forward<D>(a, i, xyz, rot, scale);
}

template <int D>
__global__ __launch_bounds__(256) void k_spline_rows(SplineCall a, SplineGrads up, double* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.P) spline_point_backward<D>(a, up, i, rows);
}

__global__ __launch_bounds__(256) void k_spline_knots(SplineCall a, SplineGrads up, const double* __restrict__ rows,
                                                      float* __restrict__ dxyz, float* __restrict__ drot,
                                                      float* __restrict__ dscale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.n_knots * a.P) spline_knot_backward(a, up, i, rows, dxyz, drot, dscale);
}

size_t spline_workspace_bytes(int T, int P, int degree) {
  return align_up(sizeof(double) * GSR_SPLINE_ROW * (size_t)(degree == 3 ? 4 : 2) * (size_t)(T > 0 ? T : 1) *
                      (size_t)(P > 0 ? P : 1),
                  256);
}

void launch_spline_forward(const SplineCall& c, float* xyz, float* rot, float* scale, hipStream_t stream) {
  const dim3 grid(div_up((long long)c.T * c.P, 256));
  float* sc = c.knots_scale != nullptr ? scale : nullptr;
  if (c.degree == 3)
    hipLaunchKernelGGL(k_spline_forward<3>, grid, dim3(256), 0, stream, c, xyz, rot, sc);
  else
    hipLaunchKernelGGL(k_spline_forward<1>, grid, dim3(256), 0, stream, c, xyz, rot, sc);
}

void launch_spline_backward(const SplineCall& c, const float* g_xyz, const float* g_rot, const float* g_scale,
                            float* dknots_xyz, float* dknots_rot, float* dknots_scale, void* workspace,
                            hipStream_t stream) {
  double* rows = (double*)workspace;
  const bool scales = c.knots_scale != nullptr;
  const SplineGrads up{g_xyz, g_rot, scales ? g_scale : nullptr};
  const dim3 grid(div_up((long long)c.T * c.P, 256));
  if (c.degree == 3)
    hipLaunchKernelGGL(k_spline_rows<3>, grid, dim3(256), 0, stream, c, up, rows);
  else
    hipLaunchKernelGGL(k_spline_rows<1>, grid, dim3(256), 0, stream, c, up, rows);
  hipLaunchKernelGGL(k_spline_knots, dim3(div_up((long long)c.n_knots * c.P, 256)), dim3(256), 0, stream, c, up, rows,
                     dknots_xyz, dknots_rot, scales ? dknots_scale : nullptr);
}

}  // namespace gsr
