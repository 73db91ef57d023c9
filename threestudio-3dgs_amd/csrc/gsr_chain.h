// gsr_chain.h — the per-(view, Gaussian) chain rule of the backward, shared by the per-Gaussian kernels of a view set
// (gsr_backward.hip) and of a timed view set (gsr_timed.hip): the gather of a Gaussian's gradient rows up to the tile
// cut-offs, conic -> 2D cov -> 3D cov and camera-space mean, the projection of the mean, 3D cov -> scale and
// quaternion.  Gradient conventions as stated at the top of gsr_backward.hip.
#pragma once

#include "gsr_kernels.h"
#include "gsr_math.h"

namespace gsr {

struct RowSums {
  float dmx, dmy, dca, dcb, dcc, dop, dcr, dcg, dcbl, ddep;
  float dmx1, dmy1, dr2, dg2, db2;  // two-colour rows (gsr_common.h BackwardState)
};

// Sum the rows of the Gaussian's instances that its tile's blend reached: the kept tiles of its
// rectangle (span_row, as emitted) whose (depth key, index) < the tile's first unblended
// instance (cut = (key, index) per tile).  Rows sit at rectangle positions.  Tiles are walked 4 at
// a time: the 4 cut tests first, then the valid rows' loads together, so a thread has up to 12
// loads in flight instead of waiting on each row in turn.
template <bool TWO>
__device__ __forceinline__ RowSums gather_rows(uint32_t idx, const GaussRec& gr, uint32_t i0, int grid_x,
                                               const uint2* cut, const float4* grow) {
  RowSums r = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  constexpr int RW = TWO ? 4 : 3;
  const uint4 gd = gr.d;
  const float4 ga = gr.a, gb = gr.b;
  const uint32_t dkey = __float_as_uint(gb.z);
  const int xmin = gd.x & 0xffff, ymin = gd.x >> 16, xmax = gd.y & 0xffff, ymax = gd.y >> 16;
  const int w = xmax - xmin;
  const SpanPrep sp = span_prep(ga.x, ga.y, ga.z, ga.w, gb.x, gb.y);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ty = ymin; ty < ymax; ++ty) {
    int t0, t1;
    span_row(sp, ty, xmin, xmax, t0, t1);  // the kept tiles of this row, as emitted
    for (int tx = t0; tx < t1; tx += 4) {
      bool val[4];
      int sl[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        val[k] = false;
        sl[k] = 0;
        if (tx + k < t1) {
          const uint2 c = cut[ty * grid_x + tx + k];
          val[k] = dkey < c.x || (dkey == c.x && idx < c.y);
          sl[k] = (ty - ymin) * w + (tx + k - xmin);
        }
      }
      float4 a[4][RW];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4* row = grow + RW * ((size_t)i0 + sl[k]);
#pragma unroll
        for (int e = 0; e < RW; ++e) a[k][e] = val[k] ? row[e] : z4;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r.dmx += a[k][0].x; r.dmy += a[k][0].y; r.dca += a[k][0].z; r.dcb += a[k][0].w;
        r.dcc += a[k][1].x; r.dop += a[k][1].y; r.dcr += a[k][1].z; r.dcg += a[k][1].w;
        r.dcbl += a[k][2].x; r.ddep += a[k][2].y;
        if (TWO) {
          r.dr2 += a[k][2].z; r.dg2 += a[k][2].w;
          r.db2 += a[k][RW - 1].x; r.dmx1 += a[k][RW - 1].y; r.dmy1 += a[k][RW - 1].z;
        }
      }
    }
  }
  return r;
}

// Camera of one view as the chain rule needs it.
struct ViewGeom {
  const float *view, *proj;
  float tanx, tany, fx, fy;
};

// computeCov2DCUDA: conic gradient -> dL/dcov3D (6, symmetric off-diagonals as scalars) and the
// camera-space-mean part of dL/dmean.
__device__ __forceinline__ void cov2d_backward(const float3 mean, const float cov3D[6], const ViewGeom& d,
                                               float dca, float dcb, float dcc, float dcov[6], float3& dmean) {
  Cov2DState st;
  const float3 cov2 = cov2d_ewa(mean, d.fx, d.fy, d.tanx, d.tany, cov3D, d.view, st);
  const float x_grad_mul = (st.txtz < -st.limx || st.txtz > st.limx) ? 0.f : 1.f;
  const float y_grad_mul = (st.tytz < -st.limy || st.tytz > st.limy) ? 0.f : 1.f;
  const float ca = cov2.x, cb = cov2.y, cc = cov2.z;
  const float denom = ca * cc - cb * cb;
  float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
  const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
  const float(&T)[2][3] = st.T;
#pragma unroll
  for (int k = 0; k < 6; ++k) dcov[k] = 0.f;
  if (denom2inv != 0.f) {
    dL_da = denom2inv * (-cc * cc * dca + 2 * cb * cc * dcb + (denom - ca * cc) * dcc);
    dL_dc = denom2inv * (-ca * ca * dcc + 2 * ca * cb * dcb + (denom - ca * cc) * dca);
    dL_db = denom2inv * 2 * (cb * cc * dca - (denom + 2 * cb * cb) * dcb + ca * cb * dcc);
    dcov[0] = (T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc);
    dcov[3] = (T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc);
    dcov[5] = (T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc);
    dcov[1] = 2 * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db +
              2 * T[1][0] * T[1][1] * dL_dc;
    dcov[2] = 2 * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db +
              2 * T[1][0] * T[1][2] * dL_dc;
    dcov[4] = 2 * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db +
              2 * T[1][1] * T[1][2] * dL_dc;
  }
  const float V[3][3] = {{cov3D[0], cov3D[1], cov3D[2]},
                         {cov3D[1], cov3D[3], cov3D[4]},
                         {cov3D[2], cov3D[4], cov3D[5]}};
  float dT0[3], dT1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float tv0 = T[0][0] * V[k][0] + T[0][1] * V[k][1] + T[0][2] * V[k][2];
    const float tv1 = T[1][0] * V[k][0] + T[1][1] * V[k][1] + T[1][2] * V[k][2];
    dT0[k] = 2 * tv0 * dL_da + tv1 * dL_db;
    dT1[k] = 2 * tv1 * dL_dc + tv0 * dL_db;
  }
  const float(&Wm)[3][3] = st.W;
  const float dJ00 = Wm[0][0] * dT0[0] + Wm[0][1] * dT0[1] + Wm[0][2] * dT0[2];
  const float dJ02 = Wm[2][0] * dT0[0] + Wm[2][1] * dT0[1] + Wm[2][2] * dT0[2];
  const float dJ11 = Wm[1][0] * dT1[0] + Wm[1][1] * dT1[1] + Wm[1][2] * dT1[2];
  const float dJ12 = Wm[2][0] * dT1[0] + Wm[2][1] * dT1[1] + Wm[2][2] * dT1[2];
  const float tz = 1.f / st.t.z, tz2 = tz * tz, tz3 = tz2 * tz;
  const float hx = d.fx, hy = d.fy;
  const float dtx = x_grad_mul * -hx * tz2 * dJ02;
  const float dty = y_grad_mul * -hy * tz2 * dJ12;
  const float dtz = -hx * tz2 * dJ00 - hy * tz2 * dJ11 + (2 * hx * st.t.x) * tz3 * dJ02 +
                    (2 * hy * st.t.y) * tz3 * dJ12;
  dmean = xform_vec4x3_T(make_float3(dtx, dty, dtz), d.view);
}

// preprocessCUDA: NDC-space mean gradient -> world-space mean through the projection.
__device__ __forceinline__ void proj_backward(const float3 mean, const float* proj, float dmx, float dmy,
                                              float3& dmean) {
  const float4 m_hom = xform_point4x4(mean, proj);
  const float m_w = 1.0f / (m_hom.w + 0.0000001f);
  const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
  const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
  dmean.x += (proj[0] * m_w - proj[3] * mul1) * dmx + (proj[1] * m_w - proj[3] * mul2) * dmy;
  dmean.y += (proj[4] * m_w - proj[7] * mul1) * dmx + (proj[5] * m_w - proj[7] * mul2) * dmy;
  dmean.z += (proj[8] * m_w - proj[11] * mul1) * dmx + (proj[9] * m_w - proj[11] * mul2) * dmy;
}

// computeCov3D backward: dL/dcov3D -> dL/d(scale_modifier * scale) and dL/d(quaternion as given).
__device__ __forceinline__ void scale_rot_backward(const float3 scale, const float4 rot, float mod,
                                                   const float dcov[6], float ds[3], float dq[4]) {
  Mat3 R;
  rot_from_quat(rot, R);
  const float s[3] = {mod * scale.x, mod * scale.y, mod * scale.z};
  // E[c][k] = s_k R[c][k];  Sigma[c][r] = sum_k E[r][k] E[c][k]; dSigma symmetric, off-diagonals split
  const float G[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                         {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                         {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
  float dE[3][3];
#pragma unroll
  for (int aa = 0; aa < 3; ++aa)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      dE[aa][k] = 2.f * (G[aa][0] * s[k] * R.m[0][k] + G[aa][1] * s[k] * R.m[1][k] + G[aa][2] * s[k] * R.m[2][k]);
  float dR[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ds[k] = dE[0][k] * R.m[0][k] + dE[1][k] * R.m[1][k] + dE[2][k] * R.m[2][k];
#pragma unroll
    for (int aa = 0; aa < 3; ++aa) dR[aa][k] = dE[aa][k] * s[k];
  }
  const float r = rot.x, x = rot.y, y = rot.z, z = rot.w;
  // d R[c][r'] / dq for R.m as built by rot_from_quat
  dq[0] = -2.f * z * dR[0][1] + 2.f * y * dR[0][2] + 2.f * z * dR[1][0] - 2.f * x * dR[1][2] -
          2.f * y * dR[2][0] + 2.f * x * dR[2][1];
  dq[1] = 2.f * y * dR[0][1] + 2.f * z * dR[0][2] + 2.f * y * dR[1][0] - 4.f * x * dR[1][1] -
          2.f * r * dR[1][2] + 2.f * z * dR[2][0] + 2.f * r * dR[2][1] - 4.f * x * dR[2][2];
  dq[2] = -4.f * y * dR[0][0] + 2.f * x * dR[0][1] + 2.f * r * dR[0][2] + 2.f * x * dR[1][0] +
          2.f * z * dR[1][2] - 2.f * r * dR[2][0] + 2.f * z * dR[2][1] - 4.f * y * dR[2][2];
  dq[3] = -4.f * z * dR[0][0] - 2.f * r * dR[0][1] + 2.f * x * dR[0][2] + 2.f * r * dR[1][0] -
          4.f * z * dR[1][1] + 2.f * y * dR[1][2] + 2.f * x * dR[2][0] + 2.f * y * dR[2][1];
}

}  // namespace gsr
