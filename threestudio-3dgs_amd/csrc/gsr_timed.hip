// gsr_timed.hip — per-Gaussian backward of a timed view set (include/gsr.h gsr_set_timed_backward).
//
// A timed set renders V views whose Gaussians each have their own position and, optionally, scale, rotation and
// second colour (the frames of dynamic SuGaR: renderer/diff_sugar_rasterizer_temporal.py:150-192 renders frame t from
// camera t).  Opacities and colours stay shared.  The blend's backward is the shared one (k_render_bwd writes the
// per-instance gradient rows and the reach bits); this file replaces k_view_grad + k_gauss_accum / k_gauss_fused.
//
// k_tv_grad, one thread per Gaussian, walks the group's views in order as k_gauss_fused does.  Per view the blend
// reached: the rows gathered up to the tile cut-offs, conic -> 2D cov -> 3D cov and camera-space mean, projection and
// depth terms, the view's means2D gradient — then, per view and not once on the summed dL/dcov3D, 3D cov -> scale and
// quaternion with THAT view's scale and rotation (the step is linear in dL/dcov3D only while the parameters are
// shared).  The view's rows of the per-view gradients are written (exactly +0 where the view's blend did not reach
// the Gaussian); the gradients of what stays shared (opacity, colour and, when they have no per-view array, scale,
// rotation and second colour) are summed in registers in view order and continue from the stored value with
// `accumulate`, so that any split into view groups and sets gives the same bits.  No atomics.
// As in gsr_backward.hip: the lanes of a wave walk the same view, so the camera comes through scalar loads; a view's
// record, row slot and geometry rows of consecutive Gaussians follow each other (coalesced); the next reached view's
// record and row slot are loaded one view ahead.
#include "gsr_chain.h"
#include "gsr_kernels.h"
#include "gsr_math.h"

namespace gsr {

// Occupancy floor: 3 waves per SIMD for both variants, as k_gauss_fused (<= 168 VGPRs, no spill; capped at 4 waves the
// two-colour variant spills 50 VGPRs inside the view loop).
template <bool TWO>
__attribute__((amdgpu_waves_per_eu(3, 8)))
__global__ __launch_bounds__(256) void k_tv_grad(GaussBackwardArgs a, ViewGradArgs va, TimedGradArgs tv) {
  const int idx = a.g0 + blockIdx.x * 256 + threadIdx.x;
  const bool valid = idx < a.g1;
  const int ix = valid ? idx : a.g0;  // (threads past the range follow the loop uniformly, write nothing)
  const bool acc = tv.accumulate != 0;
  const bool scales_shared = tv.scales_v == nullptr, rots_shared = tv.rotations_v == nullptr;
  const unsigned long long reach_word = valid ? va.reach[ix] : 0ull;
  // sums of what the views share
  float dop = 0.f, dcr = 0.f, dcg = 0.f, dcb = 0.f;
  float d2[3] = {0.f, 0.f, 0.f};
  float dss[3] = {0.f, 0.f, 0.f}, dqs[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid && acc) {
    // continue the earlier groups' sums in place (same summation order as one group)
    dop = a.dL_dopacity[idx];
    if (a.dL_dcolors) dcr = a.dL_dcolors[3 * idx], dcg = a.dL_dcolors[3 * idx + 1], dcb = a.dL_dcolors[3 * idx + 2];
    if (TWO && tv.dcolors2)
      for (int k = 0; k < 3; ++k) d2[k] = tv.dcolors2[3 * idx + k];
    if (scales_shared)
      for (int k = 0; k < 3; ++k) dss[k] = a.dL_dscales[3 * idx + k];
    if (rots_shared)
      for (int k = 0; k < 4; ++k) dqs[k] = a.dL_drotations[4 * idx + k];
  }
  // a shared scale / rotation once; the next reached view's record and row slot one view ahead.  The view's own
  // position, scale and rotation are loaded at the top of its iteration and used after the gather, whose first wait
  // covers them (a view ahead they would hold 10 more registers across the gather: 2 waves per SIMD instead of 3)
  float ss[3] = {1.f, 1.f, 1.f}, qs[4] = {1.f, 0.f, 0.f, 0.f};
  if (scales_shared)
    for (int k = 0; k < 3; ++k) ss[k] = a.scales[3 * ix + k];
  if (rots_shared)
    for (int k = 0; k < 4; ++k) qs[k] = a.rotations[4 * ix + k];
  GaussRec nrec;
  uint32_t ngo = 0u;
  auto fetch = [&](int vl) {
    const size_t o = (size_t)(va.v0 + vl) * a.P + ix;
    nrec = va.g.rec[o];
    ngo = va.g.goff[o];
  };
  const int vfirst = reach_word != 0ull ? (int)__builtin_ctzll(reach_word) : va.V;
  if (vfirst < va.V) fetch(vfirst);
#pragma unroll 1
  for (int vl = 0; vl < va.V; ++vl) {
    const int vg = va.v0 + vl;
    const size_t o = (size_t)vg * a.P + ix;
    // this (view, Gaussian)'s gradient rows: exactly +0 unless the view's blend reached the Gaussian
    auto zero_rows = [&]() {
      if (!valid) return;
      float* m2 = va.dmeans2D + 3 * o;
      m2[0] = 0.f, m2[1] = 0.f, m2[2] = 0.f;
      for (int k = 0; k < 3; ++k) tv.dmeans_v[3 * o + k] = 0.f;
      if (!scales_shared)
        for (int k = 0; k < 3; ++k) tv.dscales_v[3 * o + k] = 0.f;
      if (!rots_shared)
        for (int k = 0; k < 4; ++k) tv.drotations_v[4 * o + k] = 0.f;
      if (TWO && tv.dcolors2_v)
        for (int k = 0; k < 3; ++k) tv.dcolors2_v[3 * o + k] = 0.f;
    };
    if (!((reach_word >> vl) & 1ull)) {
      zero_rows();
      continue;
    }
    const GaussRec gr = nrec;
    const uint32_t go = ngo;
    const float3 mean = make_float3(tv.means_v[3 * o], tv.means_v[3 * o + 1], tv.means_v[3 * o + 2]);
    float3 scale = make_float3(ss[0], ss[1], ss[2]);
    float4 rot = make_float4(qs[0], qs[1], qs[2], qs[3]);
    if (!scales_shared) scale = make_float3(tv.scales_v[3 * o], tv.scales_v[3 * o + 1], tv.scales_v[3 * o + 2]);
    if (!rots_shared)
      rot = make_float4(tv.rotations_v[4 * o], tv.rotations_v[4 * o + 1], tv.rotations_v[4 * o + 2],
                        tv.rotations_v[4 * o + 3]);
    const unsigned long long later = reach_word & ~((2ull << vl) - 1ull);
    if (later != 0ull) fetch((int)__builtin_ctzll(later));
    const ViewCam& cam = va.cam[vl];
    // the view's matrices through the constant address space (wave-uniform view: s_load, no VGPRs)
    typedef __attribute__((address_space(4))) const float* cfptr;
    float viewm[16], projm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) viewm[i] = ((cfptr)cam.view)[i], projm[i] = ((cfptr)cam.proj)[i];
    ViewGeom vgm;
    vgm.view = viewm;
    vgm.proj = projm;
    vgm.tanx = cam.tanx;
    vgm.tany = cam.tany;
    vgm.fy = va.H / (2.0f * cam.tany);
    vgm.fx = va.W / (2.0f * cam.tanx);
    const float4* grow = va.grow + (size_t)(TWO ? 4 : 3) * va.row_start[vl];
    const uint2* cut = va.img.cut + (size_t)vg * va.tiles;
    const RowSums r = gather_rows<TWO>((uint32_t)ix, gr, go, va.gx, cut, grow);
    // rows that sum to zero (no pixel of the view kept the Gaussian): zero rows without the chain rule
    bool reached = (r.dmx != 0.f) | (r.dmy != 0.f) | (r.dca != 0.f) | (r.dcb != 0.f) | (r.dcc != 0.f) |
                   (r.dop != 0.f) | (r.dcr != 0.f) | (r.dcg != 0.f) | (r.dcbl != 0.f) | (r.ddep != 0.f);
    if (TWO) reached = reached | (r.dr2 != 0.f) | (r.dg2 != 0.f) | (r.db2 != 0.f);
    if (!reached) {
      zero_rows();
      continue;
    }
    float cov3D[6];
    cov3d_from_scale_rot(scale, a.scale_modifier, rot, cov3D);
    float dcv[6];
    float3 dm;
    cov2d_backward(mean, cov3D, vgm, r.dca, r.dcb, r.dcc, dcv, dm);
    proj_backward(mean, projm, r.dmx, r.dmy, dm);
    // view depth = view[2] x + view[6] y + view[10] z + view[14]
    dm.x += viewm[2] * r.ddep;
    dm.y += viewm[6] * r.ddep;
    dm.z += viewm[10] * r.ddep;
    // this view's 3D cov -> its own scale and quaternion
    float ds[3], dq[4];
    scale_rot_backward(scale, rot, a.scale_modifier, dcv, ds, dq);
    if (valid) {
      float* m2 = va.dmeans2D + 3 * o;
      // (two colours: the first call's own screen-space gradient; the chain above took both calls')
      m2[0] = TWO ? r.dmx1 : r.dmx;
      m2[1] = TWO ? r.dmy1 : r.dmy;
      m2[2] = 0.f;
      tv.dmeans_v[3 * o] = dm.x;
      tv.dmeans_v[3 * o + 1] = dm.y;
      tv.dmeans_v[3 * o + 2] = dm.z;
      if (!scales_shared)
        for (int k = 0; k < 3; ++k) tv.dscales_v[3 * o + k] = ds[k];
      if (!rots_shared)
        for (int k = 0; k < 4; ++k) tv.drotations_v[4 * o + k] = dq[k];
      if (TWO && tv.dcolors2_v) {
        tv.dcolors2_v[3 * o] = r.dr2;
        tv.dcolors2_v[3 * o + 1] = r.dg2;
        tv.dcolors2_v[3 * o + 2] = r.db2;
      }
    }
    // what the views share, summed in view order
    dcr += r.dcr;
    dcg += r.dcg;
    dcb += r.dcbl;
    dop += r.dop;
    if (TWO) {
      d2[0] += r.dr2;
      d2[1] += r.dg2;
      d2[2] += r.db2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dss[k] += ds[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) dqs[k] += dq[k];
  }
  if (!valid) return;
  // (the sums already include the earlier groups: plain stores)
  a.dL_dopacity[idx] = dop;
  if (a.dL_dcolors) {
    a.dL_dcolors[3 * idx] = dcr;
    a.dL_dcolors[3 * idx + 1] = dcg;
    a.dL_dcolors[3 * idx + 2] = dcb;
  }
  if (TWO && tv.dcolors2)
    for (int k = 0; k < 3; ++k) tv.dcolors2[3 * idx + k] = d2[k];
  if (scales_shared)
    for (int k = 0; k < 3; ++k) a.dL_dscales[3 * idx + k] = dss[k];
  if (rots_shared)
    for (int k = 0; k < 4; ++k) a.dL_drotations[4 * idx + k] = dqs[k];
}

void launch_timed_gauss_backward(const GaussBackwardArgs& a, const ViewGradArgs& va, const TimedGradArgs& tv,
                                 bool two_colors, hipStream_t stream) {
  const int n = a.g1 - a.g0;
  if (n <= 0 || va.V <= 0) return;
  auto kern = two_colors ? k_tv_grad<true> : k_tv_grad<false>;
  hipLaunchKernelGGL(kern, dim3(div_up(n, 256)), dim3(256), 0, stream, a, va, tv);
}

}  // namespace gsr
