// gsr_densify.hip — the densification statistics of a view batch (include/gsr.h gsr_densify_stats).
//
// After the backward of a batch the reference's GaussianBaseModel.update_states (geometry/gaussian_base.py:845-851)
// walks the views in Python: max_radii2D = max(max_radii2D, radii_v), xyz_gradient_accum[vis_v] += |grad_v[vis_v, :2]|,
// denom[vis_v] += 1 — about ten small launches and two or three boolean-mask indexings (a nonzero with a host sync
// each) per view.  k_dstat_views is that loop in one launch: one lane per Gaussian walks the call's views in ascending
// order and keeps the running maximum, sum and count in registers, starting from the stored values (accumulate) or
// from zero, so the sum is rounded view after view exactly as the reference's in-place adds are, and calls chained
// with accumulate give the bits of one call.  No atomics, no LDS: every row is read once.
//
// Arithmetic (contraction off, every operation rounded on its own): x*x, y*y, their sum, the correctly rounded square
// root, and the add into the running sum — bit for bit the fp32 composition (gx * gx + gy * gy).sqrt() of IEEE
// operations (densify.py's CPU path, which takes the root through fp64: torch's own fp32 sqrt is an ulp off on some
// hosts).  The maximum keeps a NaN that the running value already holds (torch.max propagates it; the radii are
// integers).
//
// Memory: lane p reads radii[v][p] (coalesced dwords), grads[v][3p], [3p + 1] (two of every three dwords of a
// contiguous row: the third column shares the cache lines, so the row's lines are fetched whole) and, with visibility
// rows, visible[v][p] (bytes).  The row pointers come by value in the kernel argument: the view index is uniform, so
// they are scalar loads.  The loop takes four views at a time — all their loads are issued before the first dependent
// add — when all four have a gradient; a group with a view without one, and the V % 4 views left, go view by view.
#include "gsr_kernels.h"

namespace gsr {

#define GSR_DSTAT_UNROLL 4

// 8 waves per SIMD: a streaming kernel (<= 64 VGPRs, no spill)
template <bool VIS>
__attribute__((amdgpu_waves_per_eu(8, 8)))
__global__ __launch_bounds__(256) void k_dstat_views(const gsr_densify_batch a) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  float m = 0.f, s = 0.f, c = 0.f;
  if (a.accumulate) m = a.max_radii[p], s = a.grad_norm_sum[p], c = a.count[p];
  // (r > m is false for a NaN m: it stays)
  auto update = [&](int r, bool seen, bool has_grad, float x, float y) {
    const float rf = (float)r;
    m = rf > m ? rf : m;
    if (seen) {
      if (has_grad) s = s + sqrtf(x * x + y * y);
      c = c + 1.0f;
    }
  };
  auto one_view = [&](int v) {
    const int r = a.radii[v][p];
    const bool seen = VIS ? a.visible[v][p] != 0 : r > 0;
    const float* g = a.grads[v];  // uniform: a scalar branch
    float x = 0.f, y = 0.f;
    if (g != nullptr) x = g[3 * p], y = g[3 * p + 1];
    update(r, seen, g != nullptr, x, y);
  };
  int v = 0;
  for (; v + GSR_DSTAT_UNROLL <= a.V; v += GSR_DSTAT_UNROLL) {
    bool all = true;
#pragma unroll
    for (int k = 0; k < GSR_DSTAT_UNROLL; ++k) all = all && a.grads[v + k] != nullptr;
    if (!all) {
#pragma unroll 1
      for (int k = 0; k < GSR_DSTAT_UNROLL; ++k) one_view(v + k);
      continue;
    }
    int r[GSR_DSTAT_UNROLL];
    float x[GSR_DSTAT_UNROLL], y[GSR_DSTAT_UNROLL];
    unsigned char vis[GSR_DSTAT_UNROLL];
#pragma unroll
    for (int k = 0; k < GSR_DSTAT_UNROLL; ++k) {
      r[k] = a.radii[v + k][p];
      x[k] = a.grads[v + k][3 * p];
      y[k] = a.grads[v + k][3 * p + 1];
      vis[k] = VIS ? a.visible[v + k][p] : (unsigned char)0;
    }
#pragma unroll
    for (int k = 0; k < GSR_DSTAT_UNROLL; ++k) update(r[k], VIS ? vis[k] != 0 : r[k] > 0, true, x[k], y[k]);
  }
#pragma unroll 1
  for (; v < a.V; ++v) one_view(v);
  a.max_radii[p] = m;
  a.grad_norm_sum[p] = s;
  a.count[p] = c;
}

void launch_densify_stats(const gsr_densify_batch& a, hipStream_t stream) {
  if (a.P <= 0 || a.V <= 0) return;
  auto kern = a.visible[0] != nullptr ? k_dstat_views<true> : k_dstat_views<false>;
  hipLaunchKernelGGL(kern, dim3(div_up(a.P, 256)), dim3(256), 0, stream, a);
}

}  // namespace gsr
