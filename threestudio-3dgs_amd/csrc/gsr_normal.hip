// gsr_normal.hip — the SuGaR regulariser's neighbour-normal loss, forward and backward (include/gsr.h
// gsr_sugar_normal_*; replaces the (M, K, 3) gathers of utils/sugar_utils.py:725-757 and the index_put scatter of
// their autograd backward).
//
// Per sample m with its own Gaussian i = own[m] and, per neighbour slot k, Gaussian j = nbr[row][k]:
//     s = sign(n_j . n_i);  a = |(x_m - c_j) . (s n_j)|;  w = op[m, k] a / max(min_scale_j, 1e-6)^2
//     W = sum_k w;  Wc = max(W, 1e-6);  wh_k = w_k / Wc;  r = n_i - sum_k wh_k s_k n_j;  loss[m] = r . r
// Only the normals receive gradients (everything else is detached in the reference):
//     dL/dn_i += 2 g_m r,   dL/dn_j += -2 g_m wh_k s_k r.
// (x - c_j) . n_j and n_j . n_i are formed in fp64 and rounded once (normal_pair); the rest is fp32.  r is summed as
//     r = (1 - W / Wc) n_i + sum_k wh_k (n_i - s_k n_j)         (1 - W / Wc = 0 exactly when W >= 1e-6)
// which is the same value without the cancellation of n_i against the sample's own slot (j = i: its term is exactly
// 0 here, and carries nearly all the weight in a trained scene).
//
// Kernels:
//   k_normal_pack    one 32-byte record per Gaussian (c | max(min_scale, 1e-6), n): a neighbour is one aligned
//                    half line instead of pieces of three arrays.
//   k_normal_sample  16 lanes per sample, lane l owns slots l and l + 16, sums by group_sum's xor butterfly.
//                    Forward: loss and the (M, 4) record (r, Wc).  Backward: with that record, the coefficient and the
//                    sort key of each of the sample's K + 1 gradient terms (slot K is the sample's own 2 g r).
//   sort_runs        (gsr_sort.hip) the stable sort of the keys and k_run_bounds: [begin, end) of every Gaussian's run.
//   k_normal_gauss   L lanes (16 or 64) per Gaussian walk its run in pair order: dL/dn += coef[p] r[m].
// No atomics: every sum's order is fixed by the input (stable sort: the terms of one Gaussian ascend by m (K + 1) + k).
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_wave.h"

namespace gsr {

#define GSR_NORMAL_WMIN 1e-6f   // the clamp of the weight sum
#define GSR_NORMAL_SMIN 1e-6f   // the clamp of the min scale

struct NormalWork {
  float4* pack;  // [N][2]
  RunWork run;   // of the M (K + 1) gradient terms
  float* coef;   // [M (K + 1)]
  static NormalWork carve(void* base, long long M, int K, int N, size_t* bytes) {
    Carver c(base);
    NormalWork w;
    const size_t n = (size_t)(N > 0 ? N : 1), mk = (size_t)(M > 0 ? M * (K + 1) : 0);
    w.pack = c.take<float4>(2 * n);
    if (bytes && M <= 0) {  // the forward's share
      *bytes = align_up(c.off, 256);
      return w;
    }
    w.run.carve(c, mk, n, &w.coef);
    if (bytes) *bytes = align_up(c.off, 256);
    return w;
  }
};

size_t normal_workspace_bytes(long long M, int K, int N) {
  size_t b = 0;
  NormalWork::carve(nullptr, M, K, N, &b);
  return b;
}

__global__ __launch_bounds__(256) void k_normal_pack(int N, const float* __restrict__ centers,
                                                     const float* __restrict__ normals,
                                                     const float* __restrict__ min_scale, float4* __restrict__ pack) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const float* c = centers + 3 * (size_t)j;
  const float* n = normals + 3 * (size_t)j;
  pack[2 * (size_t)j] = make_float4(c[0], c[1], c[2], fmaxf(min_scale[j], GSR_NORMAL_SMIN));
  pack[2 * (size_t)j + 1] = make_float4(n[0], n[1], n[2], 0.0f);
}

// one pair, shared by the forward and the backward so that both form the same bits: the sign s (0 for an exactly
// orthogonal neighbour) and the unnormalised weight w
__device__ __forceinline__ void normal_pair(float x0, float x1, float x2, const float4& rc, const float4& rn,
                                            float ni0, float ni1, float ni2, float op, float& s, float& w) {
  // both dot products in fp64: the products are exact there.  (x - c_j) . n_j cancels (samples lie near their
  // Gaussian's plane), and the sign of n_j . n_i is a discrete decision.
  const double dot = fma((double)rn.z, (double)ni2, fma((double)rn.y, (double)ni1, (double)rn.x * (double)ni0));
  s = dot > 0.0 ? 1.0f : (dot < 0.0 ? -1.0f : 0.0f);
  const double d0 = (double)x0 - (double)rc.x, d1 = (double)x1 - (double)rc.y, d2 = (double)x2 - (double)rc.z;
  const float a = s != 0.0f ? (float)fabs(fma(d2, (double)rn.z, fma(d1, (double)rn.y, d0 * (double)rn.x))) : 0.0f;
  w = op * a / (rc.w * rc.w);
}

struct NormalArgs {
  int M, K, N;
  long long R;
  const float* x;
  const long long *own, *nbr;
  int per_sample;  // nbr has one row per sample (else sample m reads row own[m])
  const float4* pack;
  const float* op;
};

template <bool BWD>
__global__ __launch_bounds__(256) void k_normal_sample(NormalArgs a, float* __restrict__ loss, float4* __restrict__ rec,
                                                       const float* __restrict__ g_loss, uint32_t* __restrict__ keys,
                                                       float* __restrict__ coef) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long m = t >> 4;
  const int l = (int)(t & 15);
  const bool live = m < (long long)a.M;
  long long i = -1;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
  if (live) {
    i = a.own[m];
    x0 = a.x[3 * m];
    x1 = a.x[3 * m + 1];
    x2 = a.x[3 * m + 2];
  }
  const long long r = a.per_sample ? m : i;
  const bool ok = live && i >= 0 && i < (long long)a.N && r >= 0 && r < a.R;  // else: loss 0, no gradient
  // the loads of both slots first (indices and opacities, then the records), every address in range: an absent or
  // out-of-range slot reads record 0 and is masked
  long long j[2];
  float opv[2];
  bool valid[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = l + 16 * h;
    const bool act = ok && k < a.K;
    j[h] = act ? a.nbr[(size_t)r * (size_t)a.K + (size_t)k] : -1;
    opv[h] = act ? a.op[(size_t)m * (size_t)a.K + (size_t)k] : 0.0f;
  }
  const float4 own_n = a.pack[2 * (size_t)(ok ? i : 0) + 1];
  float4 rc[2], rn[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    valid[h] = j[h] >= 0 && j[h] < (long long)a.N;
    const float4* p = a.pack + 2 * (size_t)(valid[h] ? j[h] : 0);
    rc[h] = p[0];
    rn[h] = p[1];
  }
  const float ni0 = own_n.x, ni1 = own_n.y, ni2 = own_n.z;
  float s[2] = {0.0f, 0.0f}, w[2] = {0.0f, 0.0f};
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (valid[h]) normal_pair(x0, x1, x2, rc[h], rn[h], ni0, ni1, ni2, opv[h], s[h], w[h]);
  if (!BWD) {
    const float W = group_sum<16>(w[0] + w[1]);
    const float Wc = fmaxf(W, GSR_NORMAL_WMIN);
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!valid[h]) continue;
      const float wh = w[h] / Wc;
      v0 = fmaf(wh, ni0 - s[h] * rn[h].x, v0);
      v1 = fmaf(wh, ni1 - s[h] * rn[h].y, v1);
      v2 = fmaf(wh, ni2 - s[h] * rn[h].z, v2);
    }
    v0 = group_sum<16>(v0);
    v1 = group_sum<16>(v1);
    v2 = group_sum<16>(v2);
    if (live && l == 0) {
      const float rest = W >= GSR_NORMAL_WMIN ? 0.0f : 1.0f - W / Wc;
      const float r0 = ok ? fmaf(rest, ni0, v0) : 0.0f;
      const float r1 = ok ? fmaf(rest, ni1, v1) : 0.0f;
      const float r2 = ok ? fmaf(rest, ni2, v2) : 0.0f;
      loss[m] = fmaf(r2, r2, fmaf(r1, r1, r0 * r0));
      if (rec != nullptr) rec[m] = make_float4(r0, r1, r2, Wc);
    }
  } else if (live) {
    const float Wc = rec[m].w;
    const float g2 = 2.0f * g_loss[m];
    const size_t base = (size_t)m * (size_t)(a.K + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = l + 16 * h;
      if (k >= a.K) continue;
      keys[base + k] = valid[h] ? (uint32_t)j[h] : (uint32_t)a.N;
      coef[base + k] = valid[h] ? -(g2 * (w[h] / Wc) * s[h]) : 0.0f;
    }
    if (l == 0) {
      keys[base + a.K] = ok ? (uint32_t)i : (uint32_t)a.N;
      coef[base + a.K] = ok ? g2 : 0.0f;
    }
  }
}

template <int L>
__global__ __launch_bounds__(256) void k_normal_gauss(int M, int K, int N, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ begin,
                                                      const uint32_t* __restrict__ end, const float* __restrict__ coef,
                                                      const float4* __restrict__ rec, float* __restrict__ dnormals) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long g = t / L;
  const int l = (int)(t % L);
  const bool live = g < (long long)N;
  uint32_t b = 0u, e = 0u;
  if (live) {
    b = begin[g];
    e = end[g];
  }
  float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
  for (uint32_t i = b + (uint32_t)l; i < e; i += (uint32_t)L) {
    const uint32_t p = vals[i];
    const uint32_t m = p / (uint32_t)(K + 1);
    if (m >= (uint32_t)M) continue;  // (cannot happen: values are term numbers below M (K + 1))
    const float c = coef[p];
    const float4 r = rec[m];
    d0 = fmaf(c, r.x, d0);
    d1 = fmaf(c, r.y, d1);
    d2 = fmaf(c, r.z, d2);
  }
  d0 = group_sum<L>(d0);
  d1 = group_sum<L>(d1);
  d2 = group_sum<L>(d2);
  if (live && l == 0) {
    dnormals[3 * g] = d0;
    dnormals[3 * g + 1] = d1;
    dnormals[3 * g + 2] = d2;
  }
}

static NormalArgs normal_args(const NormalCall& c, const float4* pack) {
  NormalArgs a;
  a.M = c.M;
  a.K = c.K;
  a.N = c.N;
  a.R = c.R;
  a.x = c.x;
  a.own = c.own;
  a.nbr = c.nbr;
  a.per_sample = c.per_sample;
  a.pack = pack;
  a.op = c.op;
  return a;
}

static void normal_pack(const NormalCall& c, float4* pack, hipStream_t stream) {
  if (c.N > 0)
    hipLaunchKernelGGL(k_normal_pack, dim3(div_up(c.N, 256)), dim3(256), 0, stream, c.N, c.centers, c.normals,
                       c.min_scale, pack);
}

void launch_normal_forward(const NormalCall& c, float* loss, float* rec, void* workspace, hipStream_t stream) {
  const NormalWork w = NormalWork::carve(workspace, 0, c.K, c.N, nullptr);
  normal_pack(c, w.pack, stream);
  hipLaunchKernelGGL((k_normal_sample<false>), dim3(div_up(c.M, 16)), dim3(256), 0, stream, normal_args(c, w.pack),
                     loss, (float4*)rec, (const float*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
}

int normal_gauss_lanes(long long M, int K, int N) { return M * (K + 1) >= 48ll * (N > 0 ? N : 1) ? 64 : 16; }

int launch_normal_backward(const NormalCall& c, const float* rec, const float* g_loss, float* dnormals,
                           void* workspace, hipStream_t stream) {
  if (c.N <= 0) return 0;  // no Gaussian: no gradient to write
  NormalWork w = NormalWork::carve(workspace, c.M, c.K, c.N, nullptr);
  normal_pack(c, w.pack, stream);
  hipLaunchKernelGGL((k_normal_sample<true>), dim3(div_up(c.M, 16)), dim3(256), 0, stream, normal_args(c, w.pack),
                     (float*)nullptr, (float4*)rec, g_loss, w.run.keys[0], w.coef);
  int res = 0;
  const int err = sort_runs(w.run, (uint32_t)((long long)c.M * (c.K + 1)), c.N, &res, stream);
  if (err != 0) return err;
  const uint32_t *begin = w.run.bounds, *end = w.run.bounds + c.N;
  if (normal_gauss_lanes(c.M, c.K, c.N) == 64)
    hipLaunchKernelGGL((k_normal_gauss<64>), dim3(div_up((long long)c.N * 64, 256)), dim3(256), 0, stream, c.M, c.K,
                       c.N, w.run.vals[res], begin, end, w.coef, (const float4*)rec, dnormals);
  else
    hipLaunchKernelGGL((k_normal_gauss<16>), dim3(div_up((long long)c.N * 16, 256)), dim3(256), 0, stream, c.M, c.K,
                       c.N, w.run.vals[res], begin, end, w.coef, (const float4*)rec, dnormals);
  return 0;
}

}  // namespace gsr
