// gsr_field.hip — the SuGaR regulariser's neighbour density field, forward and backward (include/gsr.h
// gsr_sugar_field_*; replaces the (M, K, 3, 3) gather + batched matmul of utils/sugar_utils.py:296-310 and the
// index_put scatter of its autograd backward).
//
// Per (sample m, neighbour slot k) with Gaussian j = nbr[row][k]:
//     d = x_m - c_j;  w_i = A_j[0][i] d_0 + A_j[1][i] d_1 + A_j[2][i] d_2  (w = A_j^T d);  q = min(w.w, 1e8)
//     op[m, k] = density_factor * strength_j * exp(-q / 2)
// d, w, q and the exponential are formed in fp64 and rounded once (field_pair); sums and gradients are fp32.
//
// Kernels:
//   k_field_pack    one 64-byte record per Gaussian (c | strength, A, min_scale): a neighbour is one aligned line
//                   instead of pieces of four arrays with 12 / 36 / 4 / 4-byte strides.
//   k_field_sample  16 lanes per sample (4 samples per wave), lane l owns slots k = l and l + 16; the K-sums are an
//                   xor butterfly over the 16 lanes (group_sum, gsr_wave.h).  Forward: density, beta_avg, op.  Backward
//                   (recomputed, nothing M x K kept from the forward): dL/dx by the same butterfly, and the sort key
//                   of every pair (its Gaussian, or N when the pair contributes nothing).
//   sort_runs       (gsr_sort.hip) the stable sort of the keys and k_run_bounds: [begin, end) of every Gaussian's run.
//   k_field_gauss   L lanes (16 or 64) per Gaussian walk its run in pair order, L pairs at a time, recompute the pair
//                   and add into per-lane sums; the L lanes are combined by the same butterfly.  No atomics anywhere:
//                   every sum's order is fixed by the input (stable sort: pairs of one Gaussian ascend by m K + k).
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_wave.h"

namespace gsr {

#define GSR_FIELD_QMAX 1e8f

struct FieldWork {
  float4* pack;  // [N][4]
  RunWork run;   // of the M K pairs
  static FieldWork carve(void* base, long long M, int K, int N, size_t* bytes) {
    Carver c(base);
    FieldWork w;
    const size_t n = (size_t)(N > 0 ? N : 1), mk = (size_t)(M > 0 ? M * K : 0);
    w.pack = c.take<float4>(4 * n);
    if (bytes && M <= 0) {  // the forward's share
      *bytes = align_up(c.off, 256);
      return w;
    }
    w.run.carve(c, mk, n);
    if (bytes) *bytes = align_up(c.off, 256);
    return w;
  }
};

size_t field_workspace_bytes(long long M, int K, int N) {
  size_t b = 0;
  FieldWork::carve(nullptr, M, K, N, &b);
  return b;
}

__global__ __launch_bounds__(256) void k_field_pack(int N, const float* __restrict__ centers,
                                                    const float* __restrict__ inv_sr,
                                                    const float* __restrict__ strengths,
                                                    const float* __restrict__ min_scale, float4* __restrict__ pack) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const float* c = centers + 3 * (size_t)j;
  const float* A = inv_sr + 9 * (size_t)j;
  float4* o = pack + 4 * (size_t)j;
  o[0] = make_float4(c[0], c[1], c[2], strengths[j]);
  o[1] = make_float4(A[0], A[1], A[2], A[3]);
  o[2] = make_float4(A[4], A[5], A[6], A[7]);
  o[3] = make_float4(A[8], min_scale[j], 0.0f, 0.0f);
}

// one pair, shared by the sample and the Gaussian kernels so that both recompute the same bits
struct FieldPair {
  float d0, d1, d2, w0, w1, w2, e;
  bool pass;  // the clamp lets the gradient through (w.w <= 1e8)
};
__device__ __forceinline__ FieldPair field_pair(float x0, float x1, float x2, float c0, float c1, float c2,
                                                const float (&A)[9]) {
  // d, w and q in fp64 (d is exact there), exp in fp64 too: on flat Gaussians the three products of a w_i cancel from
  // ~25 to ~1 and q reaches 174 before exp(-q / 2) leaves the fp32 range, so fp32 roundings of w and q reach op
  // (and every gradient, all proportional to it) amplified a thousandfold.  A few dozen fp64 operations per pair are
  // hidden behind the gather.
  FieldPair p;
  const double d0 = (double)x0 - (double)c0, d1 = (double)x1 - (double)c1, d2 = (double)x2 - (double)c2;
  const double w0 = fma((double)A[6], d2, fma((double)A[3], d1, (double)A[0] * d0));
  const double w1 = fma((double)A[7], d2, fma((double)A[4], d1, (double)A[1] * d0));
  const double w2 = fma((double)A[8], d2, fma((double)A[5], d1, (double)A[2] * d0));
  const double qr = fma(w2, w2, fma(w1, w1, w0 * w0));
  p.d0 = (float)d0;
  p.d1 = (float)d1;
  p.d2 = (float)d2;
  p.w0 = (float)w0;
  p.w1 = (float)w1;
  p.w2 = (float)w2;
  p.pass = qr <= (double)GSR_FIELD_QMAX;
  const double q = fmin(fmax(qr, 0.0), (double)GSR_FIELD_QMAX);
  p.e = (float)exp(-0.5 * q);
  return p;
}
// dL/dd of a pair given dL/dop and op (zero where the clamp cuts; never forms 0 x inf)
__device__ __forceinline__ void field_pair_dw(const FieldPair& p, float dop, float op, float& dw0, float& dw1,
                                              float& dw2) {
  const float dq2 = p.pass ? -(dop * op) : 0.0f;  // 2 dL/dq
  dw0 = p.pass ? p.w0 * dq2 : 0.0f;
  dw1 = p.pass ? p.w1 * dq2 : 0.0f;
  dw2 = p.pass ? p.w2 * dq2 : 0.0f;
}

struct FieldArgs {
  int M, K, N;
  long long R;
  const float* x;
  const long long *nbr, *row;
  const float4* pack;
  float density_factor;
};

template <bool BWD>
__global__ __launch_bounds__(256) void k_field_sample(FieldArgs a, float* __restrict__ density,
                                                      float* __restrict__ beta_avg, float* __restrict__ op_out,
                                                      const float* __restrict__ g_density,
                                                      const float* __restrict__ g_op, float* __restrict__ dx,
                                                      uint32_t* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long m = t >> 4;
  const int l = (int)(t & 15);
  const bool live = m < (long long)a.M;
  long long r = -1;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, gd = 0.0f;
  if (live) {
    r = a.row != nullptr ? a.row[m] : m;
    x0 = a.x[3 * m];
    x1 = a.x[3 * m + 1];
    x2 = a.x[3 * m + 2];
    if (BWD && g_density != nullptr) gd = g_density[m];
  }
  const bool rok = r >= 0 && r < a.R;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;  // forward: density, sum of min_scale; backward: dL/dx
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = l + 16 * h;
    if (!live || k >= a.K) continue;
    const size_t p = (size_t)m * (size_t)a.K + (size_t)k;
    long long j = -1;
    if (rok) j = a.nbr[(size_t)r * (size_t)a.K + (size_t)k];
    const bool valid = j >= 0 && j < (long long)a.N;
    float op = 0.0f;
    if (valid) {
      const float4* rec = a.pack + 4 * (size_t)j;
      const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
      const float A[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x};
      const FieldPair pr = field_pair(x0, x1, x2, r0.x, r0.y, r0.z, A);
      op = a.density_factor * r0.w * pr.e;
      if (!BWD) {
        s0 += op;
        s1 += r3.y;
      } else {
        const float dop = gd + (g_op != nullptr ? g_op[p] : 0.0f);
        float dw0, dw1, dw2;
        field_pair_dw(pr, dop, op, dw0, dw1, dw2);
        s0 += fmaf(A[2], dw2, fmaf(A[1], dw1, A[0] * dw0));
        s1 += fmaf(A[5], dw2, fmaf(A[4], dw1, A[3] * dw0));
        s2 += fmaf(A[8], dw2, fmaf(A[7], dw1, A[6] * dw0));
      }
    }
    if (!BWD) {
      if (op_out != nullptr) op_out[p] = op;
    } else {
      keys[p] = valid ? (uint32_t)j : (uint32_t)a.N;
    }
  }
  s0 = group_sum<16>(s0);
  s1 = group_sum<16>(s1);
  if (BWD) s2 = group_sum<16>(s2);
  if (live && l == 0) {
    if (!BWD) {
      density[m] = s0;
      beta_avg[m] = s1 / (float)a.K;
    } else {
      dx[3 * m] = s0;
      dx[3 * m + 1] = s1;
      dx[3 * m + 2] = s2;
    }
  }
}

struct FieldGaussArgs {
  int M, K, N;
  const float *x, *centers, *inv_sr, *strengths;
  float density_factor;
  const uint32_t *vals, *begin, *end;
  const float *g_density, *g_beta, *g_op;
  float *dcenters, *dinv_sr, *dstrengths, *dmin_scale;
};

template <int L>
__global__ __launch_bounds__(256) void k_field_gauss(FieldGaussArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long g = t / L;
  const int l = (int)(t % L);
  const bool live = g < (long long)a.N;
  uint32_t b = 0u, e = 0u;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, st = 0.0f;
  float A[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (live) {
    b = a.begin[g];
    e = a.end[g];
    if (e > b) {
      c0 = a.centers[3 * g];
      c1 = a.centers[3 * g + 1];
      c2 = a.centers[3 * g + 2];
      st = a.strengths[g];
#pragma unroll
      for (int i = 0; i < 9; ++i) A[i] = a.inv_sr[9 * g + i];
    }
  }
  float dc0 = 0.0f, dc1 = 0.0f, dc2 = 0.0f, ds = 0.0f, dms = 0.0f;
  float dA[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float fK = (float)a.K;
  const float dfs = a.density_factor * st;
  for (uint32_t i = b + (uint32_t)l; i < e; i += (uint32_t)L) {
    const uint32_t p = a.vals[i];
    const uint32_t m = p / (uint32_t)a.K;
    if (m >= (uint32_t)a.M) continue;  // (cannot happen: values are pair numbers below M K)
    const float x0 = a.x[3 * (size_t)m], x1 = a.x[3 * (size_t)m + 1], x2 = a.x[3 * (size_t)m + 2];
    const float dop = (a.g_density != nullptr ? a.g_density[m] : 0.0f) + (a.g_op != nullptr ? a.g_op[p] : 0.0f);
    if (a.g_beta != nullptr) dms += a.g_beta[m] / fK;
    const FieldPair pr = field_pair(x0, x1, x2, c0, c1, c2, A);
    const float fe = a.density_factor * pr.e;
    ds = fmaf(dop, fe, ds);
    float dw0, dw1, dw2;
    field_pair_dw(pr, dop, dfs * pr.e, dw0, dw1, dw2);
    dA[0] = fmaf(pr.d0, dw0, dA[0]);
    dA[1] = fmaf(pr.d0, dw1, dA[1]);
    dA[2] = fmaf(pr.d0, dw2, dA[2]);
    dA[3] = fmaf(pr.d1, dw0, dA[3]);
    dA[4] = fmaf(pr.d1, dw1, dA[4]);
    dA[5] = fmaf(pr.d1, dw2, dA[5]);
    dA[6] = fmaf(pr.d2, dw0, dA[6]);
    dA[7] = fmaf(pr.d2, dw1, dA[7]);
    dA[8] = fmaf(pr.d2, dw2, dA[8]);
    dc0 -= fmaf(A[2], dw2, fmaf(A[1], dw1, A[0] * dw0));
    dc1 -= fmaf(A[5], dw2, fmaf(A[4], dw1, A[3] * dw0));
    dc2 -= fmaf(A[8], dw2, fmaf(A[7], dw1, A[6] * dw0));
  }
  dc0 = group_sum<L>(dc0);
  dc1 = group_sum<L>(dc1);
  dc2 = group_sum<L>(dc2);
  ds = group_sum<L>(ds);
  dms = group_sum<L>(dms);
#pragma unroll
  for (int i = 0; i < 9; ++i) dA[i] = group_sum<L>(dA[i]);
  if (live && l == 0) {
    a.dcenters[3 * g] = dc0;
    a.dcenters[3 * g + 1] = dc1;
    a.dcenters[3 * g + 2] = dc2;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.dinv_sr[9 * g + i] = dA[i];
    a.dstrengths[g] = ds;
    a.dmin_scale[g] = dms;
  }
}

static FieldArgs field_args(const FieldCall& c, const float4* pack) {
  FieldArgs a;
  a.M = c.M;
  a.K = c.K;
  a.N = c.N;
  a.R = c.R;
  a.x = c.x;
  a.nbr = c.nbr;
  a.row = c.row;
  a.pack = pack;
  a.density_factor = c.density_factor;
  return a;
}

static void field_pack(const FieldCall& c, float4* pack, hipStream_t stream) {
  if (c.N > 0)
    hipLaunchKernelGGL(k_field_pack, dim3(div_up(c.N, 256)), dim3(256), 0, stream, c.N, c.centers, c.inv_sr,
                       c.strengths, c.min_scale, pack);
}

void launch_field_forward(const FieldCall& c, float* density, float* beta_avg, float* op, void* workspace,
                          hipStream_t stream) {
  const FieldWork w = FieldWork::carve(workspace, 0, c.K, c.N, nullptr);
  field_pack(c, w.pack, stream);
  hipLaunchKernelGGL((k_field_sample<false>), dim3(div_up(c.M, 16)), dim3(256), 0, stream, field_args(c, w.pack),
                     density, beta_avg, op, (const float*)nullptr, (const float*)nullptr, (float*)nullptr,
                     (uint32_t*)nullptr);
}

int field_gauss_lanes(long long M, int K, int N) { return M * K >= 48ll * (N > 0 ? N : 1) ? 64 : 16; }

int launch_field_backward(const FieldCall& c, const float* g_density, const float* g_beta, const float* g_op, float* dx,
                          float* dcenters, float* dinv_sr, float* dstrengths, float* dmin_scale, void* workspace,
                          hipStream_t stream) {
  FieldWork w = FieldWork::carve(workspace, c.M, c.K, c.N, nullptr);
  field_pack(c, w.pack, stream);
  hipLaunchKernelGGL((k_field_sample<true>), dim3(div_up(c.M, 16)), dim3(256), 0, stream, field_args(c, w.pack),
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, g_density, g_op, dx, w.run.keys[0]);
  if (c.N <= 0) return 0;
  int res = 0;
  const int err = sort_runs(w.run, (uint32_t)((long long)c.M * c.K), c.N, &res, stream);
  if (err != 0) return err;
  FieldGaussArgs a;
  a.M = c.M;
  a.K = c.K;
  a.N = c.N;
  a.x = c.x;
  a.centers = c.centers;
  a.inv_sr = c.inv_sr;
  a.strengths = c.strengths;
  a.density_factor = c.density_factor;
  a.vals = w.run.vals[res];
  a.begin = w.run.bounds;
  a.end = w.run.bounds + c.N;
  a.g_density = g_density;
  a.g_beta = g_beta;
  a.g_op = g_op;
  a.dcenters = dcenters;
  a.dinv_sr = dinv_sr;
  a.dstrengths = dstrengths;
  a.dmin_scale = dmin_scale;
  if (field_gauss_lanes(c.M, c.K, c.N) == 64)
    hipLaunchKernelGGL((k_field_gauss<64>), dim3(div_up((long long)c.N * 64, 256)), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((k_field_gauss<16>), dim3(div_up((long long)c.N * 16, 256)), dim3(256), 0, stream, a);
  return 0;
}

}  // namespace gsr
