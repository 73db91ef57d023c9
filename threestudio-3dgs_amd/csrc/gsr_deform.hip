// gsr_deform.hip — the HexPlane deformation network of dynamic SuGaR at T ticks x P fixed points, forward and backward
// (include/gsr.h gsr_sugar_deform_*; replaces DeformationNetwork.forward_dynamic_delta of geometry/deformation.py and
// the rot + (0, 0, 0, 1), normalise epilogue of _get_timed_dg_attributes_wo_spline, geometry/dynamic_sugar.py:442-480:
// 24 grid_sample calls, 20 products, a cat and 7 Linears, and the atomic scatter of grid_sample's backward).  The
// formulas are in the header.
//
// The cell and the fp64 weight of every point along every axis of every level, and of every tick, come from the caller
// (HexPlaneBinding): a kernel reads a coordinate nowhere.  Everything is fp64 from the fp32 planes and weights, every
// output and gradient rounded to fp32 once.  Feature k = 32 level + channel, K = 32 L features.
//
//   k_deform_forward   512 threads = 8 waves; the MLP in LDS (fp32, rows padded by one word so that both a row per lane
//                      and a column per lane are conflict free).  A wave owns a point and walks its ticks; lane j is
//                      hidden unit j, and lanes (level, channel) form the features: the three spatial planes are
//                      sampled once per point, the three time planes per tick.  Nothing but the outputs is written.
//   k_deform_mlp       (backward) the same walk: recomputes the forward, takes the upstream gradients through the
//                      heads to the features, writes dL/dfeature per sample (gf), per point the product of the spatial
//                      samples (sp) and sum_t dL/dfeature x the product of the time samples (at), and sums the weight
//                      and bias gradients in registers: the matrices of feature_out and of the residual layers over all
//                      samples of the block (each thread owns a slice of columns of its row), the rest per wave.
//   k_deform_reduce    adds those partial sums in block (and wave) order.
//   k_deform_spatial   one wave per texel of a spatial plane: walks the texel's row of (point, corner) entries.
//   k_deform_time      one wave per texel (i, tau) of a time plane: the row of column i against the row of time tau.
// Both texel kernels: lane = (half, channel); the half-waves take the even and the odd entries of the row in ascending
// order and one shuffle adds the two sums.  A texel with an empty row is written as +0.0.
// No atomics: every sum's order is fixed by the sizes and the tables.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

#define GSR_DEFORM_WAVES 8
#define GSR_DEFORM_PART_B (64 * 128 + 3 * 64 * 64)  // doubles per block: dL/dW of feature_out, of the residual layers
#define GSR_DEFORM_PART_W 1024  // doubles per wave: final layers (10 x 64), b0 (64), b1 (3 x 64), b2 (16)
#define GSR_DEFORM_MAX_BLOCKS 256

struct DeformArgs {
  int T, P, L, K, nh, nout, normalize;
  int r[GSR_DEFORM_MAX_L][4];  // resolution of level l along axis d
  const float* planes[GSR_DEFORM_MAX_L * 6];
  const float* mlp[GSR_DEFORM_MLP];
  const int* cell;
  const double* frac;
  const int* tcell;
  const double* tfrac;
};
struct DeformTables {
  const int *sp_order, *sp_offsets, *col_order, *col_offsets, *t_order, *t_offsets;
  int n_sp, n_col, n_t;
  int sp_base[GSR_DEFORM_MAX_L * 3 + 1];   // first texel of spatial plane (level, 0..2) in sp_offsets
  int col_base[GSR_DEFORM_MAX_L * 3 + 1];  // first column of (level, axis) in col_offsets
  int tm_base[GSR_DEFORM_MAX_L * 3 + 1];   // first texel of time plane (level, axis) in the launch
};
struct DeformPlaneGrads {
  float* p[GSR_DEFORM_MAX_L * 6];
};
struct DeformMlpGrads {
  float* p[GSR_DEFORM_MLP];
};

// plane q of itertools.combinations(range(4), 2): (a, b), a along the width
GSR_HD int plane_a(int q) { return q < 3 ? 0 : (q < 5 ? 1 : 2); }
GSR_HD int plane_b(int q) { return q < 3 ? q + 1 : (q < 5 ? q - 1 : 3); }
GSR_HD int spatial_plane(int i) { return i == 2 ? 3 : i; }  // (0, 1), (0, 2), (1, 2)
GSR_HD int time_plane(int a) { return a == 0 ? 2 : (a == 1 ? 4 : 5); }  // (a, 3)

// the two texels of a coordinate along one axis; the upper one outside the plane has weight 0 and index i0
struct DeformCell {
  int i0, i1;
  double w0, w1;
};
GSR_HD DeformCell deform_cell(int i, double f, int R) {
  DeformCell c;
  c.i0 = i < 0 ? 0 : (i > R - 1 ? R - 1 : i);
  const bool up = c.i0 + 1 <= R - 1;
  c.i1 = up ? c.i0 + 1 : c.i0;
  c.w1 = up ? f : 0.0;
  c.w0 = 1.0 - f;
  return c;
}
GSR_HD DeformCell axis_cell(const DeformArgs& a, int l, int d, int p, int t) {
  if (d == 3) return deform_cell(a.tcell[t], a.tfrac[t], a.r[l][3]);
  const size_t i = ((size_t)l * 3 + d) * (size_t)a.P + p;
  return deform_cell(a.cell[i], a.frac[i], a.r[l][d]);
}
GSR_HD double sample_plane(const DeformArgs& a, int l, int q, int ch, int p, int t) {
  const int A = plane_a(q), B = plane_b(q);
  const DeformCell x = axis_cell(a, l, A, p, t), y = axis_cell(a, l, B, p, t);
  const size_t W = (size_t)a.r[l][A], H = (size_t)a.r[l][B];
  const float* s = a.planes[l * 6 + q] + (size_t)ch * W * H;
  const double top = x.w0 * (double)s[y.i0 * W + x.i0] + x.w1 * (double)s[y.i0 * W + x.i1];
  const double bot = x.w0 * (double)s[y.i1 * W + x.i0] + x.w1 * (double)s[y.i1 * W + x.i1];
  return y.w0 * top + y.w1 * bot;
}

// the MLP in LDS: rows of feature_out and of the residual layers padded by one word
struct DeformLds {
  float w0[64 * 129];
  float w1[3][64 * 65];
  float w2[GSR_DEFORM_OUT][64];  // rows 0..2 pos, 3..6 rot, 7..9 scale
  float b0[64], b1[3][64], b2[16];
};
// per wave: the features, relu(h) and the heads' y of the sample in flight
struct DeformStage {
  double f[128], r[64], y[3][64];
};
struct DeformBackStage {
  double gy[3][64], gh[64], go[16];
  int valid;
};

GSR_HD int head_of_row(int row) { return row < 3 ? 0 : (row < 7 ? 1 : 2); }
GSR_HD int head_row0(int hd) { return hd == 0 ? 0 : (hd == 1 ? 3 : 7); }

__device__ __forceinline__ void deform_load_mlp(DeformLds& W, const DeformArgs& a) {
  const int tid = threadIdx.x, K = a.K;
  for (int i = tid; i < 64 * K; i += 512) W.w0[(i / K) * 129 + i % K] = a.mlp[0][i];
  for (int i = tid; i < 64; i += 512) W.b0[i] = a.mlp[1][i];
  for (int hd = 0; hd < 3; ++hd) {
    const bool on = hd < a.nh;
    const int r0 = head_row0(hd), rows = hd == 1 ? 4 : 3;
    for (int i = tid; i < 64 * 64; i += 512) W.w1[hd][(i >> 6) * 65 + (i & 63)] = on ? a.mlp[2 + 4 * hd][i] : 0.0f;
    for (int i = tid; i < 64; i += 512) W.b1[hd][i] = on ? a.mlp[3 + 4 * hd][i] : 0.0f;
    for (int i = tid; i < rows * 64; i += 512) W.w2[r0 + (i >> 6)][i & 63] = on ? a.mlp[4 + 4 * hd][i] : 0.0f;
    for (int i = tid; i < rows; i += 512) W.b2[r0 + i] = on ? a.mlp[5 + 4 * hd][i] : 0.0f;
  }
}

// From the lane's two features to h (before the relu) and the heads' y of hidden unit `lane`; leaves the features,
// relu(h) and y in the wave's stage.  Every thread of the block calls it (block barriers).
__device__ __forceinline__ void deform_hidden(const DeformArgs& a, const DeformLds& W, DeformStage& s,
                                              const double (&feat)[2], int lane, double& h, double (&y)[3]) {
  s.f[lane] = feat[0];
  s.f[lane + 64] = feat[1];
  __syncthreads();
  double acc = (double)W.b0[lane];
  for (int k = 0; k < a.K; ++k) acc = fma((double)W.w0[lane * 129 + k], s.f[k], acc);
  h = acc;
  s.r[lane] = acc > 0.0 ? acc : 0.0;
  __syncthreads();
#pragma unroll
  for (int hd = 0; hd < 3; ++hd) {
    acc = 0.0;
    if (hd < a.nh) {
      acc = (double)W.b1[hd][lane];
      for (int k = 0; k < 64; ++k) acc = fma((double)W.w1[hd][lane * 65 + k], s.r[k], acc);
      acc += s.r[lane];
    }
    y[hd] = acc;
    s.y[hd][lane] = acc;
  }
  __syncthreads();
}

// output row `lane` (< nout) of the final layers, the rotation with + (0, 0, 0, 1) but before the normalisation, and
// the norm n of that rotation in every lane
__device__ __forceinline__ double deform_output(const DeformArgs& a, const DeformLds& W, const DeformStage& s, int lane,
                                                double& n) {
  double o = 0.0;
  if (lane < a.nout) {
    const int hd = head_of_row(lane);
    o = (double)W.b2[lane];
    for (int j = 0; j < 64; ++j) o = fma((double)W.w2[lane][j], s.y[hd][j], o);
    if (lane == 6) o += 1.0;
  }
  const double qx = __shfl(o, 3, 64), qy = __shfl(o, 4, 64), qz = __shfl(o, 5, 64), qw = __shfl(o, 6, 64);
  n = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  return o;
}

// the point of wave w in round `it`, or -1
__device__ __forceinline__ int deform_point(const DeformArgs& a, int it, int w) {
  const long long p = ((long long)it * gridDim.x + blockIdx.x) * GSR_DEFORM_WAVES + w;
  return p < a.P ? (int)p : -1;
}

__global__ __launch_bounds__(512) void k_deform_forward(DeformArgs a, int rounds, float* __restrict__ xyz,
                                                        float* __restrict__ rot, float* __restrict__ scale) {
  __shared__ DeformLds W;
  __shared__ DeformStage stage[GSR_DEFORM_WAVES];
  deform_load_mlp(W, a);
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, ch = lane & 31;
  for (int it = 0; it < rounds; ++it) {
    const int p = deform_point(a, it, w);
    double sp[2] = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int l = (lane >> 5) + 2 * u;
      if (p >= 0 && l < a.L)
        sp[u] = sample_plane(a, l, 0, ch, p, 0) * sample_plane(a, l, 1, ch, p, 0) * sample_plane(a, l, 3, ch, p, 0);
    }
    for (int t = 0; t < a.T; ++t) {
      double feat[2] = {0.0, 0.0}, h, y[3], n;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int l = (lane >> 5) + 2 * u;
        if (p >= 0 && l < a.L)
          feat[u] = sp[u] * (sample_plane(a, l, 2, ch, p, t) * sample_plane(a, l, 4, ch, p, t) *
                             sample_plane(a, l, 5, ch, p, t));
      }
      deform_hidden(a, W, stage[w], feat, lane, h, y);
      double o = deform_output(a, W, stage[w], lane, n);
      if (p < 0 || lane >= a.nout) continue;
      const size_t s = (size_t)t * a.P + p;
      if (lane < 3) {
        xyz[3 * s + lane] = (float)o;
      } else if (lane < 7) {
        if (a.normalize) o /= n;
        rot[4 * s + lane - 3] = (float)o;
      } else {
        scale[3 * s + lane - 7] = (float)o;
      }
    }
  }
}

struct DeformUps {
  const float *g_xyz, *g_rot, *g_scale;
};
struct DeformWork {
  double *gf, *sp, *at, *part_b, *part_w;
  static DeformWork carve(void* base, int T, int P, int L, int blocks, size_t* bytes) {
    Carver c(base);
    DeformWork k;
    const size_t K = 32 * (size_t)L, S = (size_t)(T > 0 ? T : 1) * (size_t)(P > 0 ? P : 1);
    k.gf = c.take<double>(S * K);
    k.sp = c.take<double>((size_t)(P > 0 ? P : 1) * K);
    k.at = c.take<double>((size_t)(P > 0 ? P : 1) * K);
    k.part_b = c.take<double>((size_t)blocks * GSR_DEFORM_PART_B);
    k.part_w = c.take<double>((size_t)blocks * GSR_DEFORM_WAVES * GSR_DEFORM_PART_W);
    if (bytes) *bytes = align_up(c.off, 256);
    return k;
  }
};

__global__ __launch_bounds__(512) void k_deform_mlp(DeformArgs a, DeformUps up, int rounds, DeformWork ws) {
  __shared__ DeformLds W;
  __shared__ DeformStage stage[GSR_DEFORM_WAVES];
  __shared__ DeformBackStage back[GSR_DEFORM_WAVES];
  deform_load_mlp(W, a);
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, ch = lane & 31;
  const int K = a.K, kc = K / GSR_DEFORM_WAVES;  // this wave's columns of dL/dW0: [w kc, (w + 1) kc)
  double acc0[16], acc1[3][8], acc2[GSR_DEFORM_OUT], db0 = 0.0, db1[3] = {0.0, 0.0, 0.0}, db2 = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 24; ++i) acc1[i >> 3][i & 7] = 0.0;
#pragma unroll
  for (int i = 0; i < GSR_DEFORM_OUT; ++i) acc2[i] = 0.0;
  for (int it = 0; it < rounds; ++it) {
    const int p = deform_point(a, it, w);
    double sp[2] = {0.0, 0.0}, at[2] = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int l = (lane >> 5) + 2 * u;
      if (p >= 0 && l < a.L)
        sp[u] = sample_plane(a, l, 0, ch, p, 0) * sample_plane(a, l, 1, ch, p, 0) * sample_plane(a, l, 3, ch, p, 0);
    }
    for (int t = 0; t < a.T; ++t) {
      double feat[2] = {0.0, 0.0}, tp[2] = {0.0, 0.0}, h, y[3], n;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int l = (lane >> 5) + 2 * u;
        if (p >= 0 && l < a.L) {
          tp[u] = sample_plane(a, l, 2, ch, p, t) * sample_plane(a, l, 4, ch, p, t) * sample_plane(a, l, 5, ch, p, t);
          feat[u] = sp[u] * tp[u];
        }
      }
      deform_hidden(a, W, stage[w], feat, lane, h, y);
      const double o = deform_output(a, W, stage[w], lane, n);
      // the upstream gradient of output row `lane`, through the normalisation of the rotation
      const size_t s = (size_t)t * a.P + (p >= 0 ? p : 0);
      double go = 0.0;
      if (p >= 0 && lane < a.nout) {
        if (lane < 3)
          go = up.g_xyz != nullptr ? (double)up.g_xyz[3 * s + lane] : 0.0;
        else if (lane < 7)
          go = up.g_rot != nullptr ? (double)up.g_rot[4 * s + lane - 3] : 0.0;
        else
          go = up.g_scale != nullptr ? (double)up.g_scale[3 * s + lane - 7] : 0.0;
      }
      if (a.normalize) {  // r = q / n:  gq = (g - r (r . g)) / n
        const bool q = lane >= 3 && lane < 7;
        const double r = o / n, rg = q ? r * go : 0.0;
        const double d = ((__shfl(rg, 3, 64) + __shfl(rg, 4, 64)) + __shfl(rg, 5, 64)) + __shfl(rg, 6, 64);
        if (q) go = (go - r * d) / n;
      }
      if (lane < 16) back[w].go[lane] = go;
      if (lane == 0) back[w].valid = p >= 0;
      __syncthreads();
      double gy[3];
#pragma unroll
      for (int hd = 0; hd < 3; ++hd) {
        gy[hd] = 0.0;
        if (hd < a.nh) {
          const int r0 = head_row0(hd), rows = hd == 1 ? 4 : 3;
          for (int c = 0; c < rows; ++c) gy[hd] = fma((double)W.w2[r0 + c][lane], back[w].go[r0 + c], gy[hd]);
        }
        back[w].gy[hd][lane] = gy[hd];
      }
      __syncthreads();
      double gr = 0.0;
#pragma unroll
      for (int hd = 0; hd < 3; ++hd) {
        if (hd < a.nh) {
          double acc = gy[hd];
          for (int i = 0; i < 64; ++i) acc = fma((double)W.w1[hd][i * 65 + lane], back[w].gy[hd][i], acc);
          gr += acc;
        }
      }
      const double gh = h > 0.0 ? gr : 0.0;  // relu' at exactly 0 is 0
      back[w].gh[lane] = gh;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = lane + 64 * u;
        if (k < K && p >= 0) {
          double acc = 0.0;
          for (int j = 0; j < 64; ++j) acc = fma((double)W.w0[j * 129 + k], back[w].gh[j], acc);
          ws.gf[s * K + k] = acc;
          at[u] = fma(acc, tp[u], at[u]);
        }
      }
      // the matrices' gradients over the samples of all waves, in wave order
      for (int v = 0; v < GSR_DEFORM_WAVES; ++v) {
        if (!back[v].valid) continue;
        const double g0 = back[v].gh[lane];
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (i < kc) acc0[i] = fma(g0, stage[v].f[w * kc + i], acc0[i]);
#pragma unroll
        for (int hd = 0; hd < 3; ++hd) {
          if (hd < a.nh) {
            const double g1 = back[v].gy[hd][lane];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc1[hd][i] = fma(g1, stage[v].r[w * 8 + i], acc1[hd][i]);
          }
        }
      }
      if (p >= 0) {
#pragma unroll
        for (int c = 0; c < GSR_DEFORM_OUT; ++c) acc2[c] = fma(back[w].go[c], y[head_of_row(c)], acc2[c]);
        db0 += gh;
#pragma unroll
        for (int hd = 0; hd < 3; ++hd) db1[hd] += gy[hd];
        if (lane < 16) db2 += back[w].go[lane];
      }
      __syncthreads();  // the stages are rewritten by the next sample
    }
    if (p >= 0) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = lane + 64 * u;
        if (k < K) {
          ws.sp[(size_t)p * K + k] = sp[u];
          ws.at[(size_t)p * K + k] = at[u];
        }
      }
    }
  }
  double* pb = ws.part_b + (size_t)blockIdx.x * GSR_DEFORM_PART_B;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < kc) pb[lane * K + w * kc + i] = acc0[i];
#pragma unroll
  for (int hd = 0; hd < 3; ++hd)
#pragma unroll
    for (int i = 0; i < 8; ++i) pb[64 * 128 + hd * 4096 + lane * 64 + w * 8 + i] = acc1[hd][i];
  double* pw = ws.part_w + ((size_t)blockIdx.x * GSR_DEFORM_WAVES + w) * GSR_DEFORM_PART_W;
#pragma unroll
  for (int c = 0; c < GSR_DEFORM_OUT; ++c) pw[c * 64 + lane] = acc2[c];
  pw[640 + lane] = db0;
#pragma unroll
  for (int hd = 0; hd < 3; ++hd) pw[704 + hd * 64 + lane] = db1[hd];
  if (lane < 16) pw[896 + lane] = db2;
}

// one thread per element of the partial sums: adds the blocks (waves) in index order, rounds once
__global__ __launch_bounds__(256) void k_deform_reduce(int K, int nh, int blocks, DeformWork ws, DeformMlpGrads g) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= GSR_DEFORM_PART_B + GSR_DEFORM_PART_W) return;
  float* dst = nullptr;
  double sum = 0.0;
  if (i < GSR_DEFORM_PART_B) {
    if (i < 64 * 128) {
      if (i < 64 * K) dst = g.p[0] + i;
    } else {
      const int hd = (i - 64 * 128) >> 12;
      if (hd < nh) dst = g.p[2 + 4 * hd] + ((i - 64 * 128) & 4095);
    }
    if (dst == nullptr) return;
    for (int b = 0; b < blocks; ++b) sum += ws.part_b[(size_t)b * GSR_DEFORM_PART_B + i];
  } else {
    const int j = i - GSR_DEFORM_PART_B;
    if (j < 640) {
      const int row = j >> 6, hd = head_of_row(row);
      if (hd < nh) dst = g.p[4 + 4 * hd] + (row - head_row0(hd)) * 64 + (j & 63);
    } else if (j < 704) {
      dst = g.p[1] + (j - 640);
    } else if (j < 896) {
      const int hd = (j - 704) >> 6;
      if (hd < nh) dst = g.p[3 + 4 * hd] + ((j - 704) & 63);
    } else if (j < 896 + GSR_DEFORM_OUT) {
      const int row = j - 896, hd = head_of_row(row);
      if (hd < nh) dst = g.p[5 + 4 * hd] + (row - head_row0(hd));
    }
    if (dst == nullptr) return;
    for (int b = 0; b < blocks * GSR_DEFORM_WAVES; ++b) sum += ws.part_w[(size_t)b * GSR_DEFORM_PART_W + j];
  }
  *dst = (float)sum;
}

// the group (level, 0..2) of item i under the bases b[0 .. 3 L]
__device__ __forceinline__ int deform_group(const int* b, int L, int i) {
  int g = 0;
  while (g + 1 < 3 * L && i >= b[g + 1]) ++g;
  return g;
}

__global__ __launch_bounds__(256) void k_deform_spatial(DeformArgs a, DeformTables tb, const double* __restrict__ at,
                                                        DeformPlaneGrads out) {
  const int tex = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, half = lane >> 5, ch = lane & 31;
  if (tex >= tb.sp_base[3 * a.L]) return;
  const int g = deform_group(tb.sp_base, a.L, tex), l = g / 3, q = spatial_plane(g % 3);
  const int A = plane_a(q), B = plane_b(q), Wd = a.r[l][A], Ht = a.r[l][B];
  const int loc = tex - tb.sp_base[g], x = loc % Wd, y = loc / Wd;
  const int q1 = spatial_plane((g % 3 + 1) % 3), q2 = spatial_plane((g % 3 + 2) % 3);
  long long b, e;
  row_range(tb.sp_offsets, tex, tb.n_sp, b, e);
  double acc = 0.0;
  for (long long i = b + half; i < e; i += 2) {
    const int ent = tb.sp_order[i];
    if (!in_range(ent, 4ll * a.P)) continue;
    const int p = ent >> 2, cx = ent & 1, cy = (ent >> 1) & 1;
    const DeformCell ca = axis_cell(a, l, A, p, 0), cb = axis_cell(a, l, B, p, 0);
    if (ca.i0 + cx != x || cb.i0 + cy != y) continue;  // (not this texel's entry: a corrupt table)
    const double wgt = (cx ? ca.w1 : ca.w0) * (cy ? cb.w1 : cb.w0);
    const double other = sample_plane(a, l, q1, ch, p, 0) * sample_plane(a, l, q2, ch, p, 0);
    acc = fma(wgt * at[(size_t)p * a.K + l * 32 + ch], other, acc);
  }
  acc += __shfl_xor(acc, 32, 64);
  if (half == 0) out.p[l * 6 + q][((size_t)ch * Ht + y) * Wd + x] = (float)acc;
}

__global__ __launch_bounds__(256) void k_deform_time(DeformArgs a, DeformTables tb, const double* __restrict__ gf,
                                                     const double* __restrict__ sp, DeformPlaneGrads out) {
  const int tex = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, half = lane >> 5, ch = lane & 31;
  if (tex >= tb.tm_base[3 * a.L]) return;
  const int g = deform_group(tb.tm_base, a.L, tex), l = g / 3, ax = g % 3, q = time_plane(ax);
  const int Wd = a.r[l][ax], Ht = a.r[l][3];
  const int loc = tex - tb.tm_base[g], x = loc % Wd, tau = loc / Wd;
  const int q1 = time_plane((ax + 1) % 3), q2 = time_plane((ax + 2) % 3);
  long long b, e, tb0, te0;
  row_range(tb.col_offsets, tb.col_base[g] + x, tb.n_col, b, e);
  row_range(tb.t_offsets, tau, tb.n_t, tb0, te0);
  const int k = l * 32 + ch;
  double acc = 0.0;
  for (long long i = b + half; i < e; i += 2) {
    const int ent = tb.col_order[i];
    if (!in_range(ent, 2ll * a.P)) continue;
    const int p = ent >> 1, cx = ent & 1;
    const DeformCell ca = axis_cell(a, l, ax, p, 0);
    if (ca.i0 + cx != x) continue;
    const double wp = cx ? ca.w1 : ca.w0, spv = sp[(size_t)p * a.K + k];
    for (long long j = tb0; j < te0; ++j) {
      const int tent = tb.t_order[j];
      if (!in_range(tent, 2ll * a.T)) continue;
      const int t = tent >> 1, ct = tent & 1;
      const DeformCell c3 = axis_cell(a, l, 3, 0, t);
      if (c3.i0 + ct != tau) continue;
      const double wt = ct ? c3.w1 : c3.w0;
      const double other = spv * (sample_plane(a, l, q1, ch, p, t) * sample_plane(a, l, q2, ch, p, t));
      acc = fma((wp * wt) * gf[((size_t)t * a.P + p) * a.K + k], other, acc);
    }
  }
  acc += __shfl_xor(acc, 32, 64);
  if (half == 0) out.p[l * 6 + q][((size_t)ch * Ht + tau) * Wd + x] = (float)acc;
}

static int deform_blocks(int P) {
  const int b = div_up(P > 0 ? P : 1, GSR_DEFORM_WAVES);
  return b < GSR_DEFORM_MAX_BLOCKS ? b : GSR_DEFORM_MAX_BLOCKS;
}

static DeformArgs deform_args(const DeformCall& c) {
  DeformArgs a{};
  a.T = c.T, a.P = c.P, a.L = c.L, a.K = 32 * c.L;
  a.nh = c.d_scale ? 3 : 2, a.nout = c.d_scale ? 10 : 7, a.normalize = c.normalize_rot;
  for (int l = 0; l < c.L; ++l) {
    for (int d = 0; d < 4; ++d) a.r[l][d] = c.reso[4 * l + d];
    for (int q = 0; q < 6; ++q) a.planes[l * 6 + q] = c.planes[l * 6 + q];
  }
  for (int i = 0; i < GSR_DEFORM_MLP; ++i) a.mlp[i] = c.mlp[i];
  a.cell = c.cell, a.frac = c.frac, a.tcell = c.tcell, a.tfrac = c.tfrac;
  return a;
}

size_t deform_workspace_bytes(int T, int P, int L) {
  size_t bytes = 0;
  DeformWork::carve(nullptr, T, P, L, deform_blocks(P), &bytes);
  return bytes;
}

void launch_deform_forward(const DeformCall& c, float* xyz, float* rot, float* scale, hipStream_t stream) {
  const DeformArgs a = deform_args(c);
  const int blocks = deform_blocks(c.P), rounds = div_up(c.P, (long long)blocks * GSR_DEFORM_WAVES);
  hipLaunchKernelGGL(k_deform_forward, dim3(blocks), dim3(512), 0, stream, a, rounds, xyz, rot, scale);
}

void launch_deform_backward(const DeformCall& c, const DeformCsr& t, const float* g_xyz, const float* g_rot,
                            const float* g_scale, float* const* dplanes, float* const* dmlp, void* workspace,
                            hipStream_t stream) {
  const DeformArgs a = deform_args(c);
  const int blocks = deform_blocks(c.P), rounds = div_up(c.P, (long long)blocks * GSR_DEFORM_WAVES);
  const DeformWork ws = DeformWork::carve(workspace, c.T, c.P, c.L, blocks, nullptr);
  DeformTables tb{};
  tb.sp_order = t.sp_order, tb.sp_offsets = t.sp_offsets, tb.col_order = t.col_order, tb.col_offsets = t.col_offsets;
  tb.t_order = t.t_order, tb.t_offsets = t.t_offsets;
  tb.n_sp = c.n_sp, tb.n_col = c.n_col, tb.n_t = c.n_t;
  for (int l = 0; l < c.L; ++l)
    for (int i = 0; i < 3; ++i) {
      const int g = 3 * l + i, q = spatial_plane(i);
      tb.sp_base[g + 1] = tb.sp_base[g] + a.r[l][plane_a(q)] * a.r[l][plane_b(q)];
      tb.col_base[g + 1] = tb.col_base[g] + a.r[l][i];
      tb.tm_base[g + 1] = tb.tm_base[g] + a.r[l][i] * a.r[l][3];
    }
  DeformPlaneGrads pg{};
  for (int i = 0; i < 6 * c.L; ++i) pg.p[i] = dplanes[i];
  DeformMlpGrads mg{};
  for (int i = 0; i < GSR_DEFORM_MLP; ++i) mg.p[i] = dmlp[i];
  const DeformUps up{g_xyz, g_rot, c.d_scale ? g_scale : nullptr};
  hipLaunchKernelGGL(k_deform_mlp, dim3(blocks), dim3(512), 0, stream, a, up, rounds, ws);
  hipLaunchKernelGGL(k_deform_reduce, dim3(div_up(GSR_DEFORM_PART_B + GSR_DEFORM_PART_W, 256)), dim3(256), 0, stream,
                     a.K, a.nh, blocks, ws, mg);
  hipLaunchKernelGGL(k_deform_spatial, dim3(div_up(tb.sp_base[3 * c.L], 4)), dim3(256), 0, stream, a, tb, ws.at, pg);
  hipLaunchKernelGGL(k_deform_time, dim3(div_up(tb.tm_base[3 * c.L], 4)), dim3(256), 0, stream, a, tb, ws.gf, ws.sp,
                     pg);
}

}  // namespace gsr
