// gsr_arap.hip — the as-rigid-as-possible energy of dynamic SuGaR's motion stage, forward and backward (include/gsr.h
// gsr_sugar_arap_*; replaces ARAPCoach.compute_arap_energy with given rotations, utils/arap_utils.py:148-189, called
// once per frame by _compute_arap_energy of system/sugar_4dgen.py: the padded (V, max valence, 3) edge matrix scattered
// by index_put, two bmm, the norm and the weighted sum, and the atomic scatter of index_put's backward).  The formulas
// are in the header.
//
// Precision: fp64 arithmetic from the fp32 inputs, every energy and gradient rounded to fp32 once.  The rest edge
// p_ij = x_i - x_j is formed from the rest vertices in fp64, so it is exact, p_ji = -p_ij, and x' = x with identity
// rotations gives exactly 0 (as in the reference, whose two fp32 edge matrices round alike).
//
//   k_arap_forward   one lane per (t, vertex), 256 lanes per block, a block within one frame: the lane walks its CSR
//                    row; the block's 256 energies are added in a fixed order into one fp64 partial sum.
//   k_arap_reduce    one wave per frame: adds the frame's partial sums in a fixed order, writes E_t.
//   k_arap_backward  one lane per (t, vertex): recomputes its row and writes dE/dx'_i and dE/dR_i (or, chained, dE/dq_i)
//                    times the upstream g_t.  The weights are symmetric and p_ji = -p_ij, so vertex i's own row holds
//                    every term of its gradient: a gather, no atomics.
// Long rows: a lane walks a row of at most GSR_ARAP_LANE_ROW entries itself.  A longer row (a fan hub) is left for
// the lane's wave: after the short rows, the wave takes its long rows one by one in lane order, lane l adding entries
// l, l + 64, ... of the row, and the 64 partial sums are added by wave_sum_f64's butterfly; the row's lane keeps it.  So a
// hub of valence n costs its wave n / 64 rounds, not n.
// No atomics: every sum's order is fixed by the input.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

#define GSR_ARAP_BLOCK 256
#define GSR_ARAP_LANE_ROW 32  // the longest row one lane walks alone

struct M33 {  // row-major
  D3 r[3];
};
GSR_HD D3 mul(const M33& m, D3 p) { return d3(dot(m.r[0], p), dot(m.r[1], p), dot(m.r[2], p)); }

// R = I + 2 w [v]x + 2 [v]x^2 of an (x, y, z, w) quaternion of any norm (pypose's matrix(), no normalisation)
GSR_HD M33 quat_matrix(Q4 q) {
  const double x = q.v.x, y = q.v.y, z = q.v.z, w = q.w;
  M33 m;
  m.r[0] = d3(1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y));
  m.r[1] = d3(2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x));
  m.r[2] = d3(2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y));
  return m;
}
// the gradient to q of quat_matrix, given the gradient g to the matrix
GSR_HD Q4 quat_matrix_grad(Q4 q, const M33& g) {
  const double x = q.v.x, y = q.v.y, z = q.v.z, w = q.w;
  const double s01 = g.r[0].y + g.r[1].x, s02 = g.r[0].z + g.r[2].x, s12 = g.r[1].z + g.r[2].y;
  const double a0 = g.r[2].y - g.r[1].z, a1 = g.r[0].z - g.r[2].x, a2 = g.r[1].x - g.r[0].y;
  return q4(d3(2.0 * (y * s01 + z * s02 - 2.0 * x * (g.r[1].y + g.r[2].z) + w * a0),
               2.0 * (x * s01 + z * s12 - 2.0 * y * (g.r[0].x + g.r[2].z) + w * a1),
               2.0 * (x * s02 + y * s12 - 2.0 * z * (g.r[0].x + g.r[1].y) + w * a2)),
            2.0 * (x * a0 + y * a1 + z * a2));
}

GSR_HD M33 arap_rotation(const ArapCall& a, size_t tv) {
  if (a.rot_form == GSR_ARAP_QUAT) return quat_matrix(load_xyzw(a.vert_rot + 4 * tv));
  const float* m = a.vert_rot + 9 * tv;
  M33 r;
  r.r[0] = load3(m), r.r[1] = load3(m + 3), r.r[2] = load3(m + 6);
  return r;
}

// what a row adds up: the energy (forward) or the two gradient sums (backward)
template <bool BWD>
struct ArapAcc;
template <>
struct ArapAcc<false> {
  double e;
};
template <>
struct ArapAcc<true> {
  D3 gx;  // sum w (2 d - (R_i + R_j) p)
  M33 G;  // sum w s p^T
};
GSR_HD void arap_zero(ArapAcc<false>& c) { c.e = 0.0; }
GSR_HD void arap_zero(ArapAcc<true>& c) {
  c.gx = d3(0.0, 0.0, 0.0);
  c.G.r[0] = c.G.r[1] = c.G.r[2] = c.gx;
}

// the vertex i of a row at frame t
struct ArapVertex {
  size_t tbase;  // t V
  D3 x0, x1;     // rest and deformed position
  M33 R;
};
GSR_HD ArapVertex arap_vertex(const ArapCall& a, int t, int v) {
  ArapVertex vi;
  vi.tbase = (size_t)t * a.V;
  vi.x0 = load3(a.verts + 3 * (size_t)v);
  vi.x1 = load3(a.vert_xyz + 3 * (vi.tbase + v));
  vi.R = arap_rotation(a, vi.tbase + v);
  return vi;
}

// entry k of the edge arrays; an entry outside [0, V) contributes nothing and is never used as an index
GSR_HD void arap_edge(const ArapCall& a, const ArapVertex& vi, long long k, ArapAcc<false>& c) {
  const int j = a.nbr[k];
  if ((unsigned)j >= (unsigned)a.V) return;
  const D3 p = vi.x0 - load3(a.verts + 3 * (size_t)j);
  const D3 s = (vi.x1 - load3(a.vert_xyz + 3 * (vi.tbase + j))) - mul(vi.R, p);
  c.e = fma((double)a.w[k], dot(s, s), c.e);
}
GSR_HD void arap_edge(const ArapCall& a, const ArapVertex& vi, long long k, ArapAcc<true>& c) {
  const int j = a.nbr[k];
  if ((unsigned)j >= (unsigned)a.V) return;
  const double w = (double)a.w[k];
  const D3 p = vi.x0 - load3(a.verts + 3 * (size_t)j);
  const D3 d = vi.x1 - load3(a.vert_xyz + 3 * (vi.tbase + j));
  const D3 rp = mul(vi.R, p);
  const D3 ws = w * (d - rp);
  c.gx = c.gx + w * ((2.0 * d - rp) - mul(arap_rotation(a, vi.tbase + j), p));
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double wsr = r == 0 ? ws.x : r == 1 ? ws.y : ws.z;
    c.G.r[r] = c.G.r[r] + wsr * p;
  }
}

GSR_HD void arap_store_grads(const ArapCall& a, size_t tv, const ArapAcc<true>& c, double g, float* dxyz,
                             float* drot) {
  store3(dxyz + 3 * tv, (2.0 * g) * c.gx);
  M33 gR;
#pragma unroll
  for (int r = 0; r < 3; ++r) gR.r[r] = (-2.0 * g) * c.G.r[r];
  if (a.rot_form == GSR_ARAP_QUAT) {
    const Q4 gq = quat_matrix_grad(load_xyzw(a.vert_rot + 4 * tv), gR);
    *(float4*)(drot + 4 * tv) = make_float4((float)gq.v.x, (float)gq.v.y, (float)gq.v.z, (float)gq.w);
  } else {
#pragma unroll
    for (int r = 0; r < 3; ++r) store3(drot + 9 * tv + 3 * r, gR.r[r]);
  }
}
GSR_HD void arap_store_zero(const ArapCall& a, size_t tv, float* dxyz, float* drot) {  // exactly +0
  store3(dxyz + 3 * tv, d3(0.0, 0.0, 0.0));
  const int n = a.rot_form == GSR_ARAP_QUAT ? 4 : 9;
  for (int k = 0; k < n; ++k) drot[(size_t)n * tv + k] = 0.0f;
}

__device__ __forceinline__ void arap_wave_sum(ArapAcc<false>& c) { c.e = wave_sum_f64(c.e); }
__device__ __forceinline__ void arap_wave_sum(ArapAcc<true>& c) {
  c.gx = wave_sum_d3(c.gx);
#pragma unroll
  for (int r = 0; r < 3; ++r) c.G.r[r] = wave_sum_d3(c.G.r[r]);
}

// The row sums of vertex v at frame t (valid = v < V; every lane of the wave calls this, valid or not).  b .. e: the
// lane's row, clamped to [0, E], empty for an invalid lane.
template <bool BWD>
__device__ __forceinline__ void arap_rows(const ArapCall& a, int t, int v, bool valid, long long& b, long long& e,
                                          ArapAcc<BWD>& acc) {
  arap_zero(acc);
  b = e = 0;
  if (valid) {
    row_range(a.offsets, v, a.E, b, e);
    e = e < b ? b : e;
  }
  const bool is_long = e - b > GSR_ARAP_LANE_ROW;
  if (e > b && !is_long) {
    const ArapVertex vi = arap_vertex(a, t, v);
    for (long long k = b; k < e; ++k) arap_edge(a, vi, k, acc);
  }
  unsigned long long todo = __ballot(is_long);  // (wave-uniform: every lane runs the same rounds)
  const int lane = threadIdx.x & 63;
  while (todo != 0ull) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const int vs = __shfl(v, src, 64);
    const long long bs = __shfl(b, src, 64), es = __shfl(e, src, 64);
    const ArapVertex vi = arap_vertex(a, t, vs);  // (one address for the wave: a broadcast)
    ArapAcc<BWD> part;
    arap_zero(part);
    for (long long k = bs + lane; k < es; k += 64) arap_edge(a, vi, k, part);
    arap_wave_sum(part);
    if (lane == src) acc = part;
  }
}

__global__ __launch_bounds__(GSR_ARAP_BLOCK) void k_arap_forward(ArapCall a, int blocks_per_frame,
                                                                 double* __restrict__ partial) {
  __shared__ double wave_e[GSR_ARAP_BLOCK / 64];
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_ARAP_BLOCK + threadIdx.x;
  long long b, e;
  ArapAcc<false> acc;
  arap_rows<false>(a, t, v, v < a.V, b, e, acc);
  const double s = wave_sum_f64(acc.e);
  if ((threadIdx.x & 63) == 0) wave_e[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = wave_e[0];
#pragma unroll
    for (int k = 1; k < GSR_ARAP_BLOCK / 64; ++k) sum += wave_e[k];
    partial[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(64) void k_arap_reduce(int blocks_per_frame, const double* __restrict__ partial,
                                                    float* __restrict__ energy) {
  const double* p = partial + (size_t)blockIdx.x * blocks_per_frame;
  double s = 0.0;
  for (int k = threadIdx.x; k < blocks_per_frame; k += 64) s += p[k];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) energy[blockIdx.x] = (float)s;
}

__global__ __launch_bounds__(GSR_ARAP_BLOCK) void k_arap_backward(ArapCall a, int blocks_per_frame,
                                                                  const float* __restrict__ g_energy,
                                                                  float* __restrict__ dxyz,
                                                                  float* __restrict__ drot) {
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_ARAP_BLOCK + threadIdx.x;
  const bool valid = v < a.V;
  const size_t tv = (size_t)t * a.V + (valid ? v : 0);
  const double g = (double)g_energy[t];
  if (g == 0.0) {  // (the whole block: one frame per block) nothing flows to the frame
    if (valid) arap_store_zero(a, tv, dxyz, drot);
    return;
  }
  long long b, e;
  ArapAcc<true> acc;
  arap_rows<true>(a, t, v, valid, b, e, acc);
  if (!valid) return;
  if (e > b)
    arap_store_grads(a, tv, acc, g, dxyz, drot);
  else
    arap_store_zero(a, tv, dxyz, drot);  // an empty row: exactly 0
}

static int arap_blocks_per_frame(int V) { return div_up(V > 0 ? V : 1, GSR_ARAP_BLOCK); }

size_t arap_workspace_bytes(int T, int V) {
  return align_up(sizeof(double) * (size_t)(T > 0 ? T : 1) * (size_t)arap_blocks_per_frame(V), 256);
}

void launch_arap_forward(const ArapCall& c, float* energy, void* workspace, hipStream_t stream) {
  const int nb = arap_blocks_per_frame(c.V);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_arap_forward, dim3((unsigned)((long long)c.T * nb)), dim3(GSR_ARAP_BLOCK), 0, stream, c, nb,
                     partial);
  hipLaunchKernelGGL(k_arap_reduce, dim3(c.T), dim3(64), 0, stream, nb, partial, energy);
}

void launch_arap_backward(const ArapCall& c, const float* g_energy, float* dxyz, float* drot, hipStream_t stream) {
  const int nb = arap_blocks_per_frame(c.V);
  hipLaunchKernelGGL(k_arap_backward, dim3((unsigned)((long long)c.T * nb)), dim3(GSR_ARAP_BLOCK), 0, stream, c, nb,
                     g_energy, dxyz, drot);
}

}  // namespace gsr
