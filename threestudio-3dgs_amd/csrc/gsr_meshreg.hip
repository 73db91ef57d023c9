// gsr_meshreg.hip — the normal-consistency and uniform-Laplacian regularisers of the deformed SuGaR surface, forward
// and backward (include/gsr.h gsr_sugar_normal_consistency_* / gsr_sugar_laplacian_*; replace pytorch3d's
// mesh_normal_consistency and mesh_laplacian_smoothing(., "uniform") on the Meshes that system/sugar_static.py and
// system/sugar_4dgen.py rebuild every step: the edge sort, the face-pair enumeration, the sparse (V, V) Laplacian and
// the atomic scatters of their backwards).  The topology is fixed: its tables are built once (sugar_meshreg.py).  The
// formulas are in the header.
//
// Precision: fp64 arithmetic from the fp32 inputs, every loss and gradient rounded to fp32 once.
//
//   k_nc_forward     one lane per (t, pair), 256 lanes per block, a block within one frame: 1 - cos of the pair; the
//                    block's 256 terms are added in a fixed order into one fp64 partial sum.
//   k_lap_forward    one lane per (t, vertex): walks its one-ring, |d_i|; block sums as above.
//   k_meshreg_reduce one wave per frame: adds the frame's partial sums in a fixed order, divides by P (V), writes.
//   k_nc_corner_rows one lane per (t, pair): recomputes the pair and writes the four fp64 gradient rows of its corners,
//                    times g_t / P.
//   k_nc_gather      one lane per (t, vertex): adds the rows its slot row names, in order, rounds once.
//   k_lap_rows       one lane per (t, vertex): recomputes d_i and writes u_i = g_t d_i / (V |d_i|) in fp64.
//   k_lap_gather     one lane per (t, vertex): -u_i + sum over its ring of u_j / deg_j.
// Long rows: a lane walks a row of at most GSR_MESHREG_LANE_ROW entries itself.  A longer row (a fan hub: 200 ring
// entries and 200 slots) is left for the lane's wave, as in gsr_arap.hip: after the short rows the wave takes its long
// rows one by one in lane order, lane l adding entries l, l + 64, ..., and the 64 partial sums are added by
// wave_sum_f64's butterfly.  What an entry adds depends on the frame and the entry alone, so any lane can add it.
// The walks are gathers of 24-byte rows: the loops carry no dependence but the sum, so the loads of a row are in
// flight together.  No atomics: every sum's order is fixed by the input.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

#define GSR_MESHREG_BLOCK 256
#define GSR_MESHREG_LANE_ROW 32  // the longest row one lane walks alone
#define GSR_NC_EPS 1e-8          // cosine_similarity's clamp of each norm

GSR_HD D3 load3d(const double* p) { return d3(p[0], p[1], p[2]); }
GSR_HD void store3d(double* p, D3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}

// The sum of what entry(k) gives over row v of a CSR table of n entries (valid = the lane has a row; every lane of the
// wave calls this, valid or not).  len: the row's length after clamping, 0 for an invalid lane.
template <class F>
__device__ __forceinline__ D3 row_sum(const int* offsets, long long n, int v, bool valid, long long& len, F entry) {
  long long b = 0, e = 0;
  if (valid) {
    row_range(offsets, v, n, b, e);
    e = e < b ? b : e;
  }
  len = e - b;
  D3 acc = d3(0.0, 0.0, 0.0);
  const bool is_long = len > GSR_MESHREG_LANE_ROW;
  if (!is_long)
    for (long long k = b; k < e; ++k) acc = acc + entry(k);
  unsigned long long todo = __ballot(is_long);  // (wave-uniform: every lane runs the same rounds)
  const int lane = threadIdx.x & 63;
  while (todo != 0ull) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const long long bs = __shfl(b, src, 64), es = __shfl(e, src, 64);
    D3 part = d3(0.0, 0.0, 0.0);
    for (long long k = bs + lane; k < es; k += 64) part = part + entry(k);
    part = wave_sum_d3(part);
    if (lane == src) acc = part;
  }
  return acc;
}

// the block's 256 terms into partial[blockIdx.x]: the butterfly per wave, then the four wave sums in order
__device__ __forceinline__ void block_partial(double term, double* __restrict__ partial) {
  __shared__ double wave_s[GSR_MESHREG_BLOCK / 64];
  const double s = wave_sum_f64(term);
  if ((threadIdx.x & 63) == 0) wave_s[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = wave_s[0];
#pragma unroll
    for (int k = 1; k < GSR_MESHREG_BLOCK / 64; ++k) sum += wave_s[k];
    partial[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(64) void k_meshreg_reduce(int blocks_per_frame, int count,
                                                       const double* __restrict__ partial, float* __restrict__ out) {
  const double* p = partial + (size_t)blockIdx.x * blocks_per_frame;
  double s = 0.0;
  for (int k = threadIdx.x; k < blocks_per_frame; k += 64) s += p[k];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(s / (double)count);
}

// ---- normal consistency ---------------------------------------------------------------------------------------------
// pair p at frame t (tbase = t V): false when one of its entries is outside [0, V): nothing of it is then dereferenced
struct NcPair {
  int4 i;          // a, b, c0, c1
  D3 e, f0, f1;    // x_b - x_a, x_c0 - x_a, x_c1 - x_a
  D3 n0, n1;
  double l0, l1, m0, m1, cosv;
};
GSR_HD bool nc_pair(const MeshRegCall& a, size_t tbase, int p, NcPair& q) {
  q.i = *(const int4*)(a.pairs + 4 * (size_t)p);
  if (!(in_range(q.i.x, a.V) && in_range(q.i.y, a.V) && in_range(q.i.z, a.V) && in_range(q.i.w, a.V))) return false;
  const float* x = a.vert_xyz + 3 * tbase;
  const D3 xa = load3(x + 3 * (size_t)q.i.x);
  q.e = load3(x + 3 * (size_t)q.i.y) - xa;
  q.f0 = load3(x + 3 * (size_t)q.i.z) - xa;
  q.f1 = load3(x + 3 * (size_t)q.i.w) - xa;
  q.n0 = cross(q.e, q.f0);
  q.n1 = -1.0 * cross(q.e, q.f1);
  q.l0 = sqrt(dot(q.n0, q.n0));
  q.l1 = sqrt(dot(q.n1, q.n1));
  q.m0 = fmax(q.l0, GSR_NC_EPS);
  q.m1 = fmax(q.l1, GSR_NC_EPS);
  q.cosv = dot(q.n0, q.n1) / (q.m0 * q.m1);
  return true;
}

__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_nc_forward(MeshRegCall a, int blocks_per_frame,
                                                                  double* __restrict__ partial) {
  const int t = blockIdx.x / blocks_per_frame;
  const int p = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  double term = 0.0;
  NcPair q;
  if (p < a.P && nc_pair(a, (size_t)t * a.V, p, q)) term = 1.0 - q.cosv;
  block_partial(term, partial);
}

// rows (T, 4 P, 3) fp64: row 4 p + role of frame t is the gradient the pair sends to its corner `role`
__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_nc_corner_rows(MeshRegCall a, int blocks_per_frame,
                                                                      const float* __restrict__ g_nc,
                                                                      double* __restrict__ rows) {
  const int t = blockIdx.x / blocks_per_frame;
  const int p = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  const double g = (double)g_nc[t];
  if (g == 0.0 || p >= a.P) return;  // (a frame nothing flows to: k_nc_gather does not read its rows)
  double* r = rows + 3 * (4 * ((size_t)t * a.P + p));
  const D3 zero = d3(0.0, 0.0, 0.0);
  D3 ga = zero, gb = zero, gc0 = zero, gc1 = zero;
  NcPair q;
  if (nc_pair(a, (size_t)t * a.V, p, q)) {
    // d(1 - cos) g / P to the two normals.  torch clamps the value of a norm only (in place, outside autograd): the
    // norm's own gradient n / |n| flows whether the clamp holds or not, and is 0 at n = 0
    const double s = -g / (double)a.P, im = 1.0 / (q.m0 * q.m1);
    D3 gn0 = (s * im) * q.n1, gn1 = (s * im) * q.n0;
    if (q.l0 > 0.0) gn0 = gn0 - (s * q.cosv / (q.m0 * q.l0)) * q.n0;
    if (q.l1 > 0.0) gn1 = gn1 - (s * q.cosv / (q.m1 * q.l1)) * q.n1;
    // n0 = e x f0, n1 = -(e x f1)
    const D3 gm1 = -1.0 * gn1;
    gb = cross(q.f0, gn0) + cross(q.f1, gm1);
    gc0 = cross(gn0, q.e);
    gc1 = cross(gm1, q.e);
    ga = zero - (gb + gc0 + gc1);
  }
  store3d(r, ga), store3d(r + 3, gb), store3d(r + 6, gc0), store3d(r + 9, gc1);
}

__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_nc_gather(MeshRegCall a, int blocks_per_frame,
                                                                 const float* __restrict__ g_nc,
                                                                 const double* __restrict__ rows,
                                                                 float* __restrict__ dxyz) {
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  const bool valid = v < a.V;
  float* out = dxyz + 3 * ((size_t)t * a.V + (valid ? v : 0));
  if ((double)g_nc[t] == 0.0) {  // (the whole block: one frame per block)
    if (valid) store3(out, d3(0.0, 0.0, 0.0));
    return;
  }
  const long long n = 4ll * a.P;
  const double* frame = rows + 3 * ((size_t)t * (size_t)n);
  long long len;
  const D3 sum = row_sum(a.slot_offsets, n, v, valid, len, [&](long long k) {
    const int s = a.slots[k];
    return in_range(s, n) ? load3d(frame + 3 * (size_t)s) : d3(0.0, 0.0, 0.0);
  });
  if (valid) store3(out, sum);  // an empty row: exactly +0
}

// ---- the uniform Laplacian --------------------------------------------------------------------------------------------
// d_v at frame t (every lane of the wave calls this)
__device__ __forceinline__ D3 lap_d(const MeshRegCall& a, int t, int v, bool valid) {
  const float* x = a.vert_xyz + 3 * ((size_t)t * a.V);
  const long long n = 2ll * a.E;
  long long deg;
  const D3 sum = row_sum(a.ring_offsets, n, v, valid, deg, [&](long long k) {
    const int j = a.ring[k];
    return in_range(j, a.V) ? load3(x + 3 * (size_t)j) : d3(0.0, 0.0, 0.0);
  });
  if (!valid) return d3(0.0, 0.0, 0.0);
  const D3 xi = load3(x + 3 * (size_t)v);
  return deg > 0 ? (1.0 / (double)deg) * sum - xi : d3(0.0, 0.0, 0.0) - xi;
}

__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_lap_forward(MeshRegCall a, int blocks_per_frame,
                                                                   double* __restrict__ partial) {
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  const D3 d = lap_d(a, t, v, v < a.V);
  block_partial(sqrt(dot(d, d)), partial);
}

// u (T, V, 3) fp64
__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_lap_rows(MeshRegCall a, int blocks_per_frame,
                                                                const float* __restrict__ g_lap,
                                                                double* __restrict__ u) {
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  const double g = (double)g_lap[t];
  if (g == 0.0) return;  // (the whole block) k_lap_gather does not read the frame's rows
  const bool valid = v < a.V;
  const D3 d = lap_d(a, t, v, valid);
  if (!valid) return;
  const double len = sqrt(dot(d, d));
  store3d(u + 3 * ((size_t)t * a.V + v), len > 0.0 ? (g / ((double)a.V * len)) * d : d3(0.0, 0.0, 0.0));
}

__global__ __launch_bounds__(GSR_MESHREG_BLOCK) void k_lap_gather(MeshRegCall a, int blocks_per_frame,
                                                                  const float* __restrict__ g_lap,
                                                                  const double* __restrict__ u,
                                                                  float* __restrict__ dxyz) {
  const int t = blockIdx.x / blocks_per_frame;
  const int v = (blockIdx.x % blocks_per_frame) * GSR_MESHREG_BLOCK + threadIdx.x;
  const bool valid = v < a.V;
  const size_t tv = (size_t)t * a.V + (valid ? v : 0);
  if ((double)g_lap[t] == 0.0) {
    if (valid) store3(dxyz + 3 * tv, d3(0.0, 0.0, 0.0));
    return;
  }
  const long long n = 2ll * a.E;
  const double* frame = u + 3 * ((size_t)t * a.V);
  long long len;
  const D3 sum = row_sum(a.ring_offsets, n, v, valid, len, [&](long long k) {
    const int j = a.ring[k];
    if (!in_range(j, a.V)) return d3(0.0, 0.0, 0.0);
    long long b, e;
    row_range(a.ring_offsets, j, n, b, e);  // (j has i in its row: deg_j >= 1 on a symmetric table)
    return e > b ? (1.0 / (double)(e - b)) * load3d(frame + 3 * (size_t)j) : d3(0.0, 0.0, 0.0);
  });
  if (valid) store3(dxyz + 3 * tv, sum - load3d(frame + 3 * (size_t)v));
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int meshreg_blocks(int n) { return div_up(n > 0 ? n : 1, GSR_MESHREG_BLOCK); }

size_t meshreg_workspace_bytes(int T, int V, int P, int pass) {
  const size_t t = (size_t)(T > 0 ? T : 1);
  if (pass == GSR_MESHREG_FORWARD) return align_up(sizeof(double) * t * (size_t)meshreg_blocks(P > V ? P : V), 256);
  const size_t rows = pass == GSR_MESHREG_NC_BACKWARD ? 4 * (size_t)P : (size_t)V;
  return align_up(3 * sizeof(double) * t * (rows > 0 ? rows : 1), 256);
}

template <class K, class... Args>
static void launch_frames(K kernel, const MeshRegCall& c, int nb, hipStream_t stream, Args... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)c.T * nb)), dim3(GSR_MESHREG_BLOCK), 0, stream, c, nb, args...);
}

void launch_normal_consistency_forward(const MeshRegCall& c, float* nc, void* workspace, hipStream_t stream) {
  const int nb = meshreg_blocks(c.P);
  double* partial = (double*)workspace;
  launch_frames(k_nc_forward, c, nb, stream, partial);
  hipLaunchKernelGGL(k_meshreg_reduce, dim3(c.T), dim3(64), 0, stream, nb, c.P, partial, nc);
}

void launch_normal_consistency_backward(const MeshRegCall& c, const float* g_nc, float* dxyz, void* workspace,
                                        hipStream_t stream) {
  double* rows = (double*)workspace;
  launch_frames(k_nc_corner_rows, c, meshreg_blocks(c.P), stream, g_nc, rows);
  launch_frames(k_nc_gather, c, meshreg_blocks(c.V), stream, g_nc, (const double*)rows, dxyz);
}

void launch_laplacian_forward(const MeshRegCall& c, float* lap, void* workspace, hipStream_t stream) {
  const int nb = meshreg_blocks(c.V);
  double* partial = (double*)workspace;
  launch_frames(k_lap_forward, c, nb, stream, partial);
  hipLaunchKernelGGL(k_meshreg_reduce, dim3(c.T), dim3(64), 0, stream, nb, c.V, partial, lap);
}

void launch_laplacian_backward(const MeshRegCall& c, const float* g_lap, float* dxyz, void* workspace,
                               hipStream_t stream) {
  const int nb = meshreg_blocks(c.V);
  double* u = (double*)workspace;
  launch_frames(k_lap_rows, c, nb, stream, g_lap, u);
  launch_frames(k_lap_gather, c, nb, stream, g_lap, (const double*)u, dxyz);
}

}  // namespace gsr
