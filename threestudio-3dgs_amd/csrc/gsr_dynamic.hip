// gsr_dynamic.hip — the time-batched geometry of dynamic SuGaR, forward and backward (include/gsr.h gsr_sugar_skin_*
// and gsr_sugar_timed_*; replaces DynamicSuGaRModel._get_timed_vertex_attributes_from_dg, get_timed_gs_attributes,
// fuse_rotations and get_timed_gs_normals of geometry/dynamic_sugar.py:329-346, 505-575, 618-688: the (T, V, K, 4)
// node gather, pypose's Log / Exp, the dual-quaternion blend, the (T, N, 3, 4) vertex gather, the pytorch3d face
// normals and the index_put scatters of their autograd backward).  The formulas are in the header.
//
// Precision: fp64 arithmetic from the fp32 inputs, every output and gradient rounded to fp32 once; what passes
// between two kernels of a backward (the adjoint rows) is fp32, one rounding each, and is added in fp64.
//
// Skinning (T frames, V vertices, P nodes, K nodes per vertex):
//   k_skin_nodes     one lane per (t, node): q^ = q / |q|, d = 1/2 (trans, 0) (x) q^ and Log(q), 11 doubles in the
//                    workspace (88 T P bytes: L2 resident), so that no per-item work repeats per-node work.
//   k_skin_forward   one lane per (t, vertex): the K-sums over its nodes' records, the blend, three stores.
//   k_skin_vertex    (backward) one lane per (t, vertex): recomputes the sums, writes the vertex's adjoint row (to
//                    S_r, S_d and the summed Log: 11 floats) and its dL/dverts term.
//   k_skin_verts_sum one lane per vertex: dL/dverts = the sum of its T terms, t ascending.
//   k_skin_node      one wave per (t, node): w x row over the node's incidence list (lane l takes entries l, l + 64,
//                    ... in order; the 64 partial sums are added by a butterfly), then the per-node chain once.
// Timed Gaussians (F faces, G Gaussians per face, N = F G):
//   k_timed_forward  one lane per (t, face): three Logs and the normal once, then its G Gaussians.
//   k_timed_face     (backward) one lane per (t, face): recomputes, writes three corner rows (10 floats each: to the
//                    corner's position, rotation and scale).
//   k_timed_vertex   one lane per (t, vertex): adds its corner rows in corner_order.
//   k_timed_gauss    one lane per Gaussian: recomputes its rotation for t = 0 .. T-1 and adds dL/drotation0 and
//                    dL/dlog_scales in that order.
// The face normal and its adjoint, the barycentric table, the rows of the two incidence tables (corner_order,
// item_order) and the fp64 butterfly are those of gsr_sugar.h, shared with gsr_mesh.hip and gsr_arap.hip.
// No atomics: every sum's order is fixed by the input.  The bodies are host-callable functions of an item index (the
// kernels only derive the index), so they can be stepped through on the CPU.
#include <math.h>

#include "gsr_kernels.h"
#include "gsr_sugar.h"

namespace gsr {

#define GSR_SKIN_REC 11   // doubles per (t, node): q^ (4), d (4), Log q (3)
#define GSR_SKIN_ROW 11   // floats per (t, vertex): dL/dS_r (4), dL/dS_d (4), dL/dsum Log (3)
#define GSR_TIMED_ROW 10  // floats per (t, face, corner): dL/dxyz (3), dL/drot (4, xyzw), dL/dscale (3)

GSR_HD Q4 rec_q(const double* r) { return q4(d3(r[0], r[1], r[2]), r[3]); }
GSR_HD D3 rec_d3(const double* r) { return d3(r[0], r[1], r[2]); }
GSR_HD Q4 load_q_row(const float* p) { return q4(d3((double)p[0], (double)p[1], (double)p[2]), (double)p[3]); }
GSR_HD Q4 load_wxyz(const float* p) {
  const float4 q = *(const float4*)p;
  return q4(d3((double)q.y, (double)q.z, (double)q.w), (double)q.x);
}
GSR_HD void store_wxyz(float* p, Q4 q) {
  *(float4*)p = make_float4((float)q.w, (float)q.v.x, (float)q.v.y, (float)q.v.z);
}

// ---- skinning ---------------------------------------------------------------------------------------------------
GSR_HD void skin_node_record(const SkinCall& a, long long i, double* nodes) {  // i = t P + node
  const Q4 q = load_xyzw(a.node_rots + 4 * i);
  const Q4 qh = (1.0 / sqrt(dot(q, q))) * q;
  const Q4 d = 0.5 * qmul(q4(load3(a.node_trans + 3 * i), 0.0), qh);
  const D3 phi = qlog(q);
  double* r = nodes + GSR_SKIN_REC * i;
  r[0] = qh.v.x, r[1] = qh.v.y, r[2] = qh.v.z, r[3] = qh.w;
  r[4] = d.v.x, r[5] = d.v.y, r[6] = d.v.z, r[7] = d.w;
  r[8] = phi.x, r[9] = phi.y, r[10] = phi.z;
}

// The K-sums of vertex v at frame t.  With gx != null (the backward, "lbs") dp also collects sum_k w_k R(q^_k)^T gx.
struct SkinSums {
  Q4 Sr, Sd;
  D3 phi, sc, lbs, dp;
};
GSR_HD SkinSums skin_sums(const SkinCall& a, const double* nodes, int t, int v, D3 p, const D3* gx) {
  SkinSums s;
  s.Sr = s.Sd = qzero();
  s.phi = s.sc = s.lbs = s.dp = d3(0.0, 0.0, 0.0);
  for (int k = 0; k < a.K; ++k) {
    const size_t it = (size_t)v * a.K + k;
    const int j = a.nbr[it];
    if ((unsigned)j >= (unsigned)a.P) continue;  // not a node: the item contributes nothing
    const double wk = (double)a.w[it];
    const size_t tj = (size_t)t * a.P + j;
    const double* r = nodes + GSR_SKIN_REC * tj;
    const Q4 qh = rec_q(r);
    s.phi = s.phi + wk * rec_d3(r + 8);
    if (a.method == GSR_SKIN_DQS) {
      s.Sr = s.Sr + wk * qh;
      s.Sd = s.Sd + wk * rec_q(r + 4);
    } else {
      const D3 x = load3(a.node_xyz + 3 * (size_t)j);
      s.lbs = s.lbs + wk * (qrotate(qh, p - x) + x + load3(a.node_trans + 3 * tj));
      if (gx != nullptr) s.dp = s.dp + wk * qrotate_grad_p(qh, *gx);
    }
    if (a.node_scales != nullptr) s.sc = s.sc + wk * load3(a.node_scales + 3 * tj);
  }
  return s;
}

GSR_HD void skin_vertex_forward(const SkinCall& a, const double* nodes, long long i, float* xyz, float* rot,
                                float* scale) {  // i = t V + v
  const int t = (int)(i / a.V), v = (int)(i % a.V);
  const D3 p = load3(a.verts + 3 * (size_t)v);
  const SkinSums s = skin_sums(a, nodes, t, v, p, nullptr);
  D3 y = s.lbs;
  if (a.method == GSR_SKIN_DQS) {
    const double im = 1.0 / sqrt(dot(s.Sr, s.Sr));
    const Q4 r = im * s.Sr, e = im * s.Sd;
    y = qrotate(r, p) + 2.0 * qmul(e, conj(r)).v;
  }
  store3(xyz + 3 * i, y);
  store4(rot + 4 * i, qexp(s.phi));
  if (scale != nullptr) store3(scale + 3 * i, s.sc);
}

// the adjoint row of (t, vertex) and its dL/dverts term; g_xyz, g_rot: the upstream gradients or null (zero)
GSR_HD void skin_vertex_backward(const SkinCall& a, const double* nodes, long long i, const float* g_xyz,
                                 const float* g_rot, float* rows, float* dp) {
  const int t = (int)(i / a.V), v = (int)(i % a.V);
  const D3 p = load3(a.verts + 3 * (size_t)v);
  const D3 gx = g_xyz != nullptr ? load3(g_xyz + 3 * i) : d3(0.0, 0.0, 0.0);
  const SkinSums s = skin_sums(a, nodes, t, v, p, &gx);
  Q4 gSr = qzero(), gSd = qzero();
  D3 gp = s.dp;
  if (a.method == GSR_SKIN_DQS && g_xyz != nullptr) {
    // xyz = R(r) p + 2 vec(e (x) conj(r)), r = S_r / m, e = S_d / m, m = |S_r|
    const double im = 1.0 / sqrt(dot(s.Sr, s.Sr));
    const Q4 r = im * s.Sr, e = im * s.Sd;
    const Q4 g4 = q4(gx, 0.0);
    const Q4 ge = 2.0 * qmul(g4, r);
    const Q4 gr = qrotate_grad_q(r, p, gx) + conj(2.0 * qmul(conj(e), g4));
    gSr = im * (gr + (-(dot(gr, r) + dot(ge, e))) * r);
    gSd = im * ge;
    gp = qrotate_grad_p(r, gx);
  }
  D3 gphi = d3(0.0, 0.0, 0.0);
  if (g_rot != nullptr) gphi = qexp_grad(s.phi, load_xyzw(g_rot + 4 * i));
  float* row = rows + GSR_SKIN_ROW * i;
  row[0] = (float)gSr.v.x, row[1] = (float)gSr.v.y, row[2] = (float)gSr.v.z, row[3] = (float)gSr.w;
  row[4] = (float)gSd.v.x, row[5] = (float)gSd.v.y, row[6] = (float)gSd.v.z, row[7] = (float)gSd.w;
  store3(row + 8, gphi);
  store3(dp + 3 * i, gp);
}

// What one wave adds up for a (t, node): dqs: A = sum w dL/dS_r, B = sum w dL/dS_d; lbs: A = the sum of the items'
// gradients to q^, B.v = sum w dL/dxyz; both: C = sum w dL/dsum Log, D = sum w dL/dscale.
struct SkinNodeAcc {
  Q4 A, B;
  D3 C, D;
};
GSR_HD void skin_node_item(const SkinCall& a, const double* nodes, int t, int j, int item, const float* rows,
                           const float* g_xyz, const float* g_scale, SkinNodeAcc& acc) {
  const int v = item / a.K;
  const double wk = (double)a.w[item];
  const size_t tv = (size_t)t * a.V + v;
  const float* row = rows + GSR_SKIN_ROW * tv;
  if (a.method == GSR_SKIN_DQS) {
    acc.A = acc.A + wk * load_q_row(row);
    acc.B = acc.B + wk * load_q_row(row + 4);
  } else if (g_xyz != nullptr) {
    const D3 gx = load3(g_xyz + 3 * tv);
    const Q4 qh = rec_q(nodes + GSR_SKIN_REC * ((size_t)t * a.P + j));
    const D3 b = load3(a.verts + 3 * (size_t)v) - load3(a.node_xyz + 3 * (size_t)j);
    acc.A = acc.A + wk * qrotate_grad_q(qh, b, gx);
    acc.B.v = acc.B.v + wk * gx;
  }
  acc.C = acc.C + wk * load3(row + 8);
  if (g_scale != nullptr) acc.D = acc.D + wk * load3(g_scale + 3 * tv);
}

GSR_HD void skin_node_finish(const SkinCall& a, long long i, const SkinNodeAcc& acc, bool used, float* dtrans,
                             float* drots, float* dscales) {  // i = t P + node
  if (dscales != nullptr) store3(dscales + 3 * i, used ? acc.D : d3(0.0, 0.0, 0.0));
  if (!used) {  // no vertex uses the node: exactly 0
    store3(dtrans + 3 * i, d3(0.0, 0.0, 0.0));
    store4(drots + 4 * i, qzero());
    return;
  }
  const Q4 q = load_xyzw(a.node_rots + 4 * i);
  const double len = sqrt(dot(q, q));
  const Q4 qh = (1.0 / len) * q;
  Q4 gqh = acc.A;
  D3 gt = acc.B.v;
  if (a.method == GSR_SKIN_DQS) {  // d = 1/2 (trans, 0) (x) q^
    const D3 tr = load3(a.node_trans + 3 * i);
    gqh = gqh + 0.5 * qmul(q4(-1.0 * tr, 0.0), acc.B);
    gt = 0.5 * qmul(acc.B, conj(qh)).v;
  }
  store3(dtrans + 3 * i, gt);
  store4(drots + 4 * i, qnormalize_grad(gqh, qh, len) + qlog_grad(q, acc.C));
}

__global__ __launch_bounds__(256) void k_skin_nodes(SkinCall a, double* __restrict__ nodes) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.P) skin_node_record(a, i, nodes);
}

__global__ __launch_bounds__(256) void k_skin_forward(SkinCall a, const double* __restrict__ nodes,
                                                      float* __restrict__ xyz, float* __restrict__ rot,
                                                      float* __restrict__ scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.V) skin_vertex_forward(a, nodes, i, xyz, rot, scale);
}

__global__ __launch_bounds__(256) void k_skin_vertex(SkinCall a, const double* __restrict__ nodes,
                                                     const float* __restrict__ g_xyz, const float* __restrict__ g_rot,
                                                     float* __restrict__ rows, float* __restrict__ dp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.V) skin_vertex_backward(a, nodes, i, g_xyz, g_rot, rows, dp);
}

__global__ __launch_bounds__(256) void k_skin_verts_sum(int T, int V, const float* __restrict__ dp,
                                                        float* __restrict__ dverts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  D3 s = d3(0.0, 0.0, 0.0);
  for (int t = 0; t < T; ++t) s = s + load3(dp + 3 * ((size_t)t * V + v));
  store3(dverts + 3 * (size_t)v, s);
}

__global__ __launch_bounds__(64) void k_skin_node(SkinCall a, const double* __restrict__ nodes,
                                                  const int* __restrict__ item_order,
                                                  const int* __restrict__ node_offsets,
                                                  const float* __restrict__ rows, const float* __restrict__ g_xyz,
                                                  const float* __restrict__ g_scale, float* __restrict__ dtrans,
                                                  float* __restrict__ drots, float* __restrict__ dscales) {
  const long long i = blockIdx.x;  // t P + node
  const int t = (int)(i / a.P), j = (int)(i % a.P);
  const long long n = (long long)a.V * a.K;
  long long b, e;
  row_range(node_offsets, j, n, b, e);
  SkinNodeAcc acc;
  acc.A = acc.B = qzero();
  acc.C = acc.D = d3(0.0, 0.0, 0.0);
  for (long long k = b + threadIdx.x; k < e; k += 64) {
    const int item = item_order[k];
    if (!in_range(item, n)) continue;  // not an item: skipped
    skin_node_item(a, nodes, t, j, item, rows, g_xyz, g_scale, acc);
  }
  acc.A = wave_sum_q4(acc.A);
  acc.B = wave_sum_q4(acc.B);
  acc.C = wave_sum_d3(acc.C);
  acc.D = wave_sum_d3(acc.D);
  if (threadIdx.x == 0) skin_node_finish(a, i, acc, e > b, dtrans, drots, dscales);
}

size_t skin_nodes_bytes(int T, int P) {
  return align_up(sizeof(double) * GSR_SKIN_REC * (size_t)(T > 0 ? T : 1) * (size_t)(P > 0 ? P : 1), 256);
}
size_t skin_workspace_bytes(int T, int V, int P) {
  const size_t tv = (size_t)(T > 0 ? T : 1) * (size_t)(V > 0 ? V : 1);
  return skin_nodes_bytes(T, P) + align_up(sizeof(float) * GSR_SKIN_ROW * tv, 256) +
         align_up(sizeof(float) * 3 * tv, 256);
}

void launch_skin_forward(const SkinCall& c, float* xyz, float* rot, float* scale, void* workspace,
                         hipStream_t stream) {
  double* nodes = (double*)workspace;
  hipLaunchKernelGGL(k_skin_nodes, dim3(div_up((long long)c.T * c.P, 256)), dim3(256), 0, stream, c, nodes);
  hipLaunchKernelGGL(k_skin_forward, dim3(div_up((long long)c.T * c.V, 256)), dim3(256), 0, stream, c, nodes, xyz,
                     rot, scale);
}

void launch_skin_backward(const SkinCall& c, const int* item_order, const int* node_offsets, const float* g_xyz,
                          const float* g_rot, const float* g_scale, float* dverts, float* dtrans, float* drots,
                          float* dscales, void* workspace, hipStream_t stream) {
  char* ws = (char*)workspace;
  double* nodes = (double*)ws;
  float* rows = (float*)(ws + skin_nodes_bytes(c.T, c.P));
  float* dp = (float*)((char*)rows + align_up(sizeof(float) * GSR_SKIN_ROW * (size_t)c.T * (size_t)c.V, 256));
  hipLaunchKernelGGL(k_skin_nodes, dim3(div_up((long long)c.T * c.P, 256)), dim3(256), 0, stream, c, nodes);
  hipLaunchKernelGGL(k_skin_vertex, dim3(div_up((long long)c.T * c.V, 256)), dim3(256), 0, stream, c, nodes, g_xyz,
                     g_rot, rows, dp);
  hipLaunchKernelGGL(k_skin_verts_sum, dim3(div_up(c.V, 256)), dim3(256), 0, stream, c.T, c.V, dp, dverts);
  hipLaunchKernelGGL(k_skin_node, dim3(c.T * c.P), dim3(64), 0, stream, c, nodes, item_order, node_offsets, rows,
                     g_xyz, g_scale, dtrans, drots, c.node_scales != nullptr ? dscales : nullptr);
}

// ---- timed Gaussians --------------------------------------------------------------------------------------------
// a face at frame t: its corners' positions, rotations (and their Logs) and scales, the normal's chain
struct TimedFace : FaceNormal {
  int i[3];
  D3 p[3], L[3], s[3];
  Q4 q[3];
};
// false (nothing dereferenced) when a face entry is outside [0, V)
GSR_HD bool timed_face(const TimedCall& a, int t, int f, bool normal, TimedFace& fc) {
  if (!face_corners(a.faces, a.V, f, fc.i)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t tv = (size_t)t * a.V + fc.i[c];
    fc.p[c] = load3(a.vert_xyz + 3 * tv);
    fc.q[c] = load_xyzw(a.vert_rot + 4 * tv);
    fc.L[c] = qlog(fc.q[c]);
    fc.s[c] = a.vert_scale != nullptr ? load3(a.vert_scale + 3 * tv) : d3(0.0, 0.0, 0.0);
  }
  if (normal) static_cast<FaceNormal&>(fc) = face_normal(fc.p[0], fc.p[1], fc.p[2]);
  return true;
}
GSR_HD D3 bary_mix(const FaceBary& b, int g, const D3* x) {
  return (double)b.w[g][0] * x[0] + (double)b.w[g][1] * x[1] + (double)b.w[g][2] * x[2];
}
// Q = Exp(phi) (x) q0 before its normalisation
struct TimedRot {
  D3 phi;
  Q4 E, q0, Q;
  double len;
};
GSR_HD TimedRot timed_rot(const TimedCall& a, const FaceBary& b, const TimedFace& fc, int g, size_t n) {
  TimedRot r;
  r.phi = bary_mix(b, g, fc.L);
  r.E = qexp(r.phi);
  r.q0 = load_wxyz(a.rotation0 + 4 * n);
  r.Q = qmul(r.E, r.q0);
  r.len = sqrt(dot(r.Q, r.Q));
  return r;
}
// the gradient to Q of Q / max(|Q|, 1e-12), given the upstream gradient (w, x, y, z) of the rotation
GSR_HD Q4 timed_rot_grad(const TimedRot& r, const float* g_rotation) {
  const Q4 gu = load_wxyz(g_rotation);
  if (!(r.len >= 1e-12)) return 1e12 * gu;
  const Q4 u = (1.0 / r.len) * r.Q;
  return (1.0 / r.len) * (gu + (-dot(u, gu)) * u);
}

GSR_HD void timed_face_forward(const TimedCall& a, const FaceBary& b, long long i, float* xyz, float* rotation,
                               float* normals, float* scaling) {  // i = t F + f
  const int t = (int)(i / a.F), f = (int)(i % a.F);
  const size_t N = (size_t)a.F * a.G;
  TimedFace fc;
  const bool ok = timed_face(a, t, f, true, fc);
  for (int g = 0; g < a.G; ++g) {
    const size_t n = (size_t)f * a.G + g, o = (size_t)t * N + n;
    if (!ok) {  // a face entry out of range: zeros
      const D3 zero = d3(0.0, 0.0, 0.0);
      store3(xyz + 3 * o, zero);
      store3(normals + 3 * o, zero);
      store_wxyz(rotation + 4 * o, qzero());
      if (scaling != nullptr) store3(scaling + 3 * o, zero);
      continue;
    }
    store3(xyz + 3 * o, bary_mix(b, g, fc.p));
    const TimedRot r = timed_rot(a, b, fc, g, n);
    store_wxyz(rotation + 4 * o, (1.0 / fmax(r.len, 1e-12)) * r.Q);
    store3(normals + 3 * o, fc.R0);
    if (scaling != nullptr) {
      const D3 s = bary_mix(b, g, fc.s);
      const float2 ls = ((const float2*)a.log_scales)[n];
      scaling[3 * o] = a.thickness;
      scaling[3 * o + 1] = (float)exp((double)ls.x + s.y);
      scaling[3 * o + 2] = (float)exp((double)ls.y + s.z);
    }
  }
}

struct TimedGrads {
  const float *g_xyz, *g_rotation, *g_normals, *g_scaling;  // any may be null (zero)
};

GSR_HD void timed_face_backward(const TimedCall& a, const FaceBary& b, const TimedGrads& up, long long i,
                                float* rows) {  // i = t F + f
  const int t = (int)(i / a.F), f = (int)(i % a.F);
  const size_t N = (size_t)a.F * a.G;
  float* row = rows + 3 * GSR_TIMED_ROW * (size_t)i;
  TimedFace fc;
  if (!timed_face(a, t, f, true, fc)) {  // a face entry out of range: zero rows
    for (int k = 0; k < 3 * GSR_TIMED_ROW; ++k) row[k] = 0.0f;
    return;
  }
  const D3 zero = d3(0.0, 0.0, 0.0);
  D3 gp[3] = {zero, zero, zero}, gL[3] = {zero, zero, zero}, gs[3] = {zero, zero, zero};
  D3 gR0 = zero;
  const bool scales = a.vert_scale != nullptr && up.g_scaling != nullptr;
  for (int g = 0; g < a.G; ++g) {  // the face's Gaussians in ascending g
    const size_t n = (size_t)f * a.G + g, o = (size_t)t * N + n;
    const double w[3] = {(double)b.w[g][0], (double)b.w[g][1], (double)b.w[g][2]};
    if (up.g_xyz != nullptr) {
      const D3 gx = load3(up.g_xyz + 3 * o);
#pragma unroll
      for (int c = 0; c < 3; ++c) gp[c] = gp[c] + w[c] * gx;
    }
    if (up.g_normals != nullptr) gR0 = gR0 + load3(up.g_normals + 3 * o);
    if (up.g_rotation != nullptr) {
      const TimedRot r = timed_rot(a, b, fc, g, n);
      const Q4 gE = qmul(timed_rot_grad(r, up.g_rotation + 4 * o), conj(r.q0));
      const D3 gphi = qexp_grad(r.phi, gE);
#pragma unroll
      for (int c = 0; c < 3; ++c) gL[c] = gL[c] + w[c] * gphi;
    }
    if (scales) {  // component 0 of vert_scale is discarded
      const D3 s = bary_mix(b, g, fc.s);
      const float2 ls = ((const float2*)a.log_scales)[n];
      const D3 gv = d3(0.0, (double)up.g_scaling[3 * o + 1] * exp((double)ls.x + s.y),
                       (double)up.g_scaling[3 * o + 2] * exp((double)ls.y + s.z));
#pragma unroll
      for (int c = 0; c < 3; ++c) gs[c] = gs[c] + w[c] * gv;
    }
  }
  if (up.g_normals != nullptr) face_normal_grad(fc, fc.p[0], fc.p[1], fc.p[2], gR0, gp[0], gp[1], gp[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float* r = row + GSR_TIMED_ROW * c;
    store3(r, gp[c]);
    const Q4 gq = up.g_rotation != nullptr ? qlog_grad(fc.q[c], gL[c]) : qzero();
    r[3] = (float)gq.v.x, r[4] = (float)gq.v.y, r[5] = (float)gq.v.z, r[6] = (float)gq.w;
    store3(r + 7, gs[c]);
  }
}

GSR_HD void timed_vertex_backward(int T, int V, int F, long long i, const int* corner_order, const int* vert_offsets,
                                  const float* rows, float* dxyz, float* drot, float* dscale) {  // i = t V + v
  const int t = (int)(i / V), v = (int)(i % V);
  const long long n = 3ll * F;
  long long b, e;
  row_range(vert_offsets, v, n, b, e);
  D3 sp = d3(0.0, 0.0, 0.0), ss = sp;
  Q4 sq = qzero();
  const float* base = rows + 3 * GSR_TIMED_ROW * (size_t)t * (size_t)F;
  for (long long k = b; k < e; ++k) {
    const int co = corner_order[k];
    if (!in_range(co, n)) continue;  // not a corner: skipped
    const float* r = base + GSR_TIMED_ROW * (size_t)co;
    sp = sp + load3(r);
    sq = sq + load_q_row(r + 3);
    ss = ss + load3(r + 7);
  }
  store3(dxyz + 3 * i, sp);
  store4(drot + 4 * i, sq);
  if (dscale != nullptr) store3(dscale + 3 * i, ss);
}

GSR_HD void timed_gauss_backward(const TimedCall& a, const FaceBary& b, const TimedGrads& up, long long n,
                                 float* drotation0, float* dlog_scales) {  // n = f G + g
  const int f = (int)(n / a.G), g = (int)(n % a.G);
  const size_t N = (size_t)a.F * a.G;
  Q4 gq0 = qzero();
  double gl0 = 0.0, gl1 = 0.0;
  const bool scales = dlog_scales != nullptr && up.g_scaling != nullptr;
  if (up.g_rotation != nullptr || scales) {
    for (int t = 0; t < a.T; ++t) {  // the frames in ascending t
      TimedFace fc;
      if (!timed_face(a, t, f, false, fc)) break;  // a face entry out of range: zeros
      const size_t o = (size_t)t * N + n;
      if (up.g_rotation != nullptr) {
        const TimedRot r = timed_rot(a, b, fc, g, n);
        gq0 = gq0 + qmul(conj(r.E), timed_rot_grad(r, up.g_rotation + 4 * o));
      }
      if (scales) {
        const D3 s = bary_mix(b, g, fc.s);
        const float2 ls = ((const float2*)a.log_scales)[n];
        gl0 = fma((double)up.g_scaling[3 * o + 1], exp((double)ls.x + s.y), gl0);
        gl1 = fma((double)up.g_scaling[3 * o + 2], exp((double)ls.y + s.z), gl1);
      }
    }
  }
  store_wxyz(drotation0 + 4 * n, gq0);
  if (dlog_scales != nullptr) ((float2*)dlog_scales)[n] = make_float2((float)gl0, (float)gl1);
}

__global__ __launch_bounds__(256) void k_timed_forward(TimedCall a, FaceBary b, float* __restrict__ xyz,
                                                       float* __restrict__ rotation, float* __restrict__ normals,
                                                       float* __restrict__ scaling) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.F) timed_face_forward(a, b, i, xyz, rotation, normals, scaling);
}

__global__ __launch_bounds__(256) void k_timed_face(TimedCall a, FaceBary b, TimedGrads up,
                                                    float* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)a.T * a.F) timed_face_backward(a, b, up, i, rows);
}

__global__ __launch_bounds__(256) void k_timed_vertex(int T, int V, int F, const int* __restrict__ corner_order,
                                                      const int* __restrict__ vert_offsets,
                                                      const float* __restrict__ rows, float* __restrict__ dxyz,
                                                      float* __restrict__ drot, float* __restrict__ dscale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)T * V) timed_vertex_backward(T, V, F, i, corner_order, vert_offsets, rows, dxyz, drot, dscale);
}

__global__ __launch_bounds__(256) void k_timed_gauss(TimedCall a, FaceBary b, TimedGrads up,
                                                     float* __restrict__ drotation0,
                                                     float* __restrict__ dlog_scales) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n < (long long)a.F * a.G) timed_gauss_backward(a, b, up, n, drotation0, dlog_scales);
}

size_t timed_workspace_bytes(int T, int F) {
  return align_up(sizeof(float) * 3 * GSR_TIMED_ROW * (size_t)(T > 0 ? T : 1) * (size_t)(F > 0 ? F : 1), 256);
}

void launch_timed_forward(const TimedCall& c, const float* bary, float* xyz, float* rotation, float* normals,
                          float* scaling, hipStream_t stream) {
  hipLaunchKernelGGL(k_timed_forward, dim3(div_up((long long)c.T * c.F, 256)), dim3(256), 0, stream, c,
                     face_bary(c.G, bary), xyz, rotation, normals, c.vert_scale != nullptr ? scaling : nullptr);
}

void launch_timed_backward(const TimedCall& c, const float* bary, const int* corner_order, const int* vert_offsets,
                           const float* g_xyz, const float* g_rotation, const float* g_normals,
                           const float* g_scaling, float* dvert_xyz, float* dvert_rot, float* drotation0,
                           float* dvert_scale, float* dlog_scales, void* workspace, hipStream_t stream) {
  float* rows = (float*)workspace;
  const FaceBary b = face_bary(c.G, bary);
  const TimedGrads up{g_xyz, g_rotation, g_normals, g_scaling};
  const bool scales = c.vert_scale != nullptr;
  hipLaunchKernelGGL(k_timed_face, dim3(div_up((long long)c.T * c.F, 256)), dim3(256), 0, stream, c, b, up, rows);
  if (c.V > 0)
    hipLaunchKernelGGL(k_timed_vertex, dim3(div_up((long long)c.T * c.V, 256)), dim3(256), 0, stream, c.T, c.V, c.F,
                       corner_order, vert_offsets, rows, dvert_xyz, dvert_rot, scales ? dvert_scale : nullptr);
  hipLaunchKernelGGL(k_timed_gauss, dim3(div_up((long long)c.F * c.G, 256)), dim3(256), 0, stream, c, b, up,
                     drotation0, scales ? dlog_scales : nullptr);
}

}  // namespace gsr
