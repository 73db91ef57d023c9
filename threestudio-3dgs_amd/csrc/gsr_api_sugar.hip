// gsr_api_sugar.hip — the SuGaR entry points of include/gsr.h: the K-NN searches, the nine fused stages (each one
// struct of inputs, checked in place) and the densification statistics.
#include "gsr_api.h"

using namespace gsr;

extern "C" {

// ---- the K-NN searches on the distCUDA2 tree (gsr_knn.hip) ------------------------------------------
size_t gsr_knn_workspace_bytes(int P) { return knn_workspace_bytes(at_least_0(P)); }

int gsr_knn_mean_dist(int P, const float* points, float* mean_dist, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (P < 0) return invalid("negative point count");
  if (P == 0) return last_launch();
  if (points == nullptr || mean_dist == nullptr || workspace == nullptr) return null_argument();
  if (workspace_too_small(workspace_bytes, knn_workspace_bytes(P))) return GSR_EINVAL;
  launch_knn_mean_dist(P, points, mean_dist, workspace, (hipStream_t)stream);
  return last_launch();
}

size_t gsr_knn_points_workspace_bytes(int P, int K) {
  (void)K;  // the lists live in registers: the tree is all the workspace holds
  return knn_workspace_bytes(at_least_0(P));
}

int gsr_knn_points(int P, int K, const float* points, float* dists, long long* idx, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (K < 1 || K > GSR_KNN_MAX_K) return invalid("K must be in 1..32");
  if (P < 0) return invalid("negative point count");
  if (P == 0) return nothing_to_do();
  if (points == nullptr || dists == nullptr || idx == nullptr || workspace == nullptr) return null_argument();
  if (workspace_too_small(workspace_bytes, knn_workspace_bytes(P))) return GSR_EINVAL;
  launch_knn_points(P, K, points, dists, idx, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the SuGaR neighbour density field (gsr_field.hip) ---------------------------------------------
static int field_check(const gsr_sugar_field& c) {
  if (c.K < 1 || c.K > GSR_KNN_MAX_K) return invalid("K must be in 1..32");
  if (c.M < 0 || c.N < 0 || c.R < 0) return invalid("negative size");
  if ((long long)c.M * c.K >= (1ll << 31)) return invalid("M x K must stay below 2^31: split the samples");
  if (c.row == nullptr && c.R != c.M) return invalid("without row the neighbour table has M rows");
  if (c.M > 0 && (c.x == nullptr || (c.R > 0 && c.nbr == nullptr))) return null_argument();
  if (c.N > 0 && (c.centers == nullptr || c.inv_sr == nullptr || c.strengths == nullptr || c.min_scale == nullptr))
    return null_argument();
  return GSR_OK;
}

size_t gsr_sugar_field_workspace_bytes(int M, int K, int N) {
  if (K < 1 || K > GSR_KNN_MAX_K) return 0;
  return field_workspace_bytes(at_least_0(M), K, at_least_0(N));
}

int gsr_sugar_field_forward(const gsr_sugar_field* in, float* density, float* beta_avg, float* op, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (field_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (density == nullptr || beta_avg == nullptr || workspace == nullptr) return null_argument();
  if (workspace_too_small(workspace_bytes, field_workspace_bytes(0, in->K, in->N))) return GSR_EINVAL;
  launch_field_forward(*in, density, beta_avg, op, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_field_backward(const gsr_sugar_field* in, const float* dL_ddensity, const float* dL_dbeta_avg,
                             const float* dL_dop, float* dL_dx, float* dL_dcenters, float* dL_dinv_sr,
                             float* dL_dstrengths, float* dL_dmin_scale, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (in == nullptr) return null_argument();
  if (field_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (dL_dx == nullptr || workspace == nullptr ||
      (in->N > 0 && (dL_dcenters == nullptr || dL_dinv_sr == nullptr || dL_dstrengths == nullptr ||
                     dL_dmin_scale == nullptr)))
    return null_argument();
  if (workspace_too_small(workspace_bytes, field_workspace_bytes(in->M, in->K, in->N))) return GSR_EINVAL;
  GSR_HIP_CHECK((hipError_t)launch_field_backward(*in, dL_ddensity, dL_dbeta_avg, dL_dop, dL_dx, dL_dcenters,
                                                  dL_dinv_sr, dL_dstrengths, dL_dmin_scale, workspace,
                                                  (hipStream_t)stream));
  return last_launch();
}

// ---- the SuGaR neighbour-normal loss (gsr_normal.hip) ----------------------------------------------
static int normal_check(const gsr_sugar_normal& c) {
  if (c.K < 1 || c.K > GSR_KNN_MAX_K) return invalid("K must be in 1..32");
  if (c.M < 0 || c.N < 0 || c.R < 0) return invalid("negative size");
  if ((long long)c.M * (c.K + 1) >= (1ll << 31))
    return invalid("M x (K + 1) must stay below 2^31: split the samples");
  if (c.per_sample && c.R != c.M) return invalid("a per-sample neighbour table has M rows");
  if (c.M > 0 && (c.x == nullptr || c.own == nullptr || c.op == nullptr || (c.R > 0 && c.nbr == nullptr)))
    return null_argument();
  if (c.N > 0 && (c.centers == nullptr || c.normals == nullptr || c.min_scale == nullptr)) return null_argument();
  return GSR_OK;
}

size_t gsr_sugar_normal_workspace_bytes(int M, int K, int N) {
  if (K < 1 || K > GSR_KNN_MAX_K) return 0;
  return normal_workspace_bytes(at_least_0(M), K, at_least_0(N));
}

int gsr_sugar_normal_forward(const gsr_sugar_normal* in, float* loss, float* rec, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (normal_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (loss == nullptr || workspace == nullptr) return null_argument();
  if (misaligned(16, rec)) return invalid("rec must be 16-byte aligned");
  if (workspace_too_small(workspace_bytes, normal_workspace_bytes(0, in->K, in->N))) return GSR_EINVAL;
  launch_normal_forward(*in, loss, rec, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_normal_backward(const gsr_sugar_normal* in, const float* rec, const float* dL_dloss, float* dL_dnormals,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (normal_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (rec == nullptr || dL_dloss == nullptr || workspace == nullptr || (in->N > 0 && dL_dnormals == nullptr))
    return null_argument();
  if (misaligned(16, rec)) return invalid("rec must be 16-byte aligned");
  if (workspace_too_small(workspace_bytes, normal_workspace_bytes(in->M, in->K, in->N))) return GSR_EINVAL;
  GSR_HIP_CHECK((hipError_t)launch_normal_backward(*in, rec, dL_dloss, dL_dnormals, workspace, (hipStream_t)stream));
  return last_launch();
}

// ---- the geometry of mesh-bound SuGaR Gaussians (gsr_mesh.hip) -------------------------------------
static int mesh_check(const gsr_sugar_mesh& c, int N, const float* bary) {
  if (c.G < 1 || c.G > GSR_MESH_MAX_G) return invalid("G must be in 1..8");
  if (c.V < 0 || c.F < 0 || N < 0) return invalid("negative size");
  if ((long long)c.F * c.G != (long long)N) return invalid("N must equal F x G");
  if (bary == nullptr) return null_argument();
  if (c.F > 0 &&
      (c.faces == nullptr || c.cplx == nullptr || c.log_scales == nullptr || (c.V > 0 && c.verts == nullptr)))
    return null_argument();
  if (misaligned(8, c.cplx, c.log_scales)) return invalid("complex_numbers and log_scales must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_mesh_workspace_bytes(int F, int V) { return mesh_workspace_bytes(at_least_0(F), at_least_0(V)); }

int gsr_sugar_mesh_forward(const gsr_sugar_mesh* in, int N, const float* bary, float thickness, float* xyz,
                           float* scaling, float* rotation, float* normals, void* stream) {
  if (in == nullptr) return null_argument();
  if (mesh_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->F == 0) return nothing_to_do();
  if (xyz == nullptr || scaling == nullptr || rotation == nullptr || normals == nullptr) return null_argument();
  if (misaligned(16, rotation)) return invalid("rotation must be 16-byte aligned");
  launch_mesh_forward(*in, bary, thickness, xyz, scaling, rotation, normals, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_mesh_backward(const gsr_sugar_mesh* in, int N, const float* bary, const int* corner_order,
                            const int* vert_offsets, const float* dL_dxyz, const float* dL_dscaling,
                            const float* dL_drotation, const float* dL_dnormals, float* dL_dverts, float* dL_dcomplex,
                            float* dL_dlog_scales, void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (mesh_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->F == 0) return nothing_to_do();
  if (corner_order == nullptr || vert_offsets == nullptr || dL_dcomplex == nullptr || dL_dlog_scales == nullptr ||
      workspace == nullptr || (in->V > 0 && dL_dverts == nullptr))
    return null_argument();
  if (misaligned(16, dL_drotation)) return invalid("dL_drotation must be 16-byte aligned");
  if (misaligned(8, dL_dcomplex, dL_dlog_scales))
    return invalid("dL_dcomplex and dL_dlog_scales must be 8-byte aligned");
  if (workspace_too_small(workspace_bytes, mesh_workspace_bytes(in->F, in->V))) return GSR_EINVAL;
  launch_mesh_backward(*in, bary, corner_order, vert_offsets, dL_dxyz, dL_dscaling, dL_drotation, dL_dnormals,
                       dL_dverts, dL_dcomplex, dL_dlog_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the time-batched geometry of dynamic SuGaR (gsr_dynamic.hip) ----------------------------------
static int skin_check(const gsr_sugar_skin& c) {
  if (c.K < 1 || c.K > GSR_SKIN_MAX_K) return invalid("K must be in 1..32");
  if (c.method != GSR_SKIN_DQS && c.method != GSR_SKIN_LBS)
    return invalid("method must be GSR_SKIN_DQS or GSR_SKIN_LBS");
  if (c.T < 0 || c.V < 0 || c.P < 0) return invalid("negative size");
  if (!below_2_31(c.T, c.V) || !below_2_31(c.T, c.P) || !below_2_31(c.V, c.K))
    return invalid("T x V, T x P and V x K must stay below 2^31");
  if (c.T > 0 && c.V > 0 &&
      (c.P == 0 || c.verts == nullptr || c.node_xyz == nullptr || c.node_trans == nullptr || c.node_rots == nullptr ||
       c.nbr == nullptr || c.w == nullptr))
    return invalid(c.P == 0 ? "vertices without nodes" : "null pointer argument");
  if (misaligned(16, c.node_rots)) return invalid("node_rots must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_skin_workspace_bytes(int T, int V, int P) {
  return skin_workspace_bytes(at_least_0(T), at_least_0(V), at_least_0(P));
}

int gsr_sugar_skin_forward(const gsr_sugar_skin* in, float* vert_xyz, float* vert_rot, float* vert_scale,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (skin_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (vert_xyz == nullptr || vert_rot == nullptr || workspace == nullptr ||
      (in->node_scales != nullptr && vert_scale == nullptr))
    return null_argument();
  if (misaligned(16, vert_rot)) return invalid("vert_rot must be 16-byte aligned");
  if (workspace_too_small(workspace_bytes, skin_workspace_bytes(in->T, in->V, in->P))) return GSR_EINVAL;
  launch_skin_forward(*in, vert_xyz, vert_rot, vert_scale, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_skin_backward(const gsr_sugar_skin* in, const int* item_order, const int* node_offsets,
                            const float* dL_dxyz, const float* dL_drot, const float* dL_dscale, float* dL_dverts,
                            float* dL_dnode_trans, float* dL_dnode_rots, float* dL_dnode_scales, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (skin_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (item_order == nullptr || node_offsets == nullptr || dL_dverts == nullptr || dL_dnode_trans == nullptr ||
      dL_dnode_rots == nullptr || workspace == nullptr || (in->node_scales != nullptr && dL_dnode_scales == nullptr))
    return null_argument();
  if (misaligned(16, dL_drot, dL_dnode_rots)) return invalid("dL_drot and dL_dnode_rots must be 16-byte aligned");
  if (workspace_too_small(workspace_bytes, skin_workspace_bytes(in->T, in->V, in->P))) return GSR_EINVAL;
  launch_skin_backward(*in, item_order, node_offsets, dL_dxyz, dL_drot,
                       in->node_scales != nullptr ? dL_dscale : nullptr, dL_dverts, dL_dnode_trans, dL_dnode_rots,
                       dL_dnode_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

static int timed_check(const gsr_sugar_timed& c, int N, const float* bary) {
  if (c.G < 1 || c.G > GSR_MESH_MAX_G) return invalid("G must be in 1..8");
  if (c.T < 0 || c.V < 0 || c.F < 0 || N < 0) return invalid("negative size");
  if ((long long)c.F * c.G != (long long)N) return invalid("N must equal F x G");
  if (!below_2_31(c.T, N) || !below_2_31(c.T, c.V)) return invalid("T x N and T x V must stay below 2^31");
  if (bary == nullptr) return null_argument();
  if ((c.vert_scale == nullptr) != (c.log_scales == nullptr))
    return invalid("vert_scale and log_scales are given together or not at all");
  if (c.T > 0 && c.F > 0 &&
      (c.faces == nullptr || c.rotation0 == nullptr || (c.V > 0 && (c.vert_xyz == nullptr || c.vert_rot == nullptr))))
    return null_argument();
  if (misaligned(16, c.vert_rot, c.rotation0)) return invalid("vert_rot and rotation0 must be 16-byte aligned");
  if (misaligned(8, c.log_scales)) return invalid("log_scales must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_timed_workspace_bytes(int T, int F) { return timed_workspace_bytes(at_least_0(T), at_least_0(F)); }

int gsr_sugar_timed_forward(const gsr_sugar_timed* in, int N, const float* bary, float* xyz, float* rotation,
                            float* normals, float* scaling, void* stream) {
  if (in == nullptr) return null_argument();
  if (timed_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->F == 0) return nothing_to_do();
  if (xyz == nullptr || rotation == nullptr || normals == nullptr || (in->vert_scale != nullptr && scaling == nullptr))
    return null_argument();
  if (misaligned(16, rotation)) return invalid("rotation must be 16-byte aligned");
  launch_timed_forward(*in, bary, xyz, rotation, normals, scaling, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_timed_backward(const gsr_sugar_timed* in, int N, const float* bary, const int* corner_order,
                             const int* vert_offsets, const float* dL_dxyz, const float* dL_drotation,
                             const float* dL_dnormals, const float* dL_dscaling, float* dL_dvert_xyz,
                             float* dL_dvert_rot, float* dL_drotation0, float* dL_dvert_scale, float* dL_dlog_scales,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (timed_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->F == 0) return nothing_to_do();
  const bool scaled = in->vert_scale != nullptr;
  if (corner_order == nullptr || vert_offsets == nullptr || dL_drotation0 == nullptr || workspace == nullptr ||
      (in->V > 0 && (dL_dvert_xyz == nullptr || dL_dvert_rot == nullptr)) ||
      (scaled && (dL_dlog_scales == nullptr || (in->V > 0 && dL_dvert_scale == nullptr))))
    return null_argument();
  if (misaligned(16, dL_drotation, dL_dvert_rot, dL_drotation0))
    return invalid("dL_drotation, dL_dvert_rot and dL_drotation0 must be 16-byte aligned");
  if (misaligned(8, dL_dlog_scales)) return invalid("dL_dlog_scales must be 8-byte aligned");
  if (workspace_too_small(workspace_bytes, timed_workspace_bytes(in->T, in->F))) return GSR_EINVAL;
  launch_timed_backward(*in, bary, corner_order, vert_offsets, dL_dxyz, dL_drotation, dL_dnormals,
                        scaled ? dL_dscaling : nullptr, dL_dvert_xyz, dL_dvert_rot, dL_drotation0, dL_dvert_scale,
                        dL_dlog_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the ARAP energy of the deformed mesh (gsr_arap.hip) --------------------------------------------
static int arap_check(const gsr_sugar_arap& c) {
  if (c.rot_form != GSR_ARAP_QUAT && c.rot_form != GSR_ARAP_MATRIX)
    return invalid("rot_form must be GSR_ARAP_QUAT or GSR_ARAP_MATRIX");
  if (c.T < 0 || c.V < 0 || c.E < 0) return invalid("negative size");
  if (!below_2_31(c.T, c.V)) return invalid("T x V must stay below 2^31");
  if (c.T > 0 && c.V > 0 &&
      (c.verts == nullptr || c.offsets == nullptr || c.vert_xyz == nullptr || c.vert_rot == nullptr ||
       (c.E > 0 && (c.nbr == nullptr || c.w == nullptr))))
    return null_argument();
  if (c.rot_form == GSR_ARAP_QUAT && misaligned(16, c.vert_rot)) return invalid("vert_rot must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_arap_workspace_bytes(int T, int V) { return arap_workspace_bytes(at_least_0(T), at_least_0(V)); }

int gsr_sugar_arap_forward(const gsr_sugar_arap* in, float* energy, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (in == nullptr) return null_argument();
  if (arap_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (energy == nullptr || workspace == nullptr) return null_argument();
  if (workspace_too_small(workspace_bytes, arap_workspace_bytes(in->T, in->V))) return GSR_EINVAL;
  launch_arap_forward(*in, energy, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_arap_backward(const gsr_sugar_arap* in, const float* dL_denergy, float* dL_dvert_xyz,
                            float* dL_dvert_rot, void* stream) {
  if (in == nullptr) return null_argument();
  if (arap_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (dL_denergy == nullptr || dL_dvert_xyz == nullptr || dL_dvert_rot == nullptr) return null_argument();
  if (in->rot_form == GSR_ARAP_QUAT && misaligned(16, dL_dvert_rot))
    return invalid("dL_dvert_rot must be 16-byte aligned");
  launch_arap_backward(*in, dL_denergy, dL_dvert_xyz, dL_dvert_rot, (hipStream_t)stream);
  return last_launch();
}

// ---- the B-spline of the timed node attributes (gsr_spline.hip) -------------------------------------
static int spline_check(const gsr_sugar_spline& c) {
  if (c.degree != 1 && c.degree != 3) return invalid("degree must be 1 or 3");
  if (c.n_knots < c.degree + 1) return invalid("n_knots must be at least degree + 1");
  if (c.T < 0 || c.P < 0) return invalid("negative size");
  if (!(c.interval > 0.0f)) return invalid("interval must be positive");
  if (!below_2_31(c.T, c.P) || !below_2_31(c.n_knots, c.P))
    return invalid("T x P and n_knots x P must stay below 2^31");
  if (c.T > 0 && c.P > 0 && (c.timestamps == nullptr || c.knots_xyz == nullptr || c.knots_rot == nullptr))
    return null_argument();
  if (misaligned(16, c.knots_rot)) return invalid("knots_rot must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_spline_workspace_bytes(int T, int P, int degree) {
  return spline_workspace_bytes(at_least_0(T), at_least_0(P), degree);
}

int gsr_sugar_spline_forward(const gsr_sugar_spline* in, float* xyz, float* rot, float* scale, void* stream) {
  if (in == nullptr) return null_argument();
  if (spline_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (xyz == nullptr || rot == nullptr || (in->knots_scale != nullptr && scale == nullptr)) return null_argument();
  if (misaligned(16, rot)) return invalid("rot must be 16-byte aligned");
  launch_spline_forward(*in, xyz, rot, scale, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_spline_backward(const gsr_sugar_spline* in, const float* dL_dxyz, const float* dL_drot,
                              const float* dL_dscale, float* dL_dknots_xyz, float* dL_dknots_rot,
                              float* dL_dknots_scale, void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (spline_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (dL_dknots_xyz == nullptr || dL_dknots_rot == nullptr || workspace == nullptr ||
      (in->knots_scale != nullptr && dL_dknots_scale == nullptr))
    return null_argument();
  if (misaligned(16, dL_drot, dL_dknots_rot)) return invalid("dL_drot and dL_dknots_rot must be 16-byte aligned");
  if (misaligned(8, workspace)) return invalid("workspace must be 8-byte aligned");
  if (workspace_too_small(workspace_bytes, spline_workspace_bytes(in->T, in->P, in->degree))) return GSR_EINVAL;
  launch_spline_backward(*in, dL_dxyz, dL_drot, dL_dscale, dL_dknots_xyz, dL_dknots_rot, dL_dknots_scale, workspace,
                         (hipStream_t)stream);
  return last_launch();
}

// ---- the HexPlane deformation network (gsr_deform.hip) ----------------------------------------------
static int deform_check(const gsr_sugar_deform& c) {
  if (c.L < 1 || c.L > GSR_DEFORM_MAX_L) return invalid("L must be in 1..4");
  if (c.T < 0 || c.P < 0) return invalid("negative size");
  if (!below_2_31(c.T, c.P) || !below_2_31(4, c.P)) return invalid("T x P and 4 P must stay below 2^31");
  if (c.reso == nullptr || c.planes == nullptr || c.mlp == nullptr) return null_argument();
  long long texels = 0;
  for (int l = 0; l < c.L; ++l) {
    for (int d = 0; d < 4; ++d)
      if (c.reso[4 * l + d] < 2) return invalid("every resolution must be at least 2");
    if (c.reso[4 * l + 3] != c.reso[3]) return invalid("the time resolution is the same on every level");
    for (int a = 0; a < 4; ++a)
      for (int b = a + 1; b < 4; ++b) {
        const long long n = (long long)c.reso[4 * l + a] * c.reso[4 * l + b];
        if (n * 32 >= (1ll << 31)) return invalid("a plane must stay below 2^31 elements");
        texels += n;
      }
  }
  if (texels >= (1ll << 31)) return invalid("the planes must stay below 2^31 texels");
  for (int i = 0; i < 6 * c.L; ++i)
    if (c.planes[i] == nullptr) return invalid("null plane");
  for (int i = 0; i < 10; ++i)
    if (c.mlp[i] == nullptr) return null_argument();
  for (int i = 10; i < GSR_DEFORM_MLP; ++i)
    if ((c.mlp[i] != nullptr) != (c.d_scale != 0)) return invalid("the scale head is given iff d_scale is set");
  if (c.T > 0 && c.P > 0 && (c.cell == nullptr || c.frac == nullptr || c.tcell == nullptr || c.tfrac == nullptr))
    return null_argument();
  if (misaligned(8, c.frac, c.tfrac)) return invalid("frac and tfrac must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_deform_workspace_bytes(int T, int P, int L) {
  if (L < 1 || L > GSR_DEFORM_MAX_L) return 0;
  return deform_workspace_bytes(at_least_0(T), at_least_0(P), L);
}

int gsr_sugar_deform_forward(const gsr_sugar_deform* in, float* xyz, float* rot, float* scale, void* stream) {
  if (in == nullptr) return null_argument();
  if (deform_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (xyz == nullptr || rot == nullptr || (in->d_scale && scale == nullptr)) return null_argument();
  launch_deform_forward(*in, xyz, rot, scale, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_deform_backward(const gsr_sugar_deform* in, const int* sp_order, const int* sp_offsets,
                              const int* col_order, const int* col_offsets, const int* t_order, const int* t_offsets,
                              const float* dL_dxyz, const float* dL_drot, const float* dL_dscale,
                              float* const* dL_dplanes, float* const* dL_dmlp, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (in == nullptr) return null_argument();
  if (deform_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (in->n_sp < 0 || in->n_col < 0 || in->n_t < 0) return invalid("negative size");
  if (sp_offsets == nullptr || col_offsets == nullptr || t_offsets == nullptr || dL_dplanes == nullptr ||
      dL_dmlp == nullptr || workspace == nullptr || (in->n_sp > 0 && sp_order == nullptr) ||
      (in->n_col > 0 && col_order == nullptr) || (in->n_t > 0 && t_order == nullptr))
    return null_argument();
  for (int i = 0; i < 6 * in->L; ++i)
    if (dL_dplanes[i] == nullptr) return null_argument();
  for (int i = 0; i < (in->d_scale ? GSR_DEFORM_MLP : 10); ++i)
    if (dL_dmlp[i] == nullptr) return null_argument();
  if (misaligned(8, workspace)) return invalid("workspace must be 8-byte aligned");
  if (workspace_too_small(workspace_bytes, deform_workspace_bytes(in->T, in->P, in->L))) return GSR_EINVAL;
  const DeformCsr t{sp_order, sp_offsets, col_order, col_offsets, t_order, t_offsets};
  launch_deform_backward(*in, t, dL_dxyz, dL_drot, dL_dscale, dL_dplanes, dL_dmlp, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the mesh regularisers of the deformed surface (gsr_meshreg.hip) --------------------------------
static int meshreg_check(const gsr_sugar_meshreg& c) {
  if (c.T < 0 || c.V < 0 || c.E < 0 || c.P < 0) return invalid("negative size");
  const long long most = c.P > c.V ? c.P : c.V;
  if (!below_2_31(c.T, c.V) || !below_2_31(4, c.P) || !below_2_31(2, c.E) || !below_2_31(c.T, (most + 255) / 256))
    return invalid("T x V, 4 P, 2 E and T x ceil(max(P, V) / 256) must stay below 2^31");
  return GSR_OK;
}
// the arguments of one loss (nc: the normal consistency), `out` being the tensor it writes
static int meshreg_args(const gsr_sugar_meshreg& c, bool nc, const void* out, const char* out_name,
                        const void* workspace, size_t workspace_bytes, bool backward) {
  const int pass = !backward ? GSR_MESHREG_FORWARD : nc ? GSR_MESHREG_NC_BACKWARD : GSR_MESHREG_LAP_BACKWARD;
  if (c.vert_xyz == nullptr) return null_named("vert_xyz");
  if (nc) {
    if (c.pairs == nullptr) return null_named("pairs");
    if (backward && c.slot_offsets == nullptr) return null_named("slot_offsets");
    if (backward && c.slots == nullptr) return null_named("slots");
  } else {
    if (c.ring_offsets == nullptr) return null_named("ring_offsets");
    if (c.E > 0 && c.ring == nullptr) return null_named("ring");
  }
  if (out == nullptr) return null_named(out_name);
  if (workspace == nullptr) return null_named("workspace");
  if (misaligned(16, c.pairs)) return invalid("pairs must be 16-byte aligned");
  if (misaligned(8, workspace)) return invalid("workspace must be 8-byte aligned");
  if (workspace_too_small(workspace_bytes, meshreg_workspace_bytes(c.T, c.V, c.P, pass))) return GSR_EINVAL;
  return GSR_OK;
}

size_t gsr_sugar_meshreg_workspace_bytes(int T, int V, int P, int pass) {
  if (pass < GSR_MESHREG_FORWARD || pass > GSR_MESHREG_LAP_BACKWARD) return 0;
  return meshreg_workspace_bytes(at_least_0(T), at_least_0(V), at_least_0(P), pass);
}

int gsr_sugar_normal_consistency_forward(const gsr_sugar_meshreg* in, float* nc, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (meshreg_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (meshreg_args(*in, true, nc, "nc", workspace, workspace_bytes, false) != GSR_OK) return GSR_EINVAL;
  launch_normal_consistency_forward(*in, nc, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_normal_consistency_backward(const gsr_sugar_meshreg* in, const float* dL_dnc, float* dL_dvert_xyz,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (meshreg_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (dL_dnc == nullptr) return null_named("dL_dnc");
  if (meshreg_args(*in, true, dL_dvert_xyz, "dL_dvert_xyz", workspace, workspace_bytes, true) != GSR_OK)
    return GSR_EINVAL;
  launch_normal_consistency_backward(*in, dL_dnc, dL_dvert_xyz, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_laplacian_forward(const gsr_sugar_meshreg* in, float* lap, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (in == nullptr) return null_argument();
  if (meshreg_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (meshreg_args(*in, false, lap, "lap", workspace, workspace_bytes, false) != GSR_OK) return GSR_EINVAL;
  launch_laplacian_forward(*in, lap, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_laplacian_backward(const gsr_sugar_meshreg* in, const float* dL_dlap, float* dL_dvert_xyz,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (meshreg_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (dL_dlap == nullptr) return null_named("dL_dlap");
  if (meshreg_args(*in, false, dL_dvert_xyz, "dL_dvert_xyz", workspace, workspace_bytes, true) != GSR_OK)
    return GSR_EINVAL;
  launch_laplacian_backward(*in, dL_dlap, dL_dvert_xyz, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the densification statistics of a view batch (gsr_densify.hip) ---------------------------------
int gsr_densify_stats(const gsr_densify_batch* in, void* stream) {
  if (in == nullptr) return null_argument();
  if (in->V < 0 || in->V > GSR_SET_MAX) return invalid("a densification call takes 0..64 views");
  if (in->P < 0) return invalid("P must be >= 0");
  if (in->P == 0 || in->V == 0) return nothing_to_do();
  if (in->max_radii == nullptr) return null_named("max_radii");
  if (in->grad_norm_sum == nullptr) return null_named("grad_norm_sum");
  if (in->count == nullptr) return null_named("count");
  int with_rows = 0;
  for (int v = 0; v < in->V; ++v) {
    if (in->radii[v] == nullptr) return null_named("radii row");
    with_rows += in->visible[v] != nullptr;
  }
  if (with_rows != 0 && with_rows != in->V) return invalid("visibility rows must be given for every view or for none");
  launch_densify_stats(*in, (hipStream_t)stream);
  return last_launch();
}

}  // extern "C"
