/*
 * gsr.h — C ABI of the MI355X-native differentiable 3D Gaussian Splatting rasterizer.
 *
 * This is the drop-in boundary for the hot path of lizhiqi49/threestudio-3dgs.  The
 * reference never ships a rasterizer: every renderer (e.g. renderer/diff_gaussian_rasterizer.py:8-11,
 * renderer/diff_gaussian_rasterizer_background.py:119-128, renderer/diff_gaussian_rasterizer_advanced.py:122)
 * imports the external pybind module `diff_gaussian_rasterization._C` (ashawkey 4-output fork,
 * README.md:17,28).  Its three entry points are
 *     _C.rasterize_gaussians(...)          -> (num_rendered, color, depth, alpha, radii, geomBuf, binningBuf, imgBuf)
 *     _C.rasterize_gaussians_backward(...) -> 8 gradients
 *     _C.mark_visible(...)                 -> bool mask
 * (SURVEY.md §8b).  This header restates them as plain C: device pointers, sizes and a HIP stream
 * handle; no torch types.  The host binding (threestudio-3dgs_amd/diff_gaussian_rasterization/_C.py)
 * calls these through ctypes with buffers allocated by the PyTorch caching allocator.
 *
 * Conventions (unchanged from the reference call sites):
 *   - all float arrays are fp32, row-major, device-resident;
 *   - viewmatrix / projmatrix are 4x4 *transposed* (row-vector) matrices read column-major
 *     (world_view_transform / full_proj_transform, geometry/sugar.py:891-896);
 *   - shs is (P, M, 3); rotations are (w, x, y, z), used as given (not renormalised);
 *   - color output is planar (3, H, W); depth and alpha are (1, H, W);
 *   - radii is int32 (P,); means2D gradient is (P, 3) in pixel units (x W/2, H/2), z = 0.
 *
 * Work is split into the phases the reference performs inside one call so that the host can
 * size the K-dependent buffers between them (the reference does the same D2H read of K,
 * SURVEY.md §2a "cub::DeviceScan ... host sync"):
 *   1. gsr_forward_preprocess   — cull/project/EWA/SH, depth sort, instance offsets, K
 *   2. gsr_num_rendered         — read K (and the visible count) back to the host
 *   3. gsr_forward_render       — duplicate, tile sort, tile ranges, front-to-back blend
 *   4. gsr_backward             — back-to-front replay + fused per-Gaussian chain rule
 *
 * Every function returns GSR_OK (0) or an error code; gsr_last_error() gives the message for
 * the calling thread.  Kernels are enqueued on `stream` (a hipStream_t; NULL = legacy stream);
 * only gsr_num_rendered synchronises.
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_EINVAL 1 /* bad argument (shape / size / null pointer)          */
#define GSR_EHIP 2   /* a HIP runtime call failed                            */

#define GSR_TILE_X 16 /* BLOCK_X of the reference algorithm (16x16 tiles)      */
#define GSR_TILE_Y 16

/* Library identification ("gsr <version> gfx950"). */
const char* gsr_version(void);
/*
 * ABI revision of this header (GSR_ABI_VERSION), for callers binding the library at run time.
 *   2  gsr_set_backward `accumulate` CONTINUES every per-Gaussian sum from the stored value in view order
 *      (round 1's revision 1 added the new sums to the stored values); with accumulate in the scale / rotation
 *      path dL_dcov3D is required (the running dL/dcov3D carry), otherwise GSR_EINVAL.
 *   3  gsr_shade_views_forward / gsr_shade_views_backward (per-view light colours and shading modes);
 *      gsr_grad_chunk_range (per-Gaussian sums in ranges, events for overlap).
 *   4  gsr_set_image_bytes by instance counts (sized for the forward's split decision, which the buffer records);
 *      gsr_profile_kernel (the blend kernels the phases ran).
 *   5  gsr_sort_work_bytes / gsr_sort_pairs / gsr_sort_rank_mode (the library's sort, for tests);
 *      gsr_set_preprocess with colors2 (the two-colour render's second colours written into the records).
 *   6  gsr_knn_points_workspace_bytes / gsr_knn_points (the K nearest neighbours with indices).
 *   7  the view-set calls take argument structs (gsr_set_scene / _state / _outputs / _grads): one gsr_set_render and
 *      one gsr_set_backward, their variants selected by fields; the _ex, _composite, _colors, _two_colors and
 *      _chunks entry points of revisions 2-5 are gone.
 *   8  gsr_sugar_field_workspace_bytes / gsr_sugar_field_forward / gsr_sugar_field_backward (the SuGaR regulariser's
 *      neighbour density field and its deterministic backward).
 *      Added under 8 (additive: no existing call changes, binders find the new calls by symbol):
 *      gsr_sugar_normal_workspace_bytes / gsr_sugar_normal_forward / gsr_sugar_normal_backward (the regulariser's
 *      neighbour-normal loss);
 *      gsr_sugar_mesh_workspace_bytes / gsr_sugar_mesh_forward / gsr_sugar_mesh_backward (the geometry of mesh-bound
 *      SuGaR Gaussians);
 *      gsr_sugar_skin_workspace_bytes / gsr_sugar_skin_forward / gsr_sugar_skin_backward and
 *      gsr_sugar_timed_workspace_bytes / gsr_sugar_timed_forward / gsr_sugar_timed_backward (dynamic SuGaR: the
 *      deformation-graph skinning of the vertices and the Gaussians of the deformed mesh, for all frames of a batch);
 *      gsr_sugar_arap_workspace_bytes / gsr_sugar_arap_forward / gsr_sugar_arap_backward (dynamic SuGaR: the
 *      as-rigid-as-possible energy of the deformed vertices, for all frames of a batch);
 *      gsr_sugar_spline_workspace_bytes / gsr_sugar_spline_forward / gsr_sugar_spline_backward (dynamic SuGaR: the
 *      B-spline from the control knots to the timed node attributes).
 *   9  the gsr_sugar_*_forward / _backward calls take their stage's inputs as one struct (gsr_sugar_field, _normal,
 *      _mesh, _skin, _timed, _arap, _spline) followed by the tables, gradients, outputs and workspace, which stay
 *      positional; the *_workspace_bytes sizers are unchanged.
 *      Added under 9 (additive: no existing call changes, binders find the new calls by symbol):
 *      gsr_sugar_deform_workspace_bytes / gsr_sugar_deform_forward / gsr_sugar_deform_backward (dynamic SuGaR: the
 *      HexPlane deformation network that produces the control knots);
 *      gsr_sugar_meshreg_workspace_bytes / gsr_sugar_normal_consistency_forward / _backward /
 *      gsr_sugar_laplacian_forward / _backward (SuGaR: the normal-consistency and uniform-Laplacian regularisers of the
 *      deformed surface mesh, for all frames of a batch);
 *      gsr_set_timed / gsr_set_timed_grads and gsr_set_timed_preprocess / gsr_set_timed_backward (timed view sets: every
 *      view of a set renders its own frame of the Gaussians' geometry, e.g. the frames of dynamic SuGaR);
 *      gsr_densify_batch and gsr_densify_stats (the densification statistics of a view batch — running maximum of the
 *      radii, sum of the screen-space gradient norms and visibility count — in one launch).
 */
#define GSR_ABI_VERSION 9
int gsr_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* gsr_last_error(void);

/* ---- workspace sizing (bytes).  Buffers are opaque, 256-byte aligned uint8 regions. ---- */
/* Per-Gaussian state: replaces the reference's geomBuffer (rasterize_points.cu, [EXT]). */
size_t gsr_geom_bytes(int P);
/* Per-instance state for K (Gaussian, tile) pairs: replaces binningBuffer. */
size_t gsr_binning_bytes(int K, int width, int height);
/* Per-pixel state (final transmittance, last contributor, tile ranges): replaces imgBuffer. */
size_t gsr_image_bytes(int width, int height);
/* Scratch for gsr_backward (per-instance gradient rows). */
size_t gsr_backward_bytes(int P, int K);

/*
 * Phase 1 — replaces FORWARD::preprocessCUDA + InclusiveSum of rasterize_points.cu [EXT]
 * (SURVEY.md §2a rows 1-2, §8a A4-A8).  Exactly one of (shs, colors_precomp) and one of
 * ((scales, rotations), cov3D_precomp) must be non-NULL (checked; GSR_EINVAL otherwise).
 * Writes radii (P,) and the geom workspace; the visible count and K stay on the device.
 *   means3D (P,3)  scales (P,3)  rotations (P,4)  opacities (P,1)  shs (P,M,3)
 *   colors_precomp (P,3)  cov3D_precomp (P,6)  viewmatrix/projmatrix (16)  campos (3)
 * `degree` is the active SH degree; the kernel uses min(degree, sqrt(M)-1).
 */
int gsr_forward_preprocess(int P, int degree, int M,
                           const float* means3D, const float* scales, float scale_modifier,
                           const float* rotations, const float* opacities, const float* shs,
                           const float* colors_precomp, const float* cov3D_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* campos,
                           int width, int height, float tanfovx, float tanfovy, int prefiltered,
                           int* radii, void* geom, void* stream);

/* Phase 2 — D2H read of K (num_rendered) and of the visible-Gaussian count; synchronises `stream`. */
int gsr_num_rendered(const void* geom, int P, int* num_rendered, int* num_visible, void* stream);

/*
 * Phase 3 — replaces duplicateWithKeys + DeviceRadixSort::SortPairs + identifyTileRanges +
 * FORWARD::renderCUDA [EXT].  K must be the value from gsr_num_rendered.
 * bg is (3,) on the device.  Writes color (3,H,W), depth (1,H,W), alpha (1,H,W) and the
 * binning / image workspaces that gsr_backward reads.
 */
int gsr_forward_render(int P, int K, int width, int height, const float* bg,
                       void* geom, void* binning, void* image,
                       float* out_color, float* out_depth, float* out_alpha, void* stream);

/*
 * Phase 4 — replaces BACKWARD::renderCUDA + computeCov2DCUDA + preprocessCUDA [EXT]
 * (SURVEY.md §8a A11-A12).  Reads (never writes) geom/binning/image, so it may be called
 * repeatedly on the same forward state (retain_graph=True, system/gaussian_splatting.py:129,138).
 * Gradient outputs are fully overwritten (no pre-zeroing needed):
 *   dL_dmeans2D (P,3)  dL_dcolors (P,3)  dL_dopacity (P,1)  dL_dmeans3D (P,3)
 *   dL_dcov3D (P,6) [may be NULL if cov3D_precomp is NULL]  dL_dsh (P,M,3) [NULL if shs NULL]
 *   dL_dscales (P,3), dL_drotations (P,4) [NULL if scales/rotations NULL]
 * dL_ddepth / dL_dalpha may be NULL (treated as zero).
 */
int gsr_backward(int P, int degree, int M, int K, int width, int height, const float* bg,
                 const float* means3D, const float* scales, float scale_modifier,
                 const float* rotations, const float* opacities, const float* shs,
                 const float* colors_precomp, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* campos,
                 float tanfovx, float tanfovy, const int* radii,
                 const void* geom, const void* binning, const void* image,
                 const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                 float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                 void* work, void* stream);

/*
 * View sets: one set of P Gaussians rendered from V <= GSR_SET_MAX cameras
 * of the same image size by the SAME launches (every stage runs once per set, not once per view;
 * sorts are segmented by view).  The per-view functions above are sets of one.  The reference
 * renders a batch with a Python loop over views (renderer/gaussian_batch_renderer.py:9-122), one
 * rasterizer call each; these replace that loop's V forward and V backward calls.
 * Per-view arguments are HOST arrays of V values or of V device pointers; images are stacked:
 * color (V,3,H,W), depth / alpha (V,1,H,W), radii (V,P) int32, dL_dmeans2D (V,P,3).
 * Shared-parameter gradients (means3D, opacity, SH, scales, rotations, cov3D, colors) are summed
 * over the V views inside the per-Gaussian kernel.
 * The arguments travel in four structs; the calls read them and keep no pointer to them.
 */
#define GSR_SET_MAX 64
#define GSR_GRAD_CHUNKS_MAX 16
#define GSR_GRAD_CHUNK_ALIGN 4096

/* What gsr_set_preprocess, gsr_set_render and gsr_set_backward all take: the Gaussians (shapes and the
 * exactly-one-of rules as for gsr_forward_preprocess; M is ignored without shs) and the V cameras.  With shs, 1 <= M <= 50: the
 * per-Gaussian backward stages 256 rows of 3M floats in the CU's 160 KB of LDS; a wider row is rejected with
 * GSR_EINVAL by the preprocess and the backward before any launch (coefficients past 16 are never read). */
typedef struct gsr_set_scene {
  int V, P, degree, M, width, height, prefiltered;
  float scale_modifier;
  const float *means3D, *scales, *rotations, *opacities, *shs, *colors_precomp, *cov3D_precomp;
  /* host arrays of V device pointers: 4x4 matrices, camera positions (3,), background colours (3,) */
  const float *const *viewmatrices, *const *projmatrices, *const *campos, *const *bgs;
  const float *tanfovx, *tanfovy; /* host arrays of V values */
} gsr_set_scene;

/* The forward state of one set.  radii (V,P) and geom are written by gsr_set_preprocess; binning and image by
 * gsr_set_render, given num_rendered = the host array of V counts K from gsr_set_num_rendered (K = the
 * reference's num_rendered, the tiles of every visible Gaussian's 3-sigma rectangle: the capacity the binning and
 * backward scratch are sized by).  gsr_set_backward reads all of it and writes none, so it may be repeated.
 * The binning buffer belongs to this one forward until its last backward: besides the sorted tile lists the
 * forward may keep per listed instance a quadrant-mask byte in the buffer's second (free) key array, which the
 * backward's cull reads (csrc/gsr_common.h BinningState); the caller must not reuse the buffer in between. */
typedef struct gsr_set_state {
  int* radii;
  void *geom, *binning, *image;
  const int* num_rendered;
} gsr_set_state;

/* What gsr_set_render writes, and the optional fields that select what else its one blend pass forms. */
typedef struct gsr_set_outputs {
  float *out_color, *out_depth, *out_alpha; /* required */
  /*
   * out_render (V,3,H,W) non-NULL: the renderers' epilogue fused into the blend; the outputs above are written too.
   * With bg_images (V,H,W,3), the background network's outputs: the background renderer's composite (replaces
   * gsr_set_render + gsr_composite_forward for renderer/diff_gaussian_rasterizer_background.py:129-132,139),
   * out_render = clamp(color + (1 - alpha) bg, 0, 1), bit-identical to the torch expression on the stored outputs.
   * bg_images NULL: the clamp alone, out_render = clamp(color, 0, 1), the renderers' `rendered_image.clamp(0, 1)`
   * (renderer/diff_gaussian_rasterizer.py:141, renderer/diff_sugar_rasterizer_normal.py:212), bit-identical too.
   * bg_images needs out_render.
   */
  const float* bg_images;
  float* out_render;
  /*
   * Both non-NULL: two rasterizer calls that differ only in their colours, sharing one geometry (the SuGaR normal
   * renderer, renderer/diff_sugar_rasterizer_normal.py:157-191: the same Gaussians, camera and settings rendered
   * with the SH / override colours, then with colors_precomp = the face normals and a zero means2D).  The second
   * call's preprocess, sorts, binning and blend weights are the first's, so the forward blends both colour sets in
   * one pass: out_color2 (V,3,H,W) = the blend of colors2 (P,3) with the same weights and background, the second
   * call's colour output (its radii / depth / alpha equal the first call's).  Both or neither.
   * A set preprocessed with colors2 (gsr_set_preprocess) holds each Gaussian's second colour in its records and
   * remembers the pointer; the two-colour blends given that pointer read the records, given another they gather
   * from the array.  The pointer is the only key: the CONTENTS of colors2 must not change between
   * gsr_set_preprocess and the set's last backward.
   */
  const float* colors2;
  float* out_color2;
} gsr_set_outputs;

/* What gsr_set_backward reads and writes besides the scene and the forward state. */
typedef struct gsr_set_grads {
  /* dL/d(out_color) (V,3,H,W), or dL/d(out_render) when `color` is given; depth / alpha (V,1,H,W) may be NULL (zero) */
  const float *dL_dcolor, *dL_ddepth, *dL_dalpha;
  /*
   * color = the forward's out_color: the backward of a forward with out_render.  The blend's per-pixel prologue
   * masks dL/drender by the clamp (recomputed from color) and, with bg_images, adds dL/dalpha += -sum_c g_c bg_c
   * and forms dL_dbg (V,H,W,3) = g (1 - alpha) (NULL: not formed) — replaces gsr_composite_backward +
   * gsr_set_backward.  bg_images needs color; dL_dbg needs bg_images.
   */
  const float *color, *bg_images;
  float* dL_dbg;
  /*
   * The second call's backward of a two-colour forward on its own, on the shared forward state: colours =
   * colors_override (P,3), dL_dcolor = dL/d(out_color2), dL_dcolors = the gradient of colors_override, dL_dmeans2D
   * that call's screen-space gradient (the reference discards it: pass scratch).  That call has no SH, depth or alpha
   * gradient: scene->shs, dL_ddepth, dL_dalpha and dL_dsh must be NULL.  With accumulate the parameter gradients
   * continue the first call's.
   */
  const float* colors_override;
  /*
   * All three non-NULL: both calls' backward in one pass (replaces a plain or composite call followed by a
   * colors_override call): the blend is replayed once, forming both calls' dL/dalpha.  dL_dcolor2 = dL/d(out_color2),
   * dL_dcolors2 (P,3) = the gradient of colors2; dL_dmeans2D receives the first call's screen-space gradient only
   * (the second call's means2D is the reference's fresh zero tensor); the parameter gradients hold both calls'
   * (equal to the two-call sequence up to fp32 summation order).  All or none, and not with colors_override.
   * colors2 as in gsr_set_outputs.  Scratch: gsr_set_backward_bytes with two_colors != 0 (64-byte gradient rows).
   */
  const float *colors2, *dL_dcolor2;
  float* dL_dcolors2;
  /*
   * Outputs, shapes and NULL rules as for gsr_backward, summed over the set's views; dL_dmeans2D (V,P,3) is per view
   * and always overwritten.  accumulate = 0: overwritten; != 0: every per-Gaussian sum resumes from the stored value
   * in view order (a later set of the same batch, or the colors_override call after the first).  With accumulate in
   * the scale / rotation path dL_dcov3D is required: it carries the running dL/dcov3D that the scale and rotation
   * gradients are recomputed from.
   */
  float *dL_dmeans2D, *dL_dcolors, *dL_dopacity, *dL_dmeans3D, *dL_dcov3D, *dL_dsh, *dL_dscales, *dL_drotations;
  int accumulate;
  /* Scratch for the gradient rows and per-(view, Gaussian) records.  gsr_set_backward_bytes holds all V views; less
   * is accepted (>= what the largest single view needs) and the views are then walked in groups that fit.  Any
   * grouping gives bitwise the same gradients. */
  void* work;
  size_t work_bytes;
  /*
   * Overlap of the per-Gaussian sums with their reduction across ranks.  n_chunks = 0: the final
   * per-Gaussian gradients are formed in one pass after the backward blend.  1..GSR_GRAD_CHUNKS_MAX: in that many
   * Gaussian ranges, recording chunk_events[c] (hipEvent_t; the array required, an entry may be NULL) on the stream
   * after range c, so that the caller can start reducing range c (e.g. an RCCL all-reduce on another stream waiting
   * on the event) while the later ranges are computed.  Range c = [c S, min(P, (c + 1) S)) with
   * S = GSR_GRAD_CHUNK_ALIGN x ceil(ceil(P / n_chunks) / ALIGN) (gsr_grad_chunk_range); ranges may be empty.
   * Results are bitwise those of the unchunked call.
   */
  int n_chunks;
  void* const* chunk_events;
} gsr_set_grads;

size_t gsr_set_geom_bytes(int V, int P);
size_t gsr_set_binning_bytes(int V, int P, const int* num_rendered, int width, int height);
/* The image bytes of the forward with these counts: with the split backward's checkpoints only when the forward
 * writes them (a launch of <= 4096 tiles on the quadrant waves, one colour set: 335 MB for one 1024^2 view, held
 * until the backward); two_colors != 0: a render with colors2.  The forward records its decision in the buffer;
 * the backward follows it whatever the environment says then.  num_rendered NULL: the upper bound over all counts. */
size_t gsr_set_image_bytes(int V, int P, const int* num_rendered, int width, int height, int two_colors);
/* gsr_set_grads.work for all V views in one group (two_colors != 0: the one-pass two-colour backward).  0 for a bad
 * V or a NULL or negative count. */
size_t gsr_set_backward_bytes(int V, int P, const int* num_rendered, int two_colors);
/* Phase 1 of the set: writes state->radii and state->geom.  colors2 (P,3) non-NULL: the set will be blended with it
 * as the second colour set; the preprocess writes each Gaussian's second colour into the per-(view, Gaussian) record
 * it writes anyway (no extra traffic), see gsr_set_outputs.colors2. */
int gsr_set_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const float* colors2, void* stream);
/* One D2H read of every view's K, visible count (may be NULL) and num_listed (may be NULL): the instances the tile
 * lists actually hold after the exact ellipse-vs-tile culling (<= K), for diagnostics and rooflines.
 * Synchronises `stream`. */
int gsr_set_num_rendered(int V, const void* geom, int P, int* num_rendered, int* num_visible, int* num_listed,
                         void* stream);
/* Diagnostic copy (device to device, on `stream`) of the preprocess state of every (view, Gaussian):
 * out_rec (V, P, 16) 32-bit words = (pixel x, pixel y, conic a, conic b | conic c, opacity, view depth, 0 |
 * r, g, b, 0 | tile rect xmin | ymin << 16, xmax | ymax << 16, 0, SH clamp flags), written only for
 * visible Gaussians; out_tiles (V, P, 2) u32 = (3-sigma rectangle tiles, 0 = culled; tiles the
 * alpha >= 1/255 ellipse reaches).  Either may be NULL.  Parity tests compare these with the oracle's
 * per-Gaussian preprocess values (the reference's geomBuffer has no public layout). */
int gsr_set_gauss_state(int V, const void* geom, int P, void* out_rec, void* out_tiles, void* stream);
int gsr_set_render(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_outputs* outputs,
                   void* stream);
int gsr_set_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                     void* stream);
int gsr_grad_chunk_range(int P, int n_chunks, int chunk, int* g0, int* g1);

/*
 * Timed view sets: a view set whose views each carry their own Gaussian geometry — frame v of a time batch rendered
 * from camera v (renderer/diff_sugar_rasterizer_temporal.py:150-192 and renderer/diff_gaussian_rasterizer_st.py call
 * the rasterizer once per frame; gsr_sugar_timed_forward returns all frames at once as (T,N,.) arrays).  Every stage
 * stays one launch per set.  The state, the size queries, gsr_set_num_rendered and gsr_set_render are those of a plain
 * set (gsr_set_render reads no geometry array of the scene); only the preprocess and the backward have timed twins.
 *
 * gsr_set_timed: per-view arrays, view-major.  A non-NULL field replaces the scene's shared array of that name for
 * this set (the scene's field is then ignored and may be NULL); a NULL field means "shared, as in a plain set".
 * means3D_v (V,P,3) is required; scales_v (V,P,3), rotations_v (V,P,4) and colors2_v (V,P,3) are optional.  With
 * colors2_v the preprocess writes view v's second colour into view v's records and remembers the pointer: pass
 * colors2_v itself as gsr_set_outputs.colors2 and gsr_set_grads.colors2 and the blends read the records (the pointer
 * is the key, see gsr_set_outputs.colors2); a shared second colour set (P,3) is not embedded: the blends gather it.
 * Opacities and colours are shared.  Not built, rejected with GSR_EINVAL before any device work: shs (the timed
 * renderers pass precomputed colours), cov3D_precomp, and in the backward colors_override and n_chunks > 0.
 */
typedef struct gsr_set_timed {
  const float *means3D_v, *scales_v, *rotations_v, *colors2_v;
} gsr_set_timed;

/*
 * The per-view gradients of a timed set: the shapes of the inputs, one row per (view, Gaussian), NOT summed over the
 * views, and always overwritten (accumulate does not apply): a (view, Gaussian) the view's blend did not reach gets
 * exactly +0.  dL_dmeans3D_v is required; each of the others is required when its input is per view and ignored when
 * it is not.  The gradients of what stays shared go through gsr_set_grads as for a plain set, summed over the views
 * in view order and continued across sets and view groups with `accumulate`: dL_dopacity, dL_dcolors, dL_dscales
 * (scales_v NULL), dL_drotations (rotations_v NULL), dL_dcolors2 (colors2 shared).  gsr_set_grads.dL_dmeans3D,
 * dL_dcov3D and dL_dsh are not used and may be NULL (accumulate needs no dL_dcov3D here: the scale and rotation
 * gradients are formed per view from that view's dL/dcov3D and summed).  Two runs give the same bits.
 */
typedef struct gsr_set_timed_grads {
  float *dL_dmeans3D_v, *dL_dscales_v, *dL_drotations_v, *dL_dcolors2_v;
} gsr_set_timed_grads;

/* gsr_set_preprocess of a timed set. */
int gsr_set_timed_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_timed* timed,
                             void* stream);
/* gsr_set_backward of a timed set (after gsr_set_timed_preprocess + gsr_set_render with the same arrays). */
int gsr_set_timed_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                           const gsr_set_timed* timed, const gsr_set_timed_grads* timed_grads, void* stream);

/*
 * Densification statistics of a view batch: what the reference's GaussianBaseModel.update_states
 * (geometry/gaussian_base.py:845-851) accumulates view by view after the backward, for V <= GSR_SET_MAX views in one
 * launch.  Per Gaussian p, from the running values m = max_radii[p], s = grad_norm_sum[p], c = count[p] (accumulate 1)
 * or from zero (accumulate 0), for v = 0 .. V-1 in this order:
 *     m = max(m, (float)radii[v][p])                       (a NaN already in m stays, as torch.max keeps it)
 *     seen = visible[v] ? visible[v][p] != 0 : radii[v][p] > 0
 *     if seen:  s = s + sqrt(x * x + y * y)  with x = grads[v][3p], y = grads[v][3p + 1]   (skipped: grads[v] NULL)
 *               c = c + 1
 * in fp32, every operation rounded on its own (no fused multiply-add) and the square root correctly rounded: the bits
 * of the fp32 composition (gx * gx + gy * gy).sqrt() of IEEE operations, added view after view.  The update is
 * sequential and in place,
 * so a batch of more than GSR_SET_MAX views is several calls in view order with accumulate = 1, with the bits of one
 * call.  No atomics: two calls give the same bits.
 *   radii    V rows of P int32 (gsr_set_state.radii rows)
 *   grads    V rows of (P,3) float (the screen-space gradient rows, gsr_set_grads.dL_dmeans2D); an entry may be NULL
 *            (no gradient reached that view: it still counts)
 *   visible  V rows of P bytes, or all NULL: visible = radii > 0
 * The arrays are device memory; the struct is read during the call and no pointer to it is kept.  Entries past V are
 * ignored.  P == 0 or V == 0 launches nothing and leaves the three arrays as they are (also with accumulate 0).
 * GSR_EINVAL, before any device work: V outside 0..GSR_SET_MAX, P < 0, a NULL radii row, a NULL output, visibility
 * rows that are partly NULL.
 */
/* (tables of one device pointer per view, held in the struct itself: GSR_SET_MAX entries each) */
typedef const int* gsr_view_rows_i32[GSR_SET_MAX];
typedef const float* gsr_view_rows_f32[GSR_SET_MAX];
typedef const unsigned char* gsr_view_rows_u8[GSR_SET_MAX];
typedef struct gsr_densify_batch {
  int V, P, accumulate;                       /* accumulate 0: start from zero; 1: from the arrays' contents */
  gsr_view_rows_i32 radii;
  gsr_view_rows_f32 grads;
  gsr_view_rows_u8 visible;
  float *max_radii, *grad_norm_sum, *count;   /* P each */
} gsr_densify_batch;
int gsr_densify_stats(const gsr_densify_batch* in, void* stream);

/*
 * Optional phase timing with HIP events recorded on the launch stream around each phase's kernels.
 * Off by default; while on, every call above records one event pair per phase it runs.
 * gsr_profile_read synchronises the recorded events and returns, per phase, the accumulated
 * milliseconds and the number of timed launches since the last reset (arrays of GSR_NUM_PHASES).
 */
#define GSR_PHASE_PREPROCESS 0 /* k_preprocess                                              */
#define GSR_PHASE_DEPTH_SORT 1 /* per-view depth radix sort, instance counts and offsets     */
#define GSR_PHASE_BINNING 2    /* instance emission, tile radix sort, tile ranges           */
#define GSR_PHASE_RENDER_FWD 3 /* k_render_fwd: forward tile blend                          */
#define GSR_PHASE_RENDER_BWD 4 /* k_render_bwd: backward tile blend                         */
#define GSR_PHASE_GAUSS_BWD 5  /* k_gauss_bwd: fused per-Gaussian backward                   */
#define GSR_NUM_PHASES 6
int gsr_profile_enable(int enable);
int gsr_profile_read(double* ms, long long* launches, int reset);
/* The blend kernel the last GSR_PHASE_RENDER_FWD / GSR_PHASE_RENDER_BWD launch of this process used, as
 * rocprofv3 names it (e.g. "k_render_bwd<false, false>"); "" for other phases or before any launch.  Lets a
 * caller attribute committed PMC counters to the kernel actually timed. */
const char* gsr_profile_kernel(int phase);

/*
 * Fused background composite of the background renderer (replaces the torch epilogue of
 * renderer/diff_gaussian_rasterizer_background.py:129-132,139):
 *     out = clamp(color + (1 - alpha) * bg, 0, 1)       color, out (V, 3, H, W); alpha (V, 1, H, W)
 * bg_layout: GSR_BG_CONSTANT (V, 3), GSR_BG_HWC (V, H, W, 3) -- the background network's output --,
 * GSR_BG_CHW (V, 3, H, W).  Backward (pre-clamp value recomputed; clamp's inclusive-bounds gradient):
 * dL_dcolor = g, dL_dalpha = -sum_c g_c bg_c, dL_dbg = g (1 - alpha) (NULL: not computed; image
 * layouts only), with g = dL_dout where 0 <= pre <= 1, else 0.  Bit-identical to the torch expression
 * in the forward.
 */
#define GSR_BG_CONSTANT 0
#define GSR_BG_HWC 1
#define GSR_BG_CHW 2
int gsr_composite_forward(int V, int height, int width, const float* color, const float* alpha, const float* bg,
                          int bg_layout, float* out, void* stream);
int gsr_composite_backward(int V, int height, int width, const float* dL_dout, const float* color,
                           const float* alpha, const float* bg, int bg_layout, float* dL_dcolor, float* dL_dalpha,
                           float* dL_dbg, void* stream);

/*
 * SuGaR normal map (replaces the torch lines of renderer/diff_sugar_rasterizer_normal.py:192-197 after the
 * second rasterizer call): normal (V, 3, H, W) = the blended face normals, alpha (V, 1, H, W);
 *   out = (-u_x, -u_y, u_z) * 0.5 * alpha + 0.5 with u = normal / max(|normal|, 1e-12) (torch's order).
 * Backward: the gradient flows only where alpha > 0.99 (the rest is detached in the reference);
 * dL_dnormal (V, 3, H, W) and dL_dalpha (V, 1, H, W) are written whole (zeros where masked).
 */
int gsr_normal_map_forward(int V, int height, int width, const float* normal, const float* alpha, float* out,
                           void* stream);
int gsr_normal_map_backward(int V, int height, int width, const float* dL_dout, const float* normal,
                            const float* alpha, float* dL_dnormal, float* dL_dalpha, void* stream);

/*
 * Fused shading / depth-normal epilogue of the MVDream shading renderer and the SuGaR normal renderer
 * (replaces the torch ops of renderer/diff_gaussian_rasterizer_shading.py:169-208 with Depth2Normal
 * :22-51 and material/gaussian_material.py:41-104; renderer/diff_sugar_rasterizer_normal.py:170-197).
 * Per pixel of V views (planes (V, 3|1, H, W); rays (V, H, W, 3); light (V, 3)):
 *     X = rays_o + depth rays_d;  u = normalize(-(dX/dx x dX/dy)), central differences, X zero-padded;
 *     unit_normal = u;  normal_map = u 0.5 alpha + 0.5;  depth_out = depth
 * and with GSR_SHADE_MATERIAL the point-light material and background composite:
 *     s = u (or normalize(2 pred_normal - 1) when pred_normal != NULL, detached);
 *     t = max(s . normalize(light - X), 0) kd + ka;  albedo = color / (alpha + 1e-6);
 *     fg = clamp(albedo, 0, 1) t | albedo | t   (mode GSR_SHADING_DIFFUSE | _ALBEDO | _TEXTURELESS);
 *     render = clamp(fg alpha + (1 - alpha) bg, 0, 1),  bg GSR_BG_CONSTANT (V, 3) or GSR_BG_HWC.
 * ambient / diffuse: host arrays of 3 floats (ka, kd; ignored without the material flag).
 * Outputs may be NULL (not written) except render with the material flag.  Backward: gradients of
 * render / normal_map / unit_normal / depth_out (any may be NULL = zero); the normal-map, unit-normal
 * and depth_out gradients are kept only where alpha > 0.99 (the reference's in-place detach of the
 * other pixels).  Outputs dL_ddepth, dL_dalpha (required), dL_dcolor (material), dL_dbg (NULL = not
 * formed; GSR_BG_HWC only).
 */
#define GSR_SHADE_MATERIAL 1
#define GSR_SHADING_DIFFUSE 0
#define GSR_SHADING_ALBEDO 1
#define GSR_SHADING_TEXTURELESS 2
int gsr_shade_forward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                      const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                      const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                      float* render, float* normal_map, float* unit_normal, float* depth_out, void* stream);
int gsr_shade_backward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                       const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                       const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                       const float* dL_drender, const float* dL_dnormal_map, const float* dL_dunit_normal,
                       const float* dL_ddepth_out, float* dL_dcolor, float* dL_ddepth, float* dL_dalpha,
                       float* dL_dbg, void* stream);
/*
 * As gsr_shade_forward / gsr_shade_backward with the light colours and shading mode given PER VIEW:
 * modes (V,) host ints, ambient / diffuse (V, 3) host floats.  The reference's material draws its soft-shading
 * ambient ratio and its shading mode once per view (material/gaussian_material.py:59-64,80-88, called once per
 * view by renderer/diff_gaussian_rasterizer_shading.py:200-205 inside the per-view loop of
 * renderer/gaussian_batch_renderer.py:21-54), so a fused batch needs one (ka, kd, mode) per view.
 * modes / ambient / diffuse may be NULL without GSR_SHADE_MATERIAL.
 */
int gsr_shade_views_forward(int V, int height, int width, int flags, const int* modes, const float* color,
                            const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                            const float* bg, int bg_layout, const float* light, const float* pred_normal,
                            const float* ambient, const float* diffuse, float* render, float* normal_map,
                            float* unit_normal, float* depth_out, void* stream);
int gsr_shade_views_backward(int V, int height, int width, int flags, const int* modes, const float* color,
                             const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                             const float* bg, int bg_layout, const float* light, const float* pred_normal,
                             const float* ambient, const float* diffuse, const float* dL_drender,
                             const float* dL_dnormal_map, const float* dL_dunit_normal, const float* dL_ddepth_out,
                             float* dL_dcolor, float* dL_ddepth, float* dL_dalpha, float* dL_dbg, void* stream);

/*
 * Mean squared distance to the 3 nearest other points, for each of P points (P, 3) -> (P,): replaces
 * simple_knn._C.distCUDA2 (called at geometry/gaussian_base.py:434-437 to initialise scales; also imported by
 * geometry/sugar.py:18, geometry/gaussian_io.py:25, geometry/spacetime_gaussian.py:15,430,
 * geometry/dynamic_sugar.py:17, geometry/gaussian_dynamic.py:25).  Exact search; per-pair fp32 distance
 * fma(dz, dz, fma(dy, dy, dx * dx)); result (b0 + b1 + b2) / 3 over the sorted 3 best (FLT_MAX entries
 * kept when P < 4).  workspace: gsr_knn_workspace_bytes(P) bytes of device memory (256-B aligned).
 */
size_t gsr_knn_workspace_bytes(int P);
int gsr_knn_mean_dist(int P, const float* points, float* mean_dist, void* workspace, size_t workspace_bytes,
                      void* stream);

/*
 * The K nearest points of each of P points within the same cloud, (P, 3) -> dists (P, K) float, idx (P, K) int64:
 * replaces pytorch3d.ops.knn_points(points[None], points[None], K) of the SuGaR geometry and regulariser
 * (geometry/sugar.py:646, utils/sugar_utils.py:41,248).  1 <= K <= GSR_KNN_MAX_K.  Exact search over the tree of
 * gsr_knn_mean_dist with the same per-pair fp32 squared distance fma(dz, dz, fma(dy, dy, dx * dx)).  A point is its own
 * neighbour (distance 0).  Each row ascends by (distance, index): exact fp32 ties go to the lower input index, so
 * the result is a pure function of the input.  Rows of a cloud with P < K end with dists = +inf, idx = -1 in the
 * missing columns.  NaN or infinite coordinates: unspecified.  Indices refer to the input order and are written as
 * int64 directly.  workspace: gsr_knn_points_workspace_bytes(P, K) bytes of device memory (256-B aligned).  Kernels
 * run on `stream`; the library allocates nothing.  P = 0 launches nothing.
 */
#define GSR_KNN_MAX_K 32
size_t gsr_knn_points_workspace_bytes(int P, int K);
int gsr_knn_points(int P, int K, const float* points, float* dists, long long* idx, void* workspace,
                   size_t workspace_bytes, void* stream);

/*
 * The neighbour density field of the SuGaR regulariser: replaces the gathers, the batched matmul and the sum of
 * SuGaRRegularizer.get_field_values (utils/sugar_utils.py:296-310), the `average` beta of get_beta (:423), and the
 * index_put scatter of their autograd backward.  M samples, K neighbour slots (1 <= K <= GSR_KNN_MAX_K), N Gaussians,
 * M K < 2^31.  The inputs are the fields of gsr_sugar_field below; all float arrays fp32.
 * With row, sample m reads the table row nbr[row[m]] (the reference's knn_idx[gaussian_idx], R = N, never gathered
 * into an (M,K) copy); with row NULL, R must equal M and sample m reads nbr[m] (closest_gaussians_idx).
 * For slot k with j = nbr[..][k]:
 *   d = x_m - c_j;   w = inv_sr_j^T d;   q = clamp(w.w, 0, 1e8);   op[m,k] = density_factor strengths_j exp(-q / 2)
 *   density[m] = sum_k op[m,k]           (raw, the reference's fields['density'])
 *   beta_avg[m] = (sum_k min_scale_j) / K
 * op (M,K) may be NULL (not written).  d, w, q and the exponential are evaluated in fp64 per pair and rounded to fp32
 * once; the sums and the gradient arithmetic are fp32.
 * Out of range: a slot whose j is outside [0, N) (the -1 padding of gsr_knn_points included) contributes nothing to
 * any output or gradient, op = 0 there, and j is never dereferenced; beta_avg still divides by K.  A row entry
 * outside [0, R) makes every slot of that sample such a slot: density = beta_avg = op = 0 and zero gradients.
 * NaN coordinates: unspecified values, no out-of-bounds access.
 * Backward: dL_ddensity (M), dL_dbeta_avg (M), dL_dop (M,K), any may be NULL (zero).  Writes in full dL_dx (M,3),
 * dL_dcenters (N,3), dL_dinv_sr (N,3,3), dL_dstrengths (N), dL_dmin_scale (N); entries nothing contributes to are
 * exactly 0.  The clamp's gradient is 0 where w.w > 1e8.  Every pair is recomputed from the inputs; nothing of the
 * forward is kept.
 * Sum orders (no atomics; every result is a pure function of the input, two calls give the same bits):
 *   over slots (density, beta_avg, dL_dx): 16 partial sums, partial l = term l (+ term l + 16 when K > 16), terms
 *   of absent or out-of-range slots 0; the partials are combined pairwise at distances 8, 4, 2, 1
 *   (t[i] += t[i ^ 8], then ^ 4, ^ 2, ^ 1).
 *   per Gaussian (the four N-sized gradients): its pairs in ascending m K + k (a stable radix sort of the pairs by
 *   Gaussian, csrc/gsr_sort.hip); pair number i of the Gaussian goes to partial i mod L, each partial adds its pairs
 *   in that order starting from 0, and the L partials are combined pairwise at distances L/2, ..., 2, 1.
 *   L = 64 when M K >= 48 N, else 16.
 * workspace: gsr_sugar_field_workspace_bytes(M, K, N) bytes of device memory (256-B aligned) for the backward:
 * sort keys and values double-buffered (16 M K bytes), the sort's counters (M K / 16), one 64-byte record and two
 * words per Gaussian; nothing of size 9 M K.  The forward needs gsr_sugar_field_workspace_bytes(0, K, N) (the
 * records) only.  Kernels run on `stream`; the library allocates nothing.  M = 0 launches nothing and writes
 * nothing (the caller zeroes the N-sized gradients of an empty batch).
 */
typedef struct gsr_sugar_field {
  int M, K, N, R;       /* samples, neighbour slots, Gaussians, rows of nbr */
  const float* x;       /* (M,3) sample points */
  const long long* nbr; /* (R,K) int64 neighbour table */
  const long long* row; /* (M,) int64, the table row of each sample, or NULL (then R = M) */
  const float* centers; /* (N,3) */
  /* (N,3,3) row-major = R[i][j] / max(s[j], 1e-8), what get_covariance(return_full_matrix=True, return_sqrt=True,
   * inverse_scales=True) returns */
  const float* inv_sr;
  const float* strengths; /* (N,) */
  const float* min_scale; /* (N,) = scaling.min(-1) */
  float density_factor;
} gsr_sugar_field;
size_t gsr_sugar_field_workspace_bytes(int M, int K, int N);
int gsr_sugar_field_forward(const gsr_sugar_field* in, float* density, float* beta_avg, float* op, void* workspace,
                            size_t workspace_bytes, void* stream);
int gsr_sugar_field_backward(const gsr_sugar_field* in, const float* dL_ddensity, const float* dL_dbeta_avg,
                             const float* dL_dop, float* dL_dx, float* dL_dcenters, float* dL_dinv_sr,
                             float* dL_dstrengths, float* dL_dmin_scale, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * The neighbour-normal loss of the SuGaR regulariser ("sdf better normal loss"): replaces the (M,K,3) gathers, the
 * sign flip, the weight normalisation and the weighted normal sum of coarse_density_regulation
 * (utils/sugar_utils.py:725-757) and the index_put scatter of their autograd backward.  M samples, K neighbour slots
 * (1 <= K <= GSR_KNN_MAX_K), N Gaussians, M (K + 1) < 2^31.  The inputs are the fields of gsr_sugar_normal below; all
 * float arrays fp32.
 * With per_sample = 0, sample m reads the table row nbr[own[m]] (the reference's knn_idx, R = N, never gathered into
 * an (M,K) copy); with per_sample != 0, R must equal M and sample m reads nbr[m].
 * For slot k with j = nbr[..][k] and i = own[m]:
 *   s_k = sign(n_j . n_i)  (sign(0) = 0);   a_k = |(x_m - c_j) . (s_k n_j)|
 *   w_k = op[m,k] a_k / max(min_scale_j, 1e-6)^2;   W = sum_k w_k;   Wc = max(W, 1e-6);   wh_k = w_k / Wc
 *   r = n_i - sum_k wh_k s_k n_j;   loss[m] = r . r
 * s, a, op, min_scale and W are constants of the loss (detached in the reference, whose
 * sdf_better_normal_gradient_through_normal_only is always on), so only the normals receive a gradient:
 *   dL/dn_i += 2 dL_dloss[m] r;   dL/dn_j += -2 dL_dloss[m] wh_k s_k r.
 * Precision: n_j . n_i and (x_m - c_j) . n_j (which cancels: samples lie near their Gaussian's plane) are evaluated
 * in fp64 per pair and rounded once; everything else is fp32.  r is summed in the equal form
 *   r = (1 - W / Wc) n_i + sum_k wh_k (n_i - s_k n_j),      1 - W / Wc taken as exactly 0 when W >= 1e-6,
 * which spares the cancellation of n_i against the sample's own slot (j = i: that term is exactly 0).
 * Out of range: a slot whose j is outside [0, N) (the -1 padding of gsr_knn_points included) contributes nothing to
 * the loss or to any gradient, and j is never dereferenced.  A sample whose own[m] is outside [0, N), or
 * outside [0, R) when it selects the table row, has loss[m] = 0 and no gradient; no row is read for it.
 * NaN inputs: unspecified values, no out-of-bounds access.
 * rec (M,4), 16-byte aligned (checked: GSR_EINVAL otherwise), may be NULL in a forward no backward follows: the forward writes (r, Wc) per sample
 * and the backward reads it (with dL_dloss (M), required); everything else of a pair is recomputed from the inputs,
 * nothing M x K-sized is kept.  The backward writes dL_dnormals (N,3) in full; rows nothing contributes to are
 * exactly 0.
 * Sum orders (no atomics; every result is a pure function of the input, two calls give the same bits):
 *   over slots (W, and the three components of r): 16 partial sums, partial l = term l (+ term l + 16 when K > 16),
 *   terms of absent or out-of-range slots 0; the partials are combined pairwise at distances 8, 4, 2, 1
 *   (t[i] += t[i ^ 8], then ^ 4, ^ 2, ^ 1); then r = fma(1 - W / Wc, n_i, that sum), loss = fma(r2, r2, fma(r1, r1,
 *   r0 r0)).
 *   per Gaussian (dL_dnormals): every sample has K + 1 terms, term m (K + 1) + k for slot k < K (coefficient
 *   -2 dL_dloss[m] wh_k s_k, Gaussian j) and term m (K + 1) + K for the sample's own normal (coefficient
 *   2 dL_dloss[m], Gaussian i); each term is coefficient x r_m.  A Gaussian's terms are taken in ascending term
 *   number (a stable radix sort of the terms by Gaussian, csrc/gsr_sort.hip); term number t of the Gaussian goes to
 *   partial t mod L, each partial adds its terms by fma in that order starting from 0, and the L partials are
 *   combined pairwise at distances L/2, ..., 2, 1.  L = 64 when M (K + 1) >= 48 N, else 16.
 * workspace: gsr_sugar_normal_workspace_bytes(M, K, N) bytes of device memory (256-B aligned) for the backward: sort
 * keys and values double-buffered and one coefficient per term (20 M (K + 1) bytes), the sort's counters
 * (M (K + 1) / 4 bytes: 256 32-bit words per 4096 terms), one 32-byte record and two 32-bit words per Gaussian: at most 24 M (K + 1) + 80 N + 8192 bytes, nothing
 * of size 3 M K floats.  The forward needs gsr_sugar_normal_workspace_bytes(0, K, N) (the records) only.  Kernels
 * run on `stream`; the library allocates nothing.  M = 0 launches nothing and writes nothing (the caller zeroes the
 * gradient of an empty batch).
 */
typedef struct gsr_sugar_normal {
  int M, K, N, R;         /* samples, neighbour slots, Gaussians, rows of nbr */
  const float* x;         /* (M,3) sample points */
  const long long* own;   /* (M,) int64, the Gaussian i each sample was drawn in (gaussian_idx) */
  const long long* nbr;   /* (R,K) int64 neighbour table */
  int per_sample;         /* != 0: nbr has one row per sample; 0: sample m reads row own[m] */
  const float* centers;   /* (N,3) */
  const float* normals;   /* (N,3), need not be unit length */
  const float* min_scale; /* (N,) = scaling.min(-1) */
  const float* op;        /* (M,K), the op of gsr_sugar_field_forward for the same samples and table */
} gsr_sugar_normal;
size_t gsr_sugar_normal_workspace_bytes(int M, int K, int N);
int gsr_sugar_normal_forward(const gsr_sugar_normal* in, float* loss, float* rec, void* workspace,
                             size_t workspace_bytes, void* stream);
int gsr_sugar_normal_backward(const gsr_sugar_normal* in, const float* rec, const float* dL_dloss, float* dL_dnormals,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * The geometry of SuGaR Gaussians bound to a mesh: replaces SuGaRModel.points, .scaling, .quaternions and
 * .get_gs_normals (geometry/sugar.py:449-536), i.e. the (F,3,3) vertex gather, the pytorch3d face normals, the three
 * normalisations, the two cross products, the (N,3,3) concatenation, matrix_to_quaternion and the index_put scatter of
 * their autograd backward.  V vertices, F faces, G Gaussians per face (1 <= G <= GSR_MESH_MAX_G), N = F G (passed,
 * and checked: GSR_EINVAL otherwise), N < 2^31.  The inputs are the fields of gsr_sugar_mesh below and, positional,
 *   bary (G,3) fp32 in HOST memory (read during the call);  thickness, the normal-axis scale (forward only).
 * Gaussian f G + g belongs to face f.  With p0, p1, p2 = verts[faces[f]] and normalize(v, eps) = v / max(|v|, eps):
 *   c = (p1 - p0) x (p2 - p0);   n = normalize(c, 1e-6) (pytorch3d's face normal);   R0 = normalize(n, 1e-12)
 *   b1 = normalize(p0 - p1, 1e-12);   b2 = normalize(R0 x b1, 1e-12)
 *   z = normalize(cplx, 1e-12);   R1 = z0 b1 + z1 b2;   R2 = -z1 b1 + z0 b2
 *   q = matrix_to_quaternion([R0 | R1 | R2]) (columns): with a_i = sqrt_pos of 1+m00+m11+m22, 1+m00-m11-m22,
 *   1-m00+m11-m22, 1-m00-m11+m22 (sqrt_pos(x) = sqrt(x) for x > 0, else 0 with zero gradient), the candidate rows
 *   (a0^2, m21-m12, m02-m20, m10-m01), (m21-m12, a1^2, m10+m01, m02+m20), (m02-m20, m10+m01, a2^2, m12+m21),
 *   (m10-m01, m20+m02, m21+m12, a3^2), each divided by 2 max(a_i, 0.1); the row of the largest a_i is taken, the
 *   lowest index on ties; order (w, x, y, z); no sign standardisation.
 *   xyz = sum_k bary[g][k] p_k;   scaling = (thickness, exp(log_scales));   rotation = normalize(q, 1e-12);
 *   normals = R0 (the same for the G Gaussians of a face).
 * Outputs xyz (N,3), scaling (N,3), rotation (N,4), normals (N,3), all required.  rotation and dL_drotation must be
 * 16-byte aligned, cplx, log_scales and their gradients 8-byte aligned (checked: GSR_EINVAL otherwise).
 * Precision: the per-face frame, the per-Gaussian part and the gradient arithmetic are all evaluated in fp64 from the
 * fp32 inputs; every output and gradient is rounded to fp32 once, except dL_dverts: its per-corner terms are rounded
 * to fp32 once (the corner rows), added in fp64 and the sum rounded once.
 * Backward: the exact derivative of the composition above (the clamps pass the gradient where |v| >= eps and make the
 * quotient linear below; the candidate row is a constant choice).  dL_dxyz (N,3), dL_dscaling (N,3), dL_drotation
 * (N,4), dL_dnormals (N,3): any may be NULL (zero).  Writes in full dL_dverts (V,3), dL_dcomplex (N,2) and
 * dL_dlog_scales (N,2); a vertex no face uses gets exactly 0.  The frame is recomputed from the inputs: the forward
 * keeps nothing.  corner_order (3F,) int32 and vert_offsets (V+1,) int32 are the vertex incidence: the corners
 * (numbered 3 f + c) of vertex v are corner_order[vert_offsets[v] .. vert_offsets[v+1]).
 * Out of range: a face with an entry outside [0, V) has all four outputs, its Gaussians' gradients and its corner
 * rows 0, and the entry is never dereferenced.  A corner_order entry outside [0, 3F) is skipped; offsets are clamped
 * to [0, 3F].  NaN inputs: unspecified values, no out-of-bounds access.
 * Sum orders (no atomics; every result is a pure function of the input, two calls give the same bits):
 *   per face (the gradients to R0, b1, b2 and the bary-weighted dL_dxyz to each corner): its Gaussians in ascending
 *   g, each partial starting from 0; the frame's own terms are added after the last Gaussian.
 *   per vertex (dL_dverts): its corner rows in the order of corner_order, sequentially, starting from 0.
 * workspace (backward only): gsr_sugar_mesh_workspace_bytes(F, V) bytes of device memory (256-B aligned): the corner
 * rows, 36 F bytes (at least 256, also for F = 0).  Kernels run on `stream`; the library allocates nothing.  The
 * forward is one launch, the backward two.  F = 0 launches nothing and writes nothing (the caller zeroes dL_dverts).
 */
#define GSR_MESH_MAX_G 8
typedef struct gsr_sugar_mesh {
  int V, F, G;             /* vertices, faces, Gaussians per face */
  const float* verts;      /* (V,3) */
  const int* faces;        /* (F,3) int32 */
  const float* cplx;       /* (F G,2) complex_numbers, the in-plane rotation; 8-byte aligned */
  const float* log_scales; /* (F G,2); 8-byte aligned */
} gsr_sugar_mesh;
size_t gsr_sugar_mesh_workspace_bytes(int F, int V);
int gsr_sugar_mesh_forward(const gsr_sugar_mesh* in, int N, const float* bary, float thickness, float* xyz,
                           float* scaling, float* rotation, float* normals, void* stream);
int gsr_sugar_mesh_backward(const gsr_sugar_mesh* in, int N, const float* bary, const int* corner_order,
                            const int* vert_offsets, const float* dL_dxyz, const float* dL_dscaling,
                            const float* dL_drotation, const float* dL_dnormals, float* dL_dverts, float* dL_dcomplex,
                            float* dL_dlog_scales, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Dynamic SuGaR, the time-batched geometry of geometry/dynamic_sugar.py, in two calls for all T frames of a batch.
 * Quaternions marked xyzw are pypose's (x, y, z, w); `rotation` and `rotation0` are this library's (w, x, y, z).
 * (x) is the Hamilton product, conj negates the vector part, (a, 0) is the pure quaternion of a vector.
 *   Log(q), q = (v, w) != 0 of any norm: s v with s = 2 atan(|v| / w) / |v| (the plain arctangent of the quotient:
 *     Log(q) = Log(-q) = Log(c q), |s v| <= pi; pi / |v| at w = 0); for |v|^2 < 1e-8 w^2 the series
 *     s = 2 / w - 2 |v|^2 / (3 w^3), so that Log and its derivative (2 / w I to v, 0 to w) are exact at the identity.
 *   Exp(phi) = (k phi, c), theta = |phi|, k = sin(theta / 2) / theta, c = cos(theta / 2); for theta^2 < 1e-8 the series
 *     k = 1/2 - theta^2 / 48, c = 1 - theta^2 / 8.
 *   R(q) p = p + 2 v x (v x p + w p) for a unit q.
 *
 * gsr_sugar_skin_*: the deformation-graph skinning of the mesh vertices (_get_timed_vertex_attributes_from_dg,
 * dynamic_sugar.py:505-575).  T frames, V vertices, P nodes, K nodes per vertex (1 <= K <= GSR_SKIN_MAX_K);
 * T V, T P and V K < 2^31.  The inputs are the fields of gsr_sugar_skin below.
 * With q^ = q / |q| per (t, node) and p = verts[v], the sums over the K nodes of v in ascending k, from 0:
 *   GSR_SKIN_DQS:  d = 1/2 (trans, 0) (x) q^;   S_r = sum w_k q^_k;   S_d = sum w_k d_k;   m = |S_r|;
 *                  r = S_r / m;   e = S_d / m;   vert_xyz = R(r) p + 2 vec(e (x) conj(r))   (no antipodal sign fix)
 *   GSR_SKIN_LBS:  vert_xyz = sum w_k (R(q^_k) (p - node_xyz_k) + node_xyz_k + trans_k)
 *   both:          vert_rot = Exp(sum w_k Log(q_k)) (xyzw, unit, w >= 0);   vert_scale = sum w_k node_scales_k
 * A deliberate deviation in GSR_SKIN_LBS: the reference passes q_k to pypose's matrix() as it is, this header
 * normalises it first (as the reference's own "dqs" branch does).  On unit quaternions the values are equal; the
 * derivative along q_k (the quaternion's norm) is 0 here and 2 (R - I)(p - node_xyz_k) for a matrix() that does not
 * normalise.  tests/test_reference_pins.py compares that gradient without its component along q_k.
 * Outputs vert_xyz (T,V,3), vert_rot (T,V,4) 16-byte aligned, vert_scale (T,V,3) (required iff node_scales is given).
 * Backward: the exact derivative.  dL_dxyz (T,V,3), dL_drot (T,V,4), dL_dscale (T,V,3): any may be NULL (zero).
 * Writes in full dL_dverts (V,3), dL_dnode_trans (T,P,3), dL_dnode_rots (T,P,4) (through the normalisation) and, iff
 * node_scales is given, dL_dnode_scales (T,P,3); a node no vertex uses gets exactly 0.  item_order (V K,) int32 and
 * node_offsets (P+1,) int32 are the node incidence: the items (numbered v K + k) of node j are
 * item_order[node_offsets[j] .. node_offsets[j+1]).
 * Out of range: an nbr entry outside [0, P) contributes nothing and is never used as an index; an item_order entry
 * outside [0, V K) is skipped; offsets are clamped to [0, V K].  A zero node quaternion or S_r = 0: unspecified
 * values, no out-of-bounds access (as for NaN inputs).
 * Sum orders (no atomics; two calls give the same bits): per (t, vertex) its K items ascending; dL_dverts over t
 * ascending; per (t, node) lane l of one 64-lane wave adds the entries l, l + 64, ... of its list in order, from 0,
 * and the 64 partial sums are added pairwise by a butterfly (lanes 32 apart first, then 16, ... 1).
 * Precision: fp64 arithmetic from the fp32 inputs; outputs and gradients are rounded to fp32 once; the per-(t, vertex)
 * adjoint rows that pass between the backward's kernels are fp32 (one rounding each) and are added in fp64.
 * workspace (forward and backward): gsr_sugar_skin_workspace_bytes(T, V, P) bytes of device memory (256-B aligned):
 * 88 T P bytes of per-(t, node) records (q^, d, Log q in fp64) and, used by the backward only, 56 T V bytes of rows.
 * The forward is two launches, the backward four, on `stream`; the library allocates nothing.  T = 0 or V = 0
 * launches nothing and writes nothing (the caller zeroes the gradients).
 *
 * gsr_sugar_timed_*: the Gaussians of the deformed mesh (get_timed_gs_attributes, fuse_rotations and
 * get_timed_gs_normals, dynamic_sugar.py:329-346, 618-688).  F faces, G Gaussians per face (1 <= G <=
 * GSR_MESH_MAX_G), N = F G (passed and checked); T N and T V < 2^31.  The inputs are the fields of gsr_sugar_timed
 * below and, positional, bary (G,3) fp32 in HOST memory.
 * For Gaussian n = f G + g, with i_c = faces[f][c] and b = bary[g]:
 *   xyz[t,n] = sum_c b_c vert_xyz[t,i_c];   phi = sum_c b_c Log(vert_rot[t,i_c]);
 *   rotation[t,n] = normalize(Exp(phi) (x) q0, 1e-12) stored wxyz, q0 = rotation0[n] read as xyzw;
 *   normals[t,n] = R0 of gsr_sugar_mesh_forward for the deformed face (the zero vector for a degenerate face);
 *   scaling[t,n] = (thickness, exp(log_scales[n][0] + s_1), exp(log_scales[n][1] + s_2)), s = sum_c b_c
 *   vert_scale[t,i_c] (s_0 is discarded: its gradient is exactly 0).
 * Outputs xyz (T,N,3), rotation (T,N,4), normals (T,N,3), scaling (T,N,3) (required iff vert_scale is given).
 * vert_rot, rotation0, rotation and their gradients must be 16-byte aligned, log_scales and its gradient 8-byte.
 * Backward: dL_dxyz, dL_drotation, dL_dnormals, dL_dscaling: any may be NULL (zero).  Writes in full dL_dvert_xyz
 * (T,V,3), dL_dvert_rot (T,V,4), dL_drotation0 (N,4) and, iff vert_scale is given, dL_dvert_scale (T,V,3) and
 * dL_dlog_scales (N,2); a vertex no face uses gets exactly 0.  corner_order and vert_offsets as for
 * gsr_sugar_mesh_backward.  Out of range: a face with an entry outside [0, V) has zero outputs, gradients and corner
 * rows, and the entry is never dereferenced; a corner_order entry outside [0, 3F) is skipped, offsets are clamped.
 * Sum orders: per (t, face) its Gaussians in ascending g, the normal's terms last; per (t, vertex) its corner rows in
 * the order of corner_order; dL_drotation0 and dL_dlog_scales over t ascending; all from 0.
 * workspace (backward only): gsr_sugar_timed_workspace_bytes(T, F) bytes: 120 T F bytes of fp32 corner rows.  The
 * forward is one launch, the backward three.  T = 0 or F = 0 launches nothing and writes nothing.
 */
#define GSR_SKIN_MAX_K 32
#define GSR_SKIN_DQS 0
#define GSR_SKIN_LBS 1
typedef struct gsr_sugar_skin {
  int T, V, P, K;           /* frames, vertices, nodes, nodes per vertex */
  int method;               /* GSR_SKIN_DQS or GSR_SKIN_LBS */
  const float* verts;       /* (V,3) */
  const float* node_xyz;    /* (P,3) */
  const float* node_trans;  /* (T,P,3) */
  const float* node_rots;   /* (T,P,4) xyzw, non-zero, any norm; 16-byte aligned */
  const float* node_scales; /* (T,P,3) or NULL */
  const int* nbr;           /* (V,K) int32, the nodes of a vertex */
  const float* w;           /* (V,K) fp32, their weights */
} gsr_sugar_skin;
size_t gsr_sugar_skin_workspace_bytes(int T, int V, int P);
int gsr_sugar_skin_forward(const gsr_sugar_skin* in, float* vert_xyz, float* vert_rot, float* vert_scale,
                           void* workspace, size_t workspace_bytes, void* stream);
int gsr_sugar_skin_backward(const gsr_sugar_skin* in, const int* item_order, const int* node_offsets,
                            const float* dL_dxyz, const float* dL_drot, const float* dL_dscale, float* dL_dverts,
                            float* dL_dnode_trans, float* dL_dnode_rots, float* dL_dnode_scales, void* workspace,
                            size_t workspace_bytes, void* stream);
typedef struct gsr_sugar_timed {
  int T, V, F, G;          /* frames, vertices, faces, Gaussians per face */
  const float* vert_xyz;   /* (T,V,3) */
  const float* vert_rot;   /* (T,V,4) xyzw, non-zero; 16-byte aligned */
  const float* rotation0;  /* (F G,4) wxyz, the static rotation; 16-byte aligned */
  const float* vert_scale; /* (T,V,3), with log_scales: both or neither */
  const float* log_scales; /* (F G,2); 8-byte aligned */
  const int* faces;        /* (F,3) int32 */
  float thickness;         /* the normal-axis scale */
} gsr_sugar_timed;
size_t gsr_sugar_timed_workspace_bytes(int T, int F);
int gsr_sugar_timed_forward(const gsr_sugar_timed* in, int N, const float* bary, float* xyz, float* rotation,
                            float* normals, float* scaling, void* stream);
int gsr_sugar_timed_backward(const gsr_sugar_timed* in, int N, const float* bary, const int* corner_order,
                             const int* vert_offsets, const float* dL_dxyz, const float* dL_drotation,
                             const float* dL_dnormals, const float* dL_dscaling, float* dL_dvert_xyz,
                             float* dL_dvert_rot, float* dL_drotation0, float* dL_dvert_scale, float* dL_dlog_scales,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * gsr_sugar_arap_*: the as-rigid-as-possible energy of the deformed vertices with given per-vertex rotations
 * (ARAPCoach.compute_arap_energy with vert_rotations, utils/arap_utils.py:148-189, which _compute_arap_energy of
 * system/sugar_4dgen.py calls once per frame), for all T frames of a batch.  V vertices, E directed one-ring edges;
 * T V < 2^31.  The inputs are the fields of gsr_sugar_arap below: the one-rings in CSR, vertex i owning the entries
 * offsets[i] .. offsets[i+1]) of nbr and w.
 * With p_ij = verts[i] - verts[j] (formed here, exactly), d_ij = x'_i - x'_j and s_ij = d_ij - R_i p_ij at frame t:
 *   energy[t] = sum_i sum_{j in row i} w_ij |s_ij|^2                                             energy (T,)
 * Backward, given dL_denergy (T,) = g: writes in full
 *   dL_dvert_xyz[t,i] = 2 g_t sum_{j in row i} w_ij (2 d_ij - (R_i + R_j) p_ij)                   (T,V,3)
 *   dL_dvert_rot[t,i] = -2 g_t sum_{j in row i} w_ij s_ij p_ij^T   (T,V,3,3), or its chain to the four quaternion
 *   components (T,V,4), 16-byte aligned.
 * The first is the exact derivative when the rows are symmetric (j in row i iff i in row j, w_ij = w_ji), as one-rings
 * are: then row i holds every term x'_i takes part in, and the backward gathers.  No gradient to verts or w.
 * A vertex with an empty row gets exactly 0, and so does every row of a frame with g_t = 0.
 * Out of range: an nbr entry outside [0, V) contributes nothing and is never used as an index; offsets are clamped
 * to [0, E], a row whose end precedes its start is empty.
 * Sum orders (no atomics; two calls give the same bits): a row of at most 32 entries is added in ascending entry
 * order, from 0; of a longer row, lane l of a 64-lane wave adds the entries l, l + 64, ... in order, from 0, and the 64
 * partial sums are added pairwise by a butterfly (lanes 32 apart first, then 16, ... 1).  The energy: each block of 256
 * consecutive vertices of a frame adds its lanes' sums by that butterfly per wave and the four wave sums in ascending
 * order; one wave per frame adds the ceil(V / 256) block sums the same way (lane l: l, l + 64, ...; butterfly).
 * Precision: fp64 arithmetic from the fp32 inputs; energies and gradients are rounded to fp32 once.  verts = vert_xyz
 * bitwise with identity rotations gives energy and gradients exactly 0.
 * workspace (forward only): gsr_sugar_arap_workspace_bytes(T, V) bytes of device memory (256-B aligned): 8 T
 * ceil(V / 256) bytes of fp64 block sums.  The forward is two launches, the backward one, on `stream`; the library
 * allocates nothing.  T = 0 or V = 0 launches nothing and writes nothing.
 */
#define GSR_ARAP_QUAT 0
#define GSR_ARAP_MATRIX 1
typedef struct gsr_sugar_arap {
  int T, V, E;           /* frames, vertices, directed one-ring edges */
  int rot_form;          /* GSR_ARAP_QUAT or GSR_ARAP_MATRIX */
  const float* verts;    /* (V,3): the rest vertices */
  /* (E,) fp32: the edge weight w_ij (the caller's: the reference's are cotangent weights and may be negative) */
  const float* w;
  const float* vert_xyz; /* (T,V,3): the deformed vertices x' */
  /* GSR_ARAP_MATRIX: (T,V,3,3) row-major matrices R;  GSR_ARAP_QUAT: (T,V,4) xyzw quaternions of any norm, 16-byte
   * aligned, R = I + 2 w [v]x + 2 [v]x^2 (pypose's matrix(): no normalisation) */
  const float* vert_rot;
  const int* offsets;    /* (V+1,) int32 */
  const int* nbr;        /* (E,) int32: the neighbour j */
} gsr_sugar_arap;
size_t gsr_sugar_arap_workspace_bytes(int T, int V);
int gsr_sugar_arap_forward(const gsr_sugar_arap* in, float* energy, void* workspace, size_t workspace_bytes,
                           void* stream);
int gsr_sugar_arap_backward(const gsr_sugar_arap* in, const float* dL_denergy, float* dL_dvert_xyz,
                            float* dL_dvert_rot, void* stream);

/*
 * gsr_sugar_spline_*: the B-spline that turns the control knots of the deformation network into the timed node (or
 * vertex) attributes (Spline.forward, geometry/spline_utils.py:195-332, as get_timed_dg_attributes and
 * get_timed_vertex_attributes call it, dynamic_sugar.py:425-435, 488-494), for all T timestamps of a call.  P points,
 * n_knots knots, degree 1 or 3 (n_knots >= degree + 1); T P and n_knots P < 2^31.  The inputs are the fields of
 * gsr_sugar_spline below; the knots are frame-major, as _get_timed_dg_attributes_wo_spline returns them (the
 * reference's set_data tensors are their permute(1, 0, 2)).
 * The segment of a timestamp, in fp32 as the reference takes it (a discrete decision):
 *   ts = min(max(t, lo), hi);  nt = (ts - start) / interval (correctly rounded);  i = (int) floor(nt);
 *   u = nt - (float) i;  degree 3: i -= 1;  then i is clamped to [0, n_knots - degree - 1], so that no timestamp (NaN
 *   included: its outputs are unspecified) reads outside the knots.
 * With k_j = knots[i + j][p], u taken to fp64, the sums in ascending j:
 *   degree 3, xyz and scale:  sum_j c_j k_j,  c = (1/6 - u/2 + u^2/2 - u^3/6,  4/6 - u^2 + u^3/2,
 *                             1/6 + u/2 + u^2/2 - u^3/2,  u^3/6)
 *   degree 3, rot:  r_j = Log(conj(q_j) (x) q_j+1), j = 0, 1, 2;  b = (5/6 + u/2 - u^2/2 + u^3/6,
 *                   1/6 + u/2 + u^2/2 - u^3/3,  u^3/6);  rot = q_0 (x) Exp(b_0 r_0) (x) Exp(b_1 r_1) (x) Exp(b_2 r_2)
 *                   (no normalisation and no sign fix, as the reference: |rot| = |q_0|)
 *   degree 1, xyz and scale:  (1 - u) k_0 + u k_1;   rot = Exp((1 - u) Log(q_0) + u Log(q_1))
 * Log, Exp and (x) as above.  Outputs xyz (T,P,3), rot (T,P,4) xyzw 16-byte aligned, scale (T,P,3) (required iff
 * knots_scale is given): the node_trans, node_rots, node_scales of gsr_sugar_skin_*, or with P = V the vert_xyz,
 * vert_rot, vert_scale of gsr_sugar_timed_*.
 * Backward: the exact derivative to the knots (none to the timestamps).  dL_dxyz (T,P,3), dL_drot (T,P,4) 16-byte
 * aligned, dL_dscale (T,P,3): any may be NULL (zero).  Writes in full dL_dknots_xyz (n_knots,P,3), dL_dknots_rot
 * (n_knots,P,4) 16-byte aligned and, iff knots_scale is given, dL_dknots_scale (n_knots,P,3); a knot that no
 * timestamp's segment covers gets exactly 0.
 * Sum order (no atomics; two calls give the same bits): per (knot, p) the rows of the covering timestamps in ascending
 * t, from 0.  Precision: fp64 arithmetic from the fp32 inputs and the fp32 u; outputs and gradients are rounded to fp32
 * once (the rows between the backward's two kernels are fp64).
 * workspace (backward only): gsr_sugar_spline_workspace_bytes(T, P, degree) bytes of device memory (256-B aligned):
 * 80 (degree + 1) T P bytes, the fp64 rows (10 per timestamp, point and knot of its segment).  The forward is one
 * launch, the backward two, on `stream`; the library allocates nothing.  T = 0 or P = 0 launches nothing and writes
 * nothing (the caller zeroes the gradients).
 */
typedef struct gsr_sugar_spline {
  int T, P, n_knots, degree; /* timestamps, points, knots, 1 or 3 */
  float start, interval;     /* the grid: knot k at start + k interval (interval > 0) */
  /* the clamp bounds (the reference's t_lower_bound + 1e-6 and t_upper_bound - 1e-6 as it forms them in fp32) */
  float lo, hi;
  const float* timestamps;  /* (T,) */
  const float* knots_xyz;   /* (n_knots,P,3) */
  const float* knots_rot;   /* (n_knots,P,4) xyzw, non-zero, any norm; 16-byte aligned */
  const float* knots_scale; /* (n_knots,P,3) or NULL */
} gsr_sugar_spline;
size_t gsr_sugar_spline_workspace_bytes(int T, int P, int degree);
int gsr_sugar_spline_forward(const gsr_sugar_spline* in, float* xyz, float* rot, float* scale, void* stream);
int gsr_sugar_spline_backward(const gsr_sugar_spline* in, const float* dL_dxyz, const float* dL_drot,
                              const float* dL_dscale, float* dL_dknots_xyz, float* dL_dknots_rot,
                              float* dL_dknots_scale, void* workspace, size_t workspace_bytes, void* stream);

/*
 * gsr_sugar_deform_*: the HexPlane deformation network of dynamic SuGaR evaluated at T ticks x P fixed points
 * (DeformationNetwork.forward_dynamic_delta, geometry/deformation.py, as compute_control_knots calls it through
 * _get_timed_dg_attributes_wo_spline and _get_timed_vertex_attributes_wo_spline, geometry/dynamic_sugar.py:442-480,
 * 577-615, with their rot + (0, 0, 0, 1) and normalise epilogue).  T P < 2^31, 4 P < 2^31.  The inputs are the fields
 * of gsr_sugar_deform below.
 * Coordinates: sample (t, p) sees (n_p, 2 tick_t - 1), n_p = (x_p - aabb[0]) (2 / (aabb[1] - aabb[0])) - 1.  Along axis
 * d of level l with R = reso[l][d] texels the coordinate c = clamp((n + 1) / 2 (R - 1), 0, R - 1) (grid_sample's
 * align_corners = True, padding_mode = "border") lies in cell i = floor(c) at f = c - i.  The caller computes i and f
 * in fp64 once per (points, ticks): cell / frac (L,3,P) for the spatial axes, tcell / tfrac (T,) for time (the time
 * resolution is the same on every level).  A cell is clamped to [0, R - 1] here; the upper texel i + 1 of a cell at
 * the upper edge is outside the plane: it has weight 0 and is never dereferenced.
 * HexPlane: L (1..4) levels, each the 6 planes of itertools.combinations(range(4), 2) in that order; plane (a, b) of
 * level l is (32, reso[l][b], reso[l][a]) fp32, coordinate a along the width: planes[6 l + q].  Its sample is the
 * bilinear mix of its four texels per channel; the level's feature is the product of its six samples, the K = 32 L
 * features are the levels' in order.
 * MLP (mlp[0..13]: feature_out weight (64,K) and bias, then per head pos, rot, scale: the residual layer's weight
 * (64,64) and bias, the final layer's weight (H,64) and bias, H = 3, 4, 3; the scale head's four are NULL iff d_scale
 * is 0):  h = W0 feat + b0;  per head r = relu(h), y = r + W1 r + b1, o = W2 y + b2.
 * Outputs, frame-major: xyz (T,P,3) = o_pos;  rot (T,P,4) = o_rot + (0,0,0,1), divided by its norm iff normalize_rot;
 * scale (T,P,3) = o_scale (required iff d_scale): the knots_xyz, knots_rot, knots_scale of gsr_sugar_spline_*.
 * Backward: the exact derivative to the 6 L planes and the MLP tensors given (none to the points, ticks or aabb).
 * dL_dxyz, dL_drot, dL_dscale: any may be NULL (zero).  Tables (HexPlaneBinding builds them; rows in ascending entry
 * order; an entry whose corner is outside its plane is absent):
 *   sp_offsets / sp_order   per texel of the spatial planes (levels in order, planes (0,1), (0,2), (1,2), texels
 *                           row-major) the entries 4 p + 2 cy + cx whose corner (cx along the width) is that texel;
 *   col_offsets / col_order per level, spatial axis and column the entries 2 p + cx;
 *   t_offsets / t_order     per time row the entries 2 t + ct.
 *   n_sp, n_col, n_t are the lengths of the three order arrays; offsets are clamped to them, an entry out of range or
 *   not of the row's texel contributes nothing and is never used as an index.
 * Writes in full dL_dplanes[6 l + q] (device pointers in a host array, shaped like the planes; a texel that no sample
 * touches gets exactly +0.0: the caller does not zero them) and dL_dmlp[0..13] (as mlp; the scale head's are ignored
 * when d_scale is 0).  relu' at exactly 0 is 0.  The factor of a plane's sample is the upstream gradient of its level's
 * channel times the product of the other five samples (multiplied, never divided out).
 * Sum orders (no atomics; two calls give the same bits): a texel's row is split into its even and its odd entries, each
 * added in ascending order from 0, then the two sums are added; a time-plane texel walks its column row outside and
 * its time row inside.  Weights and biases: block b of B = min(256, ceil(P / 8)) owns the points 8 (b + B i) + w, wave
 * w = 0..7, i = 0, 1, ...; per point the ticks ascend; the matrices of feature_out and of the residual layers are summed
 * per block (round i, tick, wave in that order), the other tensors per wave, then the partial sums are added in block
 * (and wave) order.  Precision: fp64 arithmetic from the fp32 inputs and the fp64 frac; every output and gradient is
 * rounded to fp32 once (what passes between the backward's kernels is fp64).
 * workspace (backward only): gsr_sugar_deform_workspace_bytes(T, P, L) bytes of device memory (256-B aligned):
 * 256 L (T P + 2 P) bytes of fp64 rows and 8 B (20480 + 8192) bytes of partial sums.  The forward is one launch, the
 * backward four, on `stream`; the library allocates nothing.  T = 0 or P = 0 launches nothing and writes nothing.
 */
#define GSR_DEFORM_MAX_L 4
#define GSR_DEFORM_MLP 14
#define GSR_DEFORM_OUT 10
typedef struct gsr_sugar_deform {
  int T, P, L;               /* ticks, points, levels */
  int d_scale;               /* the scale head is evaluated */
  int normalize_rot;         /* rot is divided by its norm (the graph-node variant) */
  int n_sp, n_col, n_t;      /* lengths of sp_order, col_order, t_order (backward only) */
  const int* reso;           /* HOST (L,4): texels of level l along x, y, z, time; each >= 2 */
  const float* const* planes; /* HOST array of 6 L device pointers */
  const float* const* mlp;   /* HOST array of 14 device pointers */
  const int* cell;           /* (L,3,P) int32 */
  const double* frac;        /* (L,3,P) fp64 in [0, 1) */
  const int* tcell;          /* (T,) int32 */
  const double* tfrac;       /* (T,) fp64 */
} gsr_sugar_deform;
size_t gsr_sugar_deform_workspace_bytes(int T, int P, int L);
int gsr_sugar_deform_forward(const gsr_sugar_deform* in, float* xyz, float* rot, float* scale, void* stream);
int gsr_sugar_deform_backward(const gsr_sugar_deform* in, const int* sp_order, const int* sp_offsets,
                              const int* col_order, const int* col_offsets, const int* t_order, const int* t_offsets,
                              const float* dL_dxyz, const float* dL_drot, const float* dL_dscale,
                              float* const* dL_dplanes, float* const* dL_dmlp, void* workspace, size_t workspace_bytes,
                              void* stream);

/*
 * gsr_sugar_normal_consistency_* and gsr_sugar_laplacian_*: the two mesh regularisers the SuGaR systems put on the
 * deformed surface every step, pytorch3d.loss.mesh_normal_consistency(meshes) and mesh_laplacian_smoothing(meshes,
 * "uniform") (system/sugar_static.py:286-297, system/sugar_4dgen.py:234-250; pytorch3d is [EXT]: stated from its
 * published algorithm), for T frames of one fixed topology.  V vertices, E unique undirected edges, P face pairs;
 * T V < 2^31, 4 P < 2^31, T ceil(max(P, V) / 256) < 2^31.  The inputs are the fields of gsr_sugar_meshreg below
 * (sugar_meshreg.MeshTopology builds the tables once per mesh).
 * Normal consistency.  pairs (P,4) = (a, b, c0, c1): an edge (a, b), a < b, and the third vertices of two faces on
 * it (every unordered pair of faces incident to an edge is one row).  With e = x_b - x_a at frame t:
 *   n0 = e x (x_c0 - x_a);  n1 = -(e x (x_c1 - x_a));  cos = (n0 . n1) / (max(|n0|, 1e-8) max(|n1|, 1e-8))
 *   nc[t] = (1 / P) sum_p (1 - cos_p)                                                               nc (T,)
 * (torch's cosine_similarity: each norm clamped on its own.  torch clamps the norm's value in place, outside autograd,
 * so the backward differentiates cos as written with m = max(|n|, 1e-8) held as |n|'s function: d cos / d n0 =
 * n1 / (m0 m1) - cos n0 / (m0 |n0|), the second term 0 at n0 = 0, whether the clamp holds or not.)  A row with an entry outside [0, V) adds nothing (P still divides) and nothing of it is
 * dereferenced.
 * Backward, given dL_dnc (T,) = g: kernel 1 writes per (t, pair) the four fp64 gradient rows of its corners a, b, c0,
 * c1, scaled by g_t / P, into the workspace; kernel 2 adds, per (t, vertex i), the rows slots[slot_offsets[i] ..
 * slot_offsets[i+1]) name (entry 4 pair + role, role 0..3 = a, b, c0, c1) and rounds once: dL_dvert_xyz (T,V,3),
 * written in full.  A slot entry outside [0, 4 P) is skipped.
 * Uniform Laplacian.  The one-rings in CSR: vertex i owns ring[ring_offsets[i] .. ring_offsets[i+1]), its distinct
 * neighbours j (2 E entries in all); deg_i is the row's length.
 *   d_i = (1 / deg_i) sum_{j in row i} x_j - x_i   (deg_i = 0: d_i = -x_i, pytorch3d subtracts the identity for every
 *   vertex);   lap[t] = (1 / V) sum_i |d_i|                                                         lap (T,)
 * Backward, given dL_dlap (T,) = g: kernel 1 writes u_i = g_t d_i / (V |d_i|) (0 at |d_i| = 0, torch's norm) as fp64
 * rows; kernel 2 writes dL_dvert_xyz[t,i] = -u_i + sum_{j in row i} u_j / deg_j, the exact derivative when the rows
 * are symmetric (j in row i iff i in row j), as one-rings are.  A ring entry outside [0, V) is skipped.
 * Both: offsets are clamped to the table's length, a row whose end precedes its start is empty.  A vertex nothing
 * reaches gets exactly +0.0, and so does every vertex of a frame with g_t = 0 (its work is skipped).
 * Sum orders (no atomics; two calls give the same bits): a row of at most 32 entries is added in ascending entry
 * order, from 0; of a longer row, lane l of a 64-lane wave adds the entries l, l + 64, ... in order, from 0, and the 64
 * partial sums are added pairwise by a butterfly (lanes 32 apart first, then 16, ... 1).  The forwards: each block of
 * 256 consecutive pairs (vertices) of a frame adds its lanes' terms by that butterfly per wave and the four wave sums
 * in ascending order; one wave per frame adds the block sums the same way (lane l: l, l + 64, ...; butterfly) and
 * divides by P (V).
 * Precision: fp64 arithmetic from the fp32 inputs; nc, lap and the gradients are rounded to fp32 once.
 * workspace: gsr_sugar_meshreg_workspace_bytes(T, V, P, pass) bytes of device memory (256-B aligned; 0 for an unknown
 * pass): GSR_MESHREG_FORWARD (either forward): 8 T ceil(max(P, V, 1) / 256) bytes of fp64 block sums;
 * GSR_MESHREG_NC_BACKWARD: 96 T P bytes, GSR_MESHREG_LAP_BACKWARD: 24 T V bytes of fp64 rows.  Every call is two launches on `stream`; the library allocates nothing.  T = 0 launches
 * nothing; so does P = 0 for the normal consistency and V = 0 for the Laplacian (the caller's nc / lap / gradients
 * are then zero: nothing is written).
 */
#define GSR_MESHREG_FORWARD 0
#define GSR_MESHREG_NC_BACKWARD 1
#define GSR_MESHREG_LAP_BACKWARD 2
typedef struct gsr_sugar_meshreg {
  int T, V, E, P;          /* frames, vertices, unique undirected edges, face pairs */
  const float* vert_xyz;   /* (T,V,3): the deformed vertices */
  const int* pairs;        /* (P,4) int32 (a, b, c0, c1); 16-byte aligned */
  const int* slot_offsets; /* (V+1,) int32 */
  const int* slots;        /* (4P,) int32: 4 pair + role, ascending within a row */
  const int* ring_offsets; /* (V+1,) int32 */
  const int* ring;         /* (2E,) int32: the neighbour j, ascending within a row */
} gsr_sugar_meshreg;
size_t gsr_sugar_meshreg_workspace_bytes(int T, int V, int P, int pass);
int gsr_sugar_normal_consistency_forward(const gsr_sugar_meshreg* in, float* nc, void* workspace,
                                         size_t workspace_bytes, void* stream);
int gsr_sugar_normal_consistency_backward(const gsr_sugar_meshreg* in, const float* dL_dnc, float* dL_dvert_xyz,
                                          void* workspace, size_t workspace_bytes, void* stream);
int gsr_sugar_laplacian_forward(const gsr_sugar_meshreg* in, float* lap, void* workspace, size_t workspace_bytes,
                                void* stream);
int gsr_sugar_laplacian_backward(const gsr_sugar_meshreg* in, const float* dL_dlap, float* dL_dvert_xyz,
                                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * The view-segmented stable LSD radix sort that every sort of this library runs (the depth sort, the tile sort and
 * distCUDA2's Morton sort: csrc/gsr_sort.hip; it replaces the reference extension's cub::DeviceRadixSort::SortPairs
 * calls of one view at a time).  Exposed for tests: V (1..64) segments of n[v] (key, value) pairs laid
 * out back to back in keys / vals (device), each sorted in place by the key's low key_bits (1..32) bits, stably
 * (equal keys keep their order), in passes of at most max_bits (1..8) bits.  vals may be NULL (keys only).
 * work: gsr_sort_work_bytes(V, n) bytes of device memory.
 */
size_t gsr_sort_work_bytes(int V, const int* n);
int gsr_sort_pairs(int V, const int* n, uint32_t* keys, uint32_t* vals, int key_bits, int max_bits, void* work,
                   size_t work_bytes, void* stream);
/* How the sort's scatter ranks equal digits within a wave, decided once per process: 1 = LDS atomic adds (the device
 * was found, by a probe kernel at the first call, to service one instruction's lanes that hit the same counter in lane
 * order, which keeps the sort stable), 0 = ballot matching (the probe failed, or GSR_SORT_RANK=ballot).  Both give
 * the same bits.  Runs the probe if it has not run yet (a device synchronisation). */
int gsr_sort_rank_mode(void);

/* Replaces markVisible/checkFrustum (API completeness; unused by the reference).  present (P,) u8. */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GSR_H */
