// gsr_api.hip — extern "C" entry points declared in include/gsr.h.
//
// Phase structure mirrors what the reference's _C.rasterize_gaussians does internally
// (CudaRasterizer::Rasterizer::forward / backward [EXT]); argument checking mirrors its
// TORCH_CHECKs and Python-side exceptions (SURVEY.md §8b "Errors").
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gsr.h"
#include "gsr_kernels.h"

using namespace gsr;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, const char* what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}

#define GSR_HIP_CHECK(expr)                                                        \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(GSR_EHIP, "HIP error: %s", hipGetErrorString(e_)); \
  } while (0)

static int last_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GSR_EHIP, "HIP launch error: %s", hipGetErrorString(e));
  g_err[0] = 0;
  return GSR_OK;
}

// an empty problem: nothing to launch, no device touched
static int nothing_to_do() {
  g_err[0] = 0;
  return GSR_OK;
}

static int null_argument() { return fail(GSR_EINVAL, "%s", "null pointer argument"); }

// ---- phase profiler: event pairs on the launch stream, resolved lazily in gsr_profile_read ----
namespace {
struct PhaseEvents {
  int phase;
  hipEvent_t a, b;
};
struct Profiler {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> pool;
  std::vector<PhaseEvents> pending;
  double ms[GSR_NUM_PHASES] = {0};
  long long n[GSR_NUM_PHASES] = {0};
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
};
Profiler& prof() {
  static Profiler p;
  return p;
}
// RAII scope: records a start event at construction and an end event at destruction.
struct PhaseScope {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  int phase;
  PhaseScope(int ph, hipStream_t st) : s(st), phase(ph) {
    Profiler& p = prof();
    if (!p.on) return;
    std::lock_guard<std::mutex> g(p.mu);
    a = p.get();
    b = p.get();
    if (a) (void)hipEventRecord(a, s);
  }
  ~PhaseScope() {
    if (a == nullptr || b == nullptr) return;
    (void)hipEventRecord(b, s);
    Profiler& p = prof();
    std::lock_guard<std::mutex> g(p.mu);
    p.pending.push_back({phase, a, b});
  }
};
}  // namespace

// The instance key layout's test override (GSR_TILE_KEYS = unpacked | plain), read ONCE per process: the forward
// and the backward of a set derive the binning buffer's layout (packed keys, quadrant masks, which ping-pong array
// holds the sorted list) from it on the host, so it must not change between them.
static int tile_keys_mode() {
  static const int mode = [] {
    const char* e = getenv("GSR_TILE_KEYS");
    if (e != nullptr && strcmp(e, "unpacked") == 0) return 1;
    if (e != nullptr && strcmp(e, "plain") == 0) return 2;
    return 0;
  }();
  return mode;
}
static TilePack set_tile_pack(int P, int W, int H) { return tile_pack(P, W, H, tile_keys_mode()); }

static int effective_degree(int degree, int M) {
  // the reference reads sqrt(M)-1 coefficients at most (pred-normal pass quirk)
  int dm = (int)std::lround(std::sqrt((double)(M > 0 ? M : 1))) - 1;
  int d = degree < dm ? degree : dm;
  if (d < 0) d = 0;
  if (d > 3) d = 3;
  return d;
}

// ping-pong buffers holding the sorts' results (one pass per <= 8 key bits)
static int tile_sort_result(int W, int H) { return digit_plan(tile_key_bits(W, H)).passes & 1; }
static int depth_sort_result() { return digit_plan(32).passes & 1; }

static GaussBackwardArgs shared_args(const gsr_set_scene& sc, const gsr_set_grads& gr) {
  GaussBackwardArgs a;
  a.P = sc.P;
  a.g0 = 0;
  a.g1 = sc.P;
  a.M = sc.shs ? sc.M : 0;
  a.deg = effective_degree(sc.degree, a.M);
  a.means3D = sc.means3D;
  a.scales = sc.scales;
  a.rotations = sc.rotations;
  a.shs = sc.shs;
  a.cov3D_precomp = sc.cov3D_precomp;
  a.scale_modifier = sc.scale_modifier;
  a.dL_dcolors = gr.dL_dcolors;
  a.dL_dopacity = gr.dL_dopacity;
  a.dL_dmeans3D = gr.dL_dmeans3D;
  a.dL_dcov3D = gr.dL_dcov3D;
  a.dL_dsh = sc.shs ? gr.dL_dsh : nullptr;
  a.dL_dscales = sc.cov3D_precomp ? nullptr : gr.dL_dscales;
  a.dL_drotations = sc.cov3D_precomp ? nullptr : gr.dL_drotations;
  return a;
}

// Instance segments of a set from the host copy of K (checked: the set's total < 2^32).
static int inst_segments(int V, const int* K, SegInfo& seg, long long* total) {
  seg.V = V;
  long long run = 0;
  for (int v = 0; v < V; ++v) {
    if (K[v] < 0) return fail(GSR_EINVAL, "%s", "negative instance count");
    seg.n[v] = (uint32_t)K[v];
    seg.start[v] = (uint32_t)run;
    run += K[v];
    if (run >= (1ll << 32)) return fail(GSR_EINVAL, "%s", "instances of a view set exceed 2^32: use smaller sets");
  }
  seg_fill_blocks(seg, GSR_SORT_TILE);
  if (total) *total = run;
  return GSR_OK;
}

static int set_cams(const gsr_set_scene& sc, SetCams& cams) {
  if (sc.viewmatrices == nullptr || sc.projmatrices == nullptr || sc.campos == nullptr || sc.tanfovx == nullptr ||
      sc.tanfovy == nullptr)
    return fail(GSR_EINVAL, "%s", "null camera array");
  for (int v = 0; v < sc.V; ++v) {
    if (sc.viewmatrices[v] == nullptr || sc.projmatrices[v] == nullptr || sc.campos[v] == nullptr)
      return fail(GSR_EINVAL, "%s", "null camera pointer");
    cams.c[v].view = sc.viewmatrices[v];
    cams.c[v].proj = sc.projmatrices[v];
    cams.c[v].campos = sc.campos[v];
    cams.c[v].tanx = sc.tanfovx[v];
    cams.c[v].tany = sc.tanfovy[v];
  }
  return GSR_OK;
}

static int check_set(int V, int P) {
  if (V < 1 || V > GSR_SET_MAX) return fail(GSR_EINVAL, "%s", "a view set holds 1..64 views");
  if (P < 0) return fail(GSR_EINVAL, "%s", "P must be >= 0");
  if ((long long)V * (long long)(P > 0 ? P : 1) >= (1ll << 32))
    return fail(GSR_EINVAL, "%s", "views x Gaussians of a set exceed 2^32: use smaller sets");
  return GSR_OK;
}

// What the forward and the backward blend of a set derive alike from its carved state.  The callers set the rest: the
// composite and second-colour pointers, ckpt, ochunk, qbytes, V / v0 and the per-view tables.
static void render_set_shared(RenderSet& rs, const GeomState& g, const ImageState& img, const BinningState& b,
                              const TilePack& tp, int tres, int V, int P, int width, int height) {
  rs.P = P;
  rs.W = width;
  rs.H = height;
  rs.gx = div_up(width, GSR_TILE_X);
  rs.gy = div_up(height, GSR_TILE_Y);
  rs.gmask = tp.gmask;
  rs.col2_rec = g.drange + 130;
  rs.order = img.order;
  rs.split_mode = img.split_mode;
  rs.split_items = img.split_items;
  rs.split_cap = img.split_cap;
  rs.split_extra = split_extra(V, (size_t)rs.gx * rs.gy);
  rs.qkeys = tp.qmask ? b.key[tres] : nullptr;
}

extern "C" {

#ifndef GSR_BUILD_ID
#define GSR_BUILD_ID "unknown"
#endif
// "gsr <version> gfx950 build <id>": the id hashes the sources the library was built from (csrc/Makefile)
const char* gsr_version(void) { return "gsr 0.4.0 gfx950 build " GSR_BUILD_ID; }
int gsr_abi_version(void) { return GSR_ABI_VERSION; }
const char* gsr_last_error(void) { return g_err; }

// ---- view sets ---------------------------------------------------------------------------

size_t gsr_set_geom_bytes(int V, int P) {
  size_t b = 0;
  GeomState::carve(nullptr, V, P, &b);
  return b;
}
// instance total of a set for the sizers: false for a bad V or a NULL / negative / overflowing count
static bool set_total(int V, const int* K, SegInfo& seg, long long* total) {
  return V >= 1 && V <= GSR_SET_MAX && K != nullptr && inst_segments(V, K, seg, total) == GSR_OK;
}
size_t gsr_set_binning_bytes(int V, int P, const int* K, int width, int height) {
  SegInfo seg;
  long long total = 0;
  if (!set_total(V, K, seg, &total)) return 0;
  size_t b = 0;
  BinningState::carve(nullptr, V, total, seg.blk[V], !set_tile_pack(P, width, height).packed, &b);
  return b;
}
size_t gsr_set_image_bytes(int V, int P, const int* K, int width, int height, int two_colors) {
  SegInfo seg;
  long long total = 0;
  if (K != nullptr && !set_total(V, K, seg, &total)) return 0;
  size_t b = 0;
  // (no counts: the upper bound, with the split backward's checkpoints)
  ImageState::carve(nullptr, V, width, height, &b,
                    K == nullptr || split_forward(V, P, width, height, total, two_colors != 0));
  return b;
}
// the running dL/dcov3D (P x 6) kept at the end of the work buffer across view groups
static size_t carry_bytes(int P) { return align_up(sizeof(float) * 6 * (size_t)(P > 0 ? P : 1), 256); }

size_t gsr_set_backward_bytes(int V, int P, const int* K, int two_colors) {
  SegInfo seg;
  long long total = 0;
  if (!set_total(V, K, seg, &total)) return 0;
  return BackwardState::bytes_for(total, V, P, two_colors != 0) + carry_bytes(P);
}

// What a timed set does not build, checked before anything else (include/gsr.h gsr_set_timed).
static int check_timed(const gsr_set_scene& sc, const gsr_set_timed& tm) {
  if (sc.shs != nullptr) return fail(GSR_EINVAL, "%s", "timed view sets take precomputed colours: shs is not built");
  if (sc.cov3D_precomp != nullptr) return fail(GSR_EINVAL, "%s", "timed view sets: cov3D_precomp is not built");
  if (tm.means3D_v == nullptr && sc.P > 0) return fail(GSR_EINVAL, "%s", "timed view sets need means3D_v");
  return GSR_OK;
}
// the scene with the timed set's per-view arrays in place of the shared ones (row 0 where a shared array is read)
static gsr_set_scene timed_scene(const gsr_set_scene& sc, const gsr_set_timed& tm) {
  gsr_set_scene e = sc;
  e.means3D = tm.means3D_v;
  if (tm.scales_v != nullptr) e.scales = tm.scales_v;
  if (tm.rotations_v != nullptr) e.rotations = tm.rotations_v;
  return e;
}

// gsr_set_preprocess; timed != nullptr: gsr_set_timed_preprocess (checked), `scene` already holds the per-view arrays
static int set_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const float* colors2,
                          const gsr_set_timed* timed, void* stream) {
  const gsr_set_scene& sc = *scene;
  const int V = sc.V, P = sc.P;
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if (sc.width <= 0 || sc.height <= 0) return fail(GSR_EINVAL, "%s", "image size must be positive");
  if ((sc.shs == nullptr) == (sc.colors_precomp == nullptr))
    return fail(GSR_EINVAL, "%s", "Please provide exactly one of either SHs or precomputed colors!");
  if (((sc.scales == nullptr || sc.rotations == nullptr) && sc.cov3D_precomp == nullptr) ||
      ((sc.scales != nullptr || sc.rotations != nullptr) && sc.cov3D_precomp != nullptr))
    return fail(GSR_EINVAL, "%s",
                "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (state->geom == nullptr ||
      (P > 0 && (sc.means3D == nullptr || sc.opacities == nullptr || state->radii == nullptr)))
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (sc.shs != nullptr && sc.M <= 0) return fail(GSR_EINVAL, "%s", "M must be >= 1 with SHs");
  SetCams cams;
  if (set_cams(sc, cams) != GSR_OK) return GSR_EINVAL;
  for (int v = 0; v < V; ++v) {  // IEEE float division on the host = the device's correctly rounded one
    cams.c[v].fx = (float)sc.width / (2.0f * cams.c[v].tanx);
    cams.c[v].fy = (float)sc.height / (2.0f * cams.c[v].tany);
  }
  hipStream_t s = (hipStream_t)stream;
  GeomState g = GeomState::carve(state->geom, V, P, nullptr);

  PreprocessArgs a;
  a.V = V;
  a.P = P;
  a.deg = effective_degree(sc.degree, sc.M);
  a.M = sc.M;
  a.means3D = sc.means3D;
  a.scales = sc.scales;
  a.rotations = sc.rotations;
  a.opacities = sc.opacities;
  a.shs = sc.shs;
  a.colors_precomp = sc.colors_precomp;
  a.cov3D_precomp = sc.cov3D_precomp;
  a.scale_modifier = sc.scale_modifier;
  a.W = sc.width;
  a.H = sc.height;
  a.radii = state->radii;
  a.col2 = colors2;
  {
    PhaseScope ps(GSR_PHASE_PREPROCESS, s);
    if (timed != nullptr) {
      const size_t n = (size_t)P;
      const PreprocessTimed pt = {3 * n, timed->scales_v ? 3 * n : 0, timed->rotations_v ? 4 * n : 0, 3 * n};
      launch_preprocess(a, cams, g, s, &pt);
    } else {
      launch_preprocess(a, cams, g, s);
    }
  }
  {
    // depth sort of every view's Gaussians (culled last) -> instance counts in depth order, K_v
    PhaseScope ps(GSR_PHASE_DEPTH_SORT, s);
    SegInfo seg;
    seg.V = V;
    for (int v = 0; v < V; ++v) {
      seg.n[v] = (uint32_t)P;
      seg.start[v] = (uint32_t)((size_t)v * P);
    }
    seg.rebase = g.drange + 128;  // keys ranked relative to the set's smallest visible key (preprocess)
    const int res = seg_sort(g.dkey, g.dval, false, seg, 0, 32, g.sort_counts, g.sort_totals, s);
    if (res != depth_sort_result()) return fail(GSR_EHIP, "%s", "internal: depth sort result buffer");
    launch_binning_counts(V, P, g, s);  // reads the sorted buffer the device flag names (3 or 4 passes)
  }
  return last_launch();
}

int gsr_set_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const float* colors2, void* stream) {
  if (scene == nullptr || state == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  return set_preprocess(scene, state, colors2, nullptr, stream);
}

int gsr_set_timed_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_timed* timed,
                             void* stream) {
  if (scene == nullptr || state == nullptr || timed == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (check_timed(*scene, *timed) != GSR_OK) return GSR_EINVAL;
  const gsr_set_scene e = timed_scene(*scene, *timed);
  return set_preprocess(&e, state, timed->colors2_v, timed, stream);
}

int gsr_composite_forward(int V, int height, int width, const float* color, const float* alpha, const float* bg,
                          int bg_layout, float* out, void* stream) {
  if (V < 0 || height < 0 || width < 0 || bg_layout < 0 || bg_layout > 2) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (color == nullptr || alpha == nullptr || bg == nullptr || out == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  launch_composite_fwd(V, (size_t)height * width, color, alpha, bg, bg_layout, out, (hipStream_t)stream);
  return last_launch();
}

int gsr_composite_backward(int V, int height, int width, const float* dL_dout, const float* color,
                           const float* alpha, const float* bg, int bg_layout, float* dL_dcolor, float* dL_dalpha,
                           float* dL_dbg, void* stream) {
  if (V < 0 || height < 0 || width < 0 || bg_layout < 0 || bg_layout > 2) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (dL_dout == nullptr || color == nullptr || alpha == nullptr || bg == nullptr || dL_dcolor == nullptr ||
      dL_dalpha == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (dL_dbg != nullptr && bg_layout == GSR_BG_CONSTANT)
    return fail(GSR_EINVAL, "%s", "dL_dbg is computed for image backgrounds only");
  launch_composite_bwd(V, (size_t)height * width, dL_dout, color, alpha, bg, bg_layout, dL_dcolor, dL_dalpha,
                       dL_dbg, (hipStream_t)stream);
  return last_launch();
}

int gsr_normal_map_forward(int V, int height, int width, const float* normal, const float* alpha, float* out,
                           void* stream) {
  if (V < 0 || height < 0 || width < 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (normal == nullptr || alpha == nullptr || out == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  launch_normal_map_fwd(V, (size_t)height * width, normal, alpha, out, (hipStream_t)stream);
  return last_launch();
}

int gsr_normal_map_backward(int V, int height, int width, const float* dL_dout, const float* normal,
                            const float* alpha, float* dL_dnormal, float* dL_dalpha, void* stream) {
  if (V < 0 || height < 0 || width < 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (dL_dout == nullptr || normal == nullptr || alpha == nullptr || dL_dnormal == nullptr || dL_dalpha == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  launch_normal_map_bwd(V, (size_t)height * width, dL_dout, normal, alpha, dL_dnormal, dL_dalpha, (hipStream_t)stream);
  return last_launch();
}

static int shade_args(int V, int H, int W, int flags, const int* modes, const float* color, const float* depth,
                      const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                      const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                      ShadeArgs& A) {
  if (V < 0 || H < 0 || W < 0 || (flags & ~GSR_SHADE_MATERIAL) != 0)
    return fail(GSR_EINVAL, "%s", "bad sizes / flags");
  if (depth == nullptr || alpha == nullptr || rays_o == nullptr || rays_d == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument (depth / alpha / rays)");
  A = ShadeArgs{};
  A.V = V, A.H = H, A.W = W, A.flags = flags, A.bg_layout = bg_layout;
  A.color = color, A.depth = depth, A.alpha = alpha, A.rays_o = rays_o, A.rays_d = rays_d;
  A.bg = bg, A.light = light, A.pred_normal = pred_normal;
  if (flags & GSR_SHADE_MATERIAL) {
    if (color == nullptr || bg == nullptr || light == nullptr || ambient == nullptr || diffuse == nullptr ||
        modes == nullptr)
      return fail(GSR_EINVAL, "%s", "material: color, bg, light, ambient, diffuse and modes are required");
    if (bg_layout != GSR_BG_CONSTANT && bg_layout != GSR_BG_HWC)
      return fail(GSR_EINVAL, "%s", "material: bg_layout must be GSR_BG_CONSTANT or GSR_BG_HWC");
    for (int v = 0; v < V; ++v)
      if (modes[v] < GSR_SHADING_DIFFUSE || modes[v] > GSR_SHADING_TEXTURELESS)
        return fail(GSR_EINVAL, "%s", "bad shading mode");
  }
  return GSR_OK;
}

// Launches in chunks of GSR_SET_MAX views, each with its views' light colours and modes in the arguments.
static void shade_launch(ShadeArgs A, const ShadeGrads* G, const int* modes, const float* ambient,
                         const float* diffuse, hipStream_t s) {
  const int V = A.V;
  for (int v0 = 0; v0 < V; v0 += GSR_SET_MAX) {
    const int n = V - v0 < GSR_SET_MAX ? V - v0 : GSR_SET_MAX;
    A.v0 = v0, A.V = n;
    for (int i = 0; i < n; ++i) {
      A.mode[i] = (A.flags & GSR_SHADE_MATERIAL) ? modes[v0 + i] : 0;
      for (int k = 0; k < 3; ++k) {
        A.ka[i][k] = (A.flags & GSR_SHADE_MATERIAL) ? ambient[3 * (v0 + i) + k] : 0.0f;
        A.kd[i][k] = (A.flags & GSR_SHADE_MATERIAL) ? diffuse[3 * (v0 + i) + k] : 0.0f;
      }
    }
    if (G == nullptr)
      launch_shade_fwd(A, s);
    else
      launch_shade_bwd(A, *G, s);
  }
}

int gsr_shade_views_forward(int V, int height, int width, int flags, const int* modes, const float* color,
                            const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                            const float* bg, int bg_layout, const float* light, const float* pred_normal,
                            const float* ambient, const float* diffuse, float* render, float* normal_map,
                            float* unit_normal, float* depth_out, void* stream) {
  ShadeArgs A;
  if (shade_args(V, height, width, flags, modes, color, depth, alpha, rays_o, rays_d, bg, bg_layout, light,
                 pred_normal, ambient, diffuse, A) != GSR_OK)
    return GSR_EINVAL;
  if ((flags & GSR_SHADE_MATERIAL) && render == nullptr)
    return fail(GSR_EINVAL, "%s", "material: render output is required");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  A.render = render, A.nmap = normal_map, A.unit = unit_normal, A.depth_out = depth_out;
  shade_launch(A, nullptr, modes, ambient, diffuse, (hipStream_t)stream);
  return last_launch();
}

int gsr_shade_views_backward(int V, int height, int width, int flags, const int* modes, const float* color,
                             const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                             const float* bg, int bg_layout, const float* light, const float* pred_normal,
                             const float* ambient, const float* diffuse, const float* dL_drender,
                             const float* dL_dnormal_map, const float* dL_dunit_normal, const float* dL_ddepth_out,
                             float* dL_dcolor, float* dL_ddepth, float* dL_dalpha, float* dL_dbg, void* stream) {
  ShadeArgs A;
  if (shade_args(V, height, width, flags, modes, color, depth, alpha, rays_o, rays_d, bg, bg_layout, light,
                 pred_normal, ambient, diffuse, A) != GSR_OK)
    return GSR_EINVAL;
  if (dL_ddepth == nullptr || dL_dalpha == nullptr) return fail(GSR_EINVAL, "%s", "dL_ddepth / dL_dalpha required");
  if ((flags & GSR_SHADE_MATERIAL) && dL_dcolor == nullptr)
    return fail(GSR_EINVAL, "%s", "material: dL_dcolor is required");
  if (dL_dbg != nullptr && !((flags & GSR_SHADE_MATERIAL) && bg_layout == GSR_BG_HWC))
    return fail(GSR_EINVAL, "%s", "dL_dbg is formed for GSR_BG_HWC material shading only");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  ShadeGrads G{dL_drender, dL_dnormal_map, dL_dunit_normal, dL_ddepth_out, dL_dcolor, dL_ddepth, dL_dalpha, dL_dbg};
  shade_launch(A, &G, modes, ambient, diffuse, (hipStream_t)stream);
  return last_launch();
}

// one (ambient, diffuse, mode) for every view: the per-view tables filled with copies
struct SharedLight {
  std::vector<int> modes;
  std::vector<float> ka, kd;
  SharedLight(int V, int mode, const float* ambient, const float* diffuse)
      : modes(V > 0 ? V : 0, mode), ka(3 * (size_t)(V > 0 ? V : 0)), kd(3 * (size_t)(V > 0 ? V : 0)) {
    for (int v = 0; v < V; ++v)
      for (int k = 0; k < 3; ++k) {
        ka[3 * v + k] = ambient ? ambient[k] : 0.0f;
        kd[3 * v + k] = diffuse ? diffuse[k] : 0.0f;
      }
  }
};

int gsr_shade_forward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                      const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                      const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                      float* render, float* normal_map, float* unit_normal, float* depth_out, void* stream) {
  if (V < 0 || V > 65535 || mode < 0 || mode > 2) return fail(GSR_EINVAL, "%s", "bad sizes / mode / flags");
  if ((flags & GSR_SHADE_MATERIAL) && (ambient == nullptr || diffuse == nullptr))
    return fail(GSR_EINVAL, "%s", "material: color, bg, light, ambient, diffuse and modes are required");
  SharedLight L(V, mode, ambient, diffuse);
  return gsr_shade_views_forward(V, height, width, flags, L.modes.data(), color, depth, alpha, rays_o, rays_d, bg,
                                 bg_layout, light, pred_normal, L.ka.data(), L.kd.data(), render, normal_map,
                                 unit_normal, depth_out, stream);
}

int gsr_shade_backward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                       const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                       const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                       const float* dL_drender, const float* dL_dnormal_map, const float* dL_dunit_normal,
                       const float* dL_ddepth_out, float* dL_dcolor, float* dL_ddepth, float* dL_dalpha,
                       float* dL_dbg, void* stream) {
  if (V < 0 || V > 65535 || mode < 0 || mode > 2) return fail(GSR_EINVAL, "%s", "bad sizes / mode / flags");
  if ((flags & GSR_SHADE_MATERIAL) && (ambient == nullptr || diffuse == nullptr))
    return fail(GSR_EINVAL, "%s", "material: color, bg, light, ambient, diffuse and modes are required");
  SharedLight L(V, mode, ambient, diffuse);
  return gsr_shade_views_backward(V, height, width, flags, L.modes.data(), color, depth, alpha, rays_o, rays_d, bg,
                                  bg_layout, light, pred_normal, L.ka.data(), L.kd.data(), dL_drender,
                                  dL_dnormal_map, dL_dunit_normal, dL_ddepth_out, dL_dcolor, dL_ddepth, dL_dalpha,
                                  dL_dbg, stream);
}

size_t gsr_knn_workspace_bytes(int P) { return knn_workspace_bytes(P < 0 ? 0 : P); }

int gsr_knn_mean_dist(int P, const float* points, float* mean_dist, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (P < 0) return fail(GSR_EINVAL, "%s", "negative point count");
  if (P == 0) return last_launch();
  if (points == nullptr || mean_dist == nullptr || workspace == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (workspace_bytes < knn_workspace_bytes(P)) return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_knn_mean_dist(P, points, mean_dist, workspace, (hipStream_t)stream);
  return last_launch();
}

size_t gsr_knn_points_workspace_bytes(int P, int K) {
  (void)K;  // the lists live in registers: the tree is all the workspace holds
  return knn_workspace_bytes(P < 0 ? 0 : P);
}

int gsr_knn_points(int P, int K, const float* points, float* dists, long long* idx, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (K < 1 || K > GSR_KNN_MAX_K) return fail(GSR_EINVAL, "%s", "K must be in 1..32");
  if (P < 0) return fail(GSR_EINVAL, "%s", "negative point count");
  if (P == 0) {  // nothing to launch, no device touched
    g_err[0] = 0;
    return GSR_OK;
  }
  if (points == nullptr || dists == nullptr || idx == nullptr || workspace == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (workspace_bytes < knn_workspace_bytes(P)) return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_knn_points(P, K, points, dists, idx, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the SuGaR neighbour density field (gsr_field.hip) ---------------------------------------------
static int field_check(const gsr_sugar_field& c) {
  if (c.K < 1 || c.K > GSR_KNN_MAX_K) return fail(GSR_EINVAL, "%s", "K must be in 1..32");
  if (c.M < 0 || c.N < 0 || c.R < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if ((long long)c.M * c.K >= (1ll << 31))
    return fail(GSR_EINVAL, "%s", "M x K must stay below 2^31: split the samples");
  if (c.row == nullptr && c.R != c.M) return fail(GSR_EINVAL, "%s", "without row the neighbour table has M rows");
  if (c.M > 0 && (c.x == nullptr || (c.R > 0 && c.nbr == nullptr))) return null_argument();
  if (c.N > 0 && (c.centers == nullptr || c.inv_sr == nullptr || c.strengths == nullptr || c.min_scale == nullptr))
    return null_argument();
  return GSR_OK;
}

size_t gsr_sugar_field_workspace_bytes(int M, int K, int N) {
  if (K < 1 || K > GSR_KNN_MAX_K) return 0;
  return field_workspace_bytes(M < 0 ? 0 : M, K, N < 0 ? 0 : N);
}

int gsr_sugar_field_forward(const gsr_sugar_field* in, float* density, float* beta_avg, float* op, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (field_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (density == nullptr || beta_avg == nullptr || workspace == nullptr) return null_argument();
  if (workspace_bytes < field_workspace_bytes(0, in->K, in->N)) return fail(GSR_EINVAL, "%s", "workspace too small");
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
  if (workspace_bytes < field_workspace_bytes(in->M, in->K, in->N))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  const int e = launch_field_backward(*in, dL_ddensity, dL_dbeta_avg, dL_dop, dL_dx, dL_dcenters, dL_dinv_sr,
                                      dL_dstrengths, dL_dmin_scale, workspace, (hipStream_t)stream);
  if (e != 0) return fail(GSR_EHIP, "HIP error: %s", hipGetErrorString((hipError_t)e));
  return last_launch();
}

// ---- the SuGaR neighbour-normal loss (gsr_normal.hip) ----------------------------------------------
static int normal_check(const gsr_sugar_normal& c) {
  if (c.K < 1 || c.K > GSR_KNN_MAX_K) return fail(GSR_EINVAL, "%s", "K must be in 1..32");
  if (c.M < 0 || c.N < 0 || c.R < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if ((long long)c.M * (c.K + 1) >= (1ll << 31))
    return fail(GSR_EINVAL, "%s", "M x (K + 1) must stay below 2^31: split the samples");
  if (c.per_sample && c.R != c.M) return fail(GSR_EINVAL, "%s", "a per-sample neighbour table has M rows");
  if (c.M > 0 && (c.x == nullptr || c.own == nullptr || c.op == nullptr || (c.R > 0 && c.nbr == nullptr)))
    return null_argument();
  if (c.N > 0 && (c.centers == nullptr || c.normals == nullptr || c.min_scale == nullptr)) return null_argument();
  return GSR_OK;
}

size_t gsr_sugar_normal_workspace_bytes(int M, int K, int N) {
  if (K < 1 || K > GSR_KNN_MAX_K) return 0;
  return normal_workspace_bytes(M < 0 ? 0 : M, K, N < 0 ? 0 : N);
}

int gsr_sugar_normal_forward(const gsr_sugar_normal* in, float* loss, float* rec, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (normal_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->M == 0) return nothing_to_do();
  if (loss == nullptr || workspace == nullptr) return null_argument();
  if (((uintptr_t)rec & 15u) != 0) return fail(GSR_EINVAL, "%s", "rec must be 16-byte aligned");
  if (workspace_bytes < normal_workspace_bytes(0, in->K, in->N)) return fail(GSR_EINVAL, "%s", "workspace too small");
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
  if (((uintptr_t)rec & 15u) != 0) return fail(GSR_EINVAL, "%s", "rec must be 16-byte aligned");
  if (workspace_bytes < normal_workspace_bytes(in->M, in->K, in->N))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  const int e = launch_normal_backward(*in, rec, dL_dloss, dL_dnormals, workspace, (hipStream_t)stream);
  if (e != 0) return fail(GSR_EHIP, "HIP error: %s", hipGetErrorString((hipError_t)e));
  return last_launch();
}

// ---- the geometry of mesh-bound SuGaR Gaussians (gsr_mesh.hip) -------------------------------------
static int mesh_check(const gsr_sugar_mesh& c, int N, const float* bary) {
  if (c.G < 1 || c.G > GSR_MESH_MAX_G) return fail(GSR_EINVAL, "%s", "G must be in 1..8");
  if (c.V < 0 || c.F < 0 || N < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if ((long long)c.F * c.G != (long long)N) return fail(GSR_EINVAL, "%s", "N must equal F x G");
  if (bary == nullptr) return null_argument();
  if (c.F > 0 &&
      (c.faces == nullptr || c.cplx == nullptr || c.log_scales == nullptr || (c.V > 0 && c.verts == nullptr)))
    return null_argument();
  if ((((uintptr_t)c.cplx | (uintptr_t)c.log_scales) & 7u) != 0)
    return fail(GSR_EINVAL, "%s", "complex_numbers and log_scales must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_mesh_workspace_bytes(int F, int V) { return mesh_workspace_bytes(F < 0 ? 0 : F, V < 0 ? 0 : V); }

int gsr_sugar_mesh_forward(const gsr_sugar_mesh* in, int N, const float* bary, float thickness, float* xyz,
                           float* scaling, float* rotation, float* normals, void* stream) {
  if (in == nullptr) return null_argument();
  if (mesh_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->F == 0) return nothing_to_do();
  if (xyz == nullptr || scaling == nullptr || rotation == nullptr || normals == nullptr) return null_argument();
  if (((uintptr_t)rotation & 15u) != 0) return fail(GSR_EINVAL, "%s", "rotation must be 16-byte aligned");
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
  if (((uintptr_t)dL_drotation & 15u) != 0) return fail(GSR_EINVAL, "%s", "dL_drotation must be 16-byte aligned");
  if ((((uintptr_t)dL_dcomplex | (uintptr_t)dL_dlog_scales) & 7u) != 0)
    return fail(GSR_EINVAL, "%s", "dL_dcomplex and dL_dlog_scales must be 8-byte aligned");
  if (workspace_bytes < mesh_workspace_bytes(in->F, in->V)) return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_mesh_backward(*in, bary, corner_order, vert_offsets, dL_dxyz, dL_dscaling, dL_drotation, dL_dnormals,
                       dL_dverts, dL_dcomplex, dL_dlog_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the time-batched geometry of dynamic SuGaR (gsr_dynamic.hip) ----------------------------------
static bool below_2_31(long long a, long long b) { return a * b < (1ll << 31); }

static int skin_check(const gsr_sugar_skin& c) {
  if (c.K < 1 || c.K > GSR_SKIN_MAX_K) return fail(GSR_EINVAL, "%s", "K must be in 1..32");
  if (c.method != GSR_SKIN_DQS && c.method != GSR_SKIN_LBS)
    return fail(GSR_EINVAL, "%s", "method must be GSR_SKIN_DQS or GSR_SKIN_LBS");
  if (c.T < 0 || c.V < 0 || c.P < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if (!below_2_31(c.T, c.V) || !below_2_31(c.T, c.P) || !below_2_31(c.V, c.K))
    return fail(GSR_EINVAL, "%s", "T x V, T x P and V x K must stay below 2^31");
  if (c.T > 0 && c.V > 0 &&
      (c.P == 0 || c.verts == nullptr || c.node_xyz == nullptr || c.node_trans == nullptr || c.node_rots == nullptr ||
       c.nbr == nullptr || c.w == nullptr))
    return fail(GSR_EINVAL, "%s", c.P == 0 ? "vertices without nodes" : "null pointer argument");
  if (((uintptr_t)c.node_rots & 15u) != 0) return fail(GSR_EINVAL, "%s", "node_rots must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_skin_workspace_bytes(int T, int V, int P) {
  return skin_workspace_bytes(T < 0 ? 0 : T, V < 0 ? 0 : V, P < 0 ? 0 : P);
}

int gsr_sugar_skin_forward(const gsr_sugar_skin* in, float* vert_xyz, float* vert_rot, float* vert_scale,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (in == nullptr) return null_argument();
  if (skin_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (vert_xyz == nullptr || vert_rot == nullptr || workspace == nullptr ||
      (in->node_scales != nullptr && vert_scale == nullptr))
    return null_argument();
  if (((uintptr_t)vert_rot & 15u) != 0) return fail(GSR_EINVAL, "%s", "vert_rot must be 16-byte aligned");
  if (workspace_bytes < skin_workspace_bytes(in->T, in->V, in->P))
    return fail(GSR_EINVAL, "%s", "workspace too small");
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
  if ((((uintptr_t)dL_drot | (uintptr_t)dL_dnode_rots) & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "dL_drot and dL_dnode_rots must be 16-byte aligned");
  if (workspace_bytes < skin_workspace_bytes(in->T, in->V, in->P))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_skin_backward(*in, item_order, node_offsets, dL_dxyz, dL_drot,
                       in->node_scales != nullptr ? dL_dscale : nullptr, dL_dverts, dL_dnode_trans, dL_dnode_rots,
                       dL_dnode_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

static int timed_check(const gsr_sugar_timed& c, int N, const float* bary) {
  if (c.G < 1 || c.G > GSR_MESH_MAX_G) return fail(GSR_EINVAL, "%s", "G must be in 1..8");
  if (c.T < 0 || c.V < 0 || c.F < 0 || N < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if ((long long)c.F * c.G != (long long)N) return fail(GSR_EINVAL, "%s", "N must equal F x G");
  if (!below_2_31(c.T, N) || !below_2_31(c.T, c.V))
    return fail(GSR_EINVAL, "%s", "T x N and T x V must stay below 2^31");
  if (bary == nullptr) return null_argument();
  if ((c.vert_scale == nullptr) != (c.log_scales == nullptr))
    return fail(GSR_EINVAL, "%s", "vert_scale and log_scales are given together or not at all");
  if (c.T > 0 && c.F > 0 &&
      (c.faces == nullptr || c.rotation0 == nullptr || (c.V > 0 && (c.vert_xyz == nullptr || c.vert_rot == nullptr))))
    return null_argument();
  if ((((uintptr_t)c.vert_rot | (uintptr_t)c.rotation0) & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "vert_rot and rotation0 must be 16-byte aligned");
  if (((uintptr_t)c.log_scales & 7u) != 0) return fail(GSR_EINVAL, "%s", "log_scales must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_timed_workspace_bytes(int T, int F) { return timed_workspace_bytes(T < 0 ? 0 : T, F < 0 ? 0 : F); }

int gsr_sugar_timed_forward(const gsr_sugar_timed* in, int N, const float* bary, float* xyz, float* rotation,
                            float* normals, float* scaling, void* stream) {
  if (in == nullptr) return null_argument();
  if (timed_check(*in, N, bary) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->F == 0) return nothing_to_do();
  if (xyz == nullptr || rotation == nullptr || normals == nullptr || (in->vert_scale != nullptr && scaling == nullptr))
    return null_argument();
  if (((uintptr_t)rotation & 15u) != 0) return fail(GSR_EINVAL, "%s", "rotation must be 16-byte aligned");
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
  if ((((uintptr_t)dL_drotation | (uintptr_t)dL_dvert_rot | (uintptr_t)dL_drotation0) & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "dL_drotation, dL_dvert_rot and dL_drotation0 must be 16-byte aligned");
  if (((uintptr_t)dL_dlog_scales & 7u) != 0) return fail(GSR_EINVAL, "%s", "dL_dlog_scales must be 8-byte aligned");
  if (workspace_bytes < timed_workspace_bytes(in->T, in->F)) return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_timed_backward(*in, bary, corner_order, vert_offsets, dL_dxyz, dL_drotation, dL_dnormals,
                        scaled ? dL_dscaling : nullptr, dL_dvert_xyz, dL_dvert_rot, dL_drotation0, dL_dvert_scale,
                        dL_dlog_scales, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the ARAP energy of the deformed mesh (gsr_arap.hip) --------------------------------------------
static int arap_check(const gsr_sugar_arap& c) {
  if (c.rot_form != GSR_ARAP_QUAT && c.rot_form != GSR_ARAP_MATRIX)
    return fail(GSR_EINVAL, "%s", "rot_form must be GSR_ARAP_QUAT or GSR_ARAP_MATRIX");
  if (c.T < 0 || c.V < 0 || c.E < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if (!below_2_31(c.T, c.V)) return fail(GSR_EINVAL, "%s", "T x V must stay below 2^31");
  if (c.T > 0 && c.V > 0 &&
      (c.verts == nullptr || c.offsets == nullptr || c.vert_xyz == nullptr || c.vert_rot == nullptr ||
       (c.E > 0 && (c.nbr == nullptr || c.w == nullptr))))
    return null_argument();
  if (c.rot_form == GSR_ARAP_QUAT && ((uintptr_t)c.vert_rot & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "vert_rot must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_arap_workspace_bytes(int T, int V) { return arap_workspace_bytes(T < 0 ? 0 : T, V < 0 ? 0 : V); }

int gsr_sugar_arap_forward(const gsr_sugar_arap* in, float* energy, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (in == nullptr) return null_argument();
  if (arap_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (energy == nullptr || workspace == nullptr) return null_argument();
  if (workspace_bytes < arap_workspace_bytes(in->T, in->V)) return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_arap_forward(*in, energy, workspace, (hipStream_t)stream);
  return last_launch();
}

int gsr_sugar_arap_backward(const gsr_sugar_arap* in, const float* dL_denergy, float* dL_dvert_xyz,
                            float* dL_dvert_rot, void* stream) {
  if (in == nullptr) return null_argument();
  if (arap_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->V == 0) return nothing_to_do();
  if (dL_denergy == nullptr || dL_dvert_xyz == nullptr || dL_dvert_rot == nullptr) return null_argument();
  if (in->rot_form == GSR_ARAP_QUAT && ((uintptr_t)dL_dvert_rot & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "dL_dvert_rot must be 16-byte aligned");
  launch_arap_backward(*in, dL_denergy, dL_dvert_xyz, dL_dvert_rot, (hipStream_t)stream);
  return last_launch();
}

// ---- the B-spline of the timed node attributes (gsr_spline.hip) -------------------------------------
static int spline_check(const gsr_sugar_spline& c) {
  if (c.degree != 1 && c.degree != 3) return fail(GSR_EINVAL, "%s", "degree must be 1 or 3");
  if (c.n_knots < c.degree + 1) return fail(GSR_EINVAL, "%s", "n_knots must be at least degree + 1");
  if (c.T < 0 || c.P < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if (!(c.interval > 0.0f)) return fail(GSR_EINVAL, "%s", "interval must be positive");
  if (!below_2_31(c.T, c.P) || !below_2_31(c.n_knots, c.P))
    return fail(GSR_EINVAL, "%s", "T x P and n_knots x P must stay below 2^31");
  if (c.T > 0 && c.P > 0 && (c.timestamps == nullptr || c.knots_xyz == nullptr || c.knots_rot == nullptr))
    return null_argument();
  if (((uintptr_t)c.knots_rot & 15u) != 0) return fail(GSR_EINVAL, "%s", "knots_rot must be 16-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_spline_workspace_bytes(int T, int P, int degree) {
  return spline_workspace_bytes(T < 0 ? 0 : T, P < 0 ? 0 : P, degree);
}

int gsr_sugar_spline_forward(const gsr_sugar_spline* in, float* xyz, float* rot, float* scale, void* stream) {
  if (in == nullptr) return null_argument();
  if (spline_check(*in) != GSR_OK) return GSR_EINVAL;
  if (in->T == 0 || in->P == 0) return nothing_to_do();
  if (xyz == nullptr || rot == nullptr || (in->knots_scale != nullptr && scale == nullptr)) return null_argument();
  if (((uintptr_t)rot & 15u) != 0) return fail(GSR_EINVAL, "%s", "rot must be 16-byte aligned");
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
  if ((((uintptr_t)dL_drot | (uintptr_t)dL_dknots_rot) & 15u) != 0)
    return fail(GSR_EINVAL, "%s", "dL_drot and dL_dknots_rot must be 16-byte aligned");
  if (((uintptr_t)workspace & 7u) != 0) return fail(GSR_EINVAL, "%s", "workspace must be 8-byte aligned");
  if (workspace_bytes < spline_workspace_bytes(in->T, in->P, in->degree))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  launch_spline_backward(*in, dL_dxyz, dL_drot, dL_dscale, dL_dknots_xyz, dL_dknots_rot, dL_dknots_scale, workspace,
                         (hipStream_t)stream);
  return last_launch();
}

// ---- the HexPlane deformation network (gsr_deform.hip) ----------------------------------------------
static int deform_check(const gsr_sugar_deform& c) {
  if (c.L < 1 || c.L > GSR_DEFORM_MAX_L) return fail(GSR_EINVAL, "%s", "L must be in 1..4");
  if (c.T < 0 || c.P < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if (!below_2_31(c.T, c.P) || !below_2_31(4, c.P)) return fail(GSR_EINVAL, "%s", "T x P and 4 P must stay below 2^31");
  if (c.reso == nullptr || c.planes == nullptr || c.mlp == nullptr) return null_argument();
  long long texels = 0;
  for (int l = 0; l < c.L; ++l) {
    for (int d = 0; d < 4; ++d)
      if (c.reso[4 * l + d] < 2) return fail(GSR_EINVAL, "%s", "every resolution must be at least 2");
    if (c.reso[4 * l + 3] != c.reso[3]) return fail(GSR_EINVAL, "%s", "the time resolution is the same on every level");
    for (int a = 0; a < 4; ++a)
      for (int b = a + 1; b < 4; ++b) {
        const long long n = (long long)c.reso[4 * l + a] * c.reso[4 * l + b];
        if (n * 32 >= (1ll << 31)) return fail(GSR_EINVAL, "%s", "a plane must stay below 2^31 elements");
        texels += n;
      }
  }
  if (texels >= (1ll << 31)) return fail(GSR_EINVAL, "%s", "the planes must stay below 2^31 texels");
  for (int i = 0; i < 6 * c.L; ++i)
    if (c.planes[i] == nullptr) return fail(GSR_EINVAL, "%s", "null plane");
  for (int i = 0; i < 10; ++i)
    if (c.mlp[i] == nullptr) return null_argument();
  for (int i = 10; i < GSR_DEFORM_MLP; ++i)
    if ((c.mlp[i] != nullptr) != (c.d_scale != 0))
      return fail(GSR_EINVAL, "%s", "the scale head is given iff d_scale is set");
  if (c.T > 0 && c.P > 0 && (c.cell == nullptr || c.frac == nullptr || c.tcell == nullptr || c.tfrac == nullptr))
    return null_argument();
  if (((uintptr_t)c.frac | (uintptr_t)c.tfrac) & 7u) return fail(GSR_EINVAL, "%s", "frac and tfrac must be 8-byte aligned");
  return GSR_OK;
}

size_t gsr_sugar_deform_workspace_bytes(int T, int P, int L) {
  if (L < 1 || L > GSR_DEFORM_MAX_L) return 0;
  return deform_workspace_bytes(T < 0 ? 0 : T, P < 0 ? 0 : P, L);
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
  if (in->n_sp < 0 || in->n_col < 0 || in->n_t < 0) return fail(GSR_EINVAL, "%s", "negative size");
  if (sp_offsets == nullptr || col_offsets == nullptr || t_offsets == nullptr || dL_dplanes == nullptr ||
      dL_dmlp == nullptr || workspace == nullptr || (in->n_sp > 0 && sp_order == nullptr) ||
      (in->n_col > 0 && col_order == nullptr) || (in->n_t > 0 && t_order == nullptr))
    return null_argument();
  for (int i = 0; i < 6 * in->L; ++i)
    if (dL_dplanes[i] == nullptr) return null_argument();
  for (int i = 0; i < (in->d_scale ? GSR_DEFORM_MLP : 10); ++i)
    if (dL_dmlp[i] == nullptr) return null_argument();
  if (((uintptr_t)workspace & 7u) != 0) return fail(GSR_EINVAL, "%s", "workspace must be 8-byte aligned");
  if (workspace_bytes < deform_workspace_bytes(in->T, in->P, in->L))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  const DeformCsr t{sp_order, sp_offsets, col_order, col_offsets, t_order, t_offsets};
  launch_deform_backward(*in, t, dL_dxyz, dL_drot, dL_dscale, dL_dplanes, dL_dmlp, workspace, (hipStream_t)stream);
  return last_launch();
}

// ---- the mesh regularisers of the deformed surface (gsr_meshreg.hip) --------------------------------
static int meshreg_check(const gsr_sugar_meshreg& c) {
  if (c.T < 0 || c.V < 0 || c.E < 0 || c.P < 0) return fail(GSR_EINVAL, "%s", "negative size");
  const long long most = c.P > c.V ? c.P : c.V;
  if (!below_2_31(c.T, c.V) || !below_2_31(4, c.P) || !below_2_31(2, c.E) || !below_2_31(c.T, (most + 255) / 256))
    return fail(GSR_EINVAL, "%s", "T x V, 4 P, 2 E and T x ceil(max(P, V) / 256) must stay below 2^31");
  return GSR_OK;
}
static int null_named(const char* name) { return fail(GSR_EINVAL, "null pointer argument: %s", name); }
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
  if (((uintptr_t)c.pairs & 15u) != 0) return fail(GSR_EINVAL, "%s", "pairs must be 16-byte aligned");
  if (((uintptr_t)workspace & 7u) != 0) return fail(GSR_EINVAL, "%s", "workspace must be 8-byte aligned");
  if (workspace_bytes < meshreg_workspace_bytes(c.T, c.V, c.P, pass))
    return fail(GSR_EINVAL, "%s", "workspace too small");
  return GSR_OK;
}

size_t gsr_sugar_meshreg_workspace_bytes(int T, int V, int P, int pass) {
  if (pass < GSR_MESHREG_FORWARD || pass > GSR_MESHREG_LAP_BACKWARD) return 0;
  return meshreg_workspace_bytes(T < 0 ? 0 : T, V < 0 ? 0 : V, P < 0 ? 0 : P, pass);
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
  if (in->V < 0 || in->V > GSR_SET_MAX) return fail(GSR_EINVAL, "%s", "a densification call takes 0..64 views");
  if (in->P < 0) return fail(GSR_EINVAL, "%s", "P must be >= 0");
  if (in->P == 0 || in->V == 0) return nothing_to_do();
  if (in->max_radii == nullptr) return null_named("max_radii");
  if (in->grad_norm_sum == nullptr) return null_named("grad_norm_sum");
  if (in->count == nullptr) return null_named("count");
  int with_rows = 0;
  for (int v = 0; v < in->V; ++v) {
    if (in->radii[v] == nullptr) return null_named("radii row");
    with_rows += in->visible[v] != nullptr;
  }
  if (with_rows != 0 && with_rows != in->V)
    return fail(GSR_EINVAL, "%s", "visibility rows must be given for every view or for none");
  launch_densify_stats(*in, (hipStream_t)stream);
  return last_launch();
}

// ---- the view-segmented radix sort (tests: every sort of the library runs seg_sort) -----------------
struct SortWork {
  uint32_t *keys2, *vals2, *counts, *totals;
  static SortWork carve(void* base, int V, long long total, uint32_t blocks, size_t* bytes) {
    Carver c(base);
    SortWork w;
    w.keys2 = c.take<uint32_t>((size_t)(total > 0 ? total : 1));
    w.vals2 = c.take<uint32_t>((size_t)(total > 0 ? total : 1));
    w.counts = c.take<uint32_t>((size_t)GSR_RADIX * (blocks > 0 ? blocks : 1));
    w.totals = c.take<uint32_t>((size_t)GSR_RADIX * (size_t)V);
    if (bytes) *bytes = align_up(c.off, 256);
    return w;
  }
};

size_t gsr_sort_work_bytes(int V, const int* n) {
  SegInfo seg;
  long long total = 0;
  if (!set_total(V, n, seg, &total)) return 0;
  size_t b = 0;
  SortWork::carve(nullptr, V, total, seg.blk[V], &b);
  return b;
}

int gsr_sort_pairs(int V, const int* n, uint32_t* keys, uint32_t* vals, int key_bits, int max_bits, void* work,
                   size_t work_bytes, void* stream) {
  if (V < 1 || V > GSR_SET_MAX) return fail(GSR_EINVAL, "%s", "1..64 segments");
  if (n == nullptr || keys == nullptr || work == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (key_bits < 1 || key_bits > 32 || max_bits < 1 || max_bits > GSR_RADIX_BITS)
    return fail(GSR_EINVAL, "%s", "key_bits must be 1..32 and max_bits 1..8");
  SegInfo seg;
  long long total = 0;
  if (inst_segments(V, n, seg, &total) != GSR_OK) return GSR_EINVAL;
  size_t need = 0;
  SortWork w = SortWork::carve(work, V, total, seg.blk[V], &need);
  if (work_bytes < need) return fail(GSR_EINVAL, "%s", "sort work buffer too small");
  if (total == 0) return last_launch();
  hipStream_t s = (hipStream_t)stream;
  uint32_t* kk[2] = {keys, w.keys2};
  uint32_t* vv[2] = {vals, vals != nullptr ? w.vals2 : nullptr};
  const int r = seg_sort(kk, vals != nullptr ? vv : nullptr, false, seg, 0, key_bits, w.counts, w.totals, s,
                         max_bits);
  if (r == 1) {  // (an odd number of passes: the result is in the work buffer)
    GSR_HIP_CHECK(hipMemcpyAsync(keys, w.keys2, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToDevice, s));
    if (vals != nullptr)
      GSR_HIP_CHECK(hipMemcpyAsync(vals, w.vals2, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToDevice, s));
  }
  return last_launch();
}

int gsr_sort_rank_mode(void) { return sort_rank_mode(); }

int gsr_set_num_rendered(int V, const void* geom, int P, int* num_rendered, int* num_visible, int* num_listed,
                         void* stream) {
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if (geom == nullptr || num_rendered == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  GeomState g = GeomState::carve((void*)geom, V, P, nullptr);
  hipStream_t s = (hipStream_t)stream;
  static thread_local uint32_t* pinned = nullptr;
  if (pinned == nullptr) GSR_HIP_CHECK(hipHostMalloc((void**)&pinned, 3 * GSR_SET_MAX * sizeof(uint32_t), hipHostMallocDefault));
  GSR_HIP_CHECK(hipMemcpyAsync(pinned, g.counters, 3 * (size_t)V * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  GSR_HIP_CHECK(hipStreamSynchronize(s));
  for (int v = 0; v < V; ++v) {
    num_rendered[v] = (int)pinned[v];
    if (num_visible) num_visible[v] = (int)pinned[V + v];
    if (num_listed) num_listed[v] = (int)pinned[2 * V + v];
    if (pinned[v] > 0x7fffffffu) return fail(GSR_EINVAL, "%s", "instance count of a view exceeds 2^31");
  }
  g_err[0] = 0;
  return GSR_OK;
}

int gsr_set_gauss_state(int V, const void* geom, int P, void* out_rec, void* out_tiles, void* stream) {
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if (geom == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (P == 0) return GSR_OK;
  GeomState g = GeomState::carve((void*)geom, V, P, nullptr);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)V * (size_t)P;
  if (out_rec) GSR_HIP_CHECK(hipMemcpyAsync(out_rec, g.rec, n * sizeof(GaussRec), hipMemcpyDeviceToDevice, s));
  if (out_tiles) GSR_HIP_CHECK(hipMemcpyAsync(out_tiles, g.tiles, n * sizeof(uint2), hipMemcpyDeviceToDevice, s));
  return last_launch();
}

int gsr_set_render(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_outputs* outputs,
                   void* stream) {
  if (scene == nullptr || state == nullptr || outputs == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  const gsr_set_outputs& o = *outputs;
  const int V = scene->V, P = scene->P, width = scene->width, height = scene->height;
  const int* K = state->num_rendered;
  const float* const* bgs = scene->bgs;
  void *geom = state->geom, *binning = state->binning, *image = state->image;
  const float* colors2 = o.colors2;
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if ((colors2 == nullptr) != (o.out_color2 == nullptr)) return fail(GSR_EINVAL, "%s", "null second colour argument");
  // (out_render without bg_images: the clamp alone)
  if (o.bg_images != nullptr && o.out_render == nullptr) return fail(GSR_EINVAL, "%s", "composite needs out_render");
  if (width <= 0 || height <= 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (K == nullptr || bgs == nullptr || geom == nullptr || binning == nullptr || image == nullptr ||
      o.out_color == nullptr || o.out_depth == nullptr || o.out_alpha == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  for (int v = 0; v < V; ++v)
    if (bgs[v] == nullptr) return fail(GSR_EINVAL, "%s", "null background");
  SegInfo inst;
  long long total = 0;
  if (inst_segments(V, K, inst, &total) != GSR_OK) return GSR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  GeomState g = GeomState::carve(geom, V, P, nullptr);
  const TilePack tp = set_tile_pack(P, width, height);
  BinningState b = BinningState::carve(binning, V, total, inst.blk[V], !tp.packed, nullptr);
  // the split decision of this forward, recorded in the image state for its backward
  const bool split = split_forward(V, P, width, height, total, colors2 != nullptr);
  ImageState img = ImageState::carve(image, V, width, height, nullptr, split);
  const int gx = div_up(width, GSR_TILE_X), gy = div_up(height, GSR_TILE_Y);
  const int tres = tile_sort_result(width, height);
  inst.ndev = g.counters + 2 * V;  // kept instances per view (<= K, the list capacity)
  GSR_HIP_CHECK(hipMemsetAsync(img.split_mode, split ? 1 : 0, sizeof(uint32_t), s));
  // the forward records its cull of each listed instance for the backward (in the free ping-pong key array of the
  // binning buffer, 4 bytes per instance); [1] says in which layout: 1 = the tile-wave forward's 4-bit mask per
  // byte, 2 = one byte per (instance, quadrant) from the quadrant-wave forward's waves
  const bool tile_masks = fwd_tile_chosen(total, (long long)V * P, V);
  GSR_HIP_CHECK(hipMemsetAsync(img.split_mode + 1, total > 0 ? (tile_masks ? 1 : 2) : 0, sizeof(uint32_t), s));
  {
    PhaseScope ps(GSR_PHASE_BINNING, s);
    GSR_HIP_CHECK(hipMemsetAsync(img.ranges, 0, sizeof(uint2) * (size_t)V * gx * gy, s));
    if (total > 0) {
      launch_emit(V, P, width, g, inst, tp, b.key[0], b.val[0], s);
      const int res = seg_sort(b.key, b.val, false, inst, tp.gbits, tp.tile_bits, b.sort_counts, b.sort_totals, s);
      if (res != tres) return fail(GSR_EHIP, "%s", "internal: tile sort buffer");
      launch_tile_ranges(inst, gx * gy, tp, b.key[res], img.ranges, s);
    }
    launch_tile_order(V, gx, gy, img.ranges, img.order, s);  // always written: the backward may use it
  }
  {
    PhaseScope ps(GSR_PHASE_RENDER_FWD, s);
    RenderSet rs;
    render_set_shared(rs, g, img, b, tp, tres, V, P, width, height);
    rs.cbg = o.bg_images;
    rs.comp = o.out_render;
    rs.ccolor = nullptr;
    rs.dcbg = nullptr;
    rs.col2 = colors2;
    rs.out_col2 = o.out_color2;
    rs.dpix2 = nullptr;
    rs.ochunk = order_chunk(V, gx, gy, true);
    rs.ckpt = split ? img.ckpt : nullptr;
    rs.qbytes = total > 0 ? reinterpret_cast<uint8_t*>(b.key[tres ^ 1]) : nullptr;
    rs.V = V;
    rs.v0 = 0;
    for (int v = 0; v < V; ++v) {
      rs.inst_start[v] = inst.start[v];
      rs.row_start[v] = 0;
      rs.bg[v] = bgs[v];
    }
    launch_render_forward(rs, g, tp.packed ? b.key[tres] : b.val[tres], img, o.out_color, o.out_depth, o.out_alpha,
                          total, s);
  }
  return last_launch();
}

static int grad_chunk_size(int P, int n) {
  const int q = (P + n - 1) / n;
  return (q + GSR_GRAD_CHUNK_ALIGN - 1) / GSR_GRAD_CHUNK_ALIGN * GSR_GRAD_CHUNK_ALIGN;
}

// gsr_set_backward; timed != nullptr: gsr_set_timed_backward (checked; `scene` holds the per-view arrays, `grads`
// the second-colour fields of the timed set): the same blend backward, then the per-view per-Gaussian kernel
static int set_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                        const gsr_set_timed* timed, const gsr_set_timed_grads* tgrads, void* stream) {
  const gsr_set_scene& sc = *scene;
  const gsr_set_grads& gr = *grads;
  const int V = sc.V, P = sc.P, width = sc.width, height = sc.height;
  const int* K = state->num_rendered;
  const float* const* bgs = sc.bgs;
  const float *colors_override = gr.colors_override, *color = gr.color, *comp_bg = gr.bg_images;
  float *dL_dcov3D = gr.dL_dcov3D, *dL_dbg = gr.dL_dbg;
  const float *dL_dcolor = gr.dL_dcolor, *dL_ddepth = gr.dL_ddepth, *dL_dalpha = gr.dL_dalpha;
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  // both rasterizer calls of the SuGaR normal renderer in one pass (64-byte rows, 17-field records)
  const bool two = gr.colors2 != nullptr || gr.dL_dcolor2 != nullptr || gr.dL_dcolors2 != nullptr;
  if (two && (gr.colors2 == nullptr || gr.dL_dcolor2 == nullptr || gr.dL_dcolors2 == nullptr ||
              colors_override != nullptr))
    return fail(GSR_EINVAL, "%s", "two-colour backward needs colors2, dL_dcolor2 and dL_dcolors2");
  // (the second call of a two-colour forward on its own: precomputed colours, and the reference passes it no
  // depth / alpha gradient)
  if (colors_override != nullptr && (sc.shs != nullptr || gr.dL_dsh != nullptr || dL_ddepth != nullptr ||
                                     dL_dalpha != nullptr))
    return fail(GSR_EINVAL, "%s", "colors_override excludes SHs and the depth / alpha gradients");
  // (color without bg_images: the clamp alone; neither: no composite)
  if (comp_bg != nullptr && color == nullptr) return fail(GSR_EINVAL, "%s", "composite needs the forward's color");
  if (comp_bg == nullptr && dL_dbg != nullptr) return fail(GSR_EINVAL, "%s", "dL_dbg needs bg_images");
  if (gr.n_chunks < 0 || gr.n_chunks > GSR_GRAD_CHUNKS_MAX || (gr.n_chunks > 0 && gr.chunk_events == nullptr))
    return fail(GSR_EINVAL, "%s", "bad gradient chunk request");
  if (width <= 0 || height <= 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  if (P == 0) return last_launch();
  if (K == nullptr || bgs == nullptr || state->geom == nullptr || state->binning == nullptr ||
      state->image == nullptr || gr.work == nullptr || dL_dcolor == nullptr || gr.dL_dmeans2D == nullptr ||
      gr.dL_dcolors == nullptr || gr.dL_dopacity == nullptr || (timed == nullptr && gr.dL_dmeans3D == nullptr) ||
      state->radii == nullptr || sc.means3D == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  for (int v = 0; v < V; ++v)
    if (bgs[v] == nullptr) return fail(GSR_EINVAL, "%s", "null background");
  if (sc.shs != nullptr && gr.dL_dsh == nullptr) return fail(GSR_EINVAL, "%s", "dL_dsh required with SHs");
  // (a timed set's per-view scales / rotations have per-view gradients: gsr_set_timed_backward checked those)
  const bool need_dscales = timed == nullptr || timed->scales_v == nullptr;
  const bool need_drots = timed == nullptr || timed->rotations_v == nullptr;
  if (sc.cov3D_precomp == nullptr && (sc.scales == nullptr || sc.rotations == nullptr ||
                                      (need_dscales && gr.dL_dscales == nullptr) ||
                                      (need_drots && gr.dL_drotations == nullptr)))
    return fail(GSR_EINVAL, "%s", "scales/rotations and their gradients required");
  SetCams cams;
  if (set_cams(sc, cams) != GSR_OK) return GSR_EINVAL;
  SegInfo inst;
  long long total = 0;
  if (inst_segments(V, K, inst, &total) != GSR_OK) return GSR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  GeomState g = GeomState::carve(state->geom, V, P, nullptr);
  const TilePack tp = set_tile_pack(P, width, height);
  BinningState b = BinningState::carve(state->binning, V, total, inst.blk[V], !tp.packed, nullptr);
  // (the checkpoints, carved last, exist when the forward split: split_mode says so on the device)
  ImageState img = ImageState::carve(state->image, V, width, height, nullptr, true);
  const int gx = div_up(width, GSR_TILE_X), gy = div_up(height, GSR_TILE_Y);
  const size_t HW = (size_t)width * height;
  const int tres = tile_sort_result(width, height);
  const uint32_t* sorted = tp.packed ? b.key[tres] : b.val[tres];
  GaussBackwardArgs a = shared_args(sc, gr);
  if (timed == nullptr && gr.accumulate != 0 && sc.cov3D_precomp == nullptr && dL_dcov3D == nullptr)
    return fail(GSR_EINVAL, "%s", "accumulate needs dL_dcov3D: it carries the running dL/dcov3D between calls");
  void* work = gr.work;
  if (gr.work_bytes < carry_bytes(P)) return fail(GSR_EINVAL, "%s", "backward work buffer too small");
  // the running dL/dcov3D: the caller's output when given, else the end of the work buffer (at a 256-byte
  // boundary whatever work_bytes is)
  const size_t avail = (gr.work_bytes - carry_bytes(P)) & ~(size_t)255;
  float* carry = dL_dcov3D ? dL_dcov3D : (float*)((char*)work + avail);
  bool first = gr.accumulate == 0;
  // groups of consecutive views whose gradient rows and records fit the work buffer
  for (int g0 = 0; g0 < V;) {
    int g1 = g0;
    long long rows = 0;
    while (g1 < V && (g1 == g0 || BackwardState::bytes_for(rows + K[g1], g1 + 1 - g0, P, two) <= avail))
      rows += K[g1++];
    if (BackwardState::bytes_for(rows, g1 - g0, P, two) > avail)
      return fail(GSR_EINVAL, "%s", "backward work buffer smaller than one view's gradient rows");
    BackwardState bw = BackwardState::carve(work, rows, P, two);
    RenderSet rs;
    render_set_shared(rs, g, img, b, tp, tres, V, P, width, height);
    rs.cbg = comp_bg ? comp_bg + (size_t)g0 * HW * 3 : nullptr;
    rs.comp = nullptr;
    rs.ccolor = color ? color + (size_t)g0 * 3 * HW : nullptr;
    rs.dcbg = dL_dbg ? dL_dbg + (size_t)g0 * HW * 3 : nullptr;
    rs.col2 = two ? gr.colors2 : colors_override;
    rs.out_col2 = nullptr;
    rs.dpix2 = two ? gr.dL_dcolor2 + (size_t)g0 * 3 * HW : nullptr;
    // a one-colour backward of the first colour replays split chunks when the forward wrote them.  The host passes
    // the checkpoints whenever the set's size allows a split (split_fits, no environment read here: ADVICE r05) and
    // the kernels follow the decision the forward recorded on the device (split_mode): the extra workgroups of a
    // forward that did not split return at once, and the checkpoints are read only after one that did
    rs.ckpt = !two && colors_override == nullptr && split_fits(V, (size_t)gx * gy) ? img.ckpt : nullptr;
    rs.qbytes = reinterpret_cast<uint8_t*>(b.key[tres ^ 1]);  // (valid when img.split_mode[1] says so)
    rs.V = g1 - g0;
    rs.ochunk = order_chunk(rs.V, gx, gy, false);
    rs.v0 = g0;
    ViewGradArgs va;
    va.V = g1 - g0;
    va.v0 = g0;
    va.W = width;
    va.H = height;
    va.gx = gx;
    va.tiles = gx * gy;
    va.cut_in_lds = 0;
    va.items = 0;
    va.g = g;
    va.img = img;
    va.reach = bw.reach;
    va.grow = bw.grow;
    va.dmeans2D = gr.dL_dmeans2D;
    va.vrec = bw.vrec;
    AccumArgs ab;
    ab.V = g1 - g0;
    ab.v0 = g0;
    ab.accumulate = first ? 0 : 1;
    ab.pad_ = 0;
    ab.reach = bw.reach;
    ab.vrec = bw.vrec;
    ab.dcov_carry = carry;
    ab.dcolors2 = two ? gr.dL_dcolors2 : nullptr;
    for (int v = g0; v < g1; ++v) {
      rs.inst_start[v - g0] = inst.start[v];
      rs.row_start[v - g0] = inst.start[v] - inst.start[g0];
      rs.bg[v - g0] = bgs[v];
      va.row_start[v - g0] = rs.row_start[v - g0];
      va.cam[v - g0] = cams.c[v];
      ab.campos[v - g0] = cams.c[v].campos;
    }
    {
      PhaseScope ps(GSR_PHASE_RENDER_BWD, s);
      // the group's reach bits (set by k_render_bwd, read by the per-Gaussian backward)
      GSR_HIP_CHECK(hipMemsetAsync(bw.reach, 0, sizeof(unsigned long long) * (size_t)P, s));
      launch_render_backward(rs, g, sorted, img, dL_dcolor + (size_t)g0 * 3 * HW,
                             dL_ddepth ? dL_ddepth + (size_t)g0 * HW : nullptr,
                             dL_dalpha ? dL_dalpha + (size_t)g0 * HW : nullptr, bw, s);
    }
    {
      PhaseScope ps(GSR_PHASE_GAUSS_BWD, s);
      const bool last = g1 == V;
      if (timed != nullptr) {
        TimedGradArgs tv;
        tv.means_v = timed->means3D_v;
        tv.scales_v = timed->scales_v;
        tv.rotations_v = timed->rotations_v;
        tv.dmeans_v = tgrads->dL_dmeans3D_v;
        tv.dscales_v = timed->scales_v ? tgrads->dL_dscales_v : nullptr;
        tv.drotations_v = timed->rotations_v ? tgrads->dL_drotations_v : nullptr;
        tv.dcolors2_v = two && timed->colors2_v ? tgrads->dL_dcolors2_v : nullptr;
        tv.dcolors2 = two && !timed->colors2_v ? gr.dL_dcolors2 : nullptr;
        tv.accumulate = first ? 0 : 1;
        launch_timed_gauss_backward(a, va, tv, two, s);
      } else if (last && gr.n_chunks > 0) {
        // the final sums in Gaussian ranges, an event after each (the caller's reduction of a range starts
        // while the next range is computed)
        const int cs = grad_chunk_size(P, gr.n_chunks);
        for (int c = 0; c < gr.n_chunks; ++c) {
          GaussBackwardArgs ac = a;
          ac.g0 = c * cs < P ? c * cs : P;
          ac.g1 = (c + 1) * cs < P ? (c + 1) * cs : P;
          launch_gauss_backward(ac, va, ab, s);
          if (gr.chunk_events[c] != nullptr) GSR_HIP_CHECK(hipEventRecord((hipEvent_t)gr.chunk_events[c], s));
        }
      } else {
        launch_gauss_backward(a, va, ab, s);
      }
    }
    first = false;
    g0 = g1;
  }
  return last_launch();
}

int gsr_set_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                     void* stream) {
  if (scene == nullptr || state == nullptr || grads == nullptr) return fail(GSR_EINVAL, "%s", "null pointer argument");
  return set_backward(scene, state, grads, nullptr, nullptr, stream);
}

int gsr_set_timed_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                           const gsr_set_timed* timed, const gsr_set_timed_grads* timed_grads, void* stream) {
  if (scene == nullptr || state == nullptr || grads == nullptr || timed == nullptr || timed_grads == nullptr)
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  if (check_timed(*scene, *timed) != GSR_OK) return GSR_EINVAL;
  if (grads->n_chunks > 0) return fail(GSR_EINVAL, "%s", "timed view sets: gradient chunks (n_chunks > 0) are not built");
  if (grads->colors_override != nullptr)
    return fail(GSR_EINVAL, "%s", "timed view sets: colors_override is not built (the one-pass two-colour backward only)");
  const gsr_set_timed& tm = *timed;
  const gsr_set_timed_grads& tg = *timed_grads;
  if (tg.dL_dmeans3D_v == nullptr || (tm.scales_v != nullptr && tg.dL_dscales_v == nullptr) ||
      (tm.rotations_v != nullptr && tg.dL_drotations_v == nullptr) ||
      (tm.colors2_v != nullptr && tg.dL_dcolors2_v == nullptr))
    return fail(GSR_EINVAL, "%s", "timed view sets: a per-view array needs its per-view gradient");
  const gsr_set_scene e = timed_scene(*scene, tm);
  gsr_set_grads g = *grads;
  if (tm.colors2_v != nullptr) {
    // the set's second colours are the per-view ones (in the records): their gradient is per view too
    if (g.colors2 != nullptr && g.colors2 != tm.colors2_v)
      return fail(GSR_EINVAL, "%s", "timed view sets: colors2 must be colors2_v (or NULL) when colors2_v is given");
    if (g.dL_dcolor2 == nullptr) return fail(GSR_EINVAL, "%s", "timed view sets: colors2_v needs dL_dcolor2");
    g.colors2 = tm.colors2_v;
    g.dL_dcolors2 = tg.dL_dcolors2_v;  // (non-NULL: selects the two-colour pass; written per view)
  }
  return set_backward(&e, state, &g, timed, timed_grads, stream);
}

int gsr_grad_chunk_range(int P, int n_chunks, int chunk, int* g0, int* g1) {
  if (P < 0 || n_chunks < 1 || n_chunks > GSR_GRAD_CHUNKS_MAX || chunk < 0 || chunk >= n_chunks || g0 == nullptr ||
      g1 == nullptr)
    return fail(GSR_EINVAL, "%s", "bad gradient chunk query");
  const int cs = grad_chunk_size(P, n_chunks);
  *g0 = chunk * cs < P ? chunk * cs : P;
  *g1 = (chunk + 1) * cs < P ? (chunk + 1) * cs : P;
  return GSR_OK;
}

// ---- one view (the reference's per-call interface): a set of one --------------------------

size_t gsr_geom_bytes(int P) { return gsr_set_geom_bytes(1, P); }
// P is not known here: size for the unpacked layout, which is never smaller than the packed one.
size_t gsr_binning_bytes(int K, int width, int height) {
  SegInfo seg;
  long long total = 0;
  if (K < 0 || inst_segments(1, &K, seg, &total) != GSR_OK) return 0;
  size_t b = 0;
  BinningState::carve(nullptr, 1, total, seg.blk[1], true, &b);
  return b;
}
size_t gsr_image_bytes(int width, int height) { return gsr_set_image_bytes(1, 0, nullptr, width, height, 0); }
size_t gsr_backward_bytes(int P, int K) { return gsr_set_backward_bytes(1, P, &K, 0); }

int gsr_forward_preprocess(int P, int degree, int M, const float* means3D, const float* scales,
                           float scale_modifier, const float* rotations, const float* opacities,
                           const float* shs, const float* colors_precomp, const float* cov3D_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* campos,
                           int width, int height, float tanfovx, float tanfovy, int prefiltered,
                           int* radii, void* geom, void* stream) {
  // (host arrays of one: the arguments themselves)
  const gsr_set_scene sc{1, P, degree, M, width, height, prefiltered, scale_modifier, means3D, scales, rotations,
                         opacities, shs, colors_precomp, cov3D_precomp, &viewmatrix, &projmatrix, &campos, nullptr,
                         &tanfovx, &tanfovy};
  const gsr_set_state st{radii, geom, nullptr, nullptr, nullptr};
  return gsr_set_preprocess(&sc, &st, nullptr, stream);
}

int gsr_num_rendered(const void* geom, int P, int* num_rendered, int* num_visible, void* stream) {
  return gsr_set_num_rendered(1, geom, P, num_rendered, num_visible, nullptr, stream);
}

int gsr_forward_render(int P, int K, int width, int height, const float* bg, void* geom,
                       void* binning, void* image, float* out_color, float* out_depth,
                       float* out_alpha, void* stream) {
  if (K < 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  gsr_set_scene sc{};
  sc.V = 1, sc.P = P, sc.width = width, sc.height = height, sc.bgs = &bg;
  const gsr_set_state st{nullptr, geom, binning, image, &K};
  gsr_set_outputs o{};
  o.out_color = out_color, o.out_depth = out_depth, o.out_alpha = out_alpha;
  return gsr_set_render(&sc, &st, &o, stream);
}

int gsr_backward(int P, int degree, int M, int K, int width, int height, const float* bg,
                 const float* means3D, const float* scales, float scale_modifier,
                 const float* rotations, const float* opacities, const float* shs,
                 const float* colors_precomp, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tanfovx, float tanfovy,
                 const int* radii, const void* geom, const void* binning, const void* image,
                 const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                 float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                 void* work, void* stream) {
  if (K < 0) return fail(GSR_EINVAL, "%s", "bad sizes");
  const gsr_set_scene sc{1, P, degree, M, width, height, 0, scale_modifier, means3D, scales, rotations,
                         opacities, shs, colors_precomp, cov3D_precomp, &viewmatrix, &projmatrix, &campos, &bg,
                         &tanfovx, &tanfovy};
  // (the backward only reads the forward state)
  const gsr_set_state st{(int*)radii, (void*)geom, (void*)binning, (void*)image, &K};
  gsr_set_grads gr{};
  gr.dL_dcolor = dL_dcolor, gr.dL_ddepth = dL_ddepth, gr.dL_dalpha = dL_dalpha;
  gr.dL_dmeans2D = dL_dmeans2D, gr.dL_dcolors = dL_dcolors, gr.dL_dopacity = dL_dopacity;
  gr.dL_dmeans3D = dL_dmeans3D, gr.dL_dcov3D = dL_dcov3D, gr.dL_dsh = dL_dsh;
  gr.dL_dscales = dL_dscales, gr.dL_drotations = dL_drotations;
  gr.work = work, gr.work_bytes = gsr_backward_bytes(P, K);
  return gsr_set_backward(&sc, &st, &gr, stream);
}

int gsr_profile_enable(int enable) {
  Profiler& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  p.on = enable != 0;
  return GSR_OK;
}

int gsr_profile_read(double* ms, long long* launches, int reset) {
  Profiler& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  for (const PhaseEvents& e : p.pending) {
    float t = 0.f;
    GSR_HIP_CHECK(hipEventSynchronize(e.b));
    GSR_HIP_CHECK(hipEventElapsedTime(&t, e.a, e.b));
    p.ms[e.phase] += t;
    p.n[e.phase] += 1;
    p.pool.push_back(e.a);
    p.pool.push_back(e.b);
  }
  p.pending.clear();
  for (int i = 0; i < GSR_NUM_PHASES; ++i) {
    if (ms) ms[i] = p.ms[i];
    if (launches) launches[i] = p.n[i];
    if (reset) {
      p.ms[i] = 0;
      p.n[i] = 0;
    }
  }
  return GSR_OK;
}

const char* gsr_profile_kernel(int phase) {
  return phase == GSR_PHASE_RENDER_FWD ? blend_kernel_name(0) : phase == GSR_PHASE_RENDER_BWD ? blend_kernel_name(1) : "";
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream) {
  if (P < 0) return fail(GSR_EINVAL, "%s", "P must be >= 0");
  if (P > 0 && (means3D == nullptr || viewmatrix == nullptr || present == nullptr))
    return fail(GSR_EINVAL, "%s", "null pointer argument");
  launch_mark_visible(P, means3D, viewmatrix, projmatrix, present, (hipStream_t)stream);
  return last_launch();
}

}  // extern "C"
