// gsr_api.hip — the view-set entry points of include/gsr.h (plain and timed), their one-view wrappers, the test
// sort, the profiler and the library's version and last error.  The image epilogues are in gsr_api_image.hip, the
// SuGaR stages in gsr_api_sugar.hip; gsr_api.h holds what the three share.
//
// Phase structure mirrors what the reference's _C.rasterize_gaussians does internally (CudaRasterizer::Rasterizer::
// forward / backward [EXT]); argument checking mirrors its TORCH_CHECKs and Python-side exceptions.
#include <string.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "gsr_api.h"

using namespace gsr;

thread_local char gsr::g_err[512] = "";

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

// GSR_EMIT_SPANS=0: the emission evaluates every Gaussian's rows from its record, as a geometry buffer without span
// words makes it (the bitwise tests and A/B timing of the span-word gather); read once per process.
static bool emit_spans_mode() {
  static const bool on = [] {
    const char* e = getenv("GSR_EMIT_SPANS");
    return !(e != nullptr && strcmp(e, "0") == 0);
  }();
  return on;
}

// SH rows wider than the per-Gaussian backward's LDS staging holds (gauss_backward_max_sh) are rejected by the
// preprocess and the backward alike, before any launch
static int check_sh_width(const gsr_set_scene& sc) {
  if (sc.shs == nullptr || sc.M <= gauss_backward_max_sh()) return GSR_OK;
  char lim[16];
  snprintf(lim, sizeof(lim), "%d", gauss_backward_max_sh());
  return fail(GSR_EINVAL, "M exceeds the largest SH width the per-Gaussian backward's LDS staging holds: M <= %s", lim);
}

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
  a.P = sc.P, a.g0 = 0, a.g1 = sc.P;
  a.M = sc.shs ? sc.M : 0;
  a.deg = effective_degree(sc.degree, a.M);
  a.means3D = sc.means3D, a.scales = sc.scales, a.rotations = sc.rotations, a.shs = sc.shs;
  a.cov3D_precomp = sc.cov3D_precomp, a.scale_modifier = sc.scale_modifier;
  a.dL_dcolors = gr.dL_dcolors, a.dL_dopacity = gr.dL_dopacity;
  a.dL_dmeans3D = gr.dL_dmeans3D, a.dL_dcov3D = gr.dL_dcov3D;
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
    if (K[v] < 0) return invalid("negative instance count");
    seg.n[v] = (uint32_t)K[v];
    seg.start[v] = (uint32_t)run;
    run += K[v];
    if (run >= (1ll << 32)) return invalid("instances of a view set exceed 2^32: use smaller sets");
  }
  seg_fill_blocks(seg, GSR_SORT_TILE);
  if (total) *total = run;
  return GSR_OK;
}

static int set_cams(const gsr_set_scene& sc, SetCams& cams) {
  if (sc.viewmatrices == nullptr || sc.projmatrices == nullptr || sc.campos == nullptr || sc.tanfovx == nullptr ||
      sc.tanfovy == nullptr)
    return invalid("null camera array");
  for (int v = 0; v < sc.V; ++v) {
    if (sc.viewmatrices[v] == nullptr || sc.projmatrices[v] == nullptr || sc.campos[v] == nullptr)
      return invalid("null camera pointer");
    cams.c[v].view = sc.viewmatrices[v], cams.c[v].proj = sc.projmatrices[v], cams.c[v].campos = sc.campos[v];
    cams.c[v].tanx = sc.tanfovx[v], cams.c[v].tany = sc.tanfovy[v];
  }
  return GSR_OK;
}

static int check_set(int V, int P) {
  if (V < 1 || V > GSR_SET_MAX) return invalid("a view set holds 1..64 views");
  if (P < 0) return invalid("P must be >= 0");
  if ((long long)V * (long long)(P > 0 ? P : 1) >= (1ll << 32))
    return invalid("views x Gaussians of a set exceed 2^32: use smaller sets");
  return GSR_OK;
}

// A set's three buffers carved for its forward or its backward, and what both derive from them.
struct SetBuffers {
  GeomState g;
  TilePack tp;
  BinningState b;
  ImageState img;
  int gx, gy;              // the tile grid
  int tres;                // the ping-pong array of the binning buffer that holds the tile sort's result
  const uint32_t* sorted;  // the sorted instance list: packed keys, or the Gaussian indices
  uint8_t* qbytes;         // the forward's cull record in the free key array (BinningState's aliasing contract)
  // with_ckpt: the image buffer ends in the split backward's checkpoints.  The forward passes its split decision;
  // the backward true (they exist when the forward split: split_mode says so on the device)
  static SetBuffers carve(const gsr_set_state& st, int V, int P, int width, int height, const SegInfo& inst,
                          long long total, bool with_ckpt) {
    SetBuffers c;
    c.g = GeomState::carve(st.geom, V, P, nullptr);
    c.tp = set_tile_pack(P, width, height);
    c.b = BinningState::carve(st.binning, V, total, inst.blk[V], !c.tp.packed, nullptr);
    c.img = ImageState::carve(st.image, V, width, height, nullptr, with_ckpt);
    c.gx = div_up(width, GSR_TILE_X), c.gy = div_up(height, GSR_TILE_Y);
    c.tres = tile_sort_result(width, height);
    c.sorted = c.tp.packed ? c.b.key[c.tres] : c.b.val[c.tres];
    c.qbytes = reinterpret_cast<uint8_t*>(c.b.key[c.tres ^ 1]);
    return c;
  }
};

// What the forward and the backward blend of a set derive alike from its carved state.  The callers set the rest: the
// composite and second-colour pointers, ckpt, ochunk, qbytes, V / v0 and the per-view tables.
static void render_set_shared(RenderSet& rs, const SetBuffers& c, int V, int P, int width, int height) {
  rs.P = P, rs.W = width, rs.H = height, rs.gx = c.gx, rs.gy = c.gy;
  rs.gmask = c.tp.gmask;
  rs.col2_rec = c.g.drange + 130;
  rs.order = c.img.order;
  rs.split_mode = c.img.split_mode, rs.split_items = c.img.split_items, rs.split_cap = c.img.split_cap;
  rs.split_extra = split_extra(V, (size_t)rs.gx * rs.gy);
  rs.qkeys = c.tp.qmask ? c.b.key[c.tres] : nullptr;
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
  if (sc.shs != nullptr) return invalid("timed view sets take precomputed colours: shs is not built");
  if (sc.cov3D_precomp != nullptr) return invalid("timed view sets: cov3D_precomp is not built");
  if (tm.means3D_v == nullptr && sc.P > 0) return invalid("timed view sets need means3D_v");
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
  if (sc.width <= 0 || sc.height <= 0) return invalid("image size must be positive");
  if ((sc.shs == nullptr) == (sc.colors_precomp == nullptr))
    return invalid("Please provide exactly one of either SHs or precomputed colors!");
  if (((sc.scales == nullptr || sc.rotations == nullptr) && sc.cov3D_precomp == nullptr) ||
      ((sc.scales != nullptr || sc.rotations != nullptr) && sc.cov3D_precomp != nullptr))
    return invalid("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (state->geom == nullptr ||
      (P > 0 && (sc.means3D == nullptr || sc.opacities == nullptr || state->radii == nullptr)))
    return null_argument();
  if (sc.shs != nullptr && sc.M <= 0) return invalid("M must be >= 1 with SHs");
  if (check_sh_width(sc) != GSR_OK) return GSR_EINVAL;
  SetCams cams;
  if (set_cams(sc, cams) != GSR_OK) return GSR_EINVAL;
  for (int v = 0; v < V; ++v) {  // IEEE float division on the host = the device's correctly rounded one
    cams.c[v].fx = (float)sc.width / (2.0f * cams.c[v].tanx);
    cams.c[v].fy = (float)sc.height / (2.0f * cams.c[v].tany);
  }
  hipStream_t s = (hipStream_t)stream;
  GeomState g = GeomState::carve(state->geom, V, P, nullptr);

  PreprocessArgs a;
  a.V = V, a.P = P, a.W = sc.width, a.H = sc.height;
  a.deg = effective_degree(sc.degree, sc.M);
  a.M = sc.M;
  a.means3D = sc.means3D, a.scales = sc.scales, a.rotations = sc.rotations, a.opacities = sc.opacities;
  a.shs = sc.shs, a.colors_precomp = sc.colors_precomp, a.cov3D_precomp = sc.cov3D_precomp;
  a.scale_modifier = sc.scale_modifier;
  a.radii = state->radii;
  a.col2 = colors2;
  {
    PhaseScope ps(GSR_PHASE_PREPROCESS, s);
    const size_t n = (size_t)P;  // (the per-view strides of a timed set's arrays)
    const PreprocessTimed pt = {3 * n, timed && timed->scales_v ? 3 * n : 0, timed && timed->rotations_v ? 4 * n : 0,
                                3 * n};
    launch_preprocess(a, cams, g, s, timed != nullptr ? &pt : nullptr);
  }
  {
    // depth sort of every view's Gaussians (culled last) -> instance counts in depth order, K_v
    PhaseScope ps(GSR_PHASE_DEPTH_SORT, s);
    SegInfo seg;
    seg.V = V;
    for (int v = 0; v < V; ++v) seg.n[v] = (uint32_t)P, seg.start[v] = (uint32_t)((size_t)v * P);
    seg.rebase = g.drange + 128;  // keys ranked relative to the set's smallest visible key (preprocess)
    const int res = seg_sort(g.dkey, g.dval, false, seg, 0, 32, g.sort_counts, g.sort_totals, s);
    if (res != depth_sort_result()) return fail(GSR_EHIP, "%s", "internal: depth sort result buffer");
    launch_binning_counts(V, P, g, s);  // reads the sorted buffer the device flag names (3 or 4 passes)
  }
  return last_launch();
}

int gsr_set_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const float* colors2, void* stream) {
  if (scene == nullptr || state == nullptr) return null_argument();
  return set_preprocess(scene, state, colors2, nullptr, stream);
}

int gsr_set_timed_preprocess(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_timed* timed,
                             void* stream) {
  if (scene == nullptr || state == nullptr || timed == nullptr) return null_argument();
  if (check_timed(*scene, *timed) != GSR_OK) return GSR_EINVAL;
  const gsr_set_scene e = timed_scene(*scene, *timed);
  return set_preprocess(&e, state, timed->colors2_v, timed, stream);
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
  if (V < 1 || V > GSR_SET_MAX) return invalid("1..64 segments");
  if (n == nullptr || keys == nullptr || work == nullptr) return null_argument();
  if (key_bits < 1 || key_bits > 32 || max_bits < 1 || max_bits > GSR_RADIX_BITS)
    return invalid("key_bits must be 1..32 and max_bits 1..8");
  SegInfo seg;
  long long total = 0;
  if (inst_segments(V, n, seg, &total) != GSR_OK) return GSR_EINVAL;
  size_t need = 0;
  SortWork w = SortWork::carve(work, V, total, seg.blk[V], &need);
  if (work_bytes < need) return invalid("sort work buffer too small");
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
  if (geom == nullptr || num_rendered == nullptr) return null_argument();
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
    if (pinned[v] > 0x7fffffffu) return invalid("instance count of a view exceeds 2^31");
  }
  g_err[0] = 0;
  return GSR_OK;
}

int gsr_set_gauss_state(int V, const void* geom, int P, void* out_rec, void* out_tiles, void* stream) {
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if (geom == nullptr) return null_argument();
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
  if (scene == nullptr || state == nullptr || outputs == nullptr) return null_argument();
  const gsr_set_outputs& o = *outputs;
  const int V = scene->V, P = scene->P, width = scene->width, height = scene->height;
  const int* K = state->num_rendered;
  const float* const* bgs = scene->bgs;
  const float* colors2 = o.colors2;
  if (check_set(V, P) != GSR_OK) return GSR_EINVAL;
  if ((colors2 == nullptr) != (o.out_color2 == nullptr)) return invalid("null second colour argument");
  // (out_render without bg_images: the clamp alone)
  if (o.bg_images != nullptr && o.out_render == nullptr) return invalid("composite needs out_render");
  if (width <= 0 || height <= 0) return invalid("bad sizes");
  if (K == nullptr || bgs == nullptr || state->geom == nullptr || state->binning == nullptr ||
      state->image == nullptr || o.out_color == nullptr || o.out_depth == nullptr || o.out_alpha == nullptr)
    return null_argument();
  for (int v = 0; v < V; ++v)
    if (bgs[v] == nullptr) return invalid("null background");
  SegInfo inst;
  long long total = 0;
  if (inst_segments(V, K, inst, &total) != GSR_OK) return GSR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  // the split decision of this forward, recorded in the image state for its backward
  const bool split = split_forward(V, P, width, height, total, colors2 != nullptr);
  SetBuffers c = SetBuffers::carve(*state, V, P, width, height, inst, total, split);
  const GeomState& g = c.g;
  BinningState& b = c.b;  // (the tile sort takes its ping-pong arrays)
  const ImageState& img = c.img;
  const int gx = c.gx, gy = c.gy;
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
      launch_emit(V, P, width, g, inst, c.tp, emit_spans_mode(), b.key[0], b.val[0], s);
      const int res =
          seg_sort(b.key, b.val, false, inst, c.tp.gbits, c.tp.tile_bits, b.sort_counts, b.sort_totals, s);
      if (res != c.tres) return fail(GSR_EHIP, "%s", "internal: tile sort buffer");
      launch_tile_ranges(inst, gx * gy, c.tp, b.key[res], img.ranges, s);
    }
    launch_tile_order(V, gx, gy, img.ranges, img.order, s);  // always written: the backward may use it
  }
  {
    PhaseScope ps(GSR_PHASE_RENDER_FWD, s);
    RenderSet rs;
    render_set_shared(rs, c, V, P, width, height);
    rs.cbg = o.bg_images, rs.comp = o.out_render, rs.ccolor = nullptr, rs.dcbg = nullptr;
    rs.col2 = colors2, rs.out_col2 = o.out_color2, rs.dpix2 = nullptr;
    rs.ochunk = order_chunk(V, gx, gy, true);
    rs.ckpt = split ? img.ckpt : nullptr;
    rs.qbytes = total > 0 ? c.qbytes : nullptr;
    rs.V = V, rs.v0 = 0;
    for (int v = 0; v < V; ++v) rs.inst_start[v] = inst.start[v], rs.row_start[v] = 0, rs.bg[v] = bgs[v];
    launch_render_forward(rs, g, c.sorted, img, o.out_color, o.out_depth, o.out_alpha, total, s);
  }
  return last_launch();
}

static int grad_chunk_size(int P, int n) {
  const int q = (P + n - 1) / n;
  return (q + GSR_GRAD_CHUNK_ALIGN - 1) / GSR_GRAD_CHUNK_ALIGN * GSR_GRAD_CHUNK_ALIGN;
}

// The argument checks of set_backward up to its cameras, in the order their messages are promised.  An empty scene
// (P == 0) passes after the checks that read no array: the caller returns for it before anything else.
static int check_backward(const gsr_set_scene& sc, const gsr_set_state& st, const gsr_set_grads& gr,
                          const gsr_set_timed* timed, bool two) {
  if (check_set(sc.V, sc.P) != GSR_OK) return GSR_EINVAL;
  if (two && (gr.colors2 == nullptr || gr.dL_dcolor2 == nullptr || gr.dL_dcolors2 == nullptr ||
              gr.colors_override != nullptr))
    return invalid("two-colour backward needs colors2, dL_dcolor2 and dL_dcolors2");
  // (the second call of a two-colour forward on its own: precomputed colours, and the reference passes it no
  // depth / alpha gradient)
  if (gr.colors_override != nullptr && (sc.shs != nullptr || gr.dL_dsh != nullptr || gr.dL_ddepth != nullptr ||
                                        gr.dL_dalpha != nullptr))
    return invalid("colors_override excludes SHs and the depth / alpha gradients");
  // (color without bg_images: the clamp alone; neither: no composite)
  if (gr.bg_images != nullptr && gr.color == nullptr) return invalid("composite needs the forward's color");
  if (gr.bg_images == nullptr && gr.dL_dbg != nullptr) return invalid("dL_dbg needs bg_images");
  if (gr.n_chunks < 0 || gr.n_chunks > GSR_GRAD_CHUNKS_MAX || (gr.n_chunks > 0 && gr.chunk_events == nullptr))
    return invalid("bad gradient chunk request");
  if (sc.width <= 0 || sc.height <= 0) return invalid("bad sizes");
  if (check_sh_width(sc) != GSR_OK) return GSR_EINVAL;
  if (sc.P == 0) return GSR_OK;
  if (st.num_rendered == nullptr || sc.bgs == nullptr || st.geom == nullptr || st.binning == nullptr ||
      st.image == nullptr || gr.work == nullptr || gr.dL_dcolor == nullptr || gr.dL_dmeans2D == nullptr ||
      gr.dL_dcolors == nullptr || gr.dL_dopacity == nullptr || (timed == nullptr && gr.dL_dmeans3D == nullptr) ||
      st.radii == nullptr || sc.means3D == nullptr)
    return null_argument();
  for (int v = 0; v < sc.V; ++v)
    if (sc.bgs[v] == nullptr) return invalid("null background");
  if (sc.shs != nullptr && gr.dL_dsh == nullptr) return invalid("dL_dsh required with SHs");
  // (a timed set's per-view scales / rotations have per-view gradients: gsr_set_timed_backward checked those)
  const bool need_dscales = timed == nullptr || timed->scales_v == nullptr;
  const bool need_drots = timed == nullptr || timed->rotations_v == nullptr;
  if (sc.cov3D_precomp == nullptr && (sc.scales == nullptr || sc.rotations == nullptr ||
                                      (need_dscales && gr.dL_dscales == nullptr) ||
                                      (need_drots && gr.dL_drotations == nullptr)))
    return invalid("scales/rotations and their gradients required");
  return GSR_OK;
}

// The kernel arguments of the view group [g0, g1) of a set's backward: its blend, its per-view gradients and
// their sum over the group (first: no earlier group or call has written the running sums).
static void group_args(RenderSet& rs, ViewGradArgs& va, AccumArgs& ab, const SetBuffers& c, const BackwardState& bw,
                       const gsr_set_scene& sc, const gsr_set_grads& gr, const SetCams& cams, const SegInfo& inst,
                       int g0, int g1, bool two, bool first, float* carry) {
  const int V = sc.V, width = sc.width, height = sc.height;
  const size_t HW = (size_t)width * height;
  render_set_shared(rs, c, V, sc.P, width, height);
  rs.cbg = gr.bg_images ? gr.bg_images + (size_t)g0 * HW * 3 : nullptr;
  rs.ccolor = gr.color ? gr.color + (size_t)g0 * 3 * HW : nullptr;
  rs.dcbg = gr.dL_dbg ? gr.dL_dbg + (size_t)g0 * HW * 3 : nullptr;
  rs.col2 = two ? gr.colors2 : gr.colors_override;
  rs.comp = nullptr, rs.out_col2 = nullptr;
  rs.dpix2 = two ? gr.dL_dcolor2 + (size_t)g0 * 3 * HW : nullptr;
  // a one-colour backward of the first colour replays split chunks when the forward wrote them.  The host passes
  // the checkpoints whenever the set's size allows a split (split_fits, no environment read here: ADVICE r05) and
  // the kernels follow the decision the forward recorded on the device (split_mode): the extra workgroups of a
  // forward that did not split return at once, and the checkpoints are read only after one that did
  rs.ckpt = !two && gr.colors_override == nullptr && split_fits(V, (size_t)c.gx * c.gy) ? c.img.ckpt : nullptr;
  rs.qbytes = c.qbytes;  // (valid when img.split_mode[1] says so)
  rs.V = g1 - g0, rs.v0 = g0;
  rs.ochunk = order_chunk(rs.V, c.gx, c.gy, false);
  va.V = g1 - g0, va.v0 = g0;
  va.W = width, va.H = height, va.gx = c.gx, va.tiles = c.gx * c.gy;
  va.cut_in_lds = 0, va.items = 0;
  va.g = c.g, va.img = c.img;
  va.reach = bw.reach, va.grow = bw.grow, va.vrec = bw.vrec;
  va.dmeans2D = gr.dL_dmeans2D;
  ab.V = g1 - g0, ab.v0 = g0;
  ab.accumulate = first ? 0 : 1, ab.pad_ = 0;
  ab.reach = bw.reach, ab.vrec = bw.vrec;
  ab.dcov_carry = carry;
  ab.dcolors2 = two ? gr.dL_dcolors2 : nullptr;
  for (int v = g0; v < g1; ++v) {
    rs.inst_start[v - g0] = inst.start[v];
    rs.row_start[v - g0] = inst.start[v] - inst.start[g0];
    rs.bg[v - g0] = sc.bgs[v];
    va.row_start[v - g0] = rs.row_start[v - g0];
    va.cam[v - g0] = cams.c[v];
    ab.campos[v - g0] = cams.c[v].campos;
  }
}

// the per-view arrays of a timed set and their gradients for the per-Gaussian kernel of one view group
static TimedGradArgs timed_grad_args(const gsr_set_timed& tm, const gsr_set_timed_grads& tg, const gsr_set_grads& gr,
                                     bool two, bool first) {
  TimedGradArgs tv;
  tv.means_v = tm.means3D_v, tv.scales_v = tm.scales_v, tv.rotations_v = tm.rotations_v;
  tv.dmeans_v = tg.dL_dmeans3D_v;
  tv.dscales_v = tm.scales_v ? tg.dL_dscales_v : nullptr;
  tv.drotations_v = tm.rotations_v ? tg.dL_drotations_v : nullptr;
  tv.dcolors2_v = two && tm.colors2_v ? tg.dL_dcolors2_v : nullptr;
  tv.dcolors2 = two && !tm.colors2_v ? gr.dL_dcolors2 : nullptr;
  tv.accumulate = first ? 0 : 1;
  return tv;
}

// gsr_set_backward; timed != nullptr: gsr_set_timed_backward (checked; `scene` holds the per-view arrays, `grads`
// the second-colour fields of the timed set): the same blend backward, then the per-view per-Gaussian kernel
static int set_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                        const gsr_set_timed* timed, const gsr_set_timed_grads* tgrads, void* stream) {
  const gsr_set_scene& sc = *scene;
  const gsr_set_grads& gr = *grads;
  const int V = sc.V, P = sc.P;
  const int* K = state->num_rendered;
  // both rasterizer calls of the SuGaR normal renderer in one pass (64-byte rows, 17-field records)
  const bool two = gr.colors2 != nullptr || gr.dL_dcolor2 != nullptr || gr.dL_dcolors2 != nullptr;
  if (check_backward(sc, *state, gr, timed, two) != GSR_OK) return GSR_EINVAL;
  if (P == 0) return last_launch();
  SetCams cams;
  if (set_cams(sc, cams) != GSR_OK) return GSR_EINVAL;
  SegInfo inst;
  long long total = 0;
  if (inst_segments(V, K, inst, &total) != GSR_OK) return GSR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const SetBuffers c = SetBuffers::carve(*state, V, P, sc.width, sc.height, inst, total, true);
  const size_t HW = (size_t)sc.width * sc.height;
  GaussBackwardArgs a = shared_args(sc, gr);
  // (after the cameras' and the counts' checks: their messages come first)
  if (timed == nullptr && gr.accumulate != 0 && sc.cov3D_precomp == nullptr && gr.dL_dcov3D == nullptr)
    return invalid("accumulate needs dL_dcov3D: it carries the running dL/dcov3D between calls");
  if (gr.work_bytes < carry_bytes(P)) return invalid("backward work buffer too small");
  // the running dL/dcov3D: the caller's output when given, else the end of the work buffer (at a 256-byte
  // boundary whatever work_bytes is)
  const size_t avail = (gr.work_bytes - carry_bytes(P)) & ~(size_t)255;
  float* carry = gr.dL_dcov3D ? gr.dL_dcov3D : (float*)((char*)gr.work + avail);
  bool first = gr.accumulate == 0;
  // groups of consecutive views whose gradient rows and records fit the work buffer
  for (int g0 = 0; g0 < V;) {
    int g1 = g0;
    long long rows = 0;
    while (g1 < V && (g1 == g0 || BackwardState::bytes_for(rows + K[g1], g1 + 1 - g0, P, two) <= avail))
      rows += K[g1++];
    if (BackwardState::bytes_for(rows, g1 - g0, P, two) > avail)
      return invalid("backward work buffer smaller than one view's gradient rows");
    BackwardState bw = BackwardState::carve(gr.work, rows, P, two);
    RenderSet rs;
    ViewGradArgs va;
    AccumArgs ab;  // (kernel arguments, tables of 64 views: filled in place)
    group_args(rs, va, ab, c, bw, sc, gr, cams, inst, g0, g1, two, first, carry);
    {
      PhaseScope ps(GSR_PHASE_RENDER_BWD, s);
      // the group's reach bits (set by k_render_bwd, read by the per-Gaussian backward)
      GSR_HIP_CHECK(hipMemsetAsync(bw.reach, 0, sizeof(unsigned long long) * (size_t)P, s));
      launch_render_backward(rs, c.g, c.sorted, c.img, gr.dL_dcolor + (size_t)g0 * 3 * HW,
                             gr.dL_ddepth ? gr.dL_ddepth + (size_t)g0 * HW : nullptr,
                             gr.dL_dalpha ? gr.dL_dalpha + (size_t)g0 * HW : nullptr, bw, s);
    }
    {
      PhaseScope ps(GSR_PHASE_GAUSS_BWD, s);
      if (timed != nullptr) {
        launch_timed_gauss_backward(a, va, timed_grad_args(*timed, *tgrads, gr, two, first), two, s);
      } else if (g1 == V && gr.n_chunks > 0) {
        // the final sums in Gaussian ranges, an event after each (the caller's reduction of a range starts
        // while the next range is computed)
        const int cs = grad_chunk_size(P, gr.n_chunks);
        for (int ch = 0; ch < gr.n_chunks; ++ch) {
          GaussBackwardArgs ac = a;
          ac.g0 = ch * cs < P ? ch * cs : P;
          ac.g1 = (ch + 1) * cs < P ? (ch + 1) * cs : P;
          launch_gauss_backward(ac, va, ab, s);
          if (gr.chunk_events[ch] != nullptr) GSR_HIP_CHECK(hipEventRecord((hipEvent_t)gr.chunk_events[ch], s));
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
  if (scene == nullptr || state == nullptr || grads == nullptr) return null_argument();
  return set_backward(scene, state, grads, nullptr, nullptr, stream);
}

int gsr_set_timed_backward(const gsr_set_scene* scene, const gsr_set_state* state, const gsr_set_grads* grads,
                           const gsr_set_timed* timed, const gsr_set_timed_grads* timed_grads, void* stream) {
  if (scene == nullptr || state == nullptr || grads == nullptr || timed == nullptr || timed_grads == nullptr)
    return null_argument();
  if (check_timed(*scene, *timed) != GSR_OK) return GSR_EINVAL;
  if (grads->n_chunks > 0) return invalid("timed view sets: gradient chunks (n_chunks > 0) are not built");
  if (grads->colors_override != nullptr)
    return invalid("timed view sets: colors_override is not built (the one-pass two-colour backward only)");
  const gsr_set_timed& tm = *timed;
  const gsr_set_timed_grads& tg = *timed_grads;
  if (tg.dL_dmeans3D_v == nullptr || (tm.scales_v != nullptr && tg.dL_dscales_v == nullptr) ||
      (tm.rotations_v != nullptr && tg.dL_drotations_v == nullptr) ||
      (tm.colors2_v != nullptr && tg.dL_dcolors2_v == nullptr))
    return invalid("timed view sets: a per-view array needs its per-view gradient");
  const gsr_set_scene e = timed_scene(*scene, tm);
  gsr_set_grads g = *grads;
  if (tm.colors2_v != nullptr) {
    // the set's second colours are the per-view ones (in the records): their gradient is per view too
    if (g.colors2 != nullptr && g.colors2 != tm.colors2_v)
      return invalid("timed view sets: colors2 must be colors2_v (or NULL) when colors2_v is given");
    if (g.dL_dcolor2 == nullptr) return invalid("timed view sets: colors2_v needs dL_dcolor2");
    g.colors2 = tm.colors2_v;
    g.dL_dcolors2 = tg.dL_dcolors2_v;  // (non-NULL: selects the two-colour pass; written per view)
  }
  return set_backward(&e, state, &g, timed, timed_grads, stream);
}

int gsr_grad_chunk_range(int P, int n_chunks, int chunk, int* g0, int* g1) {
  if (P < 0 || n_chunks < 1 || n_chunks > GSR_GRAD_CHUNKS_MAX || chunk < 0 || chunk >= n_chunks || g0 == nullptr ||
      g1 == nullptr)
    return invalid("bad gradient chunk query");
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

int gsr_forward_preprocess(int P, int degree, int M, const float* means3D, const float* scales, float scale_modifier,
                           const float* rotations, const float* opacities, const float* shs,
                           const float* colors_precomp, const float* cov3D_precomp, const float* viewmatrix,
                           const float* projmatrix, const float* campos, int width, int height, float tanfovx,
                           float tanfovy, int prefiltered, int* radii, void* geom, void* stream) {
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

int gsr_forward_render(int P, int K, int width, int height, const float* bg, void* geom, void* binning, void* image,
                       float* out_color, float* out_depth, float* out_alpha, void* stream) {
  if (K < 0) return invalid("bad sizes");
  gsr_set_scene sc{};
  sc.V = 1, sc.P = P, sc.width = width, sc.height = height, sc.bgs = &bg;
  const gsr_set_state st{nullptr, geom, binning, image, &K};
  gsr_set_outputs o{};
  o.out_color = out_color, o.out_depth = out_depth, o.out_alpha = out_alpha;
  return gsr_set_render(&sc, &st, &o, stream);
}

int gsr_backward(int P, int degree, int M, int K, int width, int height, const float* bg, const float* means3D,
                 const float* scales, float scale_modifier, const float* rotations, const float* opacities,
                 const float* shs, const float* colors_precomp, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tanfovx, float tanfovy, const int* radii,
                 const void* geom, const void* binning, const void* image, const float* dL_dcolor,
                 const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans2D, float* dL_dcolors,
                 float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                 float* dL_drotations, void* work, void* stream) {
  if (K < 0) return invalid("bad sizes");
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
  if (P < 0) return invalid("P must be >= 0");
  if (P > 0 && (means3D == nullptr || viewmatrix == nullptr || present == nullptr)) return null_argument();
  launch_mark_visible(P, means3D, viewmatrix, projmatrix, present, (hipStream_t)stream);
  return last_launch();
}

}  // extern "C"
