// gsr_knn.hip — mean squared distance to the 3 nearest neighbours (replaces simple_knn.distCUDA2).
//
// The reference initialises Gaussian scales from a point cloud with
//     dist2 = torch.clamp_min(distCUDA2(points.float().cuda()), 0.0000001)
//     scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
// (geometry/gaussian_base.py:25,434-438; also geometry/sugar.py:18, geometry/gaussian_io.py:25,
// geometry/spacetime_gaussian.py:15,430, geometry/dynamic_sugar.py:17, geometry/gaussian_dynamic.py:25).
// `simple_knn` (graphdeco-inria, unpinned, installed from GitHub by the reference's README) is not in the
// reference tree.  Its published result: for every point, the mean of the squared Euclidean distances
// to its 3 nearest *other* points (duplicates count, distance 0), best distances kept sorted by the
// swap-insertion "if (best[j] > d) swap" and averaged as (best[0] + best[1] + best[2]) / 3 with the
// FLT_MAX initial values left in place when P < 4.  The search is exact, so the result depends only on
// the per-pair fp32 distance formula: here d = fma(dz, dz, fma(dy, dy, dx * dx)) (nvcc's default
// contraction of dx*dx + dy*dy + dz*dz).
//
// MI355X design (not simple_knn's 1024-point boxes scanned lane by lane):
//   1. bbox: per-block min/max partials (256 blocks), folded by every block of the Morton pass;
//   2. 30-bit Morton codes (10 bits per axis over the bbox), sorted by the segmented LSD radix sort
//      (gsr_sort.hip, one segment, identity values) — sorted points are spatially coherent;
//   3. a 3-level AABB hierarchy over the sorted points: boxes of 32, superboxes of 32 boxes (1024
//      points), hyperboxes of 32 superboxes (32768 points);
//   4. query: one wave per 64 consecutive sorted points.  The wave walks the hierarchy starting from its
//      own box / superbox / hyperbox (tight bounds early) and descends into a node only if some lane's
//      squared distance to the node's AABB is <= that lane's current 3rd-best (ballot); node AABBs and
//      a scanned box's 32 points are read with scalar loads (wave-uniform addresses -> SGPR operands, a
//      broadcast without VGPR / LDS traffic), each lane updating its sorted top-3 with min/max.  Pruning is exact: the fma-chain is monotone
//      in |dx|, |dy|, |dz|, so no box holding a closer point is skipped.
//   5. results are written back to the input order.
// HBM traffic is small (≈ 12 B read + 4 B written per point plus the sort); the query is VALU-bound.
//
// knn_points (replaces pytorch3d.ops.knn_points of a cloud against itself: the SuGaR geometry's reset_neighbors,
// geometry/sugar.py:646, utils/sugar_utils.py:41,248) runs steps 1-3 unchanged and the same walk with another
// per-lane list: the K <= 32 nearest points, the point itself included, as (distance, input index) pairs sorted
// by (distance, index), written to (P, K) float32 / int64 rows in input order (k_knn_points).
#include <float.h>

#include "gsr_kernels.h"
#include "gsr_wave.h"

namespace gsr {

namespace {
constexpr int KNN_FAN = 32;  // children per node at every level
constexpr int KNN_BOX = 32, KNN_SUPER = KNN_BOX * KNN_FAN, KNN_HYPER = KNN_SUPER * KNN_FAN;
constexpr int KNN_BBOX_BLOCKS = 256;  // bbox partials

__device__ __forceinline__ uint32_t spread10(uint32_t x) {  // 10 bits -> every third bit
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}
__device__ __forceinline__ float dist2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }
__device__ __forceinline__ float box_dist2(float4 q, float4 lo, float4 hi) {
  const float dx = fmaxf(0.0f, fmaxf(lo.x - q.x, q.x - hi.x));
  const float dy = fmaxf(0.0f, fmaxf(lo.y - q.y, q.y - hi.y));
  const float dz = fmaxf(0.0f, fmaxf(lo.z - q.z, q.z - hi.z));
  return dist2(dx, dy, dz);
}
}  // namespace

struct KnnWork {
  uint32_t* keys[2];
  uint32_t* vals[2];
  uint32_t* counts;
  uint32_t* totals;
  float* bbox;     // per-block partials: [block][min xyz, max xyz]
  float* bpts;     // Morton-sorted points, per box of 32 SoA: [box][x | y | z][32], +inf padding
  float4* lo[3];   // AABBs per level (box, super, hyper)
  float4* hi[3];
  int n[3];
  static KnnWork carve(void* base, int P, size_t* bytes) {
    Carver c(base);
    KnnWork w;
    const size_t n = (size_t)(P > 0 ? P : 1);
    for (int k = 0; k < 2; ++k) w.keys[k] = c.take<uint32_t>(n), w.vals[k] = c.take<uint32_t>(n);
    w.counts = c.take<uint32_t>((size_t)GSR_RADIX * div_up((long long)n, GSR_SORT_TILE));
    w.totals = c.take<uint32_t>(GSR_RADIX);
    w.bbox = c.take<float>(6 * KNN_BBOX_BLOCKS);
    w.bpts = c.take<float>((size_t)div_up((long long)n, KNN_BOX) * 3 * KNN_BOX);
    int cnt = (int)n;
    const int fan[3] = {KNN_BOX, KNN_FAN, KNN_FAN};
    for (int l = 0; l < 3; ++l) {
      cnt = div_up(cnt, fan[l]);
      w.n[l] = cnt;
      w.lo[l] = c.take<float4>(cnt);
      w.hi[l] = c.take<float4>(cnt);
    }
    if (bytes) *bytes = align_up(c.off, 256);
    return w;
  }
};


// per-block bbox partials (no same-address atomics: those serialise at the memory side)
__global__ __launch_bounds__(256) void k_knn_bbox(int P, const float* __restrict__ pts, float* __restrict__ part) {
  __shared__ float s[4][6];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = pts[3 * (size_t)i + k];
      mn[k] = fminf(mn[k], v);
      mx[k] = fmaxf(mx[k], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[w][k] = mn[k], s[w][3 + k] = mx[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    float r = s[0][k];
    for (int j = 1; j < 4; ++j) r = k < 3 ? fminf(r, s[j][k]) : fmaxf(r, s[j][k]);
    part[blockIdx.x * 6 + k] = r;
  }
}

// Morton code per point; every block first folds the bbox partials (6 KB, L2-resident)
__global__ __launch_bounds__(256) void k_knn_morton(int P, const float* __restrict__ pts, int nparts,
                                                    const float* __restrict__ part, uint32_t* __restrict__ keys) {
  __shared__ float s_box[4][6];
  {
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int j = threadIdx.x; j < nparts; j += 256) {
#pragma unroll
      for (int k = 0; k < 6; ++k) m[k] = k < 3 ? fminf(m[k], part[6 * j + k]) : fmaxf(m[k], part[6 * j + k]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
      for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m[k], off);
        m[k] = k < 3 ? fminf(m[k], o) : fmaxf(m[k], o);
      }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) s_box[threadIdx.x >> 6][k] = m[k];
    }
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  uint32_t code = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = fminf(fminf(s_box[0][k], s_box[1][k]), fminf(s_box[2][k], s_box[3][k]));
    const float hi = fmaxf(fmaxf(s_box[0][3 + k], s_box[1][3 + k]), fmaxf(s_box[2][3 + k], s_box[3][3 + k]));
    const float ext = hi - lo;
    const float t = ext > 0.0f ? (pts[3 * (size_t)i + k] - lo) / ext : 0.0f;
    const uint32_t q = (uint32_t)fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
    code |= spread10(q) << (2 - k);
  }
  keys[i] = code;
}

__global__ __launch_bounds__(256) void k_knn_gather(int P, int n_slots, const float* __restrict__ pts,
                                                    const uint32_t* __restrict__ order, float* __restrict__ bpts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_slots) return;
  float x = INFINITY, y = INFINITY, z = INFINITY;  // padding of the last box: never a neighbour
  if (i < P) {
    const size_t j = order[i];
    x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
  }
  float* box = bpts + (size_t)(i / KNN_BOX) * 3 * KNN_BOX + (i % KNN_BOX);
  box[0] = x, box[KNN_BOX] = y, box[2 * KNN_BOX] = z;
}

// AABB of each box of 32 sorted points (SoA, padding excluded)
__global__ __launch_bounds__(256) void k_knn_box_aabb(int P, int n_box, const float* __restrict__ bpts,
                                                      float4* __restrict__ lo, float4* __restrict__ hi) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_box) return;
  const float* box = bpts + (size_t)b * 3 * KNN_BOX;
  const int cnt = min(KNN_BOX, P - b * KNN_BOX);
  float4 a = make_float4(INFINITY, INFINITY, INFINITY, 0.f), c = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
  for (int j = 0; j < cnt; ++j) {
    const float x = box[j], y = box[KNN_BOX + j], z = box[2 * KNN_BOX + j];
    a.x = fminf(a.x, x), a.y = fminf(a.y, y), a.z = fminf(a.z, z);
    c.x = fmaxf(c.x, x), c.y = fmaxf(c.y, y), c.z = fmaxf(c.z, z);
  }
  lo[b] = a;
  hi[b] = c;
}

// AABB of each group of `fan` consecutive children (children given as lo / hi float4 arrays)
__global__ __launch_bounds__(256) void k_knn_aabb(int n_children, int fan, const float4* __restrict__ clo,
                                                  const float4* __restrict__ chi, int n_out, float4* __restrict__ lo,
                                                  float4* __restrict__ hi) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_out) return;
  float4 a = make_float4(INFINITY, INFINITY, INFINITY, 0.f), b = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
  const int e = min(n_children, (g + 1) * fan);
  for (int c = g * fan; c < e; ++c) {
    const float4 l = clo[c], h = chi[c];
    a.x = fminf(a.x, l.x), a.y = fminf(a.y, l.y), a.z = fminf(a.z, l.z);
    b.x = fmaxf(b.x, h.x), b.y = fmaxf(b.y, h.y), b.z = fmaxf(b.z, h.z);
  }
  lo[g] = a;
  hi[g] = b;
}

struct KnnQuery {
  int P;
  const float* bpts;
  const float4* lo[3];
  const float4* hi[3];
  int n[3];
  const uint32_t* order;
  float* out;
};

// Loads whose index is wave-uniform, through the constant address space: the compiler emits s_load
// (scalar cache, SGPR results used directly as VALU operands — a broadcast with no VGPR or LDS traffic).
typedef __attribute__((address_space(4))) const float* cfptr;

__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2) {
  // the "if (best[k] > d) swap" insertion, branch-free
  const float n0 = fminf(b0, d), c1 = fmaxf(b0, d);
  const float n1 = fminf(b1, c1), c2 = fmaxf(b1, c1);
  b0 = n0, b1 = n1, b2 = fminf(b2, c2);
}

// Per-lane candidate lists of the query walk (knn_walk below).  A list gives the lane's pruning bound
// (worst(): a node or point at exactly this distance is still looked at), is told which box is scanned next
// (begin_box) and is offered every point of that box (add: `slot` is the point's position in the box, a
// compile-time constant after unrolling; d its squared distance to the lane's query).

// distCUDA2: the 3 smallest distances to the other points.
struct KnnTop3 {
  float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
  int i;     // the lane's sorted position
  int self;  // position of the lane's own point in the scanned box (or outside 0..31)
  __device__ __forceinline__ float worst() const { return b2; }
  __device__ __forceinline__ void begin_box(int b) { self = i - b * KNN_BOX; }
  __device__ __forceinline__ void add(int slot, float d) { knn_insert(slot == self ? FLT_MAX : d, b0, b1, b2); }
};

// knn_points: the KCAP smallest (distance, input index) pairs, the point itself included.  An entry is one signed
// 64-bit key, distance bits << 32 | input index: distances are >= +0, so their bit patterns order like the values
// and one integer compare orders by (distance, index).  Empty entries are (+inf, KNN_NO_INDEX); a list asked for
// fewer than KCAP neighbours starts with KCAP - K negative keys in front, which no candidate displaces, so that
// the K-th best is always e[KCAP - 1].  All indices into e[] are compile-time constants (registers, no scratch).
constexpr uint32_t KNN_NO_INDEX = 0xffffffffu;
constexpr long long KNN_EMPTY = (long long)((0x7f800000ull << 32) | KNN_NO_INDEX);
template <int KCAP>
struct KnnTopK {
  long long e[KCAP];
  bool valid;             // lanes past the last point never insert
  int lane, P;
  const uint32_t* order;  // sorted position -> input index
  uint32_t ordv;          // lanes 0..31: input index of the scanned box's point `lane` (KNN_NO_INDEX: padding)
  __device__ __forceinline__ void init(int K) {
#pragma unroll
    for (int k = 0; k < KCAP; ++k) e[k] = k < KCAP - K ? (long long)(k - KCAP) : KNN_EMPTY;
  }
  __device__ __forceinline__ float worst() const { return __uint_as_float((uint32_t)(e[KCAP - 1] >> 32)); }
  __device__ __forceinline__ void begin_box(int b) {
    const int pos = b * KNN_BOX + (lane & (KNN_BOX - 1));
    ordv = pos < P ? order[pos] : KNN_NO_INDEX;  // the padding of the last box equals an empty entry: never inserted
  }
  __device__ __forceinline__ void add(int slot, float d) {
    // after warm-up most points are rejected by every lane: the chain runs only when some lane inserts
    if (__ballot(valid && d <= worst()) == 0ull) return;
    const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)ordv, slot);
    const long long c = (long long)(((unsigned long long)__float_as_uint(d) << 32) | id);
    bool lt[KCAP];  // monotone in k (the list is sorted); a lane that does not insert has none set
#pragma unroll
    for (int k = 0; k < KCAP; ++k) lt[k] = c < e[k];
#pragma unroll
    for (int k = KCAP - 1; k > 0; --k) e[k] = lt[k - 1] ? e[k - 1] : (lt[k] ? c : e[k]);
    e[0] = lt[0] ? c : e[0];
  }
};

// The query walk of one wave over the hierarchy (design point 4 above), shared by the query kernels: `base` is the
// wave's first sorted position, q the lane's query point, L the lane's candidate list.
template <class List>
__device__ __forceinline__ void knn_walk(const KnnQuery& Q, int base, int lane, bool valid, float4 q, List& L) {
#pragma clang fp contract(off)
  const float lim_invalid = -1.0f;  // invalid lanes never ask for a node
  auto need = [&](float d) { return valid ? d <= L.worst() : d <= lim_invalid; };
  // AABB of the wave's queries and the wave's loosest current bound: a node whose AABB is farther from the
  // query AABB than sqrt(max worst) holds no lane's neighbour (conservative: exactness kept)
  float ql[3] = {valid ? q.x : INFINITY, valid ? q.y : INFINITY, valid ? q.z : INFINITY};
  float qh[3] = {valid ? q.x : -INFINITY, valid ? q.y : -INFINITY, valid ? q.z : -INFINITY};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      ql[k] = fminf(ql[k], __shfl_xor(ql[k], off));
      qh[k] = fmaxf(qh[k], __shfl_xor(qh[k], off));
    }
  }
  auto bound = [&]() {
    float m = valid ? L.worst() : 0.0f;
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    return m;
  };
  // children [c0, c0 + cnt) of level l (cnt <= 64) tested in parallel, one per lane -> candidate mask
  auto children = [&](int l, int c0, int cnt) -> unsigned long long {
    const float bd = bound();
    bool t = false;
    if (lane < cnt) {
      const float4 lo = Q.lo[l][c0 + lane], hi = Q.hi[l][c0 + lane];
      const float dx = fmaxf(0.0f, fmaxf(lo.x - qh[0], ql[0] - hi.x));
      const float dy = fmaxf(0.0f, fmaxf(lo.y - qh[1], ql[1] - hi.y));
      const float dz = fmaxf(0.0f, fmaxf(lo.z - qh[2], ql[2] - hi.z));
      t = dist2(dx, dy, dz) <= bd;
    }
    return __ballot(t);
  };
  // visit the set bits of `mask` starting at bit `first` (own node first: tight bounds early), wrapping
  auto order_bits = [](unsigned long long mask, int first, unsigned long long& lo_part) {
    const unsigned long long at = first > 0 && first < 64 ? (~0ull << first) : (first <= 0 ? ~0ull : 0ull);
    lo_part = mask & ~at;
    return mask & at;
  };
  // exact per-lane test of one node (scalar loads of its AABB), ballot
  auto refine = [&](int l, int k) {
    const cfptr lo = (cfptr)Q.lo[l] + 4 * (size_t)k, hi = (cfptr)Q.hi[l] + 4 * (size_t)k;
    const float bd = box_dist2(q, make_float4(lo[0], lo[1], lo[2], 0.f), make_float4(hi[0], hi[1], hi[2], 0.f));
    return __ballot(need(bd)) != 0ull;
  };
  auto scan_box = [&](int b) {
    if (!refine(0, b)) return;
    L.begin_box(b);
    const cfptr box = (cfptr)Q.bpts + (size_t)b * 3 * KNN_BOX;
#pragma unroll
    for (int c = 0; c < KNN_BOX; c += 16) {  // 16 points = 48 SGPRs per batch of s_load_dwordx16
      float xs[16], ys[16], zs[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) xs[j] = box[c + j], ys[j] = box[KNN_BOX + c + j], zs[j] = box[2 * KNN_BOX + c + j];
#pragma unroll
      for (int j = 0; j < 16; ++j) L.add(c + j, dist2(xs[j] - q.x, ys[j] - q.y, zs[j] - q.z));
    }
  };

  const int own[3] = {base / KNN_BOX, base / KNN_SUPER, base / KNN_HYPER};
  const int nh = Q.n[2];
  for (int h0 = (own[2] / 64) * 64, hv = 0; hv < nh; hv += 64, h0 = (h0 + 64 < nh ? h0 + 64 : 0)) {
    unsigned long long hrest;
    unsigned long long hm = order_bits(children(2, h0, min(64, nh - h0)), own[2] - h0, hrest);
    for (int pass_h = 0; pass_h < 2; ++pass_h, hm = hrest) {
      while (hm) {
        const int h = h0 + __builtin_ctzll(hm);
        hm &= hm - 1;
        if (!refine(2, h)) continue;
        const int s_lo = h * KNN_FAN;
        unsigned long long srest;
        unsigned long long sm = order_bits(children(1, s_lo, min(KNN_FAN, Q.n[1] - s_lo)), own[1] - s_lo, srest);
        for (int pass_s = 0; pass_s < 2; ++pass_s, sm = srest) {
          while (sm) {
            const int sidx = s_lo + __builtin_ctzll(sm);
            sm &= sm - 1;
            if (!refine(1, sidx)) continue;
            const int x_lo = sidx * KNN_FAN;
            unsigned long long xrest;
            unsigned long long xm =
                order_bits(children(0, x_lo, min(KNN_FAN, Q.n[0] - x_lo)), own[0] - x_lo, xrest);
            for (int pass_x = 0; pass_x < 2; ++pass_x, xm = xrest) {
              while (xm) {
                const int bx = x_lo + __builtin_ctzll(xm);
                xm &= xm - 1;
                scan_box(bx);
              }
            }
          }
        }
      }
    }
  }
}

// the wave's 64 consecutive sorted points: false (uniform) when the wave has none
__device__ __forceinline__ bool knn_wave_query(const KnnQuery& Q, int& base, int& lane, int& i, bool& valid,
                                               float4& q) {
  lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  base = wave * 64;
  if (base >= Q.P) return false;
  i = base + lane;
  valid = i < Q.P;
  const int qi = valid ? i : base;
  const float* qb = Q.bpts + (size_t)(qi / KNN_BOX) * 3 * KNN_BOX + (qi % KNN_BOX);
  q = make_float4(qb[0], qb[KNN_BOX], qb[2 * KNN_BOX], 0.0f);
  return true;
}

__global__ __launch_bounds__(256) void k_knn_query(KnnQuery Q) {
  int base, lane, i;
  bool valid;
  float4 q;
  if (!knn_wave_query(Q, base, lane, i, valid, q)) return;
  KnnTop3 L;
  L.i = i;
  knn_walk(Q, base, lane, valid, q, L);
  if (valid) Q.out[Q.order[i]] = (L.b0 + L.b1 + L.b2) / 3.0f;
}

// knn_points: row order[i] of dists / idx (P x K, input order) gets the lane's K best, ascending by (distance, index)
template <int KCAP>
__global__ __launch_bounds__(256) void k_knn_points(KnnQuery Q, int K, float* __restrict__ dists,
                                                    long long* __restrict__ idx) {
  int base, lane, i;
  bool valid;
  float4 q;
  if (!knn_wave_query(Q, base, lane, i, valid, q)) return;
  KnnTopK<KCAP> L;
  L.valid = valid, L.lane = lane, L.P = Q.P, L.order = Q.order;
  L.init(K);
  knn_walk(Q, base, lane, valid, q, L);
  if (!valid) return;
  const size_t row = (size_t)Q.order[i] * (size_t)K;
#pragma unroll
  for (int k = 0; k < KCAP; ++k) {
    const int col = k - (KCAP - K);
    if (col < 0) continue;
    const uint32_t id = (uint32_t)L.e[k];
    dists[row + col] = __uint_as_float((uint32_t)(L.e[k] >> 32));
    idx[row + col] = id == KNN_NO_INDEX ? -1ll : (long long)id;
  }
}

size_t knn_workspace_bytes(int P) {
  size_t bytes = 0;
  KnnWork::carve(nullptr, P, &bytes);
  return bytes;
}

// bbox, Morton codes, sort, SoA boxes and the AABB hierarchy of `points`, in `ws`: what both queries walk
static KnnQuery knn_build_tree(int P, const float* points, void* ws, hipStream_t stream) {
  KnnWork w = KnnWork::carve(ws, P, nullptr);
  const int blocks = div_up(P, 256);
  const int nparts = min(blocks, KNN_BBOX_BLOCKS);
  hipLaunchKernelGGL(k_knn_bbox, dim3((unsigned)nparts), dim3(256), 0, stream, P, points, w.bbox);
  hipLaunchKernelGGL(k_knn_morton, dim3((unsigned)blocks), dim3(256), 0, stream, P, points, nparts,
                     (const float*)w.bbox, w.keys[0]);
  SegInfo seg{};
  seg.V = 1;
  seg.n[0] = (uint32_t)P;
  seg.start[0] = 0;
  const int r = seg_sort(w.keys, w.vals, true, seg, 0, 30, w.counts, w.totals, stream);
  const int n_slots = w.n[0] * KNN_BOX;
  hipLaunchKernelGGL(k_knn_gather, dim3((unsigned)div_up(n_slots, 256)), dim3(256), 0, stream, P, n_slots, points,
                     (const uint32_t*)w.vals[r], w.bpts);
  hipLaunchKernelGGL(k_knn_box_aabb, dim3((unsigned)div_up(w.n[0], 256)), dim3(256), 0, stream, P, w.n[0],
                     (const float*)w.bpts, w.lo[0], w.hi[0]);
  const int fan[3] = {KNN_BOX, KNN_FAN, KNN_FAN};
  int nchild = w.n[0];
  const float4* clo = w.lo[0];
  const float4* chi = w.hi[0];
  for (int l = 1; l < 3; ++l) {
    hipLaunchKernelGGL(k_knn_aabb, dim3((unsigned)div_up(w.n[l], 256)), dim3(256), 0, stream, nchild, fan[l], clo, chi,
                       w.n[l], w.lo[l], w.hi[l]);
    nchild = w.n[l];
    clo = w.lo[l];
    chi = w.hi[l];
  }
  KnnQuery Q{};
  Q.P = P;
  Q.bpts = w.bpts;
  for (int l = 0; l < 3; ++l) Q.lo[l] = w.lo[l], Q.hi[l] = w.hi[l], Q.n[l] = w.n[l];
  Q.order = w.vals[r];
  Q.out = nullptr;
  return Q;
}

int launch_knn_mean_dist(int P, const float* points, float* out, void* ws, hipStream_t stream) {
  KnnQuery Q = knn_build_tree(P, points, ws, stream);
  Q.out = out;
  hipLaunchKernelGGL(k_knn_query, dim3((unsigned)div_up(div_up(P, 64), 4)), dim3(256), 0, stream, Q);
  return 0;
}

int launch_knn_points(int P, int K, const float* points, float* dists, long long* idx, void* ws, hipStream_t stream) {
  const KnnQuery Q = knn_build_tree(P, points, ws, stream);
  const dim3 grid((unsigned)div_up(div_up(P, 64), 4)), block(256);
  // the next list capacity up: the kernel writes only K columns
  if (K <= 4)
    hipLaunchKernelGGL(k_knn_points<4>, grid, block, 0, stream, Q, K, dists, idx);
  else if (K <= 8)
    hipLaunchKernelGGL(k_knn_points<8>, grid, block, 0, stream, Q, K, dists, idx);
  else if (K <= 16)
    hipLaunchKernelGGL(k_knn_points<16>, grid, block, 0, stream, Q, K, dists, idx);
  else
    hipLaunchKernelGGL(k_knn_points<32>, grid, block, 0, stream, Q, K, dists, idx);
  return 0;
}

}  // namespace gsr
