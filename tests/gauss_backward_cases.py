"""Constructed scenes that put the per-Gaussian stage (k_preprocess of csrc/gsr_preprocess.hip; k_view_grad,
k_gauss_accum and k_gauss_fused of csrc/gsr_backward.hip) on the sizes where its launches and loops change, and the
host decisions of those launches restated in Python.  Shared by the CPU census (tests/test_gauss_backward_cases.py)
and the GPU parity tests (tests/test_gpu_gauss_backward.py).  No GPU code.

launch_plan / preprocess_plan restate launch_gauss_backward / launch_preprocess_kernel; source_constants() parses the
same numbers out of the two .hip files, and the census holds the two equal, so a retune fails there instead of moving
the cases off their edges.  view_grad_owner / accum_block give the index layout of one view group.

Scenes place small Gaussians by index.  A ring of 64 cameras (distance 8, elevation 45 degrees, 40 degree field of
view, looking at the origin) sees a Gaussian 0.5 in front of camera v in view v alone, one further out on the axis
between neighbouring cameras in two or three views, one at the origin in all 64; the rest of the indices lie far above
the ring, behind every camera, and are never listed.  Visibility is a matter of position alone, and what is listed or
receives a gradient is read from the fp64 oracle, never assumed.

The reference of a ring case is the oracle on the sub-scene of the Gaussians some view lists (their order kept, so
equal depths still blend in index order), one view per task through tests/oracle_pool.py, scattered back into rows of
zeros: census() first proves on the whole scene, in both precisions, that every other Gaussian has radius 0 in every
view.  The cases are small and well conditioned, so the slack of gsr_testutil.adjudicate is not available to them:
strict() allows no row beyond max(bar, ROW_RATIO x the fp32 oracle's miss) and no more misses of the bar than the fp32
oracle's own, which the census holds at zero (reference_alone).
"""
from __future__ import annotations

import functools
import math
import os
import pickle
import re

import numpy as np

import oracle
from blend_cases import camera as square_camera, walk
from camera_cases import world_from_view
from gsr_testutil import GRAD_TOL, adjudicate, make_camera, oracle_cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "threestudio-3dgs_amd", "csrc")

# ---- the host decisions, restated ---------------------------------------------------------------------------------
VG_ITEMS = 16                # GSR_VG_ITEMS
VG_MIN_BLOCKS = 1024         # launch_gauss_backward halves items (down to 2) below this many blocks
CUT_LDS_MAX = 48 * 1024      # GSR_CUT_LDS_MAX: bytes of tile cut-offs k_view_grad stages (8 per tile)
PRE_VIEWS = 64               # GSR_PRE_VIEWS
PRE_GAUSS = 128              # GSR_PRE_GAUSS
PRE_LDS_FLOATS = 8 * 1024    # GSR_PRE_LDS_FLOATS
SPLIT_MAX_TILES = 4096       # GSR_SPLIT_MAX_TILES (gsr_common.h split_fits)
CU_LDS_BYTES = 160 * 1024    # GSR_CU_LDS_BYTES
ACCUM_STATIC_LDS = 256 + 16  # k_gauss_accum: s_rl, s_wcnt
SH_STRIDE_EXPR = "((3 * M + 3) & ~3) + 4"


def sh_lds_stride(M):
    return ((3 * M + 3) & ~3) + 4


def _div_up(a, b):
    return -(-a // b)


def launch_plan(V_group, n, tiles, has_sh, two, fused_env=True):
    """launch_gauss_backward for one view group of V_group views over n Gaussians (a range g1 - g0) of an image of
    `tiles` tiles.  fused_env: GSR_GAUSS_FUSED is not "0"."""
    fused = not has_sh and fused_env
    if fused:
        return dict(fused=True, kernel=f"k_gauss_fused<{str(bool(two)).lower()}>", grid=_div_up(n, 256), items=None,
                    cut_in_lds=None)
    cut_in_lds = 8 * tiles <= CUT_LDS_MAX
    items = VG_ITEMS
    while items > 2 and V_group * _div_up(n, 256 * items) < VG_MIN_BLOCKS:
        items >>= 1
    return dict(fused=False, kernel=f"k_view_grad<{str(bool(two)).lower()}, {str(cut_in_lds).lower()}>", items=items,
                cut_in_lds=cut_in_lds, view_grad_grid=V_group * _div_up(n, 256 * items),
                view_grad_lds=(8 * tiles if cut_in_lds else 0) + 4 * 64 * VG_ITEMS * 2, accum_grid=_div_up(n, 256),
                odd_tail=bool(cut_in_lds and tiles & 1), last_slice=n - (_div_up(n, 256 * items) - 1) * 256 * items)


def accum_lds_bytes(M):
    """k_gauss_accum's LDS request with SH rows of M coefficients: dynamic rows plus s_rl and s_wcnt."""
    return 256 * sh_lds_stride(M) * 4 + ACCUM_STATIC_LDS


def max_sh():
    """The largest M whose k_gauss_accum request fits the CU (gsr_backward.hip gauss_backward_max_sh)."""
    M = 1
    while accum_lds_bytes(M + 1) <= CU_LDS_BYTES:
        M += 1
    return M


def preprocess_plan(V, P, M, has_sh):
    """launch_preprocess_kernel: SH staged or not, grid, LDS, the view halves of each block's chunk of views, and the
    number of floats the last block stages (a multiple of 4 only by luck of P and M)."""
    nvc = _div_up(V, PRE_VIEWS)
    want = PRE_GAUSS * (3 * M + 1) if has_sh else 0
    staged = bool(has_sh and M > 0 and want <= PRE_LDS_FLOATS)
    halves = []
    for vc in range(nvc):
        vb, ve = vc * PRE_VIEWS, min(V, (vc + 1) * PRE_VIEWS)
        vh = (ve - vb + 1) // 2
        halves.append(((vb, min(ve, vb + vh)), (vb + vh, ve)))
    rows = P - (_div_up(P, PRE_GAUSS) - 1) * PRE_GAUSS
    return dict(staged=staged, grid=nvc * _div_up(P, PRE_GAUSS), lds=4 * want if staged else 0, halves=halves,
                gauss_per_block=PRE_GAUSS, tail_floats=rows * 3 * M if has_sh else 0)


def split_fits(V, tiles):
    return V >= 1 and tiles > 0 and V * tiles <= SPLIT_MAX_TILES


def tile_bits(tiles):
    return max(1, (tiles - 1).bit_length())


def view_grad_owner(idx, items, g0=0):
    """(slice, wave) of k_view_grad that owns Gaussian idx at `items` per thread: block slice * V + view."""
    local = np.asarray(idx) - g0
    return local // (256 * items), (local % 256) // 64


def accum_block(idx, g0=0):
    return (np.asarray(idx) - g0) // 256


def source_constants():
    """The same numbers parsed from the two .hip files (and gsr_common.h / gsr_kernels.h)."""
    bwd = open(os.path.join(CSRC, "gsr_backward.hip")).read()
    pre = open(os.path.join(CSRC, "gsr_preprocess.hip")).read()
    common = open(os.path.join(CSRC, "gsr_common.h")).read()
    kern = open(os.path.join(CSRC, "gsr_kernels.h")).read()

    def define(src, name):
        m = re.search(rf"^#define\s+{name}\s+(.+?)\s*(?://.*)?$", src, flags=re.M)
        assert m, name
        expr = m.group(1)
        assert re.fullmatch(r"[\d\s\*\(\)\+]+", expr), (name, expr)
        return int(eval(expr))  # noqa: S307  (digits, *, +, parentheses only)

    floor = re.search(r"while \(va\.items > 2 && \(long long\)va\.V \* div_up\(n, 256 \* va\.items\) < (\d+)\) "
                      r"va\.items >>= 1;", bwd)
    stride = re.search(r"int sh_lds_stride\(int M\) \{ return (.+?); \}", bwd)
    want = re.search(r"\(size_t\)GSR_PRE_GAUSS \* \(3 \* a\.M \+ 1\)", pre)
    lists = re.search(r"__shared__ uint16_t s_list\[4\]\[64 \* GSR_VG_ITEMS\];", bwd)
    statics = re.search(r"__shared__ uint8_t s_rl\[256\];\s*__shared__ int s_wcnt\[4\];", bwd)
    assert floor and stride and want and lists and statics
    return dict(VG_ITEMS=define(bwd, "GSR_VG_ITEMS"), VG_MIN_BLOCKS=int(floor.group(1)),
                CUT_LDS_MAX=define(bwd, "GSR_CUT_LDS_MAX"), PRE_VIEWS=define(pre, "GSR_PRE_VIEWS"),
                PRE_GAUSS=define(pre, "GSR_PRE_GAUSS"), PRE_LDS_FLOATS=define(pre, "GSR_PRE_LDS_FLOATS"),
                SPLIT_MAX_TILES=define(common, "GSR_SPLIT_MAX_TILES"), CU_LDS_BYTES=define(kern, "GSR_CU_LDS_BYTES"),
                SH_STRIDE_EXPR=stride.group(1))


# ---- placing Gaussians ---------------------------------------------------------------------------------------------
RING_V = 64
GRAD_KEYS = ("means3D", "opacity", "sh", "scales", "rotations")
COLOR_KEYS = ("means3D", "opacity", "colors", "scales", "rotations")
C0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def ring(W, H=None, V=RING_V):
    H = H or W
    fovx = 2.0 * math.degrees(math.atan(W / H * math.tan(math.radians(20.0))))
    return tuple(make_camera(W, H, fovy_deg=40.0, fovx_deg=fovx, elevation=45.0, azimuth=360.0 * v / V, distance=8.0)
                 for v in range(V))


def project(cams, pts):
    """View depth (V, N) and ndc (V, N, 2) of world points in every camera, fp64."""
    hom = np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1)
    z, ndc = [], []
    for c in cams:
        t = hom @ np.asarray(c["view"], np.float64).reshape(4, 4)
        p = hom @ np.asarray(c["proj"], np.float64).reshape(4, 4)
        z.append(t[:, 2])
        ndc.append(p[:, :2] / (p[:, 3:4] + 1e-7))
    return np.stack(z), np.stack(ndc)


def _view_axes(cam):
    """(ax, ay): ndc = (ax x / z, ay y / z) for a view-space point (x, y, z) of this camera (blend_cases._view_axes
    for any look-at camera: the fp32 matrices of a tilted one leave ~1e-6 off the axes)."""
    z = 2.0
    w = world_from_view(np.array([[1.0, 0.0, z], [0.0, 1.0, z]]), cam)
    p = np.concatenate([w, np.ones((2, 1))], 1) @ np.asarray(cam["proj"], np.float64).reshape(4, 4)
    ndc = p[:, :2] / p[:, 3:4]
    assert abs(ndc[0, 1]) < 1e-4 and abs(ndc[1, 0]) < 1e-4
    return ndc[0, 0] * z, ndc[1, 1] * z


SIGMA_MAX = 2.0  # px, before the 0.75 .. 1.25 anisotropy


def _classify(cams, pts):
    """(inside, outside) (V, N): well inside a view's image in front of it / behind it or outside its image by more
    than the widest footprint (3 sigma of 1.25 SIGMA_MAX, + 2 px)."""
    z, ndc = project(cams, pts)
    far = np.abs(ndc).max(2)
    reach = (3.0 * 1.25 * SIGMA_MAX + 2.0) / (0.5 * min(cams[0]["W"], cams[0]["H"]))
    return (z > 0.4) & (far < 0.78), (z < 0.1) | (far > 1.0 + reach)


def _draw(cams, views, n, rng):
    """n world points seen in exactly `views` (consecutive ring views; () = in none; "all" = in every view)."""
    out = np.zeros((0, 3))
    V = len(cams)
    for _ in range(400):
        m = max(4096, 2 * n)
        if views == "all":
            pts = rng.uniform(-0.25, 0.25, size=(m, 3))
        elif len(views) == 0:
            pts = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(20, 30, m)], 1)
        else:
            mid = cams[views[len(views) // 2]]
            ax, ay = _view_axes(mid)
            zz = rng.uniform(0.5, 0.7, m) if len(views) == 1 else rng.uniform(0.9, 2.6, m)
            nx = rng.uniform(-0.7, 0.7, m) if len(views) != 3 else rng.uniform(-0.2, 0.2, m)
            pts = world_from_view(np.stack([nx / ax * zz, rng.uniform(-0.7, 0.7, m) / ay * zz, zz], 1), mid)
        inside, outside = _classify(cams, pts)
        want = np.ones(V, bool) if views == "all" else np.isin(np.arange(V), np.asarray(views, np.int64))
        ok = (inside[want].all(0) if want.any() else True) & outside[~want].all(0)
        out = np.concatenate([out, pts[ok]])
        if out.shape[0] >= n:
            return out[:n]
    raise AssertionError(f"no {n} points for views {views}")


def _focal(cam):
    return 0.5 * cam["H"] / cam["tany"]


def _fill(cams, P, groups, seed, M=16, deg=3, sigma=(1.4, SIGMA_MAX), opacity=(0.15, 0.45)):
    """A ring scene of P Gaussians: groups = [(indices, views)], every other index hidden above the ring."""
    rng = np.random.default_rng(seed)
    pos = _draw(cams, (), P, rng)
    depth = np.full(P, 1.0)
    kind = {}
    merged = {}
    for idx, views in groups:
        merged.setdefault(views, []).extend(idx)
    # the ring is symmetric about the z axis: views (a, a + 1, ..) are views (0, 1, ..) turned by a steps
    count = {}
    for views, idx in merged.items():
        base = views if isinstance(views, str) else len(views)
        count[base] = count.get(base, 0) + len(idx)
    pool = {b: _draw(cams, b if isinstance(b, str) else tuple(range(b)), n, rng) for b, n in count.items()}
    for views, idx in merged.items():
        idx = np.asarray(idx, np.int64)
        base = views if isinstance(views, str) else len(views)
        pts, pool[base] = pool[base][:idx.size], pool[base][idx.size:]
        if not isinstance(views, str):
            a = 2.0 * math.pi * views[0] / len(cams)
            pts = pts @ np.array([[math.cos(a), math.sin(a), 0.0], [-math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        pos[idx] = pts
        ref = cams[0] if views == "all" else cams[views[len(views) // 2]]
        depth[idx] = project([ref], pos[idx])[0][0]
        for i in idx:
            kind[int(i)] = views
    s = rng.uniform(*sigma, P) * depth / _focal(cams[0])
    q = rng.normal(size=(P, 4))
    sh = np.zeros((P, M, 3))
    sh[:, 0, :] = (rng.random((P, 3)) - 0.5) / C0
    sh[:, 1:, :] = rng.normal(0.0, 0.1, size=(P, M - 1, 3))
    scene = dict(means3D=pos.astype(np.float32),
                 scales=(s[:, None] * rng.uniform(0.75, 1.25, size=(P, 3))).astype(np.float32),
                 rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                 opacities=rng.uniform(*opacity, size=(P, 1)).astype(np.float32), shs=sh.astype(np.float32),
                 sh_degree=deg)
    return scene, kind


# (The large one-view images place a centre to ~1e-4 px in fp32 and get the same scale.)
# A Gaussian seen by one camera of the ring alone sits at a depth of ~0.07 of the ring's radius (closer neighbours
# would see it too), so fp32 places its centre to ~3e-5 px and its gradients, of order 10 to 1000 with unit upstream
# gradients, to ~1e-4 in their small components: the fp32 oracle then misses the absolute bar on rows it has right
# to 1e-5 of their size.  The ring cases scale the upstream gradients instead, so that the screen-space gradients are
# of order 0.1: two decades above the bar, and the reference's own error two decades below it.
UPSTREAM_SCALE = 0.02


def _ups(V, H, W, seed):
    from gsr_synthetic import upstream_grads

    return [tuple((UPSTREAM_SCALE * g).astype(np.float32) for g in upstream_grads(H, W, seed=seed + v))
            for v in range(V)]


def _bgs(V, seed):
    return np.random.default_rng(seed).random((V, 3)).astype(np.float32).tolist()


ITEMS_P = {2: 12_000, 4: 20_000, 8: 40_000, 16: 70_000}
ITEMS_SEED = {2: 121, 4: 140, 8: 180, 16: 264}  # (no fp32 / fp64 decision flips at these)


@functools.lru_cache(maxsize=None)
def items_case(items, seed=None):
    """64 views of 32 x 32, P so that one group of 64 views runs `items` per thread with a partial last slice.  Every
    97th index (97 is prime to 256: every lane and every item slot of a thread) and the last two are seen in one
    view of the ring in turn, every tenth of those in all 64."""
    P = ITEMS_P[items]
    cams = ring(32)
    seen = sorted(set(range(0, P, 97)) | {P - 2, P - 1})
    groups = [([i], "all" if k % 10 == 9 else (k % RING_V,)) for k, i in enumerate(seen)]
    scene, kind = _fill(cams, P, groups, seed=ITEMS_SEED[items] if seed is None else seed, opacity=(0.1, 0.3))
    return dict(name=f"items-{items}", scene=scene, cams=cams, bgs=_bgs(RING_V, items), ups=_ups(RING_V, 32, 32, 1000),
                kind=kind, P=P, items=items)


REACH_P = 2700
REACH_SEED = 11  # (as ITEMS_SEED)
REACH_GROUPS = (  # (first index, count, views)
    (0, 64, (0,)), (64, 64, (63,)), (128, 64, (0, 1)), (192, 64, (0, 1, 2)),  # accum block 0: all 256 reached
    (256, 64, (0,)), (320, 5, (63,)), (448, 3, "all"),                        # block 1: partial
    (768, 3, (63,)), (771, 3, (0,)),                                          # block 2 none; block 3 a few
    (2690, 10, "all"))                                                        # the last, partial block


@functools.lru_cache(maxsize=None)
def reach_case(seed=None):
    """64 views of 48 x 48, P = 2700 (items 2: a wave of k_view_grad owns indices 64 w + {0 .. 63} and 256 more).
    View 0 lists 128 Gaussians of slice 0's wave 0 (two rounds: the prefetch reload), 64 of waves 2 and 3, none of
    wave 1; view 5 lists 3 of wave 3 and none elsewhere.  Accum block 0 has every row reached, block 2 none.  View
    sets {0}, {63}, {0, 1}, {0, 1, 2} and all 64; with one view per group, {0} is first-group-only and {63}
    last-group-only."""
    cams = ring(48)
    groups = [(range(a, a + n), views) for a, n, views in REACH_GROUPS]
    scene, kind = _fill(cams, REACH_P, groups, seed=REACH_SEED if seed is None else seed)
    return dict(name="reach", scene=scene, cams=cams, bgs=_bgs(RING_V, 3), ups=_ups(RING_V, 48, 48, 2000), kind=kind,
                P=REACH_P, items=2)


def precomp(case):
    """The case with colors_precomp = SH2RGB of its DC coefficients instead of SHs (the fused kernel's launches)."""
    scene = dict(case["scene"])
    scene["colors_precomp"] = (scene.pop("shs")[:, 0, :] * np.float32(C0) + np.float32(0.5)).astype(np.float32)
    return dict(case, scene=scene, name=case["name"] + "-colors")


def scene_of_spec(spec):
    """What oracle_pool.scene_of builds in a worker for ("gauss_backward", case name, pickled sub-scene): the scene
    reference() sent, so a worker neither rebuilds the case nor repeats its census."""
    return pickle.loads(spec[2])


def sub_scene(scene, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in scene.items()}


_CENSUS = {}


def placed(case):
    """(V, P) bool: the views each Gaussian was placed for."""
    V = len(case["cams"])
    out = np.zeros((V, case["P"]), bool)
    for i, views in case["kind"].items():
        out[:, i] = True if views == "all" else np.isin(np.arange(V), np.asarray(views, np.int64))
    return out


def census(case):
    """Per view, on the whole scene: tiles (V, P) of the fp64 preprocess, and `listed` = the Gaussians with a tile
    in some view.  Asserts that in both precisions every other Gaussian has radius 0 in every view."""
    key = case["name"].replace("-colors", "")
    if key not in _CENSUS:
        P, cams = case["P"], case["cams"]
        tiles = np.zeros((len(cams), P), np.int64)
        for v, cam in enumerate(cams):
            a64 = oracle.gauss_aux(case["scene"], oracle_cam(cam), "f64")
            a32 = oracle.gauss_aux(case["scene"], oracle_cam(cam), "f32")
            assert np.array_equal(a64["tiles"] > 0, a32["tiles"] > 0), v
            tiles[v] = a64["tiles"]
        _CENSUS[key] = dict(tiles=tiles, listed=np.nonzero((tiles > 0).any(0))[0])
    return _CENSUS[key]


_REFS = {}


def reference(case):
    """(views, total, rows) of a ring case, once per process, in the rows of the sub-scene (`rows`: their indices in
    the whole scene): views[v] is a run_oracle-shaped dict of view v (f32, f64, aux64, aux32, W, H and b32 / b32r /
    b64 with the view's means2D rows), total the parameter gradients summed over the views in fp64 (b32, b32r, b64).
    Every other row of the whole scene is zero: never listed."""
    import oracle_pool

    if case["name"] not in _REFS:
        rows = census(case)["listed"]
        spec = ("gauss_backward", case["name"], pickle.dumps(sub_scene(case["scene"], rows)))
        tasks = [(spec, cam, bg, up, None, None, ("f32r", "aux32"))
                 for cam, bg, up in zip(case["cams"], case["bgs"], case["ups"])]
        views, tot = oracle_pool.views_and_sums(tasks, keep_views=True)
        for r in views:
            b = r.pop("b")
            for tag, name in (("f32", "b32"), ("f32r", "b32r"), ("f64", "b64")):
                r[name] = dict(means2D=b[tag]["means2D"])
        total = {name: dict(tot[tag]) for tag, name in (("f32", "b32"), ("f32r", "b32r"), ("f64", "b64"))}
        _REFS[case["name"]] = (views, total, rows)
    return _REFS[case["name"]]


def contributed(case):
    """(V, P) bool: the fp64 oracle gives Gaussian i a gradient in view v (a nonzero means2D row)."""
    views, _, rows = reference(case)
    out = np.zeros((len(views), case["P"]), bool)
    out[:, rows] = np.stack([(np.asarray(r["b64"]["means2D"]) != 0).any(1) for r in views])
    return out


# ---- one-view cases --------------------------------------------------------------------------------------------------
def _place(cam, u, v, z, sigma, rng, M, deg, opacity):
    n = len(u)
    ax, ay = _view_axes(cam)
    ndc = np.stack([(2.0 * u + 1.0) / cam["W"] - 1.0, (2.0 * v + 1.0) / cam["H"] - 1.0], 1)
    t = np.stack([ndc[:, 0] / ax * z, ndc[:, 1] / ay * z, z], 1)
    q = rng.normal(size=(n, 4))
    sh = rng.normal(0.0, 0.1, size=(n, M, 3))
    sh[:, 0, :] = (rng.random((n, 3)) - 0.5) / C0
    return dict(means3D=world_from_view(t, cam).astype(np.float32),
                scales=((sigma * z / _focal(cam))[:, None] * rng.uniform(0.75, 1.25, size=(n, 3))).astype(np.float32),
                rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                opacities=np.asarray(opacity, np.float64).reshape(n, 1).astype(np.float32), shs=sh.astype(np.float32),
                sh_degree=deg)


TILE_SIZES = {1: (16, 16), 63: (112, 144), 4160: (1040, 1024), 6300: (1600, 1008)}
# (seeds at which no pixel's alpha or T test lies close enough to its threshold for the fp32 and fp64 oracles to part)
TILE_SEEDS = {1: 1, 63: 63, 4160: 4162, 6300: 6309}


@functools.lru_cache(maxsize=None)
def tiles_case(tiles, n=300, seed=None):
    """One view of W x H = `tiles` tiles, n Gaussians over the whole image, the first four in the corner tiles (the
    last tile's cut-off is the odd tail of the LDS staging)."""
    from gsr_synthetic import upstream_grads

    W, H = TILE_SIZES[tiles]
    assert _div_up(W, 16) * _div_up(H, 16) == tiles
    cam = square_camera(W, H)
    rng = np.random.default_rng(TILE_SEEDS[tiles] if seed is None else seed)
    n = min(n, 40) if tiles == 1 else n
    u, v = rng.uniform(2, W - 3, n), rng.uniform(2, H - 3, n)
    c = min(4, n)
    u[:c] = np.array([5.0, W - 6.0, 5.0, W - 6.0])[:c] + rng.uniform(-1, 1, c)
    v[:c] = np.array([5.0, 5.0, H - 6.0, H - 6.0])[:c] + rng.uniform(-1, 1, c)
    sigma = rng.uniform(3.0, 8.0, n) if tiles > 63 else rng.uniform(1.5, 4.0, n)
    scene = _place(cam, u, v, rng.uniform(2.0, 3.0, n), sigma, rng, 16, 3, rng.uniform(0.2, 0.6, n))
    return dict(name=f"tiles-{tiles}", scene=scene, cams=(cam,), bgs=[[0.3, 0.2, 0.1]],
                ups=[tuple((_wide_scale(cam) * g).astype(np.float32) for g in upstream_grads(H, W, seed=tiles))], P=n,
                tiles=tiles)


def _wide_scale(cam):
    """UPSTREAM_SCALE, smaller for wide images: the screen-space gradient is per ndc unit (x W / 2) and fp32 places
    a centre to ~6e-8 W px."""
    return min(UPSTREAM_SCALE, 1.0 / max(cam["W"], cam["H"]))


def two_view(case):
    """The one-view case twice (other background and upstream gradients in the second view) with second colours."""
    from gsr_synthetic import upstream_grads

    cam = case["cams"][0]
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(case["P"], 3))
    up2 = [(_wide_scale(cam) * rng.standard_normal((3, cam["H"], cam["W"]))).astype(np.float32) for _ in range(2)]
    return dict(case, name=case["name"] + "-two", cams=(cam, cam), bgs=[case["bgs"][0], [0.9, 0.1, 0.5]],
                ups=[case["ups"][0], tuple((_wide_scale(cam) * g).astype(np.float32)
                                           for g in upstream_grads(cam["H"], cam["W"], seed=77))],
                colors2=(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32), ups2=up2)


SH_CASES = [(M, P) for M in (1, 9) for P in (1, 2, 3, 129, 131)] + [(4, 131), (16, 131), (25, 131), (25, 300)]


@functools.lru_cache(maxsize=None)
def sh_case(M, P):
    """P Gaussians with SH rows of M coefficients (every one nonzero) at sh_degree = min(3, sqrt(M) - 1), 48 x 40."""
    from gsr_synthetic import upstream_grads

    cam = square_camera(48, 40)
    rng = np.random.default_rng(100 * M + P)
    deg = min(3, int(round(math.sqrt(M))) - 1)
    scene = _place(cam, rng.uniform(3, 44, P), rng.uniform(3, 36, P), rng.uniform(2.0, 3.0, P), rng.uniform(1.5, 3.0, P),
                   rng, M, deg, rng.uniform(0.1, 0.35, P))
    return dict(name=f"sh-{M}-{P}", scene=scene, cams=(cam,), bgs=[[0.2, 0.4, 0.6]],
                ups=[upstream_grads(40, 48, seed=M + P)], P=P, M=M)


EMPTY_AT = 11


@functools.lru_cache(maxsize=None)
def empty_case():
    """One 16 x 16 tile, 24 Gaussians; the one at list position EMPTY_AT sits between four pixel centres with opacity
    0.0042: its alpha >= 1 / 255 ellipse (radius ~0.2 px) lies inside the tile, so the tile lists it, but at every
    pixel centre alpha <= 0.83 x 0.0042 < 1 / 255.  Its SH row clamps all three channels."""
    from gsr_synthetic import upstream_grads

    cam = square_camera(16, 16)
    rng = np.random.default_rng(41)
    n = 24
    u, v = rng.uniform(2, 13, n), rng.uniform(2, 13, n)
    sigma, op = rng.uniform(1.2, 2.5, n), rng.uniform(0.2, 0.5, n)
    u[EMPTY_AT], v[EMPTY_AT], sigma[EMPTY_AT], op[EMPTY_AT] = 7.5, 8.5, 1.0, 0.0042
    scene = _place(cam, u, v, 2.0 + np.arange(n) / 64.0, sigma, rng, 16, 3, op)
    scene["scales"][EMPTY_AT] = np.float32(1.0 * (2.0 + EMPTY_AT / 64.0) / _focal(cam))
    scene["shs"][EMPTY_AT] = 0.0
    scene["shs"][EMPTY_AT, 0, :] = -3.0
    return dict(name="empty", scene=scene, cams=(cam,), bgs=[[0.3, 0.2, 0.1]], ups=[upstream_grads(16, 16, seed=9)],
                P=n, empty=EMPTY_AT)


def empty_walk(case):
    """(walk of the tile over the fp64 preprocess, aux64, list position of the empty Gaussian)."""
    aux = oracle.gauss_aux(case["scene"], oracle_cam(case["cams"][0]), "f64")
    w = walk(aux, 16, 16, 0)
    return w, aux, int(np.nonzero(w["order"] == case["empty"])[0][0])


_ONE = {}


def reference_one(case, v=0):
    """run_oracle of view v of a one-view (or same-camera two-view) case, once per process."""
    from gsr_testutil import run_oracle

    key = (case["name"], v)
    if key not in _ONE:
        _ONE[key] = run_oracle(case["scene"], case["cams"][v], case["bgs"][v], grads=case["ups"][v])
    return _ONE[key]


# ---- the zero-slack rule ---------------------------------------------------------------------------------------------
def bar_of(r64):
    return GRAD_TOL * np.maximum(1.0, np.abs(np.asarray(r64, np.float64)))


def reference_alone(b32, b32r, b64, keys, what):
    """The fp32 oracle against the fp64 oracle under adjudicate: {key: stats}; the census asserts f32_miss == 0 and
    null_beyond == 0 for each."""
    return {k: adjudicate(b32[k], b32[k], b64[k], bar_of(b64[k]), what, "reference " + k, rowwise=True, r32b=b32r[k])
            for k in keys}


def strict(stats, what):
    """No slack: no row beyond max(bar, ROW_RATIO x the fp32 oracle's miss), no more bar misses than the fp32 oracle."""
    bad = [f"{what}: {k}: {st}" for k, st in stats.items() if st["beyond_ratio"] != 0 or st["gpu_miss"] > st["f32_miss"]]
    assert not bad, "\n".join(bad)
