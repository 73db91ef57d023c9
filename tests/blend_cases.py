"""Constructed one-tile scenes that put the length of a tile's depth-sorted list, or the position where its
pixels stop blending, on the sizes the blend kernels of csrc/gsr_render.hip walk in: staged batches of 64
candidates, groups of 8 per matrix-core product, split-backward chunks of GSR_SPLIT_CH = 256 with
GSR_SPLIT_NCK = 15 boundaries, and the GSR_HCAP_TW = 256 entry hit list of the two-colour backward.  Shared by
the CPU census (tests/test_blend_cases.py) and the GPU parity tests (tests/test_gpu_blend_lengths.py).  No GPU
code.

A case is (scene, cam, bg, upstream grads, meta).  The image is 16 x 16 (one tile, four 8 x 8 quadrants), so
every visible Gaussian is exactly one list entry; Gaussians are laid out in the camera space of
make_camera(16, 16, elevation=0, azimuth=0) and mapped back through the inverse view matrix.  Depths are
2 + i / 8192 for list position i (exact in fp32, distinct depth keys), rotations identity, SH degree 0.

  sparse(L)           L - 1 faint specks (sigma ~1 px, opacity U(0.02, 0.2) scaled by 256 / L beyond 256 and kept
                      at or above 2 / 255) and, at position L - 1, one faint veil that covers the tile: no pixel
                      finishes (accumulated alpha < 0.99), every quadrant's deepest blend is position L - 1
                      (quad_maxc == L), every batch, group and chunk is walked
  cut(L, c)           specks at [0, c - 13), 13 walls (sigma 60 px, opacity 0.4) at [c - 13, c) that every pixel
                      blends, one wall of opacity 1 at position c that ends every pixel without being blended
                      (T (1 - alpha) < 1e-4), specks that are never blended up to L: quad_maxc == c everywhere.
                      (With walls of opacity 0.5 the wall that drops T (1 - alpha) below 1e-4 is the one that is
                      *not* blended, and the specks in front move T by more than the 22 % between 2^-13 and 1e-4:
                      the walls are fainter and the closing wall opaque, which leaves two decades of room.)
  quadrant_cut(L, c)  as cut, but 13 narrow walls (sigma 2.5 px) centred in quadrant 0 at [c - 13, c), and every
                      later Gaussian (the last one included, a blob in the far corner) stays below alpha 1 / 255
                      on quadrant 0: quadrant 0's deepest blend is c - 1, the others walk all L
  hitcap(kind)        one batch of 64: two walls and the veil hit all 64 lanes of each quadrant, specks of
                      sigma 0.6 px a few; the fullest quadrant's hit count (the fill of k_render_bwd_tw's hit list
                      when the batch ends) is exactly 256 ("at": never flushed early) or 257 ("over")
  ragged(...)         sparse(257) / cut(557, 257) in the second tile of a 24 x 16 image, whose right half
                      (quadrants 1 and 3) lies outside the image

`walk` restates the per-pixel blend over oracle.gauss_aux(..., "f64") (the alpha formula of
gsr_testutil.flip_dependents).  Boundary rows are the Gaussians at list positions 0, L - 1, 64 k - 1, 64 k,
256 k - 1 and 256 k (k <= 16); the builders re-draw the centre of a boundary Gaussian (and of no other) until at
every pixel its alpha is 5 % away from 1 / 255 and its T (1 - alpha) 5 % away from 1e-4, so its own blend cannot
flip between two correct fp32 evaluations.  Seeds are fixed: the cases are deterministic.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle
from camera_cases import world_from_view
from gsr_testutil import make_camera, oracle_cam

ALPHA_MIN = 1.0 / 255.0
T_EPS = 1e-4
MARGIN = 0.05
CH, NCK, BATCH, HCAP = 256, 15, 64, 256  # GSR_SPLIT_CH, GSR_SPLIT_NCK, the staged batch, GSR_HCAP_TW

SPARSE_L = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 3839, 3840, 3841, 4095, 4096,
            4097, 4400)
CUT_C = (63, 64, 65, 255, 256, 257, 511, 512, 513, 3840, 3841)
QUADRANT_CUT_C = (256, 257, 300)
TWO_COLOUR_SPARSE_L = (63, 64, 65, 255, 256, 257)
N_WALLS = 13


def camera(W=16, H=16):
    """Square pixels at any width: fovy 60 deg, tan(fovx / 2) = W / H tan(fovy / 2)."""
    fovx = 2.0 * math.degrees(math.atan(W / H * math.tan(math.radians(30.0))))
    return make_camera(W, H, fovy_deg=60.0, fovx_deg=fovx, elevation=0.0, azimuth=0.0)


def _view_axes(cam):
    """(ax, ay): ndc = (ax x / z, ay y / z) for a view-space point (x, y, z) of this camera."""
    z = 2.0
    w = world_from_view(np.array([[1.0, 0.0, z], [0.0, 1.0, z]]), cam)
    p = np.concatenate([w, np.ones((2, 1))], 1) @ np.asarray(cam["proj"], np.float64).reshape(4, 4)
    ndc = p[:, :2] / p[:, 3:4]
    assert abs(ndc[0, 1]) < 1e-6 and abs(ndc[1, 0]) < 1e-6
    return ndc[0, 0] * z, ndc[1, 1] * z


def assemble(lay, cam, seed):
    """lay = dict(u, v: centre in pixels; sigma: footprint in pixels; opacity; one entry per list position)."""
    n = lay["u"].shape[0]
    W, H = cam["W"], cam["H"]
    ax, ay = _view_axes(cam)
    z = 2.0 + np.arange(n, dtype=np.float64) / 8192.0
    assert z[-1] <= 3.0
    ndc = np.stack([(2.0 * lay["u"] + 1.0) / W - 1.0, (2.0 * lay["v"] + 1.0) / H - 1.0], 1)
    t = np.stack([ndc[:, 0] / ax * z, ndc[:, 1] / ay * z, z], 1)
    focal = 0.5 * H / cam["tany"]
    rng = np.random.default_rng(seed + 7919)
    return dict(means3D=world_from_view(t, cam).astype(np.float32),
                scales=np.repeat((lay["sigma"] * z / focal)[:, None], 3, 1).astype(np.float32),
                rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1)),
                opacities=lay["opacity"][:, None].astype(np.float32),
                shs=rng.uniform(-1.0, 1.0, size=(n, 1, 3)).astype(np.float32), sh_degree=0)


def walk(aux, W, H, tile=0):
    """The reference's per-pixel blend of one tile's list, in fp64, over gauss_aux values.  Returns dict(order:
    Gaussian at each list position; last (256,): 1 + list position of each pixel's last contributor (0: none;
    row-major 16 x 16, pixels outside the image 0); quad (4,): its maximum per quadrant; final_alpha (256,);
    alpha, test (n, 256): each candidate's alpha and T (1 - alpha) where the walk evaluated it, nan elsewhere;
    hits (batches, 4): per batch of 64 counted back from the tile's deepest blend (as the backward stages them)
    and quadrant, the blends; fragile (4,): a quadrant whose deepest blend could move under a 5 % change of an
    alpha or a T (1 - alpha))."""
    gx = (W + 15) // 16
    tx, ty = tile % gx, tile // gx
    r = aux["rect"]
    cand = np.nonzero((aux["tiles"] > 0) & (r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3]))[0]
    order = cand[np.argsort(aux["depth"][cand], kind="stable")]
    n = order.shape[0]
    yy, xx = np.divmod(np.arange(256), 16)
    px, py = tx * 16 + xx, ty * 16 + yy
    inside = (px < W) & (py < H)
    quad_of = (yy >= 8) * 2 + (xx >= 8)
    dx = aux["px"][order][:, None] - px[None, :]
    dy = aux["py"][order][:, None] - py[None, :]
    con = aux["conic"][order]
    power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
    alpha = np.minimum(0.99, aux["opacity"][order][:, None] * np.exp(np.minimum(power, 0.0)))
    ok = (power <= 0) & (alpha >= ALPHA_MIN)
    T = np.ones(256)
    done = ~inside
    last = np.zeros(256, np.int64)
    blend = np.zeros((n, 256), bool)
    a_seen = np.full((n, 256), np.nan)
    t_seen = np.full((n, 256), np.nan)
    for i in range(n):
        live = ~done
        test = T * (1.0 - alpha[i])
        a_seen[i, live & (power[i] <= 0)] = alpha[i, live & (power[i] <= 0)]
        t_seen[i, live & ok[i]] = test[live & ok[i]]
        term = live & ok[i] & (test < T_EPS)
        b = live & ok[i] & ~term
        T = np.where(b, test, T)
        last[b] = i + 1
        blend[i] = b
        done |= term
    quad = np.array([last[quad_of == q].max() for q in range(4)])
    hi = int(quad.max())
    nb = (hi + BATCH - 1) // BATCH
    hits = np.zeros((nb, 4), np.int64)
    for b in range(nb):
        lo_b, hi_b = max(hi - BATCH * (b + 1), 0), hi - BATCH * b
        for q in range(4):
            hits[b, q] = int(blend[lo_b:hi_b][:, quad_of == q].sum())
    near_a = np.abs(a_seen / ALPHA_MIN - 1.0) < MARGIN
    near_t = np.abs(t_seen / T_EPS - 1.0) < MARGIN
    pos = np.arange(n)[:, None]
    fragile = np.array([bool(near_t[:, quad_of == q].any() or (near_a[:, quad_of == q] & (pos >= quad[q] - 1)).any())
                        for q in range(4)])
    return dict(order=order, last=last, quad=quad, final_alpha=np.where(inside, 1.0 - T, 0.0), alpha=a_seen,
                test=t_seen, hits=hits, fragile=fragile, n=n)


def boundary_positions(L):
    """{list position: kinds} of the rows an off-by-one touches first: "end" (0 and L - 1), "e64" (64 k - 1, 64 k),
    "e256" (256 k - 1, 256 k, k <= 16)."""
    out = {}

    def add(p, kind):
        if 0 <= p < L:
            out.setdefault(p, set()).add(kind)

    add(0, "end")
    add(L - 1, "end")
    for k in range(1, L // BATCH + 2):
        add(BATCH * k - 1, "e64")
        add(BATCH * k, "e64")
    for k in range(1, 17):
        add(CH * k - 1, "e256")
        add(CH * k, "e256")
    return out


def _margins_ok(w, positions):
    """Per given list position: alpha 5 % away from 1 / 255 and T (1 - alpha) 5 % away from 1e-4 at every pixel
    where the walk evaluated them."""
    a, t = w["alpha"][positions], w["test"][positions]
    bad = (np.abs(a / ALPHA_MIN - 1.0) < MARGIN) | (np.abs(t / T_EPS - 1.0) < MARGIN)
    return ~bad.any(1)


def _finish(lay, cam, seed, tile, redraw, must_blend=True):
    """Assemble, walk, and re-draw the centres of the list positions `redraw(walk)` names (the boundary rows) until
    their margins hold (and, with must_blend, each blends at least one pixel)."""
    rng = np.random.default_rng(seed + 104729)
    oc = oracle_cam(cam)
    for _ in range(200):
        scene = assemble(lay, cam, seed)
        aux = oracle.gauss_aux(scene, oc, "f64")
        w = walk(aux, cam["W"], cam["H"], tile)
        pos = np.array(sorted(redraw(w)), np.int64)
        pos = pos[pos < w["n"]]
        ok = _margins_ok(w, pos)
        if must_blend:
            ok &= np.isfinite(w["test"][pos]).any(1) | ~lay["free"][w["order"][pos]]
        bad = w["order"][pos[~ok]]
        if bad.size == 0:
            return scene, aux, w
        assert lay["free"][bad].all(), "a wall or veil misses its margins"  # (wide: they hold by construction)
        lo, hi = lay["box"]
        lay["u"][bad] = rng.uniform(lo[0], hi[0], bad.size)
        lay["v"][bad] = rng.uniform(lo[1], hi[1], bad.size)
    raise AssertionError("margins not reached")


def _specks(rng, n, box, op_scale, sigma=(0.8, 1.3), op=(0.02, 0.2)):
    lo, hi = box
    return dict(u=rng.uniform(lo[0], hi[0], n), v=rng.uniform(lo[1], hi[1], n), sigma=rng.uniform(*sigma, n),
                opacity=np.maximum(2.0 / 255.0, rng.uniform(*op, n) * op_scale))


def _cat(parts, box):
    lay = {k: np.concatenate([p[k] for p in parts]) for k in ("u", "v", "sigma", "opacity")}
    lay["free"] = np.concatenate([np.full(p["u"].shape[0], p.get("free", True)) for p in parts])
    lay["box"] = box
    return lay


def _wide(rng, n, centre, sigma, opacity, jitter=1.0):
    return dict(u=centre[0] + rng.uniform(-jitter, jitter, n), v=centre[1] + rng.uniform(-jitter, jitter, n),
                sigma=np.full(n, float(sigma)), opacity=np.full(n, float(opacity)), free=False)


def _geometry(W, tile):
    """(camera, box of speck centres, tile centre): centres within 0.8 of the tile's half extent (and of the
    image's, where the tile overhangs it)."""
    cam = camera(W, 16)
    x0 = 16.0 * tile
    x1 = min(x0 + 16.0, float(W))
    cx = 0.5 * (x0 + x1) - 0.5
    hw = 0.4 * (x1 - x0)
    return cam, ((cx - hw, 7.5 - 6.4), (cx + hw, 7.5 + 6.4)), (cx, 7.5)


def _case(name, scene, cam, aux, w, seed, tile, meta):
    from gsr_synthetic import upstream_grads

    bpos = boundary_positions(w["n"])
    meta = dict(meta, name=name, tile=tile, n=w["n"], quad=w["quad"].copy(), fragile=w["fragile"].copy(),
                hits=w["hits"].copy(), order=w["order"], boundary={int(w["order"][p]): k for p, k in bpos.items()},
                boundary_pos=bpos, max_alpha=float(w["final_alpha"].max()))
    bg = [0.3, 0.2, 0.1]
    return scene, cam, bg, upstream_grads(cam["H"], cam["W"], seed=seed + 3), meta


@functools.lru_cache(maxsize=None)
def sparse(L, seed=1, W=16, tile=0):
    cam, box, centre = _geometry(W, tile)
    rng = np.random.default_rng(1000 * seed + L)
    parts = [_specks(rng, L - 1, box, min(1.0, 256.0 / L)), _wide(rng, 1, centre, 60.0, 0.03)]
    scene, aux, w = _finish(_cat(parts, box), cam, seed, tile, lambda w: boundary_positions(w["n"]))
    return _case(f"sparse({L})" + ("" if W == 16 else " ragged"), scene, cam, aux, w, seed, tile,
                 dict(family="sparse", L=L, expect_quad=L))


def _cut_layout(rng, L, c, box, centre, wall_sigma, wall_centre, tail):
    front = c - N_WALLS
    assert front >= 0 and L > c + 1
    parts = [_specks(rng, front, box, min(1.0, 128.0 / max(front, 1))),
             _wide(rng, N_WALLS, wall_centre, wall_sigma, 0.4)]
    return parts + tail


@functools.lru_cache(maxsize=None)
def cut(L, c, seed=2, W=16, tile=0):
    assert L >= c + 2
    cam, box, centre = _geometry(W, tile)
    rng = np.random.default_rng(1000 * seed + c)
    tail = [_wide(rng, 1, centre, 60.0, 1.0), _specks(rng, L - c - 1, box, 1.0)]
    lay = _cat(_cut_layout(rng, L, c, box, centre, 60.0, centre, tail), box)
    # (the never-blended specks behind the closing wall have nothing to keep a margin from)
    scene, aux, w = _finish(lay, cam, seed, tile, lambda w: [p for p in boundary_positions(w["n"]) if p < c],
                            must_blend=True)
    return _case(f"cut({L}, {c})" + ("" if W == 16 else " ragged"), scene, cam, aux, w, seed, tile,
                 dict(family="cut", L=L, c=c, expect_quad=c))


@functools.lru_cache(maxsize=None)
def quadrant_cut(L, c, seed=3):
    cam, box, centre = _geometry(16, 0)
    rng = np.random.default_rng(1000 * seed + c)

    def away(r, n):  # centres at least 3.5 px from quadrant 0 (pixels 0..7 in both axes)
        u, v = r.uniform(1.1, 14.4, n), r.uniform(1.1, 14.4, n)
        flip = (u < 11.0) & (v < 11.0)
        pick = r.random(n) < 0.5
        u = np.where(flip & pick, r.uniform(11.0, 14.4, n), u)
        v = np.where(flip & ~pick, r.uniform(11.0, 14.4, n), v)
        return u, v

    n_tail = L - c - 1
    tu, tv = away(rng, n_tail)
    tail_specks = _specks(rng, n_tail, box, min(1.0, 128.0 / n_tail))
    tail_specks["u"], tail_specks["v"] = tu, tv
    blob = _wide(rng, 1, (13.0, 13.0), 4.0, 0.02, jitter=0.0)  # reaches quadrants 1, 2, 3, not 0
    lay = _cat(_cut_layout(rng, L, c, box, centre, 2.5, (3.5, 3.5), [tail_specks, blob]), box)
    front = c - N_WALLS
    # boundary rows in front of the walls are re-drawn anywhere, narrow walls about their centre, the specks
    # behind them away from quadrant 0
    oc = oracle_cam(cam)
    rr = np.random.default_rng(seed + 104729)
    for _ in range(200):
        scene = assemble(lay, cam, seed)
        aux = oracle.gauss_aux(scene, oc, "f64")
        w = walk(aux, 16, 16, 0)
        pos = np.array(sorted(boundary_positions(w["n"])), np.int64)
        ok = _margins_ok(w, pos) & (np.isfinite(w["test"][pos]).any(1) | ~lay["free"][w["order"][pos]])
        bad = w["order"][pos[~ok]]
        if bad.size == 0:
            break
        assert (bad < L - 1).all(), "the closing blob misses its margins"
        fr = bad[bad < front]
        lay["u"][fr], lay["v"][fr] = rr.uniform(box[0][0], box[1][0], fr.size), rr.uniform(box[0][1], box[1][1], fr.size)
        wl = bad[(bad >= front) & (bad < c)]
        lay["u"][wl], lay["v"][wl] = 3.5 + rr.uniform(-1.0, 1.0, wl.size), 3.5 + rr.uniform(-1.0, 1.0, wl.size)
        bk = bad[bad >= c]
        lay["u"][bk], lay["v"][bk] = away(rr, bk.size)
    else:
        raise AssertionError("margins not reached")
    return _case(f"quadrant_cut({L}, {c})", scene, cam, aux, w, seed, 0,
                 dict(family="quadrant_cut", L=L, c=c, expect_quad=(c, L, L, L)))


@functools.lru_cache(maxsize=None)
def hitcap(kind, seed=4):
    """64 candidates = one batch; the fullest quadrant's hits are HCAP ("at") or HCAP + 1 ("over")."""
    target = HCAP + (1 if kind == "over" else 0)
    cam, box, centre = _geometry(16, 0)
    L = BATCH
    for attempt in range(2000):
        rng = np.random.default_rng(100_000 * seed + attempt)
        specks = _specks(rng, L - 3, box, 1.0, sigma=(0.55, 0.65), op=(0.008, 0.012))
        n1 = 20
        parts = [{k: x[:n1] for k, x in specks.items()}, _wide(rng, 2, centre, 60.0, 0.4),
                 {k: x[n1:] for k, x in specks.items()}, _wide(rng, 1, centre, 60.0, 0.03)]
        # every Gaussian of the batch keeps its margins: the fill is the same for every correct fp32 evaluation
        scene, aux, w = _finish(_cat(parts, box), cam, seed, 0, lambda w: range(w["n"]), must_blend=False)
        if w["hits"].shape[0] == 1 and int(w["hits"][0].max()) == target and (w["quad"] == L).all():
            return _case(f"hitcap({kind})", scene, cam, aux, w, seed, 0,
                         dict(family="hitcap", L=L, kind=kind, attempt=attempt, expect_quad=L, expect_fill=target))
    raise AssertionError("no layout with the wanted fill")


def ragged(which):
    """The second tile of a 24 x 16 image: its quadrants 1 and 3 lie outside the image."""
    return sparse(257, W=24, tile=1) if which == "sparse" else cut(557, 257, W=24, tile=1)


def cut_L(c):
    return c + 300


def all_cases():
    """(id, builder) of every case, cheapest first within a family."""
    out = [(f"sparse-{L}", functools.partial(sparse, L)) for L in SPARSE_L]
    out += [(f"cut-{c}", functools.partial(cut, cut_L(c), c)) for c in CUT_C]
    out += [(f"quadrant_cut-{c}", functools.partial(quadrant_cut, 700, c)) for c in QUADRANT_CUT_C]
    out += [(f"hitcap-{k}", functools.partial(hitcap, k)) for k in ("at", "over")]
    out += [(f"ragged-{k}", functools.partial(ragged, k)) for k in ("sparse", "cut")]
    return out


GRAD_KEYS = ("means3D", "means2D", "opacity", "sh", "scales", "rotations")
KINDS = ("e64", "e256", "end")
_REFS = {}


def reference(cid, build):
    """run_oracle of a case, computed once per process and left unchanged (check_forward's gpu_only_px aside)."""
    from gsr_testutil import run_oracle

    if cid not in _REFS:
        scene, cam, bg, grads, _ = build()
        _REFS[cid] = run_oracle(scene, cam, bg, grads=grads)
    return _REFS[cid]


def boundary_rule(grads, b32, b64, keys, meta, what, excuse=None, boundary=None):
    """The boundary-row rule: every element of a boundary row satisfies |g - g64| <= max(bar, ROW_RATIO |g32 - g64|)
    with the bar of check_grads, no slack; a row is left out only where `excuse` (flip_dependents of pixels the GPU
    flipped on its own) names it.  Returns (counts per kind: [checked, excused], failures)."""
    from gsr_testutil import GRAD_TOL, REPORT, ROW_RATIO

    boundary = meta["boundary"] if boundary is None else boundary
    counts = {k: [0, 0] for k in KINDS}
    failures = []
    for g, kinds in sorted(boundary.items()):
        ex = bool(excuse is not None and excuse[g])
        for k in kinds:
            counts[k][1 if ex else 0] += 1
        if ex:
            continue
        for key in keys:
            r64 = np.asarray(b64[key], np.float64)[g]
            e_g = np.abs(np.asarray(grads["g_" + key], np.float64).reshape(np.asarray(b64[key]).shape)[g] - r64)
            e_3 = np.abs(np.asarray(b32[key], np.float64)[g] - r64)
            lim = np.maximum(GRAD_TOL * np.maximum(1.0, np.abs(r64)), ROW_RATIO * e_3)
            if (e_g > lim).any():
                failures.append(f"{what}: boundary row of Gaussian {g} ({'/'.join(sorted(kinds))}, list position "
                                f"{int(np.nonzero(meta['order'] == g)[0][0])}) grad {key}: error {e_g.max():.3e} "
                                f"beyond {lim.flat[int(np.argmax(e_g / lim))]:.3e}")
    REPORT.append((what, "boundary rows", {k: dict(checked=v[0], excused=v[1]) for k, v in counts.items()}))
    return counts, failures
