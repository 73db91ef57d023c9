"""Scenes of the span-word emission tests (tests/test_gpu_emit_spans.py; no tests here), and the rectangle rows and
kept tile spans of every Gaussian restated on the CPU from the oracle's fp32 preprocess values (csrc/gsr_common.h
span_prep / span_row step for step in float32, vectorised), so that each test can assert its scene holds the case it
names: what is encodable (csrc/gsr_span_word.h), what is not and why, in which 64-Gaussian group of the depth order.
"""
from __future__ import annotations

import numpy as np

import gsr_synthetic as gs
from gsr_testutil import make_camera, oracle_cam

f32 = np.float32
MAX_ROWS, MAX_LEN, COORD = 4, 15, 128  # the word's limits (GSR_SPAN_ROWS, GSR_SPAN_LEN, GSR_SPAN_COORD)


def spans_cpu(scene, cam):
    """Per Gaussian of one view: vis (P,), rect (P, 4) tile xmin, ymin, xmax, ymax, rows (P,), t0 / t1 (P, max rows)
    (rows past a Gaussian's own: t0 = t1 = 0), enc (P,) = the word is encodable, order = the visible Gaussians in
    the emission's depth order (depth key, then index)."""
    import oracle

    aux = oracle.gauss_aux(scene, oracle_cam(cam), "f32")
    P = aux["px"].shape[0]
    vis = aux["tiles"] > 0
    rect = aux["rect"]
    rows = np.where(vis, rect[:, 3] - rect[:, 1], 0)
    px, py = aux["px"].astype(f32), aux["py"].astype(f32)
    a, b, c = (aux["conic"][:, i].astype(f32) for i in range(3))
    o = aux["opacity"].astype(f32)
    with np.errstate(all="ignore"):
        D = a * c - b * b
        mode = np.where(~(o >= f32(1.0 / 255.0) * f32(0.9999)), 0, np.where(~((a > 0) & (c > 0) & (D > 0)), 1, 2))
        tau = np.maximum(f32(0), np.log(f32(255.0) * o).astype(f32))
        thr = f32(2.0) * (tau * f32(1.002) + f32(2e-3))
        ia = f32(1.0) / a
        thra = thr * a
        ue = np.sqrt(thr * c * (f32(1.0) / D)).astype(f32)
        ve = b * ue * (f32(1.0) / c)
        R = int(rows.max()) if P else 0
        t0 = np.zeros((P, max(R, 1)), np.int64)
        t1 = np.zeros((P, max(R, 1)), np.int64)
        xmin, xmax = rect[:, 0], rect[:, 2]
        for k in range(R):
            ty = rect[:, 1] + k
            v1 = py - (ty * 16).astype(f32)
            v0 = v1 - f32(15.0)
            umax = np.where((-ve >= v0) & (-ve <= v1), ue, f32(-3.0e38)).astype(f32)
            umin = np.where((ve >= v0) & (ve <= v1), -ue, f32(3.0e38)).astype(f32)
            for v in (v0, v1):
                e = thra - D * (v * v)
                r, m = np.sqrt(np.maximum(e, 0)).astype(f32), -b * v
                umax = np.where(e >= 0, np.maximum(umax, (m + r) * ia), umax)
                umin = np.where(e >= 0, np.minimum(umin, (m - r) * ia), umin)
            hit = umax >= umin
            lo = np.clip((px - f32(15.0) - umax - f32(0.05)) * f32(1.0 / 16.0), f32(-1.0e6), f32(1.0e6))
            hi = np.clip((px - umin + f32(0.05)) * f32(1.0 / 16.0), f32(-1.0e6), f32(1.0e6))
            a0 = np.ceil(np.nan_to_num(lo)).astype(np.int64)
            a1 = np.floor(np.nan_to_num(hi)).astype(np.int64) + 1
            s0 = np.maximum(xmin, np.minimum(a0, xmax))
            s1 = np.maximum(s0, np.minimum(a1, xmax))
            k0 = np.where((mode == 2) & hit, s0, xmin)
            k1 = np.where(mode == 1, xmax, np.where((mode == 2) & hit, s1, xmin))
            own = vis & (k < rows)
            t0[:, k] = np.where(own, k0, 0)
            t1[:, k] = np.where(own, k1, 0)
    ln = t1 - t0
    enc = vis & (rows >= 1) & (rows <= MAX_ROWS) & (rect[:, 3] <= COORD) & (ln.max(1) <= MAX_LEN) & \
        (t0.max(1) < COORD) & (t1.max(1) <= COORD)
    idx = np.nonzero(vis)[0]
    order = idx[np.lexsort((idx, aux["depth"].astype(f32)[idx]))]
    return dict(vis=vis, rect=rect, rows=rows, t0=t0, t1=t1, len=ln, enc=enc, order=order)


def groups(sp):
    """The 64-Gaussian groups of a view's depth order (the emission's waves), as index arrays."""
    return [sp["order"][i:i + 64] for i in range(0, len(sp["order"]), 64)]


def _bars(n, seed, W, H, cam, sx, sy, opacity=(0.5, 0.95), yspread=1.0):
    """n axis-aligned flat Gaussians facing the default camera, spread over its image: world half-extents sx / sy
    (ranges, in pixels of the W x H image at the origin's depth) along the image's x / y; yspread > 1 puts centres above
    and below the image too (their rectangles are clamped to it: wide and few rows)."""
    rng = np.random.default_rng(seed)
    ex, ey = 2.5 * cam["tanx"], 2.5 * cam["tany"]  # world half-extent of the image at the origin's distance
    upx, upy = 2 * ex / W, 2 * ey / H              # world units per pixel
    xyz = np.stack([rng.uniform(-ex, ex, n), rng.uniform(-ey * yspread, ey * yspread, n),
                    rng.uniform(-0.05, 0.05, n)], 1)
    sc = np.stack([rng.uniform(*sx, n) * upx, rng.uniform(*sy, n) * upy, np.full(n, 1e-3)], 1)
    scene = gs.make_scene(n, sh_degree=0, seed=seed)
    # the orbit camera at elevation 0, azimuth 0 looks down one world axis: find which axes the image's x / y follow
    view = cam["view"]  # (4, 4), row-vector convention: p_view = p @ view
    Rw = view[:3, :3]
    ax_x, ax_y = int(np.argmax(np.abs(Rw[:, 0]))), int(np.argmax(np.abs(Rw[:, 1])))
    ax_z = 3 - ax_x - ax_y
    m = np.zeros((n, 3))
    s = np.zeros((n, 3))
    m[:, ax_x], m[:, ax_y], m[:, ax_z] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    s[:, ax_x], s[:, ax_y], s[:, ax_z] = sc[:, 0], sc[:, 1], sc[:, 2]
    scene["means3D"] = m.astype(f32)
    scene["scales"] = s.astype(f32)
    scene["rotations"] = np.tile(np.array([1, 0, 0, 0], f32), (n, 1))
    scene["opacities"] = rng.uniform(*opacity, size=(n, 1)).astype(f32)
    return scene


def case(name):
    """(scene, cameras) of a named case."""
    if name == "ball":  # the plain ball scene: most Gaussians encodable
        return gs.make_scene(20_000, sh_degree=3, seed=7), [
            make_camera(200, 168, elevation=10.0 * i, azimuth=70.0 * i + 5.0) for i in range(3)]
    if name == "mixed":  # 4 and 5 rectangle rows, rows of 15 and 16 kept tiles, in the same groups
        cam = make_camera(256, 128, fovy_deg=40.0, fovx_deg=70.0, elevation=0.0, azimuth=0.0)
        a = _bars(320, 3, 256, 128, cam, sx=(2.0, 60.0), sy=(1.0, 7.0))
        # large round ones centred above and below the image: their rectangles are clamped to a few rows, full width
        b = _bars(320, 4, 256, 128, cam, sx=(25.0, 45.0), sy=(25.0, 45.0), yspread=3.0)
        scene = {k: (np.concatenate([a[k], b[k]]) if isinstance(a[k], np.ndarray) else a[k]) for k in a}
        return scene, [cam, make_camera(256, 128, fovy_deg=40.0, fovx_deg=70.0, elevation=3.0, azimuth=4.0)]
    if name == "wide":  # 2064 x 32: 129 tile columns, Gaussians on both sides of column 127
        cam = make_camera(2064, 32, fovy_deg=3.0, fovx_deg=100.0, elevation=0.0, azimuth=0.0)
        a = _bars(1200, 5, 2064, 32, cam, sx=(1.0, 12.0), sy=(1.0, 6.0))
        b = _bars(600, 6, 2064, 32, cam, sx=(1.0, 12.0), sy=(1.0, 6.0))
        # the second half pushed to the image's two ends (the last ~70 pixels of each)
        for k in range(3):
            col = b["means3D"][:, k]
            if np.abs(col).max() > 1.0:  # the axis the image's x follows
                ext = np.abs(col).max()
                b["means3D"][:, k] = np.sign(col) * (ext * (1.0 - 0.035 * np.abs(col) / ext))
        scene = {k: (np.concatenate([a[k], b[k]]) if isinstance(a[k], np.ndarray) else a[k]) for k in a}
        return scene, [cam, make_camera(2064, 32, fovy_deg=3.0, fovx_deg=100.0, elevation=0.0, azimuth=0.5)]
    if name == "faint":  # rectangles whose every row is empty (too faint), and ones whose outer rows are
        cam = make_camera(160, 144, elevation=0.0, azimuth=0.0)
        scene = _bars(1500, 9, 160, 144, cam, sx=(3.0, 10.0), sy=(3.0, 10.0))
        rng = np.random.default_rng(10)
        o = rng.uniform(0.5, 0.9, 1500)
        o[:500] = rng.uniform(0.0030, 0.0039, 500)   # below 1/255: no tile kept
        o[500:1000] = rng.uniform(0.00393, 0.0045, 500)  # just above: a dot within a many-tile rectangle
        scene["opacities"] = o.reshape(-1, 1).astype(f32)
        return scene, [cam, make_camera(160, 144, elevation=5.0, azimuth=8.0)]
    if name == "long":  # groups of more than 64 rows, row chunks of more than 64 kept tiles
        return gs.make_scene(3000, sh_degree=1, seed=11, scale_mult=2.2), [
            make_camera(256, 256, elevation=20.0 * i, azimuth=100.0 * i) for i in range(2)]
    if name == "ragged":  # P no multiple of 64 or 128; the second camera sits inside the ball (culls some)
        return gs.make_scene(5003, sh_degree=2, seed=13), [
            make_camera(176, 120, elevation=10.0, azimuth=20.0), make_camera(176, 120, distance=0.4, azimuth=200.0),
            make_camera(176, 120, distance=0.3, elevation=40.0, azimuth=90.0)]
    raise KeyError(name)


def run_case(name):
    """The case through rasterize_views, forward and backward: a list of numpy arrays (every output and radii, the
    num_rendered and listed-instance counts the Python layer recorded, every per-view means2D gradient and parameter
    gradient)."""
    from diff_gaussian_rasterization import _C
    from gsr_testutil import _gpu_views

    scene, cams = case(name)
    V = len(cams)
    ups = [gs.upstream_grads(c["H"], c["W"], seed=20 + i) for i, c in enumerate(cams)]
    out = _gpu_views(scene, cams, [[0.1, 0.2, 0.3]] * V, ups=ups)
    res = [out["color"], out["depth"], out["alpha"], out["radii"], np.asarray(out["K"], np.int64),
           np.asarray(list(_C.RECENT_LISTED)[-V:], np.int64)]
    res += list(out["g_means2D"])
    res += [out[k] for k in sorted(out) if k.startswith("g_") and k != "g_means2D"]
    return res


def run_timed_case():
    """One rasterize_timed_views call (4 frames, forward and backward) as a list of numpy arrays."""
    import timed_views_fixtures as tf

    cams = [make_camera(120, 96, elevation=8.0 * i, azimuth=40.0 * i) for i in range(4)]
    frames = tf.make_frames(1500, cams, seed=4)
    ups = [gs.upstream_grads(96, 120, seed=30 + i) for i in range(4)]
    res = tf.run_timed(frames, cams, [[0.2, 0.1, 0.0]] * 4, ups=ups)
    return [np.asarray(res[k]) for k in sorted(res)]


def run_two_colour_case():
    """One two-colour (colors2) rasterize_views call: test_gpu_parity's SuGaR case."""
    import test_gpu_parity as tp
    from diff_gaussian_rasterization import _C

    res = tp.bitwise_case("sugar_two_colors")
    return res + [np.asarray([k for k, _, _ in list(_C.RECENT_FORWARDS)[-3:]], np.int64),
                  np.asarray(list(_C.RECENT_LISTED)[-3:], np.int64)]


RUNNERS = dict(timed=run_timed_case, two_colour=run_two_colour_case)
SCENE_CASES = ("ball", "mixed", "wide", "faint", "long", "ragged")


def run_all(path):
    """Every case of this module into one .npz (the child process of the bitwise test)."""
    out = {}
    for name in SCENE_CASES + tuple(RUNNERS):
        arrs = RUNNERS[name]() if name in RUNNERS else run_case(name)
        for i, x in enumerate(arrs):
            out[f"{name}__{i:02d}"] = x
    np.savez(path, **out)
