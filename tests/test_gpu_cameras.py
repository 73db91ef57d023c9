"""HIP rasterizer vs the CPU oracle away from the default orbit: the cases of tests/camera_cases.py (near,
telephoto, off-axis and inside cameras, a deep scene, a 2^20 + 1 Gaussian scene with image-wide Gaussians).
tests/test_camera_cases.py asserts on the CPU that each case reaches what it is for; tests/test_oracle.py checks
the oracle's own reading of the guard and alpha-clamp gradient conventions against torch autograd.

Four code paths are pinned here that the orbit never runs:
  guard gradient         cov2d_backward zeroes the t.x / t.y gradient where the 1.3 tan(fov/2) clamp binds
                         (near49, offaxis, inside, the mixed view set)
  4-pass depth sort      a set whose visible depth keys span 2^24 codes or more cannot skip the last radix pass
                         (inside, offaxis, deep, the mixed view set, the 3-pass / 4-pass cross-check)
  kept-count overflow    with more than 2^20 Gaussians the depth-sort value holds at most 2047 kept tiles and
                         k_inst_count reads larger counts from memory (wide_field)
  off-screen rectangles  centres left of / above / beyond the image, radii of thousands of pixels: getRect's
                         truncation towards zero and the clamps of span_row / span_quads (near49, offaxis, inside)

Bars, ratios and slacks are those of tests/gsr_testutil.py, unchanged.
"""
import numpy as np
import pytest

import camera_cases as cc
from gsr_testutil import (adjudicate, check_forward, check_grads, flip_excuse, gpu_render, gs, make_camera,
                          print_report, run_oracle)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _parity_report():
    yield
    print_report()


def _use(name):
    return ("colors_precomp",) if name == "wide_field" else ("shs",)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_parity(name):
    """Forward and backward through the public GaussianRasterizer against the oracle, all six gradient tensors,
    seeded upstream gradients on colour, depth and alpha; radii bit-exact up to fp64-verified ceil ties and
    num_rendered exact up to rectangle ties (where a wrong getRect truncation off screen would show)."""
    scene, cam, bg = cc.get(name)
    g = gs.upstream_grads(cam["H"], cam["W"], seed=7)
    gpu = gpu_render(scene, cam, bg, grads=g, use=_use(name))
    ref = run_oracle(scene, cam, bg, grads=g)
    check_forward(gpu, ref, name, K_gpu=gpu["K"])
    check_grads(gpu, ref, cc.grad_keys(name), name)


def test_wide_field_instance_counts():
    """Three Gaussians keep all 2304 tiles, more than the 2047 the depth-sort value's field holds: the run
    cannot pass with them lost, and it is repeatable bit for bit."""
    scene, cam, bg = cc.get("wide_field")
    tiles = ((cam["W"] + 15) // 16) * ((cam["H"] + 15) // 16)
    g = gs.upstream_grads(cam["H"], cam["W"], seed=7)
    a = gpu_render(scene, cam, bg, grads=g, use=_use("wide_field"))
    b = gpu_render(scene, cam, bg, grads=g, use=_use("wide_field"))
    assert a["K"] >= 3 * tiles and a["K"] == b["K"], (a["K"], b["K"])
    assert np.sort(a["radii"])[-3] >= cam["W"]
    for k in ("color", "depth", "alpha", "radii", "g_means3D"):
        assert np.array_equal(a[k], b[k]), k


def _mixed_cameras(nviews, W, H):
    cams = [cc.camera("near49", W, H), cc.camera("inside", W, H), make_camera(W, H, azimuth=130.0),
            cc.camera("tele20", W, H)]
    if nviews > 4:  # those four again, and one view that sees nothing (it looks away from the ball)
        cams = cams + cams + [cc.make_lookat_camera((3.0, 0.0, 0.5), (6.0, 0.0, 0.5), W, H, 60.0, 60.0)]
    return cams[:nviews]


@pytest.mark.parametrize("nviews", [4, 9])
def test_mixed_view_set_vs_oracle(nviews):
    """One scene seen from near49, inside, the orbit and tele20 in one rasterize_views set.  The set's depth-key
    range and 3-pass flag live in one GeomState: the inside view alone needs the fourth sort pass, the others
    alone would not.  Images per view, means2D gradients per view, parameter gradients summed over the views."""
    from gsr_testutil import GRAD_KEYS, _gpu_views, _sum_grads, _view

    W, H = 128, 112
    scene = gs.make_scene(2000, sh_degree=1, seed=111)
    cams = _mixed_cameras(nviews, W, H)
    palette = [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.2, 0.5, 0.9], [0.7, 0.1, 0.3]]
    bgs = [palette[v % 4] for v in range(nviews)]
    ups = [gs.upstream_grads(H, W, seed=80 + v) for v in range(nviews)]
    gpu = _gpu_views(scene, cams, bgs, ups)
    refs = []
    for v, cam in enumerate(cams):
        ref = run_oracle(scene, cam, bgs[v], grads=ups[v])
        check_forward(_view(gpu, v), ref, f"mixed{nviews} view {v}", K_gpu=gpu["K"][v])
        adjudicate(gpu["g_means2D"][v], ref["b32"]["means2D"], ref["b64"]["means2D"],
                   1e-4 * np.maximum(1.0, np.abs(ref["b64"]["means2D"])), f"mixed{nviews} view {v}", "grad means2D",
                   rowwise=True, r32b=ref["b32r"]["means2D"], excuse=flip_excuse([ref]))
        refs.append(ref)
    if nviews > 4:
        assert gpu["K"][-1] == 0 and not gpu["radii"][-1].any()
    tot = dict(b32=_sum_grads(refs, "b32", GRAD_KEYS), b64=_sum_grads(refs, "b64", GRAD_KEYS),
               b32r=_sum_grads(refs, "b32r", GRAD_KEYS))
    check_grads(gpu, tot, GRAD_KEYS, f"mixed{nviews} summed", excuse=flip_excuse(refs))


def _key_span(radii, scene, cam):
    z = cc.view_space(scene["means3D"], cam)[:, 2].astype(np.float32)[np.asarray(radii).reshape(-1) > 0]
    return int(z.max().view(np.uint32)) - int(z.min().view(np.uint32))


def test_three_and_four_sort_passes_agree_bitwise():
    """The deep scene without its moved Gaussians sorts in 3 passes.  With 200 more Gaussians appended whose
    opacity 0.5 / 255 lies below every blend's 1 / 255 threshold and whose depths run from 0.25 to 60, they are
    visible, so the sort takes 4 passes, but no blend sees them: the images and the first P rows of every
    gradient are bitwise equal.  No tolerance, no oracle."""
    base, cam, bg = cc.deep(moved=False)
    full, _, _ = cc.get("deep")
    n, P = cc.DEEP_MOVED, base["means3D"].shape[0]
    ext = {k: (np.concatenate([v, full[k][:n]], 0) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    ext["opacities"][P:] = np.float32(0.5 / 255.0)
    g = gs.upstream_grads(cam["H"], cam["W"], seed=7)
    a = gpu_render(base, cam, bg, grads=g)
    b = gpu_render(ext, cam, bg, grads=g)
    assert (b["radii"][P:] > 0).all()  # visible: they widen the set's depth range
    assert _key_span(a["radii"], base, cam) < (1 << 24) - (1 << 16) and _key_span(b["radii"], ext, cam) >= 1 << 25
    assert a["K"] > 0
    for k in ("color", "depth", "alpha"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["radii"], b["radii"][:P])
    for k in ("g_means3D", "g_means2D", "g_opacity", "g_sh", "g_scales", "g_rotations"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k][:P]), k
        assert not b[k][P:].any(), k
