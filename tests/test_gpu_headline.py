"""The kernels the benchmark times, selected the way the benchmark selects them, against the oracle (VERDICT r04
"what's weak" 1 / "next" 2).

The headline launches 64-view sets: the tile-wave forward (k_render_fwd_tile, chosen from 16 views when the
Gaussians span >= 3 tiles on average), keys carrying no masks (packed), the tile-wave forward's per-instance
quadrant masks feeding the lockstep backward's cull (k_render_bwd).  C5 launches two-colour sets: the quadrant-wave
forward over unpacked keys with quadrant masks and the one-wave-per-tile hit-list backward (k_render_bwd_tw).  The
per-view and few-view parity tests exercise other selections (quadrant-wave forward, recomputed cull, split
backward), so these tests render sets whose default selection is exactly bench.KERNELS and assert that it is
(include/gsr.h gsr_profile_kernel), then hold every view's outputs and the summed gradients to the oracle with
the bars of every parity test.  The oracle runs in a pool of processes (tests/oracle_pool.py).

Reference: renderer/gaussian_batch_renderer.py:21-76 (the batch whose results these are),
renderer/diff_gaussian_rasterizer_background.py:119-132 (the headline's renderer),
renderer/diff_sugar_rasterizer_normal.py:157-191 (C5's two calls).
"""
import numpy as np
import pytest

import oracle_pool
from gsr_testutil import adjudicate, check_forward, check_grads, flip_excuse, gs, make_camera, print_report

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _parity_report():
    yield
    print_report()


def _orbit(n_el, n_az, S):
    """bench.py's orbit (elevations 0, 10, 20, 30 x evenly spaced azimuths, distance 2.5, fovy 60)."""
    return [make_camera(S, S, elevation=[0.0, 10.0, 20.0, 30.0][e], azimuth=a * 360.0 / n_az)
            for e in range(n_el) for a in range(n_az)]


def _bench_kernels(kind):
    import bench

    return {"render_fwd": bench.KERNELS[kind][0], "render_bwd": bench.KERNELS[kind][1]}


def test_headline_kernel_selection_vs_oracle():
    """16 views of the bench orbit (4 elevations x 4 azimuths), 250k Gaussians, 512^2, SH3, the background path
    with per-view background images fused into the blends (rasterize_views(background=...)), upstream gradients
    on the render, depth and alpha: K / P ~ 5 (the headline's 6.7 at 1M / 1024^2), so the set takes the
    headline's tile-wave forward and the mask-culled lockstep backward.  Every view vs the oracle (composite,
    radii, K, means2D gradient row-wise), the parameter gradients summed over the 16 views vs the oracle's sums."""
    from diff_gaussian_rasterization import _C
    from gsr_testutil import GRAD_KEYS, _gpu_views, _view

    spec = ("ball", 250_000, 3, 0)
    scene = oracle_pool.scene_of(spec)
    S, V = 512, 16
    cams = _orbit(4, 4, S)
    rng = np.random.default_rng(77)
    bg_img = rng.random((V, S, S, 3)).astype(np.float32)
    ups = [gs.upstream_grads(S, S, seed=300 + v) for v in range(V)]
    zero = [0.0, 0.0, 0.0]
    gpu = _gpu_views(scene, cams, [zero] * V, ups, background=bg_img)
    assert _C.profile_kernels() == _bench_kernels("c3"), _C.profile_kernels()
    assert sum(gpu["K"]) >= 3 * V * scene["means3D"].shape[0]  # (the selection rule's condition, gsr_render.hip)
    tasks = [(spec, cams[v], zero, ups[v], bg_img[v], gpu["color"][v], ("f32r", "aux32")) for v in range(V)]
    views, tot = oracle_pool.views_and_sums(tasks)
    for v, ref in enumerate(views):
        check_forward(_view(gpu, v), ref, f"headline view {v}", K_gpu=gpu["K"][v])
        b = ref["b"]
        adjudicate(gpu["g_means2D"][v], b["f32"]["means2D"], b["f64"]["means2D"],
                   1e-4 * np.maximum(1.0, np.abs(b["f64"]["means2D"])), f"headline view {v}", "grad means2D",
                   rowwise=True, r32b=b["f32r"]["means2D"], excuse=flip_excuse([ref]))
    refs = dict(b32=tot["f32"], b64=tot["f64"], b32r=tot["f32r"])
    check_grads(gpu, refs, GRAD_KEYS, "headline summed", excuse=flip_excuse(views))


def test_c5_kernel_selection_vs_oracle():
    """C5's kernels on a 16-view set: SuGaR surface Gaussians (subdiv 4: 30,720 Gaussians), 256^2, pass 1 with
    colors_precomp = SH2RGB(dc) and the face normals as the second colour set (one forward blending both, one
    two-colour backward replay: rasterize_views(colors2=...)), as bench.py --workload sugar launches them.  Every
    view's colour / depth / alpha vs the oracle's first call and its second colour image vs the oracle's second
    call; the parameter gradients summed over both calls and the 16 views vs the oracle's (fp32 / fp64)."""
    import torch

    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization.batched import rasterize_views
    from gsr_testutil import _settings

    spec1, spec2 = ("sugar", 4, 0, 5, True), ("sugar", 4, 0, 5, False)
    s1 = oracle_pool.scene_of(spec1)
    normals = oracle_pool.scene_of(spec2)["normals"]
    S, V = 256, 16
    cams = _orbit(4, 4, S)
    P = s1["means3D"].shape[0]
    bg = [0.3, 0.1, 0.5]
    rng = np.random.default_rng(12)
    ups = [(rng.standard_normal((3, S, S)).astype(np.float32), rng.standard_normal((1, S, S)).astype(np.float32),
            rng.standard_normal((1, S, S)).astype(np.float32), rng.standard_normal((3, S, S)).astype(np.float32))
           for _ in range(V)]
    dev = "cuda"
    t = {k: torch.tensor(s1[k], device=dev, requires_grad=True)
         for k in ("means3D", "scales", "rotations", "opacities", "colors_precomp")}
    t["normals"] = torch.tensor(normals, device=dev, requires_grad=True)
    m2 = [torch.zeros((P, 3), device=dev, requires_grad=True) for _ in cams]
    st = [_settings(c, bg, 0) for c in cams]
    c, r, d, a, c2 = rasterize_views(st, t["means3D"], m2, t["opacities"], colors_precomp=t["colors_precomp"],
                                     scales=t["scales"], rotations=t["rotations"], colors2=t["normals"])
    u = [torch.tensor(np.stack([x[i] for x in ups]), device=dev) for i in range(4)]
    ((c * u[0]).sum() + (d * u[1]).sum() + (a * u[2]).sum() + (c2 * u[3]).sum()).backward()
    assert _C.profile_kernels() == _bench_kernels("sugar"), _C.profile_kernels()
    # the oracle's two calls per view: pass 1 (colours, its depth / alpha / means2D) and pass 2 (normals as
    # colors_precomp, no depth / alpha upstream; its means2D gradient is discarded, as the reference's zero means2D
    # of that call is)
    z = np.zeros((1, S, S), np.float32)
    spec_n = ("sugar", 4, 0, 5, "normals")
    views1, tot1 = oracle_pool.views_and_sums(
        [(spec1, cams[v], bg, ups[v][:3], None, c[v].detach().cpu().numpy(), ("aux32", "f32r", "cov32")) for v in range(V)])
    views2, tot2 = oracle_pool.views_and_sums(
        [(spec_n, cams[v], bg, (ups[v][3], z, z), None, c2[v].detach().cpu().numpy(), ("f32r", "cov32")) for v in range(V)])
    cn, dn, an, rn = (c.detach().cpu().numpy(), d.detach().cpu().numpy(), a.detach().cpu().numpy(), r.cpu().numpy())
    c2n = c2.detach().cpu().numpy()
    for v in range(V):
        check_forward(dict(color=cn[v], depth=dn[v], alpha=an[v], radii=rn[v]), views1[v], f"C5 set view {v}")
        # the second colour image (its depth / alpha are pass 1's: the same geometry and blend)
        check_forward(dict(color=c2n[v], depth=dn[v], alpha=an[v]), views2[v], f"C5 set view {v} normals")
        b = views1[v]["b"]
        adjudicate(m2[v].grad.cpu().numpy(), b["f32"]["means2D"], b["f64"]["means2D"],
                   1e-4 * np.maximum(1.0, np.abs(b["f64"]["means2D"])), f"C5 set view {v}", "grad means2D",
                   rowwise=True, r32b=b["f32r"]["means2D"], excuse=flip_excuse([views1[v], views2[v]]))
    keys = ("means3D", "opacity", "scales", "rotations")
    tags = (("b32", "f32"), ("b64", "f64"), ("b32r", "f32r"))
    refs = {tag: {k: tot1[p][k] + tot2[p][k] for k in keys} for tag, p in tags}
    for tag, p in tags:
        refs[tag]["colors"], refs[tag]["normals"] = tot1[p]["colors"], tot2[p]["colors"]
    # the scale / rotation gradients' null model is the GPU's association: per view the two calls' fp32 dL/dcov3D
    # added, summed over the 16 views in view order in fp32, then one fp32 chain rule (the oracle applies the chain
    # rule per view and call, and its sums over views are float64; on SuGaR's flat Gaussians, whose third scale is
    # ~0, the cancellation makes the association visible)
    acc = np.zeros_like(views1[0]["b"]["f32"]["cov3D"], dtype=np.float32)
    for v in range(V):
        acc = (acc + (views1[v]["b"]["f32"]["cov3D"].astype(np.float32)
                      + views2[v]["b"]["f32"]["cov3D"].astype(np.float32))).astype(np.float32)
    refs["b32r"]["scales"], refs["b32r"]["rotations"] = oracle_pool.scale_rot_chain(acc, s1["scales"],
                                                                                     s1["rotations"])
    g = {"g_" + k: t[n].grad.cpu().numpy() for k, n in (("means3D", "means3D"), ("opacity", "opacities"),
                                                        ("scales", "scales"), ("rotations", "rotations"),
                                                        ("colors", "colors_precomp"), ("normals", "normals"))}
    check_grads(g, refs, list(keys) + ["colors", "normals"], "C5 set summed", excuse=flip_excuse(views1 + views2))
