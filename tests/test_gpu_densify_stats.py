"""The fused densification statistics on the GPU (csrc/gsr_densify.hip through diff_gaussian_rasterization/densify.py):
bitwise the CPU path on the same inputs at the wave, block, unroll and chunk edges; repeatable; nothing written past
the arrays; on the lists a real render returns (plain and timed view sets, a gradient summed over two backward calls);
and update_states_fused against update_states on a DensifyModel."""
import ctypes
import math

import numpy as np
import pytest
import torch

import densify_cases as dc
import densify_reference as dr
from gsr_testutil import gs

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, FILL = 64, -7.25
# views without a gradient: the first, a middle and the last view of a chunk of 64 (and of the four-view groups)
NONE_AT = {1: (), 3: (1,), 64: (0, 31, 63), 65: (0, 63, 64), 130: (0, 63, 64, 100, 127, 128, 129)}


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).reshape(-1).view(np.uint32)


def _stats(views, rows, **state):
    from diff_gaussian_rasterization.densify import densify_stats

    return densify_stats(views["radii"], views["viewspace_points"], views["visibility_filter"] if rows else None,
                         **state)


def _guarded(values):
    """A (P,) array holding `values` in front of GUARD elements of FILL (the test's own memory)."""
    buf = torch.full((values.numel() + GUARD,), FILL, device=DEV)
    buf[:values.numel()] = values.reshape(-1).to(DEV)
    return buf


def _state(P, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(P, generator=g) * 8
    m[::5] = float("nan")
    return m, torch.rand(P, generator=g) * 3, torch.randint(0, 4, (P,), generator=g).float()


@pytest.mark.parametrize("rows", [False, True], ids=["radii", "rows"])
@pytest.mark.parametrize("V", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 1000])
def test_kernel_equals_cpu_path_bitwise(P, V, rows):
    """From zero and from a non-zero state (a NaN in the running maximum), with and without visibility rows, views
    without a gradient at the first, a middle and the last place of a chunk."""
    cpu = dc.make_views(V, P, seed=7, none_at=NONE_AT[V], explicit=range(0, V, 2) if rows else ())
    gpu = dc.clone_views(cpu, DEV)
    want = _stats(cpu, rows)
    got = _stats(gpu, rows)
    for g, w, name in zip(got, want, ("max", "sum", "count")):
        assert g.is_cuda and g.shape == (P,)
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"from zero: {name}")
    # from a state, in place, in guarded arrays
    start = _state(P, seed=P + V)
    cpu_state = [t.clone() for t in start]
    _stats(cpu, rows, max_radii=cpu_state[0], grad_norm_sum=cpu_state[1], count=cpu_state[2])
    bufs = [_guarded(t) for t in start]
    out = _stats(gpu, rows, max_radii=bufs[0][:P], grad_norm_sum=bufs[1][:P], count=bufs[2][:P])
    for b, o, w, name in zip(bufs, out, cpu_state, ("max", "sum", "count")):
        assert o.data_ptr() == b.data_ptr()
        np.testing.assert_array_equal(_bits(b[:P]), _bits(w), err_msg=f"continued: {name}")
        assert bool((b[P:] == FILL).all()), f"{name}: written past P"
    assert bool(torch.isnan(bufs[0][:P:5]).all())


def test_a_single_view_without_a_gradient_only_counts():
    cpu = dc.make_views(1, 300, seed=9, none_at=(0,))
    m, s, c = _stats(dc.clone_views(cpu, DEV), False)
    assert float(s.abs().max()) == 0 and torch.equal(c.cpu(), (cpu["radii"][0] > 0).float())
    assert torch.equal(m.cpu(), cpu["radii"][0].float())


def _library_call(views, P, bufs, accumulate, rows):
    from diff_gaussian_rasterization import _C

    V = len(views["radii"])
    a = _C.DensifyBatch(V=V, P=P, accumulate=accumulate, max_radii=bufs[0].data_ptr(),
                        grad_norm_sum=bufs[1].data_ptr(), count=bufs[2].data_ptr())
    keep = []
    for k in range(V):
        a.radii[k] = views["radii"][k].data_ptr()
        g = views["viewspace_points"][k].grad
        a.grads[k] = None if g is None else g.data_ptr()
        if rows:
            keep.append(views["visibility_filter"][k].view(torch.uint8))
            a.visible[k] = keep[-1].data_ptr()
    rc = _C.load_library().gsr_densify_stats(ctypes.byref(a), _C._stream(torch.device(DEV, torch.cuda.current_device())))
    assert rc == 0, _C.load_library().gsr_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [False, True], ids=["radii", "rows"])
def test_library_call_from_zero_is_repeatable_and_stays_in_bounds(rows):
    """accumulate = 0 ignores what the arrays hold (NaNs here); two calls give the same bits; the guard elements
    behind the arrays keep their fill; V = 0 and P = 0 write nothing."""
    P, V = 257, 7
    cpu = dc.make_views(V, P, seed=11, none_at=(5,), explicit=(2, 3) if rows else ())
    gpu = dc.clone_views(cpu, DEV)
    want = _stats(cpu, rows)
    runs = []
    for _ in range(2):
        bufs = [_guarded(torch.full((P,), float("nan"))) for _ in range(3)]
        _library_call(gpu, P, bufs, 0, rows)
        assert all(bool((b[P:] == FILL).all()) for b in bufs)
        runs.append([_bits(b[:P]) for b in bufs])
    for a, b, w in zip(runs[0], runs[1], want):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, _bits(w))
    # nothing to do: the arrays keep what they hold
    bufs = [_guarded(torch.full((P,), 2.5)) for _ in range(3)]
    _library_call({k: [] for k in gpu}, P, bufs, 0, rows)
    _library_call(gpu, 0, bufs, 0, rows)
    assert all(bool((b[:P] == 2.5).all()) and bool((b[P:] == FILL).all()) for b in bufs)


def test_empty_batches_on_the_gpu():
    from diff_gaussian_rasterization.densify import densify_stats

    m = torch.full((9, 1), 3.0, device=DEV)
    out = densify_stats([], [], None, max_radii=m)
    assert out[0] is m and float(m.min()) == 3.0 and out[1].is_cuda and float(out[1].abs().sum()) == 0
    out = densify_stats([torch.zeros(0, dtype=torch.int32, device=DEV)], [None])
    assert all(t.shape == (0,) and t.is_cuda for t in out)


def _cams(n, size=64):
    from gsr_testutil import make_camera

    return [make_camera(size, size, azimuth=360.0 * v / n, elevation=10.0 + 5 * v) for v in range(n)]


def _check_render_lists(radii, m2s):
    """densify_stats on a render's lists: bitwise the CPU path on copies, and the reference form (count and max
    exactly, the sum within the bound)."""
    from diff_gaussian_rasterization.densify import densify_stats

    V, P = radii.shape
    rows = [radii[v] for v in range(V)]
    assert all(m.grad is not None and m.grad.shape == (P, 3) for m in m2s)
    got = densify_stats(rows, m2s, None)
    got_rows = densify_stats(rows, m2s, [r > 0 for r in rows])
    views = dc.clone_views({"radii": rows, "viewspace_points": m2s, "visibility_filter": [r > 0 for r in rows]}, "cpu")
    want = densify_stats(views["radii"], views["viewspace_points"], None)
    for g, g2, w in zip(got, got_rows, want):
        np.testing.assert_array_equal(_bits(g), _bits(w))
        np.testing.assert_array_equal(_bits(g2), _bits(w))
    m = torch.zeros(P)
    s, c = torch.zeros(P, 1), torch.zeros(P, 1)
    m = dc.reference_form(views, m, s, c)
    assert torch.equal(got[0].cpu(), m) and torch.equal(got[2].cpu(), c[:, 0])
    ref = s[:, 0].double().numpy()
    assert (np.abs(got[1].cpu().double().numpy() - ref) <= dc.bound(V) * ref).all()
    assert float(c.max()) == V and (ref > 0).sum() > P // 4  # most Gaussians are seen and receive a gradient


def test_end_to_end_on_a_rendered_view_set():
    """rasterize_views, two backward calls (retain_graph: .grad holds their sum), then the statistics."""
    from diff_gaussian_rasterization.batched import rasterize_views
    from gsr_testutil import _settings

    scene = gs.make_scene(2_000, sh_degree=1, seed=4)
    cams = _cams(4)
    t = {k: torch.tensor(scene[k], device=DEV, requires_grad=True)
         for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    m2s = [torch.zeros((2_000, 3), device=DEV, requires_grad=True) for _ in cams]
    color, radii, depth, alpha = rasterize_views([_settings(c, [0.0, 0.0, 0.0], 1) for c in cams], t["means3D"], m2s,
                                                 t["opacities"], shs=t["shs"], scales=t["scales"],
                                                 rotations=t["rotations"])
    ups = [gs.upstream_grads(64, 64, seed=20 + v) for v in range(4)]
    gc, gd, ga = (torch.stack([torch.tensor(u[i], device=DEV) for u in ups]) for i in range(3))
    loss = (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()
    loss.backward(retain_graph=True)
    once = [m.grad.clone() for m in m2s]
    (color * gc).sum().backward()
    assert any(not torch.equal(a, m.grad) for a, m in zip(once, m2s))
    _check_render_lists(radii, m2s)


def test_end_to_end_on_a_timed_view_set():
    from diff_gaussian_rasterization.batched import rasterize_timed_views
    from gsr_testutil import _settings
    from timed_views_fixtures import make_frames

    cams = _cams(3)
    frames = make_frames(2_000, cams, seed=6)
    leaf = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV, requires_grad=True)  # noqa: E731
    m2s = [torch.zeros((2_000, 3), device=DEV, requires_grad=True) for _ in cams]
    color, radii, depth, alpha = rasterize_timed_views(
        [_settings(c, [0.0, 0.0, 0.0], 0) for c in cams], leaf(np.stack([f["means3D"] for f in frames])), m2s,
        leaf(frames[0]["opacities"]), leaf(frames[0]["colors_precomp"]), leaf(np.stack([f["scales"] for f in frames])),
        leaf(np.stack([f["rotations"] for f in frames])))
    ups = [gs.upstream_grads(64, 64, seed=30 + v) for v in range(3)]
    gc, ga = (torch.stack([torch.tensor(u[i], device=DEV) for u in ups]) for i in (0, 2))
    ((color * gc).sum() + (alpha * ga).sum()).backward()
    _check_render_lists(radii, m2s)


def test_update_states_fused_on_the_gpu():
    """A DensifyModel on the GPU at an iteration that does not densify and at one that does, against update_states
    on a clone; no Gaussian lies within the bound of the threshold (asserted), so the selections must agree."""
    from diff_gaussian_rasterization.densify import update_states_fused

    P, V, threshold = 500, 6, 2.0
    scene = gs.make_scene(P, sh_degree=1, seed=8, radius=0.5)
    cfg = dc.quiet_cfg(densify_grad_threshold=threshold,
                       split_thresh=float(np.median(np.linalg.norm(scene["scales"], axis=1))))
    ref, fused = dr.DensifyModel(scene, DEV, **cfg), dr.DensifyModel(scene, DEV, **cfg)
    outs = dc.make_views(V, P, seed=3, device=DEV)
    lists = (outs["visibility_filter"], outs["radii"], outs["viewspace_points"])
    ref.update_states(5, *lists)
    update_states_fused(fused, 5, outs)
    assert not fused.pruned_or_densified
    assert torch.equal(fused.max_radii2D, ref.max_radii2D) and torch.equal(fused.denom, ref.denom)
    want = ref.xyz_gradient_accum.double()
    assert bool(((fused.xyz_gradient_accum.double() - want).abs() <= dc.bound(V) * want).all())
    assert dc.borderline(ref.xyz_gradient_accum, ref.denom, threshold, V) == 0
    sel_ref, sel_fused = dc.select_masks(ref, threshold), dc.select_masks(fused, threshold)
    assert all(torch.equal(a, b) for a, b in zip(sel_ref, sel_fused))
    assert int(sel_ref[0].sum()) > 0 and int(sel_ref[1].sum()) > 0

    ref, fused = dr.DensifyModel(scene, DEV, **cfg), dr.DensifyModel(scene, DEV, **cfg)
    torch.manual_seed(21)
    ref.update_states(1000, *lists)
    torch.manual_seed(21)
    update_states_fused(fused, 1000, outs)
    assert ref.pruned_or_densified and fused.pruned_or_densified
    assert fused.get_xyz.shape[0] == ref.get_xyz.shape[0] == P + int(sel_ref[0].sum()) + int(sel_ref[1].sum())
    assert torch.equal(fused.get_xyz, ref.get_xyz)
    assert math.isfinite(float(fused.get_xyz.detach().sum()))
