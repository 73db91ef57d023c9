"""The fused shading / depth-normal epilogue and the SuGaR normal map (csrc/gsr_shading.hip, gsr_normal_map_*) on
inputs that look like a render: an empty background, a silhouette, one-pixel spurs on the tile seams and image
borders, opaque surfaces across every seam, a light on the surface (tests/shading_cases.py).  Every output and
gradient is held per pixel to `check_pixels` against the torch restatement in fp64, with the fp32 restatement as the
null; only the decision ties the two references leave open are excused (tests/test_shading_cases.py caps them)."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import shading_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_SHAPES = [("silhouette",) + sc.SILHOUETTE_SHAPE] + [(n, H, W) for n in ("spurs", "seams", "light_on_surface")
                                                          for (H, W) in sc.SHAPES]
IDS = [f"{n}-{H}x{W}" for n, H, W in CASE_SHAPES]


def _stack(scenes, k):
    return torch.stack([s[k] for s in scenes]).cuda()


def _gpu_shade(scenes, shading, use_pred=False, ka=sc.KA, kd=sc.KD, bg_const=False, which=None):
    """Per view, the outputs and gradients of shade_views by the names of shading_cases.reference."""
    from diff_gaussian_rasterization.shading import shade_views

    leaves = {k: _stack(scenes, k).requires_grad_(True) for k in ("color", "depth", "alpha")}
    bg = torch.stack([s["bg"][0, 0] for s in scenes]).cuda() if bg_const else _stack(scenes, "bg")
    leaves["bg"] = bg.requires_grad_(True)
    outs = shade_views(leaves["color"], leaves["depth"], leaves["alpha"], _stack(scenes, "rays_o"),
                       _stack(scenes, "rays_d"), leaves["bg"], _stack(scenes, "light"), ka, kd, shading,
                       _stack(scenes, "pred") if use_pred else None)
    return _finish(scenes, "shade", outs, leaves, which)


def _gpu_depth_normal(scenes, which=None):
    from diff_gaussian_rasterization.shading import depth_normal_views

    leaves = {k: _stack(scenes, k).requires_grad_(True) for k in ("depth", "alpha")}
    outs = depth_normal_views(leaves["depth"], leaves["alpha"], _stack(scenes, "rays_o"), _stack(scenes, "rays_d"))
    return _finish(scenes, "depth_normal", outs, leaves, which)


def _finish(scenes, entry, outs, leaves, which):
    names = sc.ENTRY_OUTPUTS[entry]
    which = tuple(range(len(names))) if which is None else tuple(which)
    loss = sum((outs[i] * torch.stack([s["ups"][i] for s in scenes]).cuda()).sum() for i in which)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return [dict({n: o[v].detach().cpu() for n, o in zip(names, outs)},
                 **{"d" + k: g[v].cpu() for k, g in zip(leaves, grads)}) for v in range(len(scenes))]


def _check_views(tag, scenes, got, ties=None, **ref_kw):
    """Every view against its references; per-view keywords are given as lists."""
    for v, s in enumerate(scenes):
        kw = {k: (x[v] if isinstance(x, list) else x) for k, x in ref_kw.items()}
        r64, n32 = sc.references(s, **kw)
        sc.check_pixels(got[v], r64, n32, None if ties is None else ties[v], tag=f"{tag} view {v}")


@pytest.mark.parametrize("name,H,W", CASE_SHAPES, ids=IDS)
def test_shade_views_cases(name, H, W):
    """The three modes, with and without a predicted normal map, per-pixel background; and the constant-background
    layout (diffuse)."""
    scenes = sc.get(name, H, W, 2)
    for shading in sc.MODES:
        for use_pred in (False, True):
            ties, _ = sc.tie_masks(scenes, shading, use_pred)
            got = _gpu_shade(scenes, shading, use_pred)
            _check_views(f"{name} {H}x{W} {shading}{' pred' if use_pred else ''}", scenes, got, ties, shading=shading,
                         use_pred=use_pred)
    ties, _ = sc.tie_masks(scenes, "diffuse", bg_const=True)
    got = _gpu_shade(scenes, "diffuse", bg_const=True)
    _check_views(f"{name} {H}x{W} diffuse constant-bg", scenes, got, ties, shading="diffuse", bg_const=True)


@pytest.mark.parametrize("bg_const", [False, True], ids=["hwc", "constant"])
def test_shade_views_view_tables_across_the_launch_chunk(bg_const):
    """65 views of the silhouette with per-view (mode, ka, kd): the 65th view runs in the second launch with its own
    table entry."""
    H, W = sc.CHUNK_SHAPE
    scenes = sc.get("silhouette", H, W, sc.CHUNK_VIEWS)
    modes, ka, kd = sc.view_tables(sc.CHUNK_VIEWS)
    assert set(modes) == set(sc.MODES) and modes[64] != modes[0]
    ties, _ = sc.tie_masks(scenes, modes, False, ka, kd, bg_const)
    got = _gpu_shade(scenes, modes, False, ka, kd, bg_const)
    _check_views(f"silhouette {H}x{W} V=65 tables{' constant-bg' if bg_const else ''}", scenes, got, ties,
                 shading=modes, ka=ka, kd=kd, bg_const=bg_const)


@pytest.mark.parametrize("name,H,W", CASE_SHAPES + [("silhouette",) + sc.CHUNK_SHAPE], ids=IDS + ["silhouette-V65"])
def test_depth_normal_views_cases(name, H, W):
    V = sc.CHUNK_VIEWS if (name, (H, W)) == ("silhouette", sc.CHUNK_SHAPE) else 2
    scenes = sc.get(name, H, W, V)
    _check_views(f"{name} {H}x{W} depth_normal", scenes, _gpu_depth_normal(scenes), entry="depth_normal")


@pytest.mark.parametrize("name,H,W", sc.NORMAL_MAP_CASES)
def test_sugar_normal_map_cases(name, H, W):
    from diff_gaussian_rasterization.shading import sugar_normal_map

    scenes = sc.normal_map_scene(name, H, W)
    leaves = {k: _stack(scenes, k).requires_grad_(True) for k in ("normal", "alpha")}
    out = sugar_normal_map(leaves["normal"], leaves["alpha"])
    got = _finish(scenes, "normal_map", (out,), leaves, None)
    _check_views(f"{name} {H}x{W} normal_map", scenes, got, entry="normal_map")


SUBSET_CASES = [("silhouette",) + sc.SILHOUETTE_SHAPE, ("spurs", 17, 65)]


@pytest.mark.parametrize("name,H,W", SUBSET_CASES)
def test_upstream_subsets(name, H, W):
    """An upstream gradient on one output only: what nothing feeds is exactly zero, the rest matches the reference."""
    scenes = sc.get(name, H, W, 2)
    ties, _ = sc.tie_masks(scenes, "diffuse")
    fed = {0: ("dcolor", "ddepth", "dalpha", "dbg"), 1: ("ddepth", "dalpha"), 2: ("ddepth",)}
    for i, out in enumerate(sc.ENTRY_OUTPUTS["shade"]):
        got = _gpu_shade(scenes, "diffuse", which=(i,))
        for v in range(len(scenes)):
            for k in ("dcolor", "ddepth", "dalpha", "dbg"):
                if k not in fed[i]:
                    assert not got[v][k].any(), (name, out, v, k)
        _check_views(f"{name} {H}x{W} upstream {out}", scenes, got, ties, shading="diffuse", which=(i,))
    for i, out in enumerate(sc.ENTRY_OUTPUTS["depth_normal"]):
        got = _gpu_depth_normal(scenes, which=(i,))
        if out == "unit":  # the unit normal does not depend on alpha
            assert all(not g["dalpha"].any() for g in got)
        _check_views(f"{name} {H}x{W} depth_normal upstream {out}", scenes, got, entry="depth_normal", which=(i,))


def _abi_backward(scenes, material, g_render=None, g_nmap=None, g_unit=None, g_depth=None):
    """gsr_shade_views_backward called directly, so that an absent upstream gradient is a NULL pointer (autograd
    hands the Python wrapper zeros instead).  The outputs start as NaN: whatever the kernel leaves unwritten shows."""
    from diff_gaussian_rasterization import _C

    lib = _C.load_library()
    V = len(scenes)
    _, H, W = scenes[0]["depth"].shape
    t = {k: _stack(scenes, k).contiguous() for k in ("color", "depth", "alpha", "rays_o", "rays_d", "bg", "light")}
    nan = lambda x: torch.full_like(x, float("nan"))  # noqa: E731
    d = dict(dcolor=nan(t["color"]) if material else None, ddepth=nan(t["depth"]), dalpha=nan(t["alpha"]),
             dbg=nan(t["bg"]) if material else None)
    modes = (ctypes.c_int * V)(*([0] * V))
    ka, kd = (ctypes.c_float * (3 * V))(*(sc.KA * V)), (ctypes.c_float * (3 * V))(*(sc.KD * V))
    p = _C._ptr
    _C._check(lib.gsr_shade_views_backward(
        V, H, W, 1 if material else 0, modes, p(t["color"]) if material else None, p(t["depth"]), p(t["alpha"]),
        p(t["rays_o"]), p(t["rays_d"]), p(t["bg"]) if material else None, 1 if material else 0,
        p(t["light"]) if material else None, None, ka, kd, p(g_render), p(g_nmap), p(g_unit), p(g_depth),
        p(d["dcolor"]), p(d["ddepth"]), p(d["dalpha"]), p(d["dbg"]), _C._stream(t["depth"].device)))
    torch.cuda.synchronize()
    return [{k: x[v].cpu() for k, x in d.items() if x is not None} for v in range(V)]


@pytest.mark.parametrize("name,H,W", SUBSET_CASES)
def test_absent_upstream_pointers_equal_zero_upstreams(name, H, W):
    """include/gsr.h: any upstream gradient may be NULL = zero.  Each single-upstream backward with the others NULL
    gives the bits of the autograd path (which passes zero tensors), and every output is written whole."""
    scenes = sc.get(name, H, W, 2)
    ups = [torch.stack([s["ups"][i] for s in scenes]).cuda().contiguous() for i in range(3)]
    for i, kw in enumerate(({"g_render": ups[0]}, {"g_nmap": ups[1]}, {"g_depth": ups[2]})):
        want = _gpu_shade(scenes, "diffuse", which=(i,))
        got = _abi_backward(scenes, True, **kw)
        for v in range(len(scenes)):
            for k in ("dcolor", "ddepth", "dalpha", "dbg"):
                assert torch.isfinite(got[v][k]).all(), (name, i, v, k, "left unwritten")
                assert torch.equal(got[v][k], want[v][k]), (name, i, v, k)
    for i, kw in enumerate(({"g_unit": ups[0]}, {"g_nmap": ups[1]})):
        want = _gpu_depth_normal(scenes, which=(i,))
        got = _abi_backward(scenes, False, **kw)
        for v in range(len(scenes)):
            for k in ("ddepth", "dalpha"):
                assert torch.equal(got[v][k], want[v][k]), (name, i, v, k)
    got = _abi_backward(scenes, True)  # nothing upstream at all: everything exactly zero
    assert all(not g[k].any() for g in got for k in g)


def test_two_calls_give_the_same_bits():
    scenes = sc.get("silhouette", *sc.SILHOUETTE_SHAPE, 2)
    for run in (lambda: _gpu_shade(scenes, "diffuse"), lambda: _gpu_depth_normal(scenes)):
        a, b = run(), run()
        for x, y in zip(a, b):
            for k in x:
                assert torch.equal(x[k], y[k]), k
