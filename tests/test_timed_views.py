"""Timed view sets without a GPU: the argument rules of the new C entry points, the shape rules of
rasterize_timed_views, and the batch renderer's "sugar_temporal" mode on the torch stand-ins."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

import renderer_fixtures as rf
import timed_views_fixtures as tf
from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization import batch_renderer as br
from diff_gaussian_rasterization import batched
from gsr_testutil import gs
from test_batch_renderer import _cpu, _run

H, W = 24, 20


def _structs(**scene_over):
    a = 16  # (never dereferenced: every call below must fail validation first)
    K = (ctypes.c_int * 1)(100)
    ptrs = (ctypes.c_void_p * 1)(a)
    tan = (ctypes.c_float * 1)(0.5)
    fields = dict(V=1, P=10, degree=0, M=0, width=64, height=64, scale_modifier=1.0, scales=a, rotations=a,
                  opacities=a, colors_precomp=a, viewmatrices=ptrs, projmatrices=ptrs, campos=ptrs, bgs=ptrs,
                  tanfovx=tan, tanfovy=tan)
    fields.update(scene_over)
    scene = _C.SetScene(**fields)
    scene._keep = (K, ptrs, tan)
    state = _C.SetState(radii=a, geom=a, binning=a, image=a, num_rendered=K)
    return a, scene, state


def test_entry_points_reject_what_is_not_built():
    lib = _C.load_library()
    a, scene, state = _structs()
    timed = _C.SetTimed(means3D_v=a, scales_v=a, rotations_v=a)
    tg = _C.SetTimedGrads(dL_dmeans3D_v=a, dL_dscales_v=a, dL_drotations_v=a)
    g = dict(dL_dcolor=a, dL_dmeans2D=a, dL_dcolors=a, dL_dopacity=a, work=a, work_bytes=1 << 30)

    def err(rc):
        assert rc == 1
        return lib.gsr_last_error()

    def both(sc, tm, what):
        assert what in err(lib.gsr_set_timed_preprocess(sc, state, tm, None))
        assert what in err(lib.gsr_set_timed_backward(sc, state, _C.SetGrads(**g), tm, tg, None))

    both(_structs(shs=a, colors_precomp=None, M=1)[1], timed, b"shs is not built")
    both(_structs(cov3D_precomp=a, scales=None, rotations=None)[1], timed, b"cov3D_precomp is not built")
    both(scene, _C.SetTimed(scales_v=a, rotations_v=a), b"need means3D_v")
    events = (ctypes.c_void_p * 2)()
    assert b"n_chunks > 0" in err(lib.gsr_set_timed_backward(
        scene, state, _C.SetGrads(n_chunks=2, chunk_events=events, **g), timed, tg, None))
    assert b"colors_override is not built" in err(lib.gsr_set_timed_backward(
        scene, state, _C.SetGrads(colors_override=a, **g), timed, tg, None))
    # a per-view array without its per-view gradient, and a NULL struct
    assert b"per-view gradient" in err(lib.gsr_set_timed_backward(
        scene, state, _C.SetGrads(**g), timed, _C.SetTimedGrads(dL_dmeans3D_v=a, dL_dscales_v=a), None))
    assert b"null pointer argument" in err(lib.gsr_set_timed_preprocess(scene, state, None, None))


def test_null_background_is_rejected_before_any_device_work():
    """A NULL entry of the bgs table fails the validation of gsr_set_render and gsr_set_backward: with no GPU here,
    a call that reached HIP first would report a HIP failure (2) instead."""
    lib = _C.load_library()
    null_bg = (ctypes.c_void_p * 1)(None)
    a, scene, state = _structs(means3D=16, bgs=null_bg)
    out = _C.SetOutputs(out_color=a, out_depth=a, out_alpha=a)
    assert lib.gsr_set_render(scene, state, out, None) == 1
    assert b"null background" in lib.gsr_last_error()
    g = _C.SetGrads(dL_dcolor=a, dL_dmeans2D=a, dL_dcolors=a, dL_dopacity=a, dL_dmeans3D=a, dL_dscales=a,
                    dL_drotations=a, work=a, work_bytes=1 << 30)
    assert lib.gsr_set_backward(scene, state, g, None) == 1
    assert b"null background" in lib.gsr_last_error()


class _StubLib:
    """Stands in for the library under the Python drivers: records the calls' names; sizes are 64 bytes, every view
    renders one instance, everything else succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name == "gsr_set_num_rendered":
                for v in range(args[0]):
                    args[3][v] = 1
            return 64 if name.endswith("_bytes") else 0
        return call


def test_plain_and_timed_forwards_share_one_driver(monkeypatch):
    """Without a device: the forwards of rasterize_views and rasterize_timed_views (V = 3, sets of 2) record the same
    host phases and issue the same library calls in the same order, but for the preprocess entry."""
    V, P = 3, 7
    s = [rf.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                          torch.zeros(3), False, False) for _ in range(V)]
    monkeypatch.setattr(_C, "HOST_TRACE", True)
    monkeypatch.setattr(_C, "_require_gpu", lambda dev: None)
    monkeypatch.setattr(_C, "_stream", lambda dev: None)
    monkeypatch.setattr(_C, "_f32", lambda t, name, dev: None if t is None or t.numel() == 0 else t.contiguous())
    monkeypatch.setattr(batched, "SET_MAX", 2)
    ctx = types.SimpleNamespace(save_for_backward=lambda *t: None, mark_non_differentiable=lambda *t: None)
    m2 = [torch.zeros(P, 3) for _ in range(V)]
    op, col, sc, rot = torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 4)
    runs = {}
    for name in ("plain", "timed"):
        lib = _StubLib()
        monkeypatch.setattr(_C, "load_library", lambda lib=lib: lib)
        _C.host_trace_read(reset=True)
        if name == "plain":
            out = batched._RasterizeViews.forward(ctx, s, None, "fused", False, torch.zeros(P, 3), None, col, op, sc,
                                                  rot, None, None, None, *m2)
        else:
            out = batched._RasterizeTimedViews.forward(ctx, s, False, torch.zeros(V, P, 3), col, op, sc, rot, None,
                                                       None, *m2)
        assert [tuple(t.shape) for t in out] == [(V, 3, H, W), (V, P), (V, 1, H, W), (V, 1, H, W)]
        assert [(vs.lo, vs.hi, vs.K) for vs in ctx.sets] == [(0, 2, [1, 1]), (2, 3, [1])]
        runs[name] = (set(_C.host_trace_read(reset=True)), lib.calls)
    _C.host_trace_read(reset=True)
    assert runs["plain"][0] == runs["timed"][0] == {"fwd_setup", "fwd_preprocess_launch", "fwd_sync_wait",
                                                    "fwd_render_launch"}
    assert "gsr_set_timed_preprocess" in runs["timed"][1] and runs["plain"][1].count("gsr_set_preprocess") == 2
    assert [c.replace("gsr_set_timed_preprocess", "gsr_set_preprocess") for c in runs["timed"][1]] == runs["plain"][1]
    # both preprocesses are enqueued before the first host sync
    assert runs["plain"][1].index("gsr_set_num_rendered") > max(
        i for i, c in enumerate(runs["plain"][1]) if c == "gsr_set_preprocess")


def test_rasterize_timed_views_checks_shapes_before_device_work():
    """Every bad argument raises ValueError on CPU tensors: nothing reaches the library (which has no CPU path)."""
    V, P = 3, 7
    s = [rf.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                          torch.zeros(3), False, False) for _ in range(V)]
    ok = dict(means3D=torch.zeros(V, P, 3), means2D_list=[torch.zeros(P, 3) for _ in range(V)],
              opacities=torch.zeros(P, 1), colors_precomp=torch.zeros(P, 3), scales=torch.zeros(V, P, 3),
              rotations=torch.zeros(P, 4))

    def bad(match, **over):
        with pytest.raises(ValueError, match=match):
            batched.rasterize_timed_views(s, **dict(ok, **over))

    bad("means3D has shape", means3D=torch.zeros(P, 3))
    bad("means3D has shape", means3D=torch.zeros(V + 1, P, 3))
    bad("scales has shape", scales=torch.zeros(V, P + 1, 3))
    bad("rotations has shape", rotations=torch.zeros(V, P, 3))
    bad("colors2 has shape", colors2=torch.zeros(V, P, 4))
    bad("colors_precomp has shape", colors_precomp=torch.zeros(V, P, 3))
    bad("opacities has", opacities=torch.zeros(V, P, 1))
    bad("one means2D placeholder per view", means2D_list=[torch.zeros(P, 3)])
    bad("background must hold", background=torch.zeros(V, H, W))
    bad("expected torch.float32", means3D=torch.zeros(V, P, 3, dtype=torch.float64))
    bad("grad_reduce", grad_reduce=object())
    bad("no CPU path")  # (all shapes right: the device is checked last, still before any library call)
    with pytest.raises(ValueError, match="at least one view"):
        batched.rasterize_timed_views([], **ok)


def _scene():
    sc = gs.make_sugar_scene(1, sh_degree=0, seed=2)
    sc["shs"] = sc["shs"][:, :1]
    return sc


@pytest.mark.parametrize("d_scale", [True, False])
def test_sugar_temporal_equals_per_view_loop(d_scale, monkeypatch):
    """The fused "sugar_temporal" mode against the reference's per-view loop over the same renderer (fp64 torch
    stand-ins, B = 5 frames that differ): outputs, per-view viewspace gradients and parameter gradients within the
    tolerances of test_batch_renderer.test_fused_equals_per_view_loop; no RNG draw consumed; the timed getters
    called once per batch."""
    _cpu(monkeypatch)
    monkeypatch.setattr(br, "_rasterize_timed_views", tf.torch_rasterize_timed_views)
    B = 5
    batch = tf.make_timed_batch(B, H, W, "cpu", torch.float64)
    random.seed(11), np.random.seed(11)
    want_draws = (random.random(), np.random.rand())
    random.seed(11), np.random.seed(11)
    r_fused = tf.TimedRenderer("sugar_temporal", _scene(), "cpu", torch.float64, training=True, d_scale=d_scale)
    fused, g_fused = _run(r_fused, dict(batch))
    assert (random.random(), np.random.rand()) == want_draws, "sugar_temporal consumed a random draw"
    assert r_fused.geometry.calls == dict(attributes=1, normals=1)
    r_ref = tf.TimedRenderer("per_view", _scene(), "cpu", torch.float64, training=True, d_scale=d_scale)
    ref, g_ref = _run(r_ref, dict(batch))
    assert r_ref.geometry.calls == dict(attributes=B, normals=B)
    keys = set(k for k in ref if k.startswith("comp_"))
    assert keys == set(k for k in fused if k.startswith("comp_"))
    assert keys == {"comp_rgb", "comp_normal", "comp_normal_from_dist", "comp_depth", "comp_mask"}
    # the frames differ: frame 0's geometry in every view would be another image
    assert float((ref["comp_rgb"][0] - ref["comp_rgb"][B - 1]).detach().abs().max()) > 0.1
    for k in keys:
        assert fused[k].shape == ref[k].shape, k
        torch.testing.assert_close(fused[k], ref[k], rtol=1e-12, atol=1e-12)
    for i in range(B):
        assert torch.equal(fused["radii"][i], ref["radii"][i])
        assert torch.equal(fused["visibility_filter"][i], ref["visibility_filter"][i])
        torch.testing.assert_close(fused["viewspace_points"][i].grad, ref["viewspace_points"][i].grad,
                                   rtol=1e-10, atol=1e-12)
    assert set(g_ref) == set(g_fused) and "drift" in g_ref
    for k in g_ref:
        torch.testing.assert_close(g_fused[k], g_ref[k], rtol=1e-10, atol=1e-12)


def test_sugar_temporal_is_opt_in():
    class R:
        pass

    R.__module__ = "threestudio_3dgs.renderer.diff_sugar_rasterizer_temporal"
    assert br.batch_mode(R()) is None
    r = R()
    r.batch_render_mode = "sugar_temporal"
    assert br.batch_mode(r) == "sugar_temporal" and "sugar_temporal" in br.MODES
