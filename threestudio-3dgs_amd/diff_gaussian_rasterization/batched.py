"""View-batched rasterization: one set of Gaussians, V cameras, one autograd node.

Equivalent to calling GaussianRasterizer once per view (same per-view outputs and gradients), but the
views are rendered as view sets of up to 64 (include/gsr.h, gsr_set_*): every stage — preprocess,
depth sort, instance emission, tile sort, blend, backward blend, per-Gaussian backward — is ONE launch
per set instead of one per view, sorts are segmented by view, and the instance counts of all views are
read back with one host sync.  The reference renders a batch with a Python loop over views
(renderer/gaussian_batch_renderer.py:9-122); this replaces the loop's V rasterizer calls.

Per-view outputs (color, radii, depth, alpha) and per-view means2D gradients (the densification
statistic of geometry/gaussian_base.py:815-818) are kept; shared-parameter gradients are summed over
views inside the per-Gaussian kernel.
"""
from __future__ import annotations

import ctypes
import math
import os
import time
import types

import torch

from . import _C

SET_MAX = 64
# device memory the backward may use at once for gradient rows (views are walked in groups that fit)
WORK_BUDGET = int(os.environ.get("GSR_BWD_WORK_BYTES", str(24 << 30))) & ~255  # (256-byte granularity)


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _ptrs(ts):
    return _arr(ctypes.c_void_p, [t.data_ptr() for t in ts])


def _addr(t):
    """The device address of a tensor for a struct field (None: NULL)."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


class _ViewSet:
    """Forward state of one set of views: the scene and state structs of include/gsr.h, built once in the forward
    and reused by the backward, and the Python objects whose addresses they hold."""

    def __init__(self, lo, hi, cams, tanx, tany, gaussians, radii, **shared):
        self.lo, self.hi = lo, hi
        # [(view, proj, campos, bg)], the Gaussians' arrays and the set's rows of radii: contiguous fp32 / int32
        # device tensors, kept alive with the structs that point at them
        self.cams, self.gaussians, self.radii = cams, gaussians, radii
        self.K = None
        self.geom = self.binning = self.image = None
        self.scene = _C.SetScene(
            V=hi - lo, viewmatrices=_ptrs([c[0] for c in cams]), projmatrices=_ptrs([c[1] for c in cams]),
            campos=_ptrs([c[2] for c in cams]), bgs=_ptrs([c[3] for c in cams]),
            tanfovx=_arr(ctypes.c_float, tanx), tanfovy=_arr(ctypes.c_float, tany), **shared,
            **{name: _addr(t) for name, t in gaussians.items()})
        self.state = _C.SetState(radii=_addr(radii))

    @property
    def V(self):
        return self.hi - self.lo

    def allocate(self, **buffers):
        """Keep the set's geom / binning / image buffers and point the state at them."""
        for name, t in buffers.items():
            setattr(self, name, t)
            setattr(self.state, name, _addr(t))


def _view_set(lo, settings, gaussians, radii):
    """The _ViewSet of views lo .. lo + len(settings) of a batch: their cameras, the Gaussians' arrays and their rows
    of radii (the sizes and flags the views of a batch share are read from the first)."""
    s0, dev = settings[0], radii.device
    f = lambda t, n: _C._f32(t, n, dev)  # noqa: E731
    cams = [(f(s.viewmatrix, "viewmatrix"), f(s.projmatrix, "projmatrix"), f(s.campos, "campos"), f(s.bg, "bg"))
            for s in settings]
    return _ViewSet(lo, lo + len(settings), cams, [float(s.tanfovx) for s in settings],
                    [float(s.tanfovy) for s in settings], gaussians, radii, P=int(radii.shape[1]),
                    degree=int(s0.sh_degree), M=_C.sh_coeff_count(gaussians["shs"]), width=int(s0.image_width),
                    height=int(s0.image_height), prefiltered=int(bool(s0.prefiltered)),
                    scale_modifier=float(s0.scale_modifier))


def _forward_sets(settings_list, gaussians, P, dev, composite_bg, clamp, preprocess, colors2_of=None):
    """The forward of a batch as view sets.  preprocess(vs, stream) enqueues a set's preprocess; colors2_of(vs) is the
    set's second colours (None: one colour).  Every preprocess is enqueued before the first host sync.  Returns the
    sets and the output tensors."""
    t0 = time.perf_counter()
    lib = _C.load_library()
    V = len(settings_list)
    H, W = int(settings_list[0].image_height), int(settings_list[0].image_width)
    stream = _C._stream(dev)
    fopt = dict(dtype=torch.float32, device=dev)
    color = torch.empty((V, 3, H, W), **fopt)
    cbg = None
    # the renderer's clamp(0, 1) fused into the blends without a background image (clamp_only) or with it
    clamp_only = bool(clamp) and composite_bg is None
    if composite_bg is not None:
        cbg = _C._f32(composite_bg, "background", dev).reshape(V, H, W, 3)
    fused_out = cbg is not None or clamp_only
    render = torch.empty((V, 3, H, W), **fopt) if fused_out else None
    depth = torch.empty((V, 1, H, W), **fopt)
    alpha = torch.empty((V, 1, H, W), **fopt)
    color2 = torch.empty((V, 3, H, W), **fopt) if colors2_of is not None else None
    radii = torch.empty((V, P), dtype=torch.int32, device=dev)
    sets = []
    for lo in range(0, V, SET_MAX):
        vs = _view_set(lo, settings_list[lo:lo + SET_MAX], gaussians, radii[lo:lo + SET_MAX])
        vs.allocate(geom=torch.empty(int(lib.gsr_set_geom_bytes(vs.V, P)), dtype=torch.uint8, device=dev))
        t0 = _C.host_mark("fwd_setup", t0)
        preprocess(vs, stream)
        sets.append(vs)
        t0 = _C.host_mark("fwd_preprocess_launch", t0)
    for vs in sets:
        K = (ctypes.c_int * vs.V)()
        L = (ctypes.c_int * vs.V)()
        # the reference's one host sync: the instance counts size the binning buffers
        _C._check(lib.gsr_set_num_rendered(vs.V, _C._ptr(vs.geom), P, K, None, L, stream))
        t0 = _C.host_mark("fwd_sync_wait", t0)
        vs.K = list(K)
        _C.RECENT_LISTED.extend(L)
        _C.RECENT_FORWARDS.extend((k, H, W) for k in vs.K)
        vs.state.num_rendered = K
        vs.allocate(
            binning=torch.empty(int(lib.gsr_set_binning_bytes(vs.V, P, K, W, H)), dtype=torch.uint8, device=dev),
            image=torch.empty(int(lib.gsr_set_image_bytes(vs.V, P, K, W, H, int(colors2_of is not None))),
                              dtype=torch.uint8, device=dev))
        sl = slice(vs.lo, vs.hi)
        out = _C.SetOutputs(out_color=_addr(color[sl]), out_depth=_addr(depth[sl]), out_alpha=_addr(alpha[sl]))
        if cbg is not None:
            out.bg_images = _addr(cbg[sl])
        if fused_out:
            out.out_render = _addr(render[sl])
        if colors2_of is not None:
            out.colors2, out.out_color2 = _addr(colors2_of(vs)), _addr(color2[sl])
        _C._check(lib.gsr_set_render(vs.scene, vs.state, out, stream))
        t0 = _C.host_mark("fwd_render_launch", t0)
    return types.SimpleNamespace(sets=sets, color=color, render=render, depth=depth, alpha=alpha, color2=color2,
                                 radii=radii, cbg=cbg)


def _outputs(r):
    """(render if the forward fused a clamp or composite else color, radii, depth, alpha[, color2])."""
    first = r.color if r.render is None else r.render
    return (first, r.radii, r.depth, r.alpha) if r.color2 is None else (first, r.radii, r.depth, r.alpha, r.color2)


def _set_work(lib, vs, two):
    """The backward's work buffer for a set: all its views' gradient rows when WORK_BUDGET allows, one view's at the
    least (the scratch grows with K: the largest single view bounds what a view group needs)."""
    P = vs.scene.P
    kmax = _arr(ctypes.c_int, [max(vs.K)])
    need = int(lib.gsr_set_backward_bytes(vs.V, P, vs.state.num_rendered, int(two)))
    largest = int(lib.gsr_set_backward_bytes(1, P, kmax, int(two)))
    return torch.empty(max(largest, min(need, WORK_BUDGET)), dtype=torch.uint8, device=vs.geom.device)


def _upstream(g):
    return g.float().contiguous() if g is not None else None


def _set_grads(g, vs, rows, work, accumulate):
    """Point the per-set fields of a SetGrads at the set's views: rows maps a field to its (V, ...) tensor or None."""
    for name, t in rows.items():
        setattr(g, name, _addr(t[vs.lo:vs.hi]) if t is not None else None)
    g.accumulate = int(accumulate)
    g.work, g.work_bytes = _addr(work), work.numel()


def _masked_grads(ctx, grads, bg_at):
    """The backward's gradient list with dL/dbackground (at bg_at) in the caller's shape and None where no gradient is
    needed."""
    if grads[bg_at] is not None:
        grads[bg_at] = grads[bg_at].reshape(ctx.bg_shape)
    return [g if need else None for g, need in zip(grads, ctx.needs_input_grad)]


def _check_views(settings_list, background, size_error):
    """The rules every view of a batch obeys (size_error: what a mismatch of image sizes raises)."""
    s0 = settings_list[0]
    H, W = int(s0.image_height), int(s0.image_width)
    if any(int(s.image_height) != H or int(s.image_width) != W for s in settings_list):
        raise size_error("all views of a batch must have the same image size")
    if any(int(s.sh_degree) != int(s0.sh_degree) or float(s.scale_modifier) != float(s0.scale_modifier)
           or bool(s.prefiltered) != bool(s0.prefiltered) for s in settings_list):
        raise ValueError("sh_degree, scale_modifier and prefiltered must be shared by the views of a batch")
    if background is not None and background.numel() != len(settings_list) * H * W * 3:
        raise ValueError("background must hold (V, H, W, 3) values")


# A two-colour forward hands colors2 to the preprocess too (gsr_set_preprocess), which writes each Gaussian's
# second colour into the record it writes anyway; the blends then read it from the record's line.  False: the
# blends gather colors2 apart (the same bits; tests/test_gpu_configs.py compares the two).
EMBED_COLORS2 = True


class _RasterizeViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, settings_list, grad_reduce, two_color_bwd, clamp, means3D, sh, colors_precomp, opacities, scales,
                rotations, cov3D_precomp, composite_bg, colors2, *means2D):
        t0 = time.perf_counter()
        lib = _C.load_library()
        dev = means3D.device
        _C._require_gpu(dev)
        P = int(means3D.shape[0])
        f = lambda t, n: _C._f32(t, n, dev)  # noqa: E731
        m3, shc, col, op, sc, rot, c3 = (f(means3D, "means3D"), f(sh, "sh"), f(colors_precomp, "colors_precomp"),
                                         f(opacities, "opacities"), f(scales, "scales"), f(rotations, "rotations"),
                                         f(cov3D_precomp, "cov3D_precomp"))
        if (shc is None) == (col is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        c2 = None
        if colors2 is not None:
            c2 = f(colors2, "colors2")
            if c2.numel() != 3 * P:
                raise _C.GSRError(f"colors2 has {c2.numel()} elements, expected {3 * P}")
        gaussians = dict(means3D=m3, scales=sc, rotations=rot, opacities=op, shs=shc, colors_precomp=col,
                         cov3D_precomp=c3)

        # (the second colour set, when there is one, rides in the records the preprocess writes: the two-colour
        # blends then read it with the record instead of gathering it apart)
        def preprocess(vs, stream):
            _C._check(lib.gsr_set_preprocess(vs.scene, vs.state, _C._ptr(c2) if EMBED_COLORS2 else None, stream))

        _C.host_mark("fwd_setup", t0)
        r = _forward_sets(settings_list, gaussians, P, dev, composite_bg, clamp, preprocess,
                          (lambda vs: c2) if c2 is not None else None)
        ctx.settings = settings_list
        ctx.grad_reduce = grad_reduce
        ctx.two_color_bwd = two_color_bwd
        ctx.sets = r.sets
        ctx.bg_shape = tuple(composite_bg.shape) if composite_bg is not None else None
        ctx.save_for_backward(m3, shc, col, sc, rot, c3, r.radii, r.cbg, r.color if r.render is not None else None, c2)
        ctx.mark_non_differentiable(r.radii)
        return _outputs(r)

    @staticmethod
    def backward(ctx, g_color, _g_radii, g_depth, g_alpha, g_color2=None):
        t0 = time.perf_counter()
        lib = _C.load_library()
        m3, shc, col, sc, rot, c3, radii, cbg, color, c2 = ctx.saved_tensors
        second = c2 is not None and g_color2 is not None
        V = len(ctx.settings)
        dev = m3.device
        P = int(m3.shape[0])
        M = _C.sh_coeff_count(shc)
        fopt = dict(dtype=torch.float32, device=dev)
        d_m2 = torch.empty((V, P, 3), **fopt)
        # the per-Gaussian gradients are carved from one buffer (means3D, scales, rotations, opacities,
        # SH, cov3D, colours): autograd hands these views to the leaves as their .grad, and
        # view_shard.allreduce_grads then sums them over ranks in place as one span, without copies
        widths = [("m3", (3,)), ("sc", (3,) if c3 is None else None), ("rot", (4,) if c3 is None else None),
                  ("op", (1,)), ("sh", (M, 3) if shc is not None else None), ("c3", (6,) if c3 is not None else None),
                  ("col", (3,))]
        flat = torch.empty(P * sum(math.prod(w) for _, w in widths if w is not None), **fopt)
        carved, off = {}, 0
        for name, w in widths:
            carved[name] = None
            if w is not None:
                n = P * math.prod(w)
                carved[name] = flat[off:off + n].view((P,) + w)
                off += n
        d_m3, d_sc, d_rot, d_op = carved["m3"], carved["sc"], carved["rot"], carved["op"]
        d_sh, d_c3, d_col = carved["sh"], carved["c3"], carved["col"]
        d_bg = torch.empty_like(cbg) if cbg is not None and ctx.needs_input_grad[11] else None
        # more than one view set in the scale / rotation path: the running dL/dcov3D the later sets
        # continue from (include/gsr.h gsr_set_backward, accumulate)
        d_c2 = torch.zeros((P, 3), **fopt) if second else None
        if d_c3 is None and (len(ctx.sets) > 1 or second):
            d_c3 = torch.empty((P, 6), **fopt)
            ctx.needs_c3_scratch = True
        if P == 0:
            if d_bg is not None:
                d_bg.zero_()
            for t in (d_m2, d_m3, d_op, d_col, d_sh, d_c3, d_sc, d_rot, d_c2):
                if t is not None:
                    t.zero_()
        else:
            stream = _C._stream(dev)
            # both calls of a two-colour forward in one backward pass (the colors2 fields of gsr_set_grads);
            # two_color_backward="separate" runs the second call's backward after the first's instead
            fused2 = second and ctx.two_color_bwd != "separate"
            g2 = _upstream(g_color2) if second else None
            # (a forward with a fused clamp or composite: dL_dcolor is dL/drender, masked by the forward's colour)
            rows = dict(dL_dcolor=_upstream(g_color), dL_ddepth=_upstream(g_depth), dL_dalpha=_upstream(g_alpha),
                        color=color, bg_images=cbg, dL_dbg=d_bg, dL_dmeans2D=d_m2, dL_dcolor2=g2 if fused2 else None)
            reducer = ctx.grad_reduce if ctx.grad_reduce is not None and ctx.grad_reduce.active() else None
            # per-range events only when the last set's call is the last writer of the per-Gaussian sums: with
            # the second colour's backward run separately after it (two_color_backward="separate"), that call
            # adds into the same gradients, so the reduction waits for the whole stream instead
            events = reducer.chunk_events(dev) if reducer is not None and (fused2 or not second) else None
            # what every call of this backward shares; the per-set fields are assigned in the loop
            shared = dict(dL_dopacity=_addr(d_op), dL_dmeans3D=_addr(d_m3), dL_dcov3D=_addr(d_c3),
                          dL_dscales=_addr(d_sc), dL_drotations=_addr(d_rot))
            g = _C.SetGrads(dL_dcolors=_addr(d_col), dL_dsh=_addr(d_sh), **shared)
            if fused2:
                g.colors2, g.dL_dcolors2 = _addr(c2), _addr(d_c2)
            for si, vs in enumerate(ctx.sets):
                if events is not None and si == len(ctx.sets) - 1:
                    # the last set's call forms the final per-Gaussian sums: in ranges, an event after each
                    g.n_chunks, g.chunk_events = len(events), _arr(ctypes.c_void_p, [e.cuda_event for e in events])
                work = _set_work(lib, vs, fused2)
                _set_grads(g, vs, rows, work, accumulate=si > 0)
                _C._check(lib.gsr_set_backward(vs.scene, vs.state, g, stream))
                if second and not fused2:
                    # the second call's backward on the shared forward state: precomputed colours, so a scene
                    # without SHs (its screen-space gradient is discarded, as the reference's fresh zero means2D
                    # of that call is)
                    scene2 = _C.SetScene.from_buffer_copy(vs.scene)
                    scene2.shs = None
                    m2_scratch = torch.empty((vs.V, P, 3), **fopt)
                    _C._check(lib.gsr_set_backward(scene2, vs.state, _C.SetGrads(
                        colors_override=_addr(c2), dL_dcolor=_addr(g2[vs.lo:vs.hi]), dL_dmeans2D=_addr(m2_scratch),
                        dL_dcolors=_addr(d_c2), accumulate=1, work=_addr(work), work_bytes=work.numel(), **shared),
                        stream))
        if getattr(ctx, "needs_c3_scratch", False):
            d_c3 = None
        grads = _masked_grads(ctx, [None, None, None, None, d_m3, d_sh, d_col, d_op, d_sc, d_rot, d_c3, d_bg, d_c2]
                              + [d_m2[v] for v in range(V)], bg_at=11)
        if ctx.grad_reduce is not None and P > 0:
            # the per-Gaussian gradients' sums over ranks, range by range as the backward finishes them
            shared = [grads[k] for k in (4, 5, 6, 7, 8, 9, 10, 12)]
            ctx.grad_reduce.launch(shared, P, events if P > 0 else None)
        _C.host_mark("bwd_host", t0)
        return tuple(grads)


def rasterize_views(settings_list, means3D, means2D_list, opacities, shs=None, colors_precomp=None, scales=None,
                    rotations=None, cov3D_precomp=None, background=None, colors2=None, grad_reduce=None,
                    two_color_backward="fused", clamp=False):
    """Render V views of one set of Gaussians.  settings_list: V GaussianRasterizationSettings (same image
    size, same sh_degree, scale_modifier and prefiltered flag); means2D_list: V screen-space placeholders
    (P, 3) whose .grad receives each view's viewspace gradient.  Returns (color (V,3,H,W), radii (V,P),
    depth (V,1,H,W), alpha (V,1,H,W)).

    background: the background renderer's composite fused into the blends — the background network's
    images (V, H, W, 3) (renderer/diff_gaussian_rasterizer_background.py:116,129-132,139); the first
    output is then render = clamp(color + (1 - alpha) * background, 0, 1) (bit-identical to the torch
    expression, same gradients incl. the background's) instead of color.

    clamp=True without a background: the first output is the renderers' ``rendered_image.clamp(0, 1)``
    (e.g. renderer/diff_sugar_rasterizer_normal.py:212, renderer/diff_gaussian_rasterizer.py:141) formed in the
    blend kernels, its gradient mask in the backward's per-pixel prologue: the same bits as clamping the colour
    output in torch, without its four elementwise passes over the images.

    colors2 (P, 3): a second rasterizer call that differs only in its colours — the SuGaR normal renderer's
    ``rasterizer(..., means2D=zeros_like(means2D), shs=None, colors_precomp=pc.get_gs_normals, ...)``
    (renderer/diff_sugar_rasterizer_normal.py:182-191) — rendered from the same geometry, sorts and blend
    weights (include/gsr.h gsr_set_outputs.colors2); a fifth output holds its colour image (V, 3, H, W).
    Its backward adds that call's parameter gradients (colors2 receives its colour gradient); its
    screen-space gradient is not added to means2D, as in the reference.

    grad_reduce (view_shard.ChunkedGradReduce): with torch.distributed initialised, the per-Gaussian
    parameter gradients are summed over ranks inside the backward, range by range as they are formed
    (overlapping the per-Gaussian backward); the screen-space and background gradients stay per rank.

    two_color_backward: "fused" (default) replays both calls of a colors2 forward in one backward pass;
    "separate" runs the second call's backward after the first's, as two rasterizer calls would (same
    gradients up to fp32 summation order; tests compare the two)."""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    if len(means2D_list) != len(settings_list):
        raise ValueError("one means2D placeholder per view")
    if not settings_list:
        raise ValueError("at least one view")
    _check_views(settings_list, background, size_error=_C.GSRError)
    if two_color_backward not in ("fused", "separate"):
        raise ValueError("two_color_backward is 'fused' or 'separate'")
    return _RasterizeViews.apply(list(settings_list), grad_reduce, two_color_backward, bool(clamp), means3D, shs,
                                 colors_precomp, opacities, scales, rotations, cov3D_precomp, background, colors2,
                                 *means2D_list)


class _RasterizeTimedViews(torch.autograd.Function):
    """rasterize_timed_views: the view sets of _RasterizeViews with per-view geometry (include/gsr.h gsr_set_timed)."""

    @staticmethod
    def forward(ctx, settings_list, clamp, means3D, colors_precomp, opacities, scales, rotations, composite_bg, colors2,
                *means2D):
        t0 = time.perf_counter()
        lib = _C.load_library()
        dev = means3D.device
        P = int(means3D.shape[1])
        keep = lambda t: t.detach().contiguous()  # noqa: E731  (fp32 on `dev`: rasterize_timed_views checked)
        m3, col, op, sc, rot = keep(means3D), keep(colors_precomp), keep(opacities), keep(scales), keep(rotations)
        c2 = keep(colors2) if colors2 is not None else None
        sc_v, rot_v, c2_v = sc.dim() == 3, rot.dim() == 3, c2 is not None and c2.dim() == 3
        # what the views share goes into the scene; the per-view arrays into the set's gsr_set_timed
        gaussians = dict(means3D=None, scales=None if sc_v else sc, rotations=None if rot_v else rot, opacities=op,
                         shs=None, colors_precomp=col, cov3D_precomp=None)

        def preprocess(vs, stream):
            sl = slice(vs.lo, vs.hi)
            vs.timed = _C.SetTimed(means3D_v=_addr(m3[sl]), scales_v=_addr(sc[sl]) if sc_v else None,
                                   rotations_v=_addr(rot[sl]) if rot_v else None,
                                   colors2_v=_addr(c2[sl]) if c2_v else None)
            _C._check(lib.gsr_set_timed_preprocess(vs.scene, vs.state, vs.timed, stream))

        _C.host_mark("fwd_setup", t0)
        # (second colours per view: the pointer the preprocess embedded, the blends read the records; shared: gathered)
        r = _forward_sets(settings_list, gaussians, P, dev, composite_bg, clamp, preprocess,
                          (lambda vs: c2[vs.lo:vs.hi] if c2_v else c2) if c2 is not None else None)
        ctx.settings = settings_list
        ctx.sets = r.sets
        ctx.bg_shape = tuple(composite_bg.shape) if composite_bg is not None else None
        ctx.save_for_backward(m3, col, sc, rot, r.radii, r.cbg, r.color if r.render is not None else None, c2)
        ctx.mark_non_differentiable(r.radii)
        return _outputs(r)

    @staticmethod
    def backward(ctx, g_color, _g_radii, g_depth, g_alpha, g_color2=None):
        t0 = time.perf_counter()
        lib = _C.load_library()
        m3, col, sc, rot, radii, cbg, color, c2 = ctx.saved_tensors
        V, P = int(m3.shape[0]), int(m3.shape[1])
        dev = m3.device
        fopt = dict(dtype=torch.float32, device=dev)
        second = c2 is not None and g_color2 is not None
        sc_v, rot_v, c2_v = sc.dim() == 3, rot.dim() == 3, c2 is not None and c2.dim() == 3
        # per-view rows are always overwritten by the kernel; the shared sums too (accumulate continues them)
        d_m2 = torch.empty((V, P, 3), **fopt)
        d_m3 = torch.empty_like(m3)
        d_sc, d_rot = torch.empty_like(sc), torch.empty_like(rot)
        d_op, d_col = torch.empty((P, 1), **fopt), torch.empty((P, 3), **fopt)
        d_c2 = (torch.empty_like(c2) if second else torch.zeros_like(c2)) if c2 is not None else None
        d_bg = torch.empty_like(cbg) if cbg is not None and ctx.needs_input_grad[7] else None
        if P == 0:
            for t in (d_m2, d_m3, d_sc, d_rot, d_op, d_col, d_c2, d_bg):
                if t is not None:
                    t.zero_()
        else:
            rows = dict(dL_dcolor=_upstream(g_color), dL_ddepth=_upstream(g_depth), dL_dalpha=_upstream(g_alpha),
                        color=color, bg_images=cbg, dL_dbg=d_bg, dL_dmeans2D=d_m2,
                        dL_dcolor2=_upstream(g_color2) if second else None)
            stream = _C._stream(dev)
            g = _C.SetGrads(dL_dcolors=_addr(d_col), dL_dopacity=_addr(d_op), dL_dscales=None if sc_v else _addr(d_sc),
                            dL_drotations=None if rot_v else _addr(d_rot))
            if second and not c2_v:
                g.colors2, g.dL_dcolors2 = _addr(c2), _addr(d_c2)
            for si, vs in enumerate(ctx.sets):
                work = _set_work(lib, vs, second)
                _set_grads(g, vs, rows, work, accumulate=si > 0)
                sl = slice(vs.lo, vs.hi)
                timed = vs.timed
                if c2_v and not second:
                    # the second colour's image took no gradient: the one-colour backward of the first call
                    timed = _C.SetTimed.from_buffer_copy(vs.timed)
                    timed.colors2_v = None
                tg = _C.SetTimedGrads(dL_dmeans3D_v=_addr(d_m3[sl]), dL_dscales_v=_addr(d_sc[sl]) if sc_v else None,
                                      dL_drotations_v=_addr(d_rot[sl]) if rot_v else None,
                                      dL_dcolors2_v=_addr(d_c2[sl]) if second and c2_v else None)
                _C._check(lib.gsr_set_timed_backward(vs.scene, vs.state, g, timed, tg, stream))
        grads = _masked_grads(ctx, [None, None, d_m3, d_col, d_op, d_sc, d_rot, d_bg, d_c2]
                              + [d_m2[v] for v in range(V)], bg_at=7)
        _C.host_mark("bwd_host", t0)
        return tuple(grads)


def _timed_shape(name, t, V, P, width, per_view_only=False):
    """ValueError unless t is (V, P, width) or, when allowed, (P, width)."""
    ok = tuple(t.shape) == (V, P, width) or (not per_view_only and tuple(t.shape) == (P, width))
    if not ok:
        want = f"({V}, {P}, {width})" + ("" if per_view_only else f" or ({P}, {width})")
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {want}")


def rasterize_timed_views(settings_list, means3D, means2D_list, opacities, colors_precomp, scales, rotations,
                          colors2=None, background=None, clamp=False, grad_reduce=None):
    """Render V views that each carry their own frame of the Gaussians' geometry — frame v of a time batch from camera
    v, as the timed renderers do with one rasterizer call per frame (renderer/diff_sugar_rasterizer_temporal.py:150-192,
    renderer/diff_gaussian_rasterizer_st.py) — as view sets: one launch per stage and one host sync per set.

    means3D (V, P, 3); scales (V, P, 3) or (P, 3); rotations (V, P, 4) or (P, 4); colors2 (V, P, 3), (P, 3) or None;
    opacities (P, 1) and colors_precomp (P, 3) are shared by the views.  fp32 tensors on one GPU.  Frame t of
    sugar_dynamic.timed_gaussians' outputs is view t: ``means3D=xyz, rotations=rotation, colors2=normals``.

    Outputs, means2D_list, background, clamp and colors2 as for rasterize_views: (color, radii, depth, alpha
    [, color2]).  Gradients: a per-view input receives per-view rows (exactly zero where the view's blend did not
    reach the Gaussian), a shared one the sum over the views; a repeated backward (retain_graph) gives the same bits.

    Not built: shs, cov3D_precomp, per-view opacities / colours, the separate two-colour backward, and the in-backward
    rank reduction (grad_reduce raises: reduce after the backward, as view_shard.allreduce_grads does)."""
    if grad_reduce is not None:
        raise ValueError("rasterize_timed_views: the in-backward reduction (grad_reduce) is not built for timed sets; "
                         "reduce the gradients after the backward (view_shard.allreduce_grads)")
    if not settings_list:
        raise ValueError("at least one view")
    V = len(settings_list)
    if len(means2D_list) != V:
        raise ValueError("one means2D placeholder per view")
    if means3D.dim() != 3 or means3D.shape[0] != V or means3D.shape[2] != 3:
        raise ValueError(f"means3D has shape {tuple(means3D.shape)}, expected ({V}, P, 3): one frame per view")
    P = int(means3D.shape[1])
    if scales is None or rotations is None or colors_precomp is None or opacities is None:
        raise ValueError("rasterize_timed_views needs opacities, colors_precomp, scales and rotations")
    _timed_shape("scales", scales, V, P, 3)
    _timed_shape("rotations", rotations, V, P, 4)
    if colors2 is not None:
        _timed_shape("colors2", colors2, V, P, 3)
    if tuple(colors_precomp.shape) != (P, 3):
        raise ValueError(f"colors_precomp has shape {tuple(colors_precomp.shape)}, expected ({P}, 3): shared by the views")
    if opacities.numel() != P:
        raise ValueError(f"opacities has {opacities.numel()} elements, expected {P}: shared by the views")
    for m2 in means2D_list:
        if tuple(m2.shape) != (P, 3):
            raise ValueError(f"a means2D placeholder has shape {tuple(m2.shape)}, expected ({P}, 3)")
    _check_views(settings_list, background, size_error=ValueError)
    named = [("means3D", means3D), ("opacities", opacities), ("colors_precomp", colors_precomp), ("scales", scales),
             ("rotations", rotations), ("colors2", colors2)]
    for name, t in named:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{name} is {t.dtype}, expected torch.float32")
    if means3D.device.type != "cuda":
        raise ValueError("rasterize_timed_views requires tensors on a ROCm GPU (device 'cuda'): there is no CPU path")
    for name, t in named + [("background", background)]:
        if t is not None and t.device != means3D.device:
            raise ValueError(f"{name} is on {t.device}, expected {means3D.device}")
    return _RasterizeTimedViews.apply(list(settings_list), bool(clamp), means3D, colors_precomp, opacities, scales,
                                      rotations, background, colors2, *means2D_list)
