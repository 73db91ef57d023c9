"""The B-spline of the timed node attributes of dynamic SuGaR over the C ABI (include/gsr.h gsr_sugar_spline_*,
csrc/gsr_spline.hip).

With ``cfg.use_spline`` (the reference's default) every motion-stage step evaluates the deformation network at the
control knots (``compute_control_knots``, geometry/dynamic_sugar.py:362-416) and every render or ARAP call then asks
``self.spliner(timestamp)`` for the node (or vertex) attributes at its timestamps (``Spline.forward``,
geometry/spline_utils.py:195-332): a gather of degree + 1 knots per point and timestamp, pypose's ``Inv @``, ``Log``,
``Exp`` and a ``cumprod`` of quaternions for the rotation, ``bvv`` outer products and sums for the translation and
the scale, with every intermediate kept by autograd and an ``index_put`` scatter in its backward.  Here it is one fused
call for all T timestamps:

    grid = SplineGrid.for_frames(num_frames)                       # init_cubic_spliner's grid
    node_trans, node_rots, node_scales = spline_attributes(timestamps, knots_xyz, knots_rot, grid, knots_scale)

whose outputs are the arguments of ``sugar_dynamic.skin_vertices`` (or, with the vertices as points, of
``timed_gaussians``) and whose backward recomputes from the inputs and adds in a fixed order (no atomics: two calls give
the same bits).  Quaternions are pypose's (x, y, z, w).  GPU only, like ``sugar_dynamic``.
"""
from __future__ import annotations

import numpy as np
import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import aligned, float_tensor, on_gpu, ups, workspace

__all__ = ["SplineGrid", "spline_attributes"]

_EPS = np.float32(1e-6)  # spline_utils._EPS, added to a float32 tensor


def _number(x, name):
    if isinstance(x, bool):
        raise ValueError(f"{name} must be a number")
    if isinstance(x, torch.Tensor):
        if x.numel() != 1:
            raise ValueError(f"{name} must be a number")
        x = x.item()
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number")
    x = np.float32(x)
    if not np.isfinite(x):
        raise ValueError(f"{name} must be finite")
    return x


class SplineGrid:
    """The knot times of a ``Spline`` and the bounds its ``forward`` clamps to: ``Spline.set_start_time`` and
    ``update_end_time`` restated in numpy float32, in the reference's operation order, so that every attribute has the
    bits of the reference's 0-dim float32 tensors (``init_cubic_spliner`` builds its ``SplineConfig`` from those).

    degree 1 or 3; sampling_interval > 0 and start_time: numbers, rounded to float32; n_knots >= degree + 1.  Knot k is
    at ``start_time + k sampling_interval``; ``end_time = start_time + sampling_interval * (n_knots - 1)``; degree 3:
    ``t_lower = start_time + sampling_interval``, ``t_upper = end_time - sampling_interval``; degree 1: ``start_time``
    and ``end_time``; ``clamp_lo = t_lower + 1e-6`` and ``clamp_hi = t_upper - 1e-6``.  All numpy float32.  No tensors:
    works without a GPU.
    """

    def __init__(self, degree, sampling_interval, start_time, n_knots):
        if isinstance(degree, bool) or not isinstance(degree, int) or degree not in (1, 3):
            raise ValueError(f"degree must be 1 or 3, got {degree!r}")
        if isinstance(n_knots, bool) or not isinstance(n_knots, int) or n_knots < degree + 1:
            raise ValueError(f"n_knots must be an integer >= degree + 1 = {degree + 1}, got {n_knots!r}")
        if n_knots >= 2 ** 31:
            raise ValueError("n_knots must stay below 2^31")
        interval, start = _number(sampling_interval, "sampling_interval"), _number(start_time, "start_time")
        if not interval > 0:
            raise ValueError(f"sampling_interval must be positive, got {sampling_interval!r}")
        self.degree, self.n_knots = degree, n_knots
        self.sampling_interval, self.start_time = interval, start
        self.end_time = np.float32(start + np.float32(interval * np.float32(n_knots - 1)))
        if degree == 3:
            self.t_lower = np.float32(start + interval)
            self.t_upper = np.float32(self.end_time - interval)
        else:
            self.t_lower, self.t_upper = start, self.end_time
        self.clamp_lo = np.float32(self.t_lower + _EPS)
        self.clamp_hi = np.float32(self.t_upper - _EPS)

    @classmethod
    def for_frames(cls, num_frames, degree=3):
        """``DynamicSuGaRModel.init_cubic_spliner`` (dynamic_sugar.py:349-360): ``num_frames`` knots, of which the
        first is one interval before t = 0 and the last one after t = 1; interval = float32(1 / (num_frames - 3))."""
        if isinstance(num_frames, bool) or not isinstance(num_frames, int) or num_frames < 4:
            raise ValueError(f"num_frames must be an integer >= 4, got {num_frames!r}")
        interval = np.float32(1 / (num_frames - 3))
        return cls(degree, interval, -interval, num_frames)

    def __repr__(self):
        return (f"SplineGrid(degree={self.degree}, sampling_interval={self.sampling_interval!r}, "
                f"start_time={self.start_time!r}, n_knots={self.n_knots})")


def _spline_in(knots_xyz, knots_rot, knots_scale, timestamps, grid):
    """The gsr_sugar_spline of these tensors (addresses only: the caller keeps the tensors)."""
    p = _gsr._ptr
    return _gsr.SugarSpline(T=int(timestamps.shape[0]), P=int(knots_xyz.shape[1]), n_knots=grid.n_knots,
                            degree=grid.degree, start=float(grid.start_time), interval=float(grid.sampling_interval),
                            lo=float(grid.clamp_lo), hi=float(grid.clamp_hi), timestamps=p(timestamps),
                            knots_xyz=p(knots_xyz), knots_rot=p(knots_rot), knots_scale=p(knots_scale))


class _SplineAttributes(torch.autograd.Function):
    """(knots_xyz, knots_rot, knots_scale) -> (xyz, rot, scale)."""

    @staticmethod
    def forward(ctx, knots_xyz, knots_rot, knots_scale, timestamps, grid):
        dev = knots_xyz.device
        lib = _gsr.load_library()
        T, P = int(timestamps.shape[0]), int(knots_xyz.shape[1])
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(knots_xyz, knots_rot, knots_scale, timestamps)
        ctx.grid = grid
        fopt = dict(dtype=torch.float32, device=dev)
        xyz, rot = torch.empty((T, P, 3), **fopt), torch.empty((T, P, 4), **fopt)
        scale = None if knots_scale is None else torch.empty((T, P, 3), **fopt)
        if T > 0 and P > 0:
            _gsr._check(lib.gsr_sugar_spline_forward(
                _spline_in(knots_xyz, knots_rot, knots_scale, timestamps, grid), _gsr._ptr(xyz), _gsr._ptr(rot),
                _gsr._ptr(scale), _gsr._stream(dev)))
        return xyz, rot, scale

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_rot, g_scale):
        knots_xyz, knots_rot, knots_scale, timestamps = ctx.saved_tensors
        grid = ctx.grid
        dev = knots_xyz.device
        T, P = int(timestamps.shape[0]), int(knots_xyz.shape[1])
        if knots_scale is None:
            g_scale = None
        inputs = (knots_xyz, knots_rot, knots_scale)
        if T == 0 or P == 0 or all(g is None for g in (g_xyz, g_rot, g_scale)):
            return (*(torch.zeros_like(t) if t is not None else None for t in inputs), None, None)
        lib = _gsr.load_library()
        g_ups = ups((g_xyz, g_rot, g_scale), dev)
        grads = [torch.empty_like(t) if t is not None else None for t in inputs]
        nbytes = int(lib.gsr_sugar_spline_workspace_bytes(T, P, grid.degree))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_spline_backward(
            _spline_in(knots_xyz, knots_rot, knots_scale, timestamps, grid), *(_gsr._ptr(g) for g in g_ups),
            *(_gsr._ptr(g) for g in grads), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return (*grads, None, None)


def spline_attributes(timestamps, knots_xyz, knots_rot, grid, knots_scale=None):
    """``Spline.forward`` for all T timestamps and the three attributes: ``(xyz (T, P, 3), rot (T, P, 4), scale
    (T, P, 3) or None)`` = the reference's ``self.spliner(timestamp)`` "xyz", "rotation" and "scale".

    timestamps (T,); knots_xyz (n_knots, P, 3); knots_rot (n_knots, P, 4), (x, y, z, w) of any non-zero norm;
    knots_scale (n_knots, P, 3) or None (``d_scale``); all float32 on the GPU; grid: the ``SplineGrid`` (its n_knots
    is the knots' first size).  The knots are frame-major, as ``_get_timed_dg_attributes_wo_spline`` returns them at
    the knot times: the tensors the reference passes to ``Spline.set_data`` are their ``.permute(1, 0, 2)``.  The
    outputs are the ``node_trans``, ``node_rots`` and ``node_scales`` of ``sugar_dynamic.skin_vertices``; with the
    mesh vertices as points (``use_deform_graph=False``) the ``vert_xyz``, ``vert_rot`` and ``vert_scale`` of
    ``timed_gaussians``.

    A timestamp is clamped to the grid's bounds and its segment chosen in float32 exactly as the reference does; the
    rest is fp64 with one rounding per output (the formulas: include/gsr.h).  rot is neither normalised nor
    sign-fixed, as in the reference: it has the norm of its segment's first knot (degree 3) or norm 1 (degree 1).
    Gradients flow to knots_xyz, knots_rot and knots_scale, bitwise reproducible; a knot that no timestamp's segment
    covers gets exactly zero.  No gradient to timestamps, no double backward.
    """
    if not isinstance(grid, SplineGrid):
        raise ValueError("grid must be a SplineGrid")
    timestamps = float_tensor(timestamps, "timestamps", (None,))
    T, n = int(timestamps.shape[0]), grid.n_knots
    try:
        knots_xyz = float_tensor(knots_xyz, "knots_xyz", (n, None, 3))
        P = int(knots_xyz.shape[1])
        knots_rot = float_tensor(knots_rot, "knots_rot", (n, P, 4))
        if knots_scale is not None:
            knots_scale = float_tensor(knots_scale, "knots_scale", (n, P, 3))
    except ValueError as e:
        raise ValueError(f"{e} (the grid has n_knots = {n})") from None
    if max(T, n) * P >= 2 ** 31:
        raise ValueError("the call is too large: T x P and n_knots x P must stay below 2^31")
    on_gpu("spline_attributes", knots_xyz, (("knots_rot", knots_rot), ("knots_scale", knots_scale),
                                            ("timestamps", timestamps)))
    out = _SplineAttributes.apply(knots_xyz.contiguous(), aligned(knots_rot),
                                  None if knots_scale is None else knots_scale.contiguous(),
                                  timestamps.detach().contiguous(), grid)
    return out[0], out[1], out[2]
