"""The HexPlane deformation network of dynamic SuGaR over the C ABI (include/gsr.h gsr_sugar_deform_*,
csrc/gsr_deform.hip): from the trained planes and MLP to the control knots of the spline.

With ``dynamic_mode: deformation`` and ``use_spline: true`` (both shipped 4-D configs) every motion-stage step calls
``compute_control_knots`` (geometry/dynamic_sugar.py:362-416), which evaluates
``DeformationNetwork.forward_dynamic_delta`` (geometry/deformation.py) at ``num_frames`` ticks x the graph nodes (or
the mesh vertices), adds (0, 0, 0, 1) to the rotation and, for the nodes, normalises it: 24 ``grid_sample`` calls, 20
products, a ``cat`` and 7 ``Linear`` layers, on ``repeat_interleave``d copies of the points and ticks, with an atomic
scatter into the planes in the backward.  Here it is one fused call:

    binding = HexPlaneBinding(node_xyz, ticks, aabb)                 # once per (points, ticks)
    weights = DeformationWeights.from_state_dict(sd, d_scale=True)   # the reference's ``_deformation`` state dict
    knots_xyz, knots_rot, knots_scale = deformation_knots(binding, weights)

whose outputs are the arguments of ``sugar_spline.spline_attributes`` and whose backward gathers per texel over the
binding's tables and adds the weight gradients in a fixed order (no atomics: two calls give the same bits).  GPU only,
like the other stages.
"""
from __future__ import annotations

import ctypes
import itertools
import math

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import Binding, float_tensor, on_gpu, row_offsets, ups, workspace

__all__ = ["HexPlaneBinding", "DeformationWeights", "deformation_knots"]

COMBOS = tuple(itertools.combinations(range(4), 2))  # plane q is (a, b), a along the width
SPATIAL_PLANES, TIME_PLANES = (0, 1, 3), (2, 4, 5)
FEATURES, HIDDEN, MAX_LEVELS = 32, 64, 4
HEADS = (("pos_deform", 3), ("rotations_deform", 4), ("scales_deform", 3))
PREFIX = "deformation_net."


def mlp_names(d_scale=True):
    """The reference's state-dict keys of the 14 (10 without the scale head) trained MLP tensors, in the C ABI's order."""
    names = [PREFIX + "feature_out.0.weight", PREFIX + "feature_out.0.bias"]
    for head, _ in HEADS[:3 if d_scale else 2]:
        names += [f"{PREFIX}{head}.feature_out.0.main_stream.weight", f"{PREFIX}{head}.feature_out.0.main_stream.bias",
                  f"{PREFIX}{head}.feature_out.1.weight", f"{PREFIX}{head}.feature_out.1.bias"]
    return names


def plane_name(level, q):
    return f"{PREFIX}grid.grids.{level}.{q}"


def level_resolutions(resolution, multires):
    """[[x, y, z, time] per level]: the multiplier applies to the spatial axes only."""
    resolution, multires = [int(r) for r in resolution], [int(m) for m in multires]
    if len(resolution) != 4 or not 1 <= len(multires) <= MAX_LEVELS:
        raise ValueError("resolution must have 4 entries and multires 1 to 4")
    reso = [[r * m for r in resolution[:3]] + [resolution[3]] for m in multires]
    if min(min(r) for r in reso) < 2:
        raise ValueError("every resolution must be at least 2")
    return reso


def _table(texel, entry, n):
    """The rows of a table: the entries grouped by texel in ascending entry order, and the n + 1 row offsets."""
    order = torch.sort(texel, stable=True)[1]
    return entry[order].to(torch.int32).contiguous(), row_offsets(torch.bincount(texel, minlength=n))


class HexPlaneBinding(Binding):
    """Where P fixed points and T ticks fall in the planes of a HexPlane, built once per (points, ticks).

    points (P, 3), ticks (T,), aabb (2, 3) float32 (``HexPlaneField.aabb``: [[b, b, b], [-b, -b, -b]]); resolution and
    multires as ``kplanes_config["resolution"]`` and ``multires``.  Sample (t, p) sees
    ``(normalize_aabb(x_p), 2 tick_t - 1)`` with ``normalize_aabb(x) = (x - aabb[0]) (2 / (aabb[1] - aabb[0])) - 1``;
    along an axis of R texels the coordinate is ``clamp((n + 1) / 2 (R - 1), 0, R - 1)`` (``grid_sample`` with
    ``align_corners=True, padding_mode="border"``).  All of it in float64 from the float32 inputs.

    Holds ``cell`` (L, 3, P) int32 and ``frac`` (L, 3, P) float64, the lower texel and the weight of the upper one,
    ``tcell`` / ``tfrac`` (T,) for the ticks, and the tables of the backward's gather, rows in ascending entry order,
    corners outside a plane absent: ``sp_order`` / ``sp_offsets`` (per texel of the spatial planes the entries
    4 p + 2 cy + cx), ``col_order`` / ``col_offsets`` (per level, axis and column the entries 2 p + cx) and ``t_order`` /
    ``t_offsets`` (per time row the entries 2 t + ct).

    Size in bytes (``nbytes``): 36 L P + 12 T for the cells and weights, 4 per table entry and 4 per row offset:
    ``36 L P + 12 T + 4 (n_sp + n_col + n_t) + 4 (texels + columns + time rows + 3)`` with n_sp <= 12 L P,
    n_col <= 6 L P and n_t <= 2 T, so at most ``108 L P + 20 T + 4 (texels + columns + time rows + 3)``, where texels
    and columns count the spatial planes' texels and the spatial axes' columns over all levels (the shipped
    resolution: 1 044 480 and 2 880, 25 time rows).
    """

    _TENSORS = ("cell", "frac", "tcell", "tfrac", "sp_order", "sp_offsets", "col_order", "col_offsets", "t_order",
                "t_offsets")

    def __init__(self, points, ticks, aabb, resolution=(64, 64, 64, 25), multires=(1, 2, 4, 8)):
        points = float_tensor(points, "points", (None, 3)).detach()
        ticks = float_tensor(ticks, "ticks", (None,)).detach().to(points.device)
        aabb = float_tensor(aabb, "aabb", (2, 3)).detach().to(points.device)
        if not (torch.isfinite(points).all() and torch.isfinite(ticks).all() and torch.isfinite(aabb).all()):
            raise ValueError("points, ticks and aabb must be finite")
        if bool((aabb[0] == aabb[1]).any()):
            raise ValueError("aabb must have a non-zero extent along every axis")
        self.reso = level_resolutions(resolution, multires)
        self.P, self.T, self.L = int(points.shape[0]), int(ticks.shape[0]), len(self.reso)
        P, T, L = self.P, self.T, self.L
        if T * P >= 2 ** 31 or 12 * L * P >= 2 ** 31:
            raise ValueError("the call is too large: T x P and 12 L P must stay below 2^31")
        pts, box = points.double(), aabb.double()
        n = (pts - box[0]) * (2.0 / (box[1] - box[0])) - 1.0
        tn = ticks.double() * 2 - 1

        def cells(x, R):
            c = ((x + 1.0) / 2.0 * (R - 1)).clamp(0, R - 1)
            i = torch.floor(c)
            return i.long(), c - i

        cell, frac = zip(*(cells(n[:, d], self.reso[l][d]) for l in range(L) for d in range(3)))
        tcell, tfrac = cells(tn, self.reso[0][3])
        # the tables
        ar = lambda k: torch.arange(k, device=points.device)  # noqa: E731
        tex, ent, base = [], [], 0
        e4 = ar(4 * P)
        for l in range(L):
            for q in SPATIAL_PLANES:
                a, b = COMBOS[q]
                Ra, Rb = self.reso[l][a], self.reso[l][b]
                x, y = cell[3 * l + a][e4 >> 2] + (e4 & 1), cell[3 * l + b][e4 >> 2] + ((e4 >> 1) & 1)
                ok = (x < Ra) & (y < Rb)
                tex.append(base + (y * Ra + x)[ok])
                ent.append(e4[ok])
                base += Ra * Rb
        self.n_sp_texels = base
        sp_order, sp_offsets = _table(torch.cat(tex), torch.cat(ent), base)
        tex, ent, base = [], [], 0
        e2 = ar(2 * P)
        for l in range(L):
            for d in range(3):
                x = cell[3 * l + d][e2 >> 1] + (e2 & 1)
                ok = x < self.reso[l][d]
                tex.append(base + x[ok])
                ent.append(e2[ok])
                base += self.reso[l][d]
        self.n_columns = base
        col_order, col_offsets = _table(torch.cat(tex), torch.cat(ent), base)
        et = ar(2 * T)
        row = tcell[et >> 1] + (et & 1)
        ok = row < self.reso[0][3]
        t_order, t_offsets = _table(row[ok], et[ok], self.reso[0][3])
        self.cell = torch.stack(cell).reshape(L, 3, P).to(torch.int32).contiguous()
        self.frac = torch.stack(frac).reshape(L, 3, P).contiguous()
        self.tcell, self.tfrac = tcell.to(torch.int32).contiguous(), tfrac.contiguous()
        self.sp_order, self.sp_offsets = sp_order, sp_offsets
        self.col_order, self.col_offsets = col_order, col_offsets
        self.t_order, self.t_offsets = t_order, t_offsets

    @property
    def nbytes(self):
        return sum(getattr(self, k).numel() * getattr(self, k).element_size() for k in self._TENSORS)


class DeformationWeights:
    """The trained tensors of the deformation network as leaves: ``planes`` (6 L tensors in the reference's own
    (1, 32, H, W) layout, level-major, plane q of ``itertools.combinations(range(4), 2)``) and ``mlp`` (the 14 weight
    and bias tensors of ``feature_out`` and of the heads ``pos_deform``, ``rotations_deform``, ``scales_deform``; 10
    without the scale head), named as in the reference's state dict (``names``)."""

    def __init__(self, planes, mlp):
        planes, mlp = list(planes), list(mlp)
        if len(planes) % 6 or not 1 <= len(planes) // 6 <= MAX_LEVELS:
            raise ValueError("planes must hold six tensors for each of 1 to 4 levels")
        if len(mlp) not in (10, 14):
            raise ValueError("mlp must hold 14 tensors, or 10 without the scale head")
        self.L, self.d_scale = len(planes) // 6, len(mlp) == 14
        self.reso = []
        for l in range(self.L):
            r = [int(planes[6 * l].shape[3]), int(planes[6 * l].shape[2]), int(planes[6 * l + 1].shape[2]),
                 int(planes[6 * l + 2].shape[2])] if planes[6 * l].dim() == 4 else None
            for q, (a, b) in enumerate(COMBOS):
                float_tensor(planes[6 * l + q], plane_name(l, q), (1, FEATURES, r[b], r[a]) if r else (1,) * 4)
            self.reso.append(r)
        shapes = [(HIDDEN, FEATURES * self.L), (HIDDEN,)]
        for _, H in HEADS[:3 if self.d_scale else 2]:
            shapes += [(HIDDEN, HIDDEN), (HIDDEN,), (H, HIDDEN), (H,)]
        for t, name, shape in zip(mlp, mlp_names(self.d_scale), shapes):
            float_tensor(t, name, shape)
        self.planes, self.mlp = planes, mlp

    @property
    def names(self):
        return [plane_name(l, q) for l in range(self.L) for q in range(6)] + mlp_names(self.d_scale)

    def parameters(self):
        return self.planes + self.mlp

    def state_dict(self):
        return dict(zip(self.names, self.parameters()))

    def to(self, device):
        return DeformationWeights(*([t.detach().to(device).requires_grad_(t.requires_grad) for t in ts]
                                    for ts in (self.planes, self.mlp)))

    def requires_grad_(self, on=True):
        for t in self.parameters():
            t.requires_grad_(on)
        return self

    @classmethod
    def from_state_dict(cls, sd, d_scale=True):
        """From the reference's ``_deformation`` state dict under its own key names; ``timenet``, ``opacity_deform``,
        the aabb and the frequency buffers are ignored (nothing evaluates them), and so is the scale head without
        ``d_scale``."""
        L = 0
        while plane_name(L, 0) in sd:
            L += 1
        missing = [k for k in [plane_name(l, q) for l in range(L) for q in range(6)] + mlp_names(d_scale) if k not in sd]
        if L == 0 or missing:
            raise ValueError(f"not a deformation-network state dict: missing {missing or plane_name(0, 0)}")
        take = lambda k: sd[k].detach().clone().float().contiguous().requires_grad_()  # noqa: E731
        return cls([take(plane_name(l, q)) for l in range(L) for q in range(6)], [take(k) for k in mlp_names(d_scale)])

    @classmethod
    def init_like_reference(cls, generator=None, resolution=(64, 64, 64, 25), multires=(1, 2, 4, 8), d_scale=True,
                            device="cpu"):
        """The reference's initialisation (``init_grid_param``, ``initialize_weights`` and the heads'
        ``initialize_weights``): spatial planes U(0.1, 0.5), time planes 1, ``feature_out`` xavier-uniform with
        ``nn.Linear``'s default bias, every layer of the heads zero."""
        opt = dict(dtype=torch.float32, device=device)
        planes = []
        for r in level_resolutions(resolution, multires):
            for a, b in COMBOS:
                shape = (1, FEATURES, r[b], r[a])
                planes.append(torch.ones(shape, **opt) if b == 3
                              else torch.rand(shape, generator=generator, **opt) * 0.4 + 0.1)
        K = FEATURES * len(multires)
        bound = math.sqrt(6.0 / (K + HIDDEN))
        mlp = [(torch.rand((HIDDEN, K), generator=generator, **opt) * 2 - 1) * bound,
               (torch.rand((HIDDEN,), generator=generator, **opt) * 2 - 1) / math.sqrt(K)]
        for _, H in HEADS[:3 if d_scale else 2]:
            mlp += [torch.zeros((HIDDEN, HIDDEN), **opt), torch.zeros((HIDDEN,), **opt), torch.zeros((H, HIDDEN), **opt),
                    torch.zeros((H,), **opt)]
        return cls(planes, mlp).requires_grad_()


def _pointers(tensors, n):
    """A host array of n device addresses (None past the tensors given)."""
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])


def _deform_in(binding, planes, mlp, normalize_rot):
    """The gsr_sugar_deform of these tensors and the host arrays it points to (the caller keeps both)."""
    reso = (ctypes.c_int * (4 * binding.L))(*[r for level in binding.reso for r in level])
    pl, ml = _pointers(planes, len(planes)), _pointers(mlp, 14)
    p = _gsr._ptr
    c = _gsr.SugarDeform(T=binding.T, P=binding.P, L=binding.L, d_scale=int(len(mlp) == 14),
                         normalize_rot=int(normalize_rot), n_sp=int(binding.sp_order.numel()),
                         n_col=int(binding.col_order.numel()), n_t=int(binding.t_order.numel()), reso=reso, planes=pl,
                         mlp=ml, cell=p(binding.cell), frac=p(binding.frac), tcell=p(binding.tcell),
                         tfrac=p(binding.tfrac))
    return c, (reso, pl, ml)


class _DeformationKnots(torch.autograd.Function):
    """(planes..., mlp...) -> (knots_xyz, knots_rot, knots_scale)."""

    @staticmethod
    def forward(ctx, binding, normalize_rot, n_planes, *tensors):
        dev = binding.device
        lib = _gsr.load_library()
        T, P = binding.T, binding.P
        planes, mlp = tensors[:n_planes], tensors[n_planes:]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*tensors)
        ctx.binding, ctx.normalize_rot, ctx.n_planes = binding, normalize_rot, n_planes
        fopt = dict(dtype=torch.float32, device=dev)
        xyz, rot = torch.empty((T, P, 3), **fopt), torch.empty((T, P, 4), **fopt)
        scale = torch.empty((T, P, 3), **fopt) if len(mlp) == 14 else None
        if T > 0 and P > 0:
            c, keep = _deform_in(binding, planes, mlp, normalize_rot)
            _gsr._check(lib.gsr_sugar_deform_forward(c, _gsr._ptr(xyz), _gsr._ptr(rot), _gsr._ptr(scale),
                                                     _gsr._stream(dev)))
            del keep
        return xyz, rot, scale

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_rot, g_scale):
        tensors = ctx.saved_tensors
        binding, n_planes = ctx.binding, ctx.n_planes
        planes, mlp = tensors[:n_planes], tensors[n_planes:]
        dev = binding.device
        T, P = binding.T, binding.P
        if len(mlp) != 14:
            g_scale = None
        if T == 0 or P == 0 or all(g is None for g in (g_xyz, g_rot, g_scale)):
            return (None, None, None, *(torch.zeros_like(t) for t in tensors))
        lib = _gsr.load_library()
        g_ups = ups((g_xyz, g_rot, g_scale), dev)
        grads = [torch.empty_like(t) for t in tensors]  # (written in full: untouched texels get +0.0)
        nbytes = int(lib.gsr_sugar_deform_workspace_bytes(T, P, binding.L))
        ws = workspace(nbytes, dev)
        c, keep = _deform_in(binding, planes, mlp, ctx.normalize_rot)
        dplanes, dmlp = _pointers(grads[:n_planes], n_planes), _pointers(grads[n_planes:], 14)
        p = _gsr._ptr
        _gsr._check(lib.gsr_sugar_deform_backward(
            c, p(binding.sp_order), p(binding.sp_offsets), p(binding.col_order), p(binding.col_offsets),
            p(binding.t_order), p(binding.t_offsets), *(p(g) for g in g_ups), dplanes, dmlp, p(ws), nbytes,
            _gsr._stream(dev)))
        del keep
        return (None, None, None, *grads)


def deformation_knots(binding, weights, normalize_rot=True, d_scale=True):
    """``forward_dynamic_delta`` at every (tick, point) of the binding and the epilogue of
    ``_get_timed_dg_attributes_wo_spline``: ``(knots_xyz (T, P, 3), knots_rot (T, P, 4), knots_scale (T, P, 3) or
    None)``, frame-major: the knots of ``sugar_spline.spline_attributes``.

    binding: the ``HexPlaneBinding`` (on the GPU); weights: the ``DeformationWeights`` (on the same GPU, planes of the
    binding's resolutions).  ``knots_rot`` is the rotation head's output + (0, 0, 0, 1), divided by its norm when
    ``normalize_rot`` (the graph nodes); ``normalize_rot=False`` is the vertex variant, which leaves it as it is.
    ``d_scale=False`` does not evaluate the scale head: ``knots_scale`` is None and the head gets no gradient.

    fp64 arithmetic from the float32 tensors, one rounding per output.  Gradients flow to the 6 L planes and to the 14
    (10) MLP tensors, bitwise reproducible; a texel that no sample touches gets exactly +0.0; relu' at exactly 0 is 0.
    No gradient to the points, the ticks or the aabb, no double backward.
    """
    if not isinstance(binding, HexPlaneBinding) or not isinstance(weights, DeformationWeights):
        raise ValueError("binding must be a HexPlaneBinding and weights a DeformationWeights")
    if d_scale and not weights.d_scale:
        raise ValueError("d_scale needs weights with the scale head")
    if weights.reso != binding.reso:
        raise ValueError(f"the planes have resolutions {weights.reso}, the binding was built for {binding.reso}")
    mlp = weights.mlp[:14 if d_scale else 10]
    tensors = list(weights.planes) + list(mlp)
    on_gpu("deformation_knots", binding.cell, [(n, t) for n, t in zip(weights.names, tensors)])
    out = _DeformationKnots.apply(binding, bool(normalize_rot), len(weights.planes), *(t.contiguous() for t in tensors))
    return out[0], out[1], out[2]
