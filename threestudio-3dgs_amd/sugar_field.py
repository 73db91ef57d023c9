"""The SuGaR regulariser's neighbour density field over the C ABI (include/gsr.h gsr_sugar_field_*, csrc/gsr_field.hip).

The reference evaluates, every training step of system/sugar_static.py:260-285, ``SuGaRRegularizer.get_field_values``
(utils/sugar_utils.py:278-353) at M = 500 000 samples against K = 16 neighbours each: it gathers (M, K, 3, 3) inverse
scaled rotations, (M, K, 3) centres and (M, K) strengths, runs a batched matmul over them, keeps all of it for autograd
and scatters the backward into the Gaussians with ``index_put`` atomics.  Here one fused kernel gathers and reduces,
and the backward recomputes from the inputs and sums per Gaussian in a fixed order (no atomics: two calls give the
same bits).

``neighbor_density`` is the fused, differentiable part; ``get_field_values`` composes the M-sized remainder in torch in
the reference's own order and returns its ``fields`` dict.  For the reference to pick this up, two lines change in
``SuGaRRegularizer.get_field_values``: its body becomes

    from sugar_field import get_field_values
    return get_field_values(x, points=gaussian_centers, inv_scaled_rotation=gaussian_inv_scaled_rotation,
                            strengths=gaussian_strengths, scaling=self.scaling, knn_idx=self.knn_idx,
                            gaussian_idx=gaussian_idx, closest_gaussians_idx=closest_gaussians_idx,
                            beta_mode=self.beta_mode, log_beta=getattr(self, "_log_beta", None), ...)

after the three ``if ... is None`` defaults it already has.  GPU only, like ``simple_knn.knn_points``.

``neighbor_normal_loss`` (include/gsr.h gsr_sugar_normal_*, csrc/gsr_normal.hip) is the other M x K half of the
regulariser step, the "sdf better normal loss" of ``coarse_density_regulation`` (utils/sugar_utils.py:725-757), fused
the same way; ``smallest_axis``, ``sample_points_in_gaussians`` and ``coarse_density_regulation`` restate the N- and
M-sized remainder of that step in torch, so that the body of the reference's ``coarse_density_regulation`` below its
parameter block becomes one call.
"""
from __future__ import annotations

import math
import operator

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import float_tensor, on_gpu, ups, workspace

__all__ = ["neighbor_density", "get_field_values", "neighbor_normal_loss", "smallest_axis",
           "sample_points_in_gaussians", "coarse_density_regulation", "FIELD_MAX_K"]

FIELD_MAX_K = 32  # include/gsr.h GSR_KNN_MAX_K


def _field_in(x, centers, inv_sr, strengths, min_scale, nbr, row, density_factor):
    """The gsr_sugar_field of these tensors (addresses only: the caller keeps the tensors)."""
    p = _gsr._ptr
    return _gsr.SugarField(M=int(x.shape[0]), K=int(nbr.shape[1]), N=int(centers.shape[0]), R=int(nbr.shape[0]),
                           x=p(x), nbr=p(nbr), row=p(row), centers=p(centers), inv_sr=p(inv_sr),
                           strengths=p(strengths), min_scale=p(min_scale), density_factor=density_factor)


class _NeighborDensity(torch.autograd.Function):
    """(x, centers, inv_sr, strengths, min_scale) -> (density, beta_avg, op | None); nbr / row are index tensors."""

    @staticmethod
    def forward(ctx, x, centers, inv_sr, strengths, min_scale, nbr, row, density_factor, want_op):
        dev = x.device
        lib = _gsr.load_library()
        M, K, N = int(x.shape[0]), int(nbr.shape[1]), int(centers.shape[0])
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, centers, inv_sr, strengths, min_scale, nbr, row)
        ctx.density_factor = density_factor
        fopt = dict(dtype=torch.float32, device=dev)
        density = torch.empty((M,), **fopt)
        beta_avg = torch.empty((M,), **fopt)
        op = torch.empty((M, K), **fopt) if want_op else None
        if M > 0:
            nbytes = int(lib.gsr_sugar_field_workspace_bytes(0, K, N))
            ws = workspace(nbytes, dev)
            _gsr._check(lib.gsr_sugar_field_forward(
                _field_in(x, centers, inv_sr, strengths, min_scale, nbr, row, density_factor), _gsr._ptr(density),
                _gsr._ptr(beta_avg), _gsr._ptr(op), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        if op is None:
            return density, beta_avg, None
        return density, beta_avg, op

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_density, g_beta, g_op):
        x, centers, inv_sr, strengths, min_scale, nbr, row = ctx.saved_tensors
        dev = x.device
        M, K, N = int(x.shape[0]), int(nbr.shape[1]), int(centers.shape[0])
        if M == 0 or (g_density is None and g_beta is None and g_op is None):
            grads = tuple(torch.zeros_like(t) for t in (x, centers, inv_sr, strengths, min_scale))
            return grads + (None, None, None, None)
        lib = _gsr.load_library()
        g_density, g_beta, g_op = ups((g_density, g_beta, g_op), dev)
        dx, dc, dA, ds, dms = (torch.empty_like(t) for t in (x, centers, inv_sr, strengths, min_scale))
        nbytes = int(lib.gsr_sugar_field_workspace_bytes(M, K, N))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_field_backward(
            _field_in(x, centers, inv_sr, strengths, min_scale, nbr, row, ctx.density_factor), _gsr._ptr(g_density),
            _gsr._ptr(g_beta), _gsr._ptr(g_op), _gsr._ptr(dx), _gsr._ptr(dc), _gsr._ptr(dA), _gsr._ptr(ds),
            _gsr._ptr(dms), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return dx, dc, dA, ds, dms, None, None, None, None


def _index_tensor(t, name, dims):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != dims:
        raise ValueError(f"{name} must be an int64 tensor with {dims} dimension(s)")
    return t


def _neighbour_table(M, knn_idx, gaussian_idx, closest_gaussians_idx):
    """(nbr (R, K), row (M,) | None) of the one index form given."""
    table = knn_idx is not None and gaussian_idx is not None
    if table == (closest_gaussians_idx is not None) or (not table and (knn_idx is not None
                                                                      or gaussian_idx is not None)):
        raise ValueError("give either knn_idx with gaussian_idx, or closest_gaussians_idx (one of the two forms)")
    if table:
        nbr, row = _index_tensor(knn_idx, "knn_idx", 2), _index_tensor(gaussian_idx, "gaussian_idx", 1)
        if int(row.shape[0]) != M:
            raise ValueError(f"gaussian_idx must have one entry per sample ({M}), got {int(row.shape[0])}")
    else:
        nbr, row = _index_tensor(closest_gaussians_idx, "closest_gaussians_idx", 2), None
        if int(nbr.shape[0]) != M:
            raise ValueError(f"closest_gaussians_idx must have one row per sample ({M}), got {int(nbr.shape[0])}")
    if not 1 <= int(nbr.shape[1]) <= FIELD_MAX_K:
        raise ValueError(f"the neighbour table must have 1..{FIELD_MAX_K} columns, got {int(nbr.shape[1])}")
    return nbr, row


def neighbor_density(x, centers, inv_scaled_rotation, strengths, min_scaling, *, knn_idx=None, gaussian_idx=None,
                     closest_gaussians_idx=None, density_factor=1.0, return_opacities=False):
    """The neighbour sum of ``get_field_values`` and the ``average`` beta, fused and differentiable.

    x (M, 3) samples; centers (N, 3); inv_scaled_rotation (N, 3, 3) = ``get_covariance(return_full_matrix=True,
    return_sqrt=True, inverse_scales=True)``; strengths (N,) or (N, 1); min_scaling (N,) = ``scaling.min(-1)[0]``; all
    float32 on the GPU.  Neighbours: either ``knn_idx`` (N, K) with ``gaussian_idx`` (M,) — sample m uses the row
    ``knn_idx[gaussian_idx[m]]``, read in the kernel — or ``closest_gaussians_idx`` (M, K); int64, 1 <= K <= 32.

    Returns ``(density, beta_avg, opacities)``: density (M,) = sum_k op[m, k] (raw, before any normalisation),
    beta_avg (M,) = mean_k min_scaling[j], and op (M, K) = density_factor strengths_j exp(-clamp(|A_j^T (x - c_j)|^2,
    0, 1e8) / 2) when ``return_opacities`` (else None).  A neighbour index outside [0, N) (``knn_points``' -1 padding)
    contributes nothing; a ``gaussian_idx`` outside the table gives zeros.  Gradients flow to all five float inputs,
    bitwise reproducible; no double backward.
    """
    x = float_tensor(x, "x", (None, 3))
    M = int(x.shape[0])
    centers = float_tensor(centers, "centers", (None, 3))
    N = int(centers.shape[0])
    inv_sr = float_tensor(inv_scaled_rotation, "inv_scaled_rotation", (N, 3, 3))
    if isinstance(strengths, torch.Tensor) and strengths.dim() == 2:
        strengths = float_tensor(strengths, "strengths", (N, 1)).reshape(N)
    strengths = float_tensor(strengths, "strengths", (N,))
    min_scaling = float_tensor(min_scaling, "min_scaling", (N,))
    nbr, row = _neighbour_table(M, knn_idx, gaussian_idx, closest_gaussians_idx)
    try:
        density_factor = float(density_factor)
    except (TypeError, ValueError):
        raise ValueError("density_factor must be a number") from None
    on_gpu("neighbor_density", x, (("centers", centers), ("inv_scaled_rotation", inv_sr), ("strengths", strengths),
                                   ("min_scaling", min_scaling), ("neighbour indices", nbr), ("gaussian_idx", row)),
           error=_gsr.GSRError)
    return _NeighborDensity.apply(x.contiguous(), centers.contiguous(), inv_sr.contiguous(), strengths.contiguous(),
                                  min_scaling.contiguous(), nbr.contiguous(),
                                  None if row is None else row.contiguous(), density_factor,
                                  bool(operator.truth(return_opacities)))


def get_field_values(x, *, points, inv_scaled_rotation, strengths, scaling, knn_idx=None, gaussian_idx=None,
                     closest_gaussians_idx=None, beta_mode="average", log_beta=None, return_sdf=True,
                     density_threshold=1., density_factor=1., return_sdf_grad=False, opacity_min_clamp=1e-16,
                     return_closest_gaussian_opacities=False, return_beta=False):
    """``SuGaRRegularizer.get_field_values`` (utils/sugar_utils.py:278-353) with ``get_beta`` (:400-471) as a function of
    the regulariser's tensors: points (N, 3), inv_scaled_rotation (N, 3, 3), strengths (N, 1) or (N,), scaling (N, 3).
    Returns the reference's ``fields`` dict: 'density' always, 'closest_gaussian_opacities', 'beta', 'sdf' on request.
    The fused kernel supplies density, opacities and the ``average`` beta; the rest is the reference's own torch
    arithmetic in its order.  ``return_sdf_grad`` is not built."""
    if return_sdf_grad:
        raise NotImplementedError("get_field_values: return_sdf_grad is not supported")
    if beta_mode not in ("learnable", "average", "weighted_average"):
        raise ValueError("Unknown beta_mode.")
    need_beta = return_sdf or return_beta
    if need_beta and beta_mode == "learnable" and not isinstance(log_beta, torch.Tensor):
        raise ValueError("beta_mode='learnable' needs log_beta")
    scaling = float_tensor(scaling, "scaling", (None, 3))
    min_scaling = scaling.min(dim=-1)[0]
    weighted = need_beta and beta_mode == "weighted_average"
    density, beta_avg, opacities = neighbor_density(
        x, points, inv_scaled_rotation, strengths, min_scaling, knn_idx=knn_idx, gaussian_idx=gaussian_idx,
        closest_gaussians_idx=closest_gaussians_idx, density_factor=density_factor,
        return_opacities=return_closest_gaussian_opacities or weighted)
    fields = {"density": density}
    # normalize density bigger or equal than 1 (by its detached self + 1e-12), on a copy as the reference does
    densities = density.clone()
    density_mask = densities >= 1.
    densities[density_mask] = densities[density_mask] / (densities[density_mask].detach() + 1e-12)
    if return_closest_gaussian_opacities:
        fields["closest_gaussian_opacities"] = opacities
    if need_beta:
        if beta_mode == "learnable":
            beta = torch.exp(log_beta).expand(len(x))
        elif beta_mode == "average":
            beta = beta_avg
        else:
            idx = closest_gaussians_idx if closest_gaussians_idx is not None else knn_idx[gaussian_idx]
            inside = (idx >= 0) & (idx < min_scaling.shape[0])  # padded slots carry weight 0 and scale 0
            neighbor_min_scaling = min_scaling[idx.clamp(0, max(int(min_scaling.shape[0]) - 1, 0))] * inside
            opacities_sum = opacities.sum(dim=-1, keepdim=True)
            weights = opacities / opacities_sum.clamp(min=opacity_min_clamp)
            beta = (neighbor_min_scaling * weights).sum(dim=-1)
            with torch.no_grad():
                # all opacities 0: far from every Gaussian, beta must not be 0 -> the largest min scale at hand
                beta[opacities_sum[..., 0] == 0.] = neighbor_min_scaling.max().detach()
        clamped_densities = densities.clamp(min=opacity_min_clamp)
    if return_beta:
        fields["beta"] = beta
    if return_sdf:
        fields["sdf"] = beta * (torch.sqrt(-2. * torch.log(clamped_densities))
                                - math.sqrt(-2. * math.log(min(density_threshold, 1.))))
    return fields


def _normal_in(x, centers, normals, min_scale, op, own, nbr, per_sample):
    """The gsr_sugar_normal of these tensors (addresses only: the caller keeps the tensors)."""
    p = _gsr._ptr
    return _gsr.SugarNormal(M=int(x.shape[0]), K=int(nbr.shape[1]), N=int(centers.shape[0]), R=int(nbr.shape[0]),
                            x=p(x), own=p(own), nbr=p(nbr), per_sample=int(per_sample), centers=p(centers),
                            normals=p(normals), min_scale=p(min_scale), op=p(op))


class _NeighborNormalLoss(torch.autograd.Function):
    """(x, centers, normals, min_scale, op) -> loss (M,); own / nbr are index tensors.  Only normals gets a gradient."""

    @staticmethod
    def forward(ctx, x, centers, normals, min_scale, op, own, nbr, per_sample):
        dev = x.device
        lib = _gsr.load_library()
        M, K, N = int(x.shape[0]), int(nbr.shape[1]), int(centers.shape[0])
        fopt = dict(dtype=torch.float32, device=dev)
        loss = torch.empty((M,), **fopt)
        rec = torch.empty((M, 4), **fopt) if ctx.needs_input_grad[2] else None  # (r, Wc): all the backward keeps
        if M > 0:
            nbytes = int(lib.gsr_sugar_normal_workspace_bytes(0, K, N))
            ws = workspace(nbytes, dev)
            _gsr._check(lib.gsr_sugar_normal_forward(
                _normal_in(x, centers, normals, min_scale, op, own, nbr, per_sample), _gsr._ptr(loss), _gsr._ptr(rec),
                _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        ctx.save_for_backward(x, centers, normals, min_scale, op, own, nbr, rec)
        ctx.per_sample = per_sample
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        x, centers, normals, min_scale, op, own, nbr, rec = ctx.saved_tensors
        dev = x.device
        M, K, N = int(x.shape[0]), int(nbr.shape[1]), int(centers.shape[0])
        if not ctx.needs_input_grad[2]:
            return (None,) * 8
        if M == 0 or N == 0:
            return (None, None, torch.zeros_like(normals)) + (None,) * 5
        lib = _gsr.load_library()
        (g_loss,) = ups((g_loss,), dev)
        dnormals = torch.empty_like(normals)
        nbytes = int(lib.gsr_sugar_normal_workspace_bytes(M, K, N))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_normal_backward(
            _normal_in(x, centers, normals, min_scale, op, own, nbr, ctx.per_sample), _gsr._ptr(rec),
            _gsr._ptr(g_loss), _gsr._ptr(dnormals), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return (None, None, dnormals) + (None,) * 5


def neighbor_normal_loss(x, centers, normals, min_scaling, opacities, *, gaussian_idx, knn_idx=None,
                         closest_gaussians_idx=None, gradient_through_normal_only=True):
    """The "sdf better normal loss" of ``coarse_density_regulation`` (utils/sugar_utils.py:725-757) per sample, fused.

    x (M, 3) samples; centers (N, 3); normals (N, 3) = ``get_normals()``, not necessarily unit; min_scaling (N,) =
    ``scaling.min(-1)[0]``; opacities (M, K) = the ``closest_gaussian_opacities`` of ``get_field_values`` for the same
    samples; all float32 on the GPU.  gaussian_idx (M,) int64 is the Gaussian i each sample was drawn in.  Neighbours:
    either ``knn_idx`` (N, K), sample m using the row ``knn_idx[gaussian_idx[m]]`` read in the kernel, or
    ``closest_gaussians_idx`` (M, K); int64, 1 <= K <= 32.

    Returns loss_normal (M,) = |n_i - sum_k wh_k s_k n_j|^2 with s_k = sign(n_j . n_i), wh_k = w_k / max(sum_k w_k,
    1e-6) and w_k = op[m, k] |(x_m - c_j) . n_j| / max(min_scaling_j, 1e-6)^2 (zero weight where s_k = 0).  As in the
    reference, whose ``sdf_better_normal_gradient_through_normal_only`` is always on, the signs and weights are
    constants and the gradient flows to ``normals`` only; ``gradient_through_normal_only=False`` is not built.  A
    neighbour index outside [0, N) contributes nothing; a ``gaussian_idx`` outside [0, N) gives 0 and no gradient.
    Bitwise reproducible, forward and backward; no double backward.
    """
    if not gradient_through_normal_only:
        raise NotImplementedError("neighbor_normal_loss: gradient_through_normal_only=False is not supported")
    x = float_tensor(x, "x", (None, 3))
    M = int(x.shape[0])
    centers = float_tensor(centers, "centers", (None, 3))
    N = int(centers.shape[0])
    normals = float_tensor(normals, "normals", (N, 3))
    min_scaling = float_tensor(min_scaling, "min_scaling", (N,))
    own = _index_tensor(gaussian_idx, "gaussian_idx", 1)
    if int(own.shape[0]) != M:
        raise ValueError(f"gaussian_idx must have one entry per sample ({M}), got {int(own.shape[0])}")
    if (knn_idx is None) == (closest_gaussians_idx is None):
        raise ValueError("give either knn_idx or closest_gaussians_idx (one of the two forms)")
    nbr, _ = _neighbour_table(M, knn_idx, None if knn_idx is None else own, closest_gaussians_idx)
    opacities = float_tensor(opacities, "opacities", (M, int(nbr.shape[1])))
    on_gpu("neighbor_normal_loss", x, (("centers", centers), ("normals", normals), ("min_scaling", min_scaling),
                                       ("opacities", opacities), ("neighbour indices", nbr), ("gaussian_idx", own)),
           error=_gsr.GSRError)
    return _NeighborNormalLoss.apply(x.contiguous(), centers.contiguous(), normals.contiguous(),
                                     min_scaling.contiguous(), opacities.contiguous(), own.contiguous(),
                                     nbr.contiguous(), knn_idx is None)


def _quaternion_to_matrix(q):
    """Rotation matrices (..., 3, 3) of quaternions (w, x, y, z), normalised here."""
    w, x, y, z = torch.nn.functional.normalize(q, dim=-1).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                       -1).reshape(q.shape[:-1] + (3, 3))


def _quaternion_multiply(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _quaternion_apply(q, p):
    """q (0, p) q^-1 for unit q: the rotation of the points p by the quaternions q."""
    pq = torch.cat([torch.zeros_like(p[..., :1]), p], -1)
    inv = q * q.new_tensor([1., -1., -1., -1.])
    return _quaternion_multiply(_quaternion_multiply(q, pq), inv)[..., 1:]


def smallest_axis(quaternions, scaling):
    """``get_smallest_axis`` (utils/sugar_utils.py:355-372), the normals of ``get_normals()`` for Gaussians not bound
    to a mesh: the column of each rotation matrix at the argmin of its scales, (N, 3).  quaternions (N, 4) are
    (w, x, y, z) and are normalised here; scaling (N, 3)."""
    quaternions = float_tensor(quaternions, "quaternions", (None, 4))
    scaling = float_tensor(scaling, "scaling", (int(quaternions.shape[0]), 3))
    idx = scaling.min(dim=-1)[1][..., None, None].expand(-1, 3, -1)
    return _quaternion_to_matrix(quaternions).gather(2, idx).squeeze(dim=2)


def sample_points_in_gaussians(points, quaternions, scaling, num_samples, sampling_scale_factor=1., *, strengths=None,
                               mask=None, probabilities_proportional_to_opacity=False,
                               probabilities_proportional_to_volume=True, generator=None):
    """``sample_points_in_gaussians`` (utils/sugar_utils.py:183-230): ``(random_points, random_indices)``.

    Faithful to the reference, including that ``torch.multinomial`` is fed the *cumulative* probabilities
    ``areas.cumsum() / areas.sum()`` as its weights (:214-218), not the probabilities: Gaussian number n of the
    (masked) list is drawn with a weight proportional to the summed area of Gaussians 0..n, so even the "uniform"
    setting (neither proportional flag) favours high indices linearly.  quaternions are normalised here;
    ``generator`` seeds both the draw of the indices and the Gaussian noise (None: the default generator)."""
    points = float_tensor(points, "points", (None, 3))
    n = int(points.shape[0])
    quaternions = float_tensor(quaternions, "quaternions", (n, 4))
    all_scaling = float_tensor(scaling, "scaling", (n, 3))
    scaling = all_scaling if mask is None else all_scaling[mask]
    if probabilities_proportional_to_volume:
        areas = scaling[..., 0] * scaling[..., 1] * scaling[..., 2]
    else:
        areas = torch.ones_like(scaling[..., 0])
    if probabilities_proportional_to_opacity:
        if strengths is None:
            raise ValueError("probabilities_proportional_to_opacity needs strengths")
        areas = areas * (strengths.view(-1) if mask is None else strengths[mask].view(-1))
    areas = areas.abs()
    cum_probs = areas.cumsum(dim=-1) / areas.sum(dim=-1, keepdim=True)
    random_indices = torch.multinomial(cum_probs, num_samples=num_samples, replacement=True, generator=generator)
    if mask is not None:
        random_indices = torch.arange(n, device=points.device)[mask][random_indices]
    centers = points[random_indices]
    noise = torch.randn(centers.shape, dtype=centers.dtype, device=centers.device, generator=generator)
    q = torch.nn.functional.normalize(quaternions, dim=-1)[random_indices]
    random_points = centers + _quaternion_apply(q, sampling_scale_factor * all_scaling[random_indices] * noise)
    return random_points, random_indices


def coarse_density_regulation(points, quaternions, scaling, strengths, knn_idx, *, n_samples,
                              use_sdf_better_normal_loss, beta_mode="average", log_beta=None, generator=None):
    """The regulation losses of ``SuGaRRegularizer.coarse_density_regulation`` (utils/sugar_utils.py:683-759) as a
    function of the regulariser's tensors: points (N, 3), quaternions (N, 4) (w, x, y, z), scaling (N, 3) and
    strengths (N, 1) or (N,) as activated by the Gaussian model, knn_idx (N, K).  Returns the reference's
    ``{"density_regulation", "normal_regulation"}`` with its constants (density_factor 1, density_threshold 1,
    sampling_scale_factor 1.5, sampling not proportional to volume or opacity).  The two M x K parts are the fused
    ``neighbor_density`` and ``neighbor_normal_loss``; the rest is the reference's torch arithmetic in its order.
    ``normal_regulation`` is 0 when ``use_sdf_better_normal_loss`` is off, as is everything for an empty cloud."""
    loss = {"density_regulation": 0, "normal_regulation": 0}
    if int(points.shape[0]) == 0:
        return loss
    sdf_samples, sdf_gaussian_idx = sample_points_in_gaussians(
        points, quaternions, scaling, n_samples, 1.5, probabilities_proportional_to_volume=False, generator=generator)
    rotation = _quaternion_to_matrix(quaternions)
    inv_scaled_rotation = rotation * (1. / scaling.clamp(min=1e-8))[:, None]
    fields = get_field_values(
        sdf_samples, points=points, inv_scaled_rotation=inv_scaled_rotation, strengths=strengths, scaling=scaling,
        knn_idx=knn_idx, gaussian_idx=sdf_gaussian_idx, beta_mode=beta_mode, log_beta=log_beta, return_sdf=False,
        density_threshold=1., density_factor=1., return_closest_gaussian_opacities=use_sdf_better_normal_loss,
        return_beta=True)
    gaussians_normals = smallest_axis(quaternions, scaling)
    samples_gaussian_normals = gaussians_normals[sdf_gaussian_idx]
    sdf_estimation = ((sdf_samples - points[sdf_gaussian_idx]) * samples_gaussian_normals).sum(dim=-1)
    target_densities = torch.exp(-0.5 * sdf_estimation.pow(2) / fields["beta"].pow(2))
    loss["density_regulation"] = loss["density_regulation"] + (fields["density"] - target_densities).abs().mean()
    if use_sdf_better_normal_loss:
        loss["normal_regulation"] = loss["normal_regulation"] + neighbor_normal_loss(
            sdf_samples.detach(), points.detach(), gaussians_normals, scaling.min(dim=-1)[0].detach(),
            fields["closest_gaussian_opacities"].detach(), gaussian_idx=sdf_gaussian_idx, knn_idx=knn_idx).mean()
    return loss
