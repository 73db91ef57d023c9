"""The densification statistics of a view batch in one call (include/gsr.h gsr_densify_stats, csrc/gsr_densify.hip).

After every backward the reference's ``GaussianBaseModel.update_states`` (geometry/gaussian_base.py:821-869) walks the
batch in Python: per view ``max_radii2D = max(max_radii2D, radii_i.float())``,
``xyz_gradient_accum[vis_i] += norm(viewspace_i.grad[vis_i, :2])`` and ``denom[vis_i] += 1`` (:845-851, :815-819) —
about ten small launches and two or three boolean-mask indexings (a ``nonzero`` with a host sync each) per view.
``densify_stats`` takes the per-view lists the batch renderer returns (batch_renderer.py ``viewspace_points`` /
``radii`` / ``visibility_filter``) and updates the three per-Gaussian arrays in place in one kernel launch per 64
views, without a host sync, adding view after view in the reference's order (the norm is ``(gx * gx + gy * gy).sqrt()``
in fp32, every operation rounded on its own).  ``update_states_fused`` is ``geometry.update_states`` on top of it.

GPU tensors go to the library (no torch fall-back there: a missing kernel is an ImportError from the binding); CPU
tensors take ``_densify_stats_torch``, the same arithmetic in the same order spelled in elementwise torch operations,
which the gloo and CPU tests run and the GPU tests use as the bit reference of the kernel.
"""
from __future__ import annotations

import torch

from . import _C, view_shard

CHUNK = _C.SET_MAX  # views per library call (include/gsr.h GSR_SET_MAX: the struct's pointer tables)


def _row(t, dtype, P, name, width=None):
    """`t` as a contiguous row of `dtype` with P entries ((P, width) with width)."""
    want = (P,) if width is None else (P, width)
    if tuple(t.shape) != want:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {want}")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _state(t, P, device, name):
    """(tensor to return, flat fp32 contiguous (P,) working array, needs copying back) of one statistic."""
    if t is None:
        return None, None, False
    if t.numel() != P or tuple(t.shape) not in ((P,), (P, 1)):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected ({P},) or ({P}, 1)")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, the views are on {device}")
    if t.dtype == torch.float32 and t.is_contiguous():
        return t, t.view(-1), False
    return t, t.to(torch.float32).contiguous().view(-1), True


def _densify_stats_torch(radii, grads, visible, m, s, c):
    """The kernel's arithmetic in its order (csrc/gsr_densify.hip k_dstat_views), elementwise and without mask
    indexing: fp32, every operation rounded on its own, view after view into the running values.  `radii`: int32 rows,
    `grads`: (P,3) fp32 rows or None, `visible`: bool rows or None; m, s, c are updated in place."""
    for v, r in enumerate(radii):
        rf = r.to(torch.float32)
        m.copy_(torch.where(rf > m, rf, m))  # (a NaN in m stays: rf > NaN is False; torch.max keeps it too)
        seen = visible[v] if visible is not None else r > 0
        g = grads[v]
        if g is not None:
            gx, gy = g[:, 0], g[:, 1]
            # the correctly rounded fp32 root, as the kernel's: through fp64 (53 >= 2 * 24 + 2 bits: the second rounding
            # cannot change it).  torch's own fp32 sqrt on the CPU is an ulp off on some hosts' vector units.
            norm = (gx * gx + gy * gy).double().sqrt().float()
            s.copy_(torch.where(seen, s + norm, s))
        c.copy_(torch.where(seen, c + 1.0, c))


def _densify_stats_hip(radii, grads, visible, m, s, c, accumulate, device):
    lib = _C.load_library()
    stream = _C._stream(device)
    V, P = len(radii), int(m.numel())
    vis8 = None if visible is None else [x.view(torch.uint8) for x in visible]
    for v0 in range(0, V, CHUNK):
        n = min(CHUNK, V - v0)
        a = _C.DensifyBatch(V=n, P=P, accumulate=1 if (accumulate or v0 > 0) else 0, max_radii=m.data_ptr(),
                            grad_norm_sum=s.data_ptr(), count=c.data_ptr())
        for k in range(n):
            a.radii[k] = radii[v0 + k].data_ptr()
            g = grads[v0 + k]
            a.grads[k] = None if g is None else g.data_ptr()
            a.visible[k] = None if vis8 is None else vis8[v0 + k].data_ptr()
        _C._check(lib.gsr_densify_stats(a, stream))


@torch.no_grad()
def densify_stats(radii, viewspace_points, visibility_filter=None, *, max_radii=None, grad_norm_sum=None, count=None):
    """Per-Gaussian densification statistics of a view batch, view after view in list order:

        max_radii     = max(max_radii, radii[v].float())
        grad_norm_sum += |viewspace_points[v].grad[:, :2]|   where the view sees the Gaussian
        count         += 1                                   where the view sees the Gaussian

    radii: list of (P,) integer rows.  viewspace_points: list of the (P,3) leaves whose ``.grad`` is read (the sum of
    every backward call so far); an entry, or its ``.grad``, may be None: that view adds no norm but still counts.
    visibility_filter: list of (P,) bool rows, or None for ``radii > 0``.  The three keyword tensors, (P,) or (P,1), are
    updated in place (the reference's max_radii2D, xyz_gradient_accum and denom); one that is not given starts from
    zero.  Returns (max_radii, grad_norm_sum, count).  No host sync; GPU tensors: one launch per 64 views on the current
    stream; CPU tensors: the same arithmetic in torch."""
    radii = list(radii)
    V = len(radii)
    if len(viewspace_points) != V or (visibility_filter is not None and len(visibility_filter) != V):
        raise ValueError("radii, viewspace_points and visibility_filter must list the same views")
    given = [t for t in (max_radii, grad_norm_sum, count) if t is not None]
    if V == 0 and not given:
        raise ValueError("densify_stats: no view and no statistic to tell the number of Gaussians from")
    P = int(radii[0].shape[0]) if V else int(given[0].numel())
    device = radii[0].device if V else given[0].device
    rows = [_row(r, torch.int32, P, "radii") for r in radii]
    grads = []
    for vp in viewspace_points:
        g = None if vp is None else vp.grad
        grads.append(None if g is None else _row(g, torch.float32, P, "viewspace_points.grad", 3))
    visible = None
    if visibility_filter is not None:
        visible = [rows[v] > 0 if f is None else _row(f, torch.bool, P, "visibility_filter")
                   for v, f in enumerate(visibility_filter)]
    for t in rows + [g for g in grads if g is not None] + (visible or []):
        if t.device != device:
            raise ValueError(f"the views' tensors are on {t.device} and {device}")
    hip = device.type == "cuda"
    # (from zero on the GPU with no statistic given: the first call overwrites, the arrays need no fill)
    fresh = torch.empty if (hip and not given and V > 0 and P > 0) else torch.zeros
    out, work, back = [], [], []
    for t, name in ((max_radii, "max_radii"), (grad_norm_sum, "grad_norm_sum"), (count, "count")):
        ret, flat, copy = _state(t, P, device, name)
        if ret is None:
            ret = flat = fresh((P,), dtype=torch.float32, device=device)
        out.append(ret)
        work.append(flat)
        back.append(copy)
    if V > 0 and P > 0:
        if hip:
            _densify_stats_hip(rows, grads, visible, *work, accumulate=bool(given), device=device)
        else:
            _densify_stats_torch(rows, grads, visible, *work)
    for ret, flat, copy in zip(out, work, back):
        if copy:
            ret.copy_(flat.view_as(ret))
    return tuple(out)


def update_states_fused(geometry, iteration, outputs: dict, group=None):
    """``geometry.update_states(iteration, visibility_filter, radii, viewspace_points)``
    (geometry/gaussian_base.py:821-869) for a whole batch: ``outputs`` is the batch renderer's dict.

    The per-view loop (:845-851) is one ``densify_stats`` call that updates ``max_radii2D``, ``xyz_gradient_accum`` and
    ``denom`` in place in the reference's order; it is skipped exactly where the reference returns before it (the SuGaR
    prune :830-834 and the max_num prune :836-841).  The rest of ``update_states`` — those prunes, the scheduled prune
    and densify — then runs with empty view lists.  In a process group of more than one rank (view_shard: every rank
    holds its own views) the ranks' partial statistics, formed from zero, are reduced first (MAX / SUM) and added, and
    the rest runs under ``view_shard.replica_rng`` so that the replicas stay identical, as
    ``view_shard.update_states_sharded`` does."""
    cfg = geometry.cfg
    P = int(geometry.get_xyz.shape[0])
    early = (getattr(cfg, "sugar_prune_at", None) is not None and iteration == cfg.sugar_prune_at) or \
        P >= cfg.max_num + 100
    world, _ = view_shard._world()
    lists = (outputs["radii"], outputs["viewspace_points"], outputs["visibility_filter"])
    with torch.no_grad():
        if not early and world == 1:
            densify_stats(*lists, max_radii=geometry.max_radii2D, grad_norm_sum=geometry.xyz_gradient_accum,
                          count=geometry.denom)
        elif not early:  # (every rank takes this branch: `early` follows from the replicated state)
            dev = geometry.get_xyz.device
            max_r, gsum, cnt = densify_stats(*lists, **{k: torch.zeros(P, device=dev) for k in
                                                        ("max_radii", "grad_norm_sum", "count")})
            view_shard.dist.all_reduce(max_r, op=view_shard.dist.ReduceOp.MAX, group=group)
            both = torch.stack([gsum, cnt])
            view_shard.dist.all_reduce(both, group=group)
            geometry.max_radii2D = torch.max(geometry.max_radii2D, max_r)
            geometry.xyz_gradient_accum += both[0][:, None]
            geometry.denom += both[1][:, None]
        with view_shard.replica_rng(group):
            geometry.update_states(iteration, [], [], [])
