"""Inputs and restatements for the densification-statistics tests (test infrastructure, no tests here).

- ``make_views``: the per-view lists a batch renderer returns (radii, viewspace leaves with a ``.grad``, visibility
  rows), seeded per view, so that a slice of views is the same whoever builds it.
- ``loop_fp32``: the statistic as a direct fp32 loop over the views in numpy, every operation rounded on its own.
- ``sum_fp64``: the gradient-norm sum in fp64, and ``bound``: the fp32 error bound against it.
- ``reference_form``: the reference's own statements (geometry/gaussian_base.py:845-851, :815-819): ``torch.max`` and
  ``torch.norm(grad[vis, :2], dim=-1)`` added per view by mask indexing.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of fp32


def bound(V):
    """Relative bound of the fp32 sequential sum of V norms against the fp64 one: (V + 3) 2^-24.  Each norm carries at
    most 2 * 2^-24: a square and the sum of the squares put 2 * 2^-24 under the root, which halves it, and the root
    rounds once more.  Each of the V sequential adds of non-negative terms adds at most 2^-24 of the running sum, which
    never exceeds the final one.  One more unit covers the second-order terms."""
    return (V + 3) * U


def make_views(V, P, seed=0, none_at=(), explicit=(), device="cpu", first=0):
    """Views first .. first + V - 1 of a batch.  Radii in 0..5 with a few large ones (a sixth are 0: not visible);
    gradient magnitudes log-uniform in [1e-6, 1e2] with random signs and a tenth exact zeros (no square is subnormal);
    the third gradient column holds NaNs (nobody may read it), and so do the first two where radii == 0 (nobody may
    add them).  Views in `none_at` have no gradient; views in `explicit` get visibility rows that differ from
    radii > 0 in about a fifth of the Gaussians (the other views' rows are radii > 0)."""
    radii, vps, vis = [], [], []
    for v in range(first, first + V):
        g = torch.Generator().manual_seed(seed * 100_003 + v)
        r = torch.randint(0, 6, (P,), generator=g, dtype=torch.int32)
        big = torch.rand(P, generator=g) < 0.05
        r = torch.where(big & (r > 0), r * 37 + v, r)
        mag = 10.0 ** (torch.rand(P, 3, generator=g) * 8.0 - 6.0)
        sign = torch.where(torch.rand(P, 3, generator=g) < 0.5, -1.0, 1.0)
        grad = (mag * sign).float()
        grad[torch.rand(P, 3, generator=g) < 0.1] = 0.0
        grad[:, 2] = float("nan")
        seen = r > 0
        if v in explicit:
            seen = seen ^ (torch.rand(P, generator=g) < 0.2)
        grad[~seen, :2] = float("nan")
        vp = torch.zeros(P, 3, device=device, requires_grad=True)
        if v not in none_at:
            vp.grad = grad.to(device)
        radii.append(r.to(device))
        vps.append(vp)
        vis.append(seen.to(device))
    return {"radii": radii, "viewspace_points": vps, "visibility_filter": vis}


def clone_views(views, device):
    """The same views on `device`, sharing nothing."""
    vps = []
    for vp in views["viewspace_points"]:
        q = torch.zeros(vp.shape, device=device, requires_grad=True)
        if vp.grad is not None:
            q.grad = vp.grad.detach().to(device).clone()
        vps.append(q)
    return {"radii": [r.to(device).clone() for r in views["radii"]], "viewspace_points": vps,
            "visibility_filter": [f.to(device).clone() for f in views["visibility_filter"]]}


def loop_fp32(views, m=None, s=None, c=None):
    """(max, sum, count) as float32 numpy arrays: the views in order, each operation a float32 operation."""
    P = views["radii"][0].shape[0]
    m = np.zeros(P, np.float32) if m is None else np.array(m, np.float32).reshape(P)
    s = np.zeros(P, np.float32) if s is None else np.array(s, np.float32).reshape(P)
    c = np.zeros(P, np.float32) if c is None else np.array(c, np.float32).reshape(P)
    one = np.float32(1.0)
    for r, vp, seen in zip(views["radii"], views["viewspace_points"], views["visibility_filter"]):
        rf = r.cpu().numpy().astype(np.float32)
        seen = seen.cpu().numpy()
        for p in range(P):
            if rf[p] > m[p]:  # (false for a NaN m[p]: it stays)
                m[p] = rf[p]
            if not seen[p]:
                continue
            if vp.grad is not None:
                x, y = (np.float32(t) for t in vp.grad[p, :2].cpu().numpy())
                xx, yy = np.float32(x * x), np.float32(y * y)
                # (the correctly rounded fp32 root whatever the host's fp32 sqrt does: an fp32 number's root, taken
                # in fp64 and rounded to fp32, is the correctly rounded one)
                root = np.float32(np.sqrt(np.float64(np.float32(xx + yy))))
                s[p] = np.float32(s[p] + root)
            c[p] = np.float32(c[p] + one)
    return m, s, c


def sum_fp64(views):
    """The gradient-norm sum over the views in fp64 (numpy)."""
    P = views["radii"][0].shape[0]
    s = np.zeros(P, np.float64)
    for vp, seen in zip(views["viewspace_points"], views["visibility_filter"]):
        if vp.grad is None:
            continue
        g = vp.grad.detach().cpu().numpy().astype(np.float64)
        seen = seen.cpu().numpy()
        s[seen] += np.sqrt(g[seen, 0] ** 2 + g[seen, 1] ** 2)
    return s


def reference_form(views, max_radii2D, xyz_gradient_accum, denom):
    """geometry/gaussian_base.py:845-851 with add_densification_stats (:815-819) on the given state ((P,), (P,1),
    (P,1)); a view without a gradient only counts (view_shard.reduce_densify_stats).  Returns the new max_radii2D
    (the reference rebinds it); the other two are updated in place."""
    with torch.no_grad():
        for r, vp, seen in zip(views["radii"], views["viewspace_points"], views["visibility_filter"]):
            max_radii2D = torch.max(max_radii2D, r.float())
            if vp.grad is not None:
                xyz_gradient_accum[seen] += torch.norm(vp.grad[seen, :2], dim=-1, keepdim=True)
            denom[seen] += 1
    return max_radii2D


def quiet_cfg(**over):
    """DensifyModel settings under which update_states neither prunes nor densifies before iteration 1000, and then
    densifies only (no prune, so that the selected masks are the whole difference)."""
    cfg = dict(prune_from_iter=100_000, prune_until_iter=100_001, densify_from_iter=999, densify_until_iter=10_000,
               densification_interval=1000)
    cfg.update(over)
    return cfg


def borderline(accum, denom, threshold, V):
    """Number of Gaussians whose mean gradient norm accum / denom lies within the sum's bound of the densification
    threshold (either side): a faithful fp32 evaluation may select them or not."""
    g = (accum.double() / denom.double()).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    return int(((g - threshold).abs() <= bound(V) * g.abs()).sum())


def select_masks(model, threshold):
    """The clone and split selections of densify (geometry/gaussian_base.py:771-777, :715-725) from the model's
    statistics, without applying them."""
    with torch.no_grad():
        grads = model.xyz_gradient_accum / model.denom
        grads[grads.isnan()] = 0.0
        big = torch.norm(model.get_scaling, dim=1) > model.cfg.split_thresh
        over = torch.norm(grads, dim=-1) >= threshold
        return over & ~big, (grads.squeeze() >= threshold) & big
