"""The deformation network of dynamic SuGaR restated in plain tensor expressions, in either dtype: what
sugar_deform.deformation_knots computes (include/gsr.h gsr_sugar_deform_*), i.e. ``forward_dynamic_delta`` of
geometry/deformation.py at T ticks x P points with the epilogue of ``_get_timed_dg_attributes_wo_spline``.  The bilinear
gather is written out (no ``grid_sample``), so that this is an independent statement; tests/test_sugar_deform.py pins it
to the reference's own code through tests/golden/reference_deform.npz."""
import itertools
import os

import numpy as np
import torch

COMBOS = tuple(itertools.combinations(range(4), 2))
OUTPUTS = ("xyz", "rot", "scale")


def normalize_aabb(pts, aabb):
    return (pts - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0


def bilinear(plane, x, y):
    """plane (1, C, H, W) at the normalised coordinates x (along W) and y (n,): (n, C); align_corners, border."""
    g = plane[0]
    H, W = g.shape[1:]

    def axis(c, R):
        c = ((c + 1) / 2 * (R - 1)).clamp(0, R - 1)
        i = torch.floor(c)
        f = c - i
        i = i.long()
        return i, (i + 1).clamp(max=R - 1), 1 - f, f

    x0, x1, wx0, wx1 = axis(x, W)
    y0, y1, wy0, wy1 = axis(y, H)
    out = (g[:, y0, x0] * (wx0 * wy0) + g[:, y0, x1] * (wx1 * wy0) + g[:, y1, x0] * (wx0 * wy1)
           + g[:, y1, x1] * (wx1 * wy1))
    return out.t()


def features(pts4, planes):
    """(n, 4) normalised coordinates -> (n, 32 L): per level the product of the six plane samples."""
    out = []
    for l in range(len(planes) // 6):
        f = 1.0
        for q, (a, b) in enumerate(COMBOS):
            f = f * bilinear(planes[6 * l + q], pts4[:, a], pts4[:, b])
        out.append(f)
    return torch.cat(out, -1)


def deformation_reference(points, ticks, aabb, planes, mlp, normalize_rot=True):
    """(xyz (T, P, 3), rot (T, P, 4), scale (T, P, 3) or None); mlp: 14 tensors, or 10 without the scale head."""
    T, P = ticks.shape[0], points.shape[0]
    pts = normalize_aabb(points, aabb).repeat(T, 1)
    ts = (ticks * 2 - 1).repeat_interleave(P)[:, None]
    h = features(torch.cat([pts, ts], -1), planes) @ mlp[0].t() + mlp[1]
    outs = []
    for i in range(2, len(mlp), 4):
        r = torch.relu(h)
        y = r + (r @ mlp[i].t() + mlp[i + 1])
        outs.append(y @ mlp[i + 2].t() + mlp[i + 3])
    xyz, rot = outs[0].reshape(T, P, 3), outs[1].reshape(T, P, 4)
    rot = rot + torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=rot.dtype)
    if normalize_rot:
        rot = rot / rot.norm(dim=-1, keepdim=True)
    return xyz, rot, outs[2].reshape(T, P, 3) if len(outs) > 2 else None


def evaluate(dtype, points, ticks, aabb, planes, mlp, ups, normalize_rot=True):
    """Outputs and autograd gradients in ``dtype``: {"xyz", "rot", "scale", "dplane<i>", "dmlp<i>"}; ups: the upstream
    gradients by output name (a missing one is zero)."""
    pl = [t.detach().to(dtype).requires_grad_() for t in planes]
    ml = [t.detach().to(dtype).requires_grad_() for t in mlp]
    out = deformation_reference(points.to(dtype), ticks.to(dtype), aabb.to(dtype), pl, ml, normalize_rot)
    res = {k: o.detach() for k, o in zip(OUTPUTS, out) if o is not None}
    loss = sum((o * ups[k].to(dtype)).sum() for k, o in zip(OUTPUTS, out) if o is not None and k in ups)
    grads = torch.autograd.grad(loss, pl + ml, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, pl + ml)]
    res.update({f"dplane{i}": g for i, g in enumerate(grads[:len(pl)])})
    res.update({f"dmlp{i}": g for i, g in enumerate(grads[len(pl):])})
    return res


def keys(n_planes, n_mlp):
    return (("xyz", "rot") + (("scale",) if n_mlp == 14 else ()) + tuple(f"dplane{i}" for i in range(n_planes))
            + tuple(f"dmlp{i}" for i in range(n_mlp)))


# ---- the reference's own DeformationNetwork: tests/golden/reference_deform.npz ---------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"dg": (True, True), "dg_noscale": (True, False), "vert": (False, True)}  # normalize_rot, d_scale
_CACHE = {}


def fixture():
    if "z" not in _CACHE:
        z = np.load(os.path.join(HERE, "golden", "reference_deform.npz"))
        _CACHE["z"] = {k: (z[k] if z[k].dtype.kind == "U" else torch.from_numpy(z[k])) for k in z.files}
    return _CACHE["z"]


def fixture_weights(z, d_scale):
    from sugar_deform import DeformationWeights

    return DeformationWeights.from_state_dict({k: z["w_" + k] for k in z["names"]}, d_scale)


def fixture_reference(z, case, tag, weights):
    """{key of sugar_deform_reference.evaluate: the reference's tensor} for what the fixture stores of the case."""
    out = {k: z[f"{case}_{n}_{tag}"] for k, n in zip(OUTPUTS, ("xyz", "rotation", "scale"))
           if f"{case}_{n}_{tag}" in z}
    L6 = len(weights.planes)
    for i, name in enumerate(weights.names):
        key = f"{case}_d_{name}_{tag}"
        if key in z:
            out[f"dplane{i}" if i < L6 else f"dmlp{i - L6}"] = z[key]
    return out


def fixture_ups(z, d_scale):
    ups = {"xyz": z["up_xyz"], "rot": z["up_rotation"]}
    if d_scale:
        ups["scale"] = z["up_scale"]
    return ups
