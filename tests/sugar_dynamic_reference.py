"""A torch restatement of the dynamic-SuGaR geometry (include/gsr.h gsr_sugar_skin_* and gsr_sugar_timed_*),
differentiated by autograd: the checker of tests/test_sugar_dynamic.py and tests/test_gpu_sugar_dynamic.py.  It follows
the formulas of the header literally, in the dtype of its inputs (float64: the reference; float32: the "fp32 null" the
GPU bars are calibrated on, i.e. what the torch composition the kernels replace would give).  pypose is spelled out:
quaternions are (x, y, z, w), ``Log`` takes the plain arctangent of |v| / w and works on a quaternion of any norm,
``Exp`` yields w = cos(theta / 2); both switch to their series near 0 (below a threshold that follows the dtype, where
the first dropped term is under half an ulp)."""
import math

import torch
import torch.nn.functional as F


def _series_threshold(dtype):
    return 1e-8 if dtype == torch.float64 else 1e-4


def qmul(a, b):
    """The Hamilton product of (..., 4) xyzw quaternions."""
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    v = aw * bv + bw * av + torch.cross(av, bv, dim=-1)
    w = aw * bw - (av * bv).sum(-1, keepdim=True)
    return torch.cat([v, w], -1)


def qconj(a):
    return torch.cat([-a[..., :3], a[..., 3:]], -1)


def qlog(q):
    """(..., 4) xyzw, non-zero, any norm -> (..., 3): theta v / |v| with theta = 2 atan(|v| / w) (pi at w = 0)."""
    v, w = q[..., :3], q[..., 3:]
    n2 = (v * v).sum(-1, keepdim=True)
    small = n2 < _series_threshold(q.dtype) * w * w
    one = torch.ones_like(w)
    n = torch.sqrt(torch.where(small, one, n2))
    w_zero = w == 0
    w_big = torch.where(small | w_zero, one, w)
    s_big = torch.where(w_zero, math.pi / n, 2 * torch.atan(n / w_big) / n)
    w_small = torch.where(small, w, one)
    s_small = 2 / w_small - 2 * n2 / (3 * w_small ** 3)
    return torch.where(small, s_small, s_big) * v


def qexp(phi):
    """(..., 3) -> (..., 4) xyzw: (sin(theta / 2) / theta phi, cos(theta / 2)), theta = |phi|."""
    t2 = (phi * phi).sum(-1, keepdim=True)
    small = t2 < _series_threshold(phi.dtype)
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    k = torch.where(small, 0.5 - t2 / 48, torch.sin(t / 2) / t)
    c = torch.where(small, 1 - t2 / 8, torch.cos(t / 2))
    return torch.cat([k * phi, c], -1)


def qmatrix(q):
    """The rotation matrix (..., 3, 3) of a unit xyzw quaternion."""
    x, y, z, w = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def qrotate(q, p):
    """R(q) p, elementwise (no batched matrix product: the batch would be every (frame, vertex, node) item)."""
    return (qmatrix(q) * p[..., None, :]).sum(-1)


def skin_vertices_reference(verts, node_xyz, node_trans, node_rots, nbr, w, method="dqs", node_scales=None):
    """(vert_xyz (T, V, 3), vert_rot (T, V, 4) xyzw, vert_scale (T, V, 3) or None); nbr (V, K) int64, w (V, K)."""
    w = w.to(verts.dtype)[None, :, :, None]
    qhat = node_rots / node_rots.norm(dim=-1, keepdim=True)
    q = qhat[:, nbr]  # (T, V, K, 4)
    trans = node_trans[:, nbr]
    if method == "dqs":
        d = 0.5 * qmul(torch.cat([trans, torch.zeros_like(trans[..., :1])], -1), q)
        s_r, s_d = (w * q).sum(-2), (w * d).sum(-2)
        m = s_r.norm(dim=-1, keepdim=True)
        r, e = s_r / m, s_d / m
        t = 2 * qmul(e, qconj(r))[..., :3]
        xyz = qrotate(r, verts[None]) + t
    elif method == "lbs":
        x = node_xyz[nbr][None]  # (1, V, K, 3)
        y = qrotate(q, verts[None, :, None] - x) + x + trans
        xyz = (w * y).sum(-2)
    else:
        raise ValueError(method)
    rot = qexp((w * qlog(node_rots)[:, nbr]).sum(-2))
    scale = None if node_scales is None else (w * node_scales[:, nbr]).sum(-2)
    return xyz, rot, scale


def face_normals(vert_xyz, faces):
    """The unit normals (T, F, 3) of the deformed faces by the formula of gsr_sugar_mesh_forward (0 if degenerate)."""
    fv = vert_xyz[:, faces]
    p0, p1, p2 = fv[:, :, 0], fv[:, :, 1], fv[:, :, 2]
    n = F.normalize(torch.cross(p1 - p0, p2 - p0, dim=-1), eps=1e-6, dim=-1)
    return F.normalize(n, eps=1e-12, dim=-1)


def timed_gaussians_reference(vert_xyz, vert_rot, rotation0, faces, bary, vert_scale=None, log_scales=None,
                              thickness=None):
    """(xyz (T, N, 3), rotation (T, N, 4) wxyz, normals (T, N, 3), scaling (T, N, 3) or None); faces (F, 3) int64,
    bary (G, 3), N = F G."""
    dt = vert_xyz.dtype
    T = vert_xyz.shape[0]
    b = bary.to(dt)[None, None, :, :, None]  # (1, 1, G, 3, 1)
    G = bary.shape[0]
    xyz = (vert_xyz[:, faces][:, :, None] * b).sum(-2).reshape(T, -1, 3)
    phi = (qlog(vert_rot)[:, faces][:, :, None] * b).sum(-2).reshape(T, -1, 3)
    q0 = rotation0[None, :, [1, 2, 3, 0]]
    rotation = F.normalize(qmul(qexp(phi), q0)[..., [3, 0, 1, 2]], eps=1e-12, dim=-1)
    normals = face_normals(vert_xyz, faces).repeat_interleave(G, dim=1)
    scaling = None
    if vert_scale is not None:
        s = (vert_scale[:, faces][:, :, None] * b).sum(-2).reshape(T, -1, 3)
        thick = torch.full(s.shape[:-1] + (1,), thickness, dtype=dt, device=s.device)
        scaling = torch.cat([thick, torch.exp(log_scales[None] + s[..., 1:])], -1)
    return xyz, rotation, normals, scaling


SKIN_INPUTS = ("verts", "node_trans", "node_rots", "node_scales")
SKIN_OUTPUTS = ("xyz", "rot", "scale")
TIMED_INPUTS = ("vert_xyz", "vert_rot", "rotation0", "vert_scale", "log_scales")
TIMED_OUTPUTS = ("xyz", "rotation", "normals", "scaling")


def _evaluate(fn, names_in, names_out, dtype, inputs, ups):
    leaves = {k: None if inputs.get(k) is None else inputs[k].detach().to(dtype).clone().requires_grad_()
              for k in names_in}
    out = fn(leaves)
    res = {k: None if v is None else v.detach() for k, v in zip(names_out, out)}
    loss = 0
    for k, v in zip(names_out, out):
        g = ups.get(k)
        if g is not None and v is not None:
            loss = loss + (v * g.to(dtype)).sum()
    have = [k for k in names_in if leaves[k] is not None]
    if torch.is_tensor(loss) and loss.requires_grad:
        grads = torch.autograd.grad(loss, [leaves[k] for k in have], allow_unused=True)
    else:
        grads = [None] * len(have)
    for k, g in zip(have, grads):
        res["d" + k] = torch.zeros_like(leaves[k]) if g is None else g
    return res


def evaluate_skin(dtype, inputs, node_xyz, nbr, w, method, ups):
    """Outputs (by SKIN_OUTPUTS) and gradients ("d" + name of SKIN_INPUTS) of the restatement in `dtype`.  inputs: a
    dict over SKIN_INPUTS (node_scales may be None); ups: the upstream gradients by output name (absent = zero)."""
    return _evaluate(lambda x: skin_vertices_reference(x["verts"], node_xyz.to(dtype), x["node_trans"], x["node_rots"],
                                                       nbr.long(), w, method, x["node_scales"]),
                     SKIN_INPUTS, SKIN_OUTPUTS, dtype, inputs, ups)


def evaluate_timed(dtype, inputs, faces, bary, thickness, ups):
    """The same for timed_gaussians_reference, over TIMED_INPUTS / TIMED_OUTPUTS."""
    return _evaluate(lambda x: timed_gaussians_reference(x["vert_xyz"], x["vert_rot"], x["rotation0"], faces.long(),
                                                         bary, x["vert_scale"], x["log_scales"], thickness),
                     TIMED_INPUTS, TIMED_OUTPUTS, dtype, inputs, ups)


# ---- the reference's own skinning and timed Gaussians: tests/golden/reference_dynamic.npz ----------------------------
SKIN_KEYS = ("xyz", "rotation", "scale", "dverts", "dnode_trans", "dnode_rots", "dnode_scales")
TIMED_KEYS = ("xyz", "rotation", "scale", "dvert_xyz", "dvert_rot", "drotation0", "dvert_scale", "dlog_scales")


def tangent(g, q):
    """The part of a gradient g to unit quaternions q that is orthogonal to q: its component along q is the derivative
    with respect to the quaternion's norm."""
    q = q.to(g.dtype)
    return g - (g * q).sum(-1, keepdim=True) * q
