"""A torch restatement of the mesh-bound SuGaR Gaussian geometry (include/gsr.h gsr_sugar_mesh_*), differentiated by
autograd: the checker of tests/test_sugar_mesh.py and tests/test_gpu_sugar_mesh.py.  It follows the formulas of the
header literally, in the dtype of its inputs (float64: the reference; float32: the "fp32 null" the GPU bars are
calibrated on, i.e. what the torch composition the kernel replaces would give).  pytorch3d is spelled out:
``faces_normals`` is normalize(cross, eps=1e-6), ``matrix_to_quaternion`` the four candidate rows, each divided by
2 max(a_i, 0.1), the row of the largest a_i taken (torch.argmax: the first on ties), no sign standardisation."""
import torch
import torch.nn.functional as F


class _SqrtPos(torch.autograd.Function):
    """sqrt(x) for x > 0, else 0 with zero gradient (pytorch3d's _sqrt_positive_part)."""

    @staticmethod
    def forward(ctx, x):
        pos = x > 0
        ret = torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))
        ctx.save_for_backward(ret, pos)
        return ret

    @staticmethod
    def backward(ctx, g):
        ret, pos = ctx.saved_tensors
        return torch.where(pos, g / (2 * torch.where(pos, ret, torch.ones_like(ret))), torch.zeros_like(g))


def matrix_to_quaternion(m, branch=None):
    """(N, 3, 3) -> (N, 4) (w, x, y, z), not normalised further; also returns the row index taken.  `branch`
    (N,) int64 forces the rows."""
    m00, m01, m02 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m10, m11, m12 = m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    m20, m21, m22 = m[:, 2, 0], m[:, 2, 1], m[:, 2, 2]
    a = _SqrtPos.apply(torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22,
                                    1 - m00 - m11 + m22], -1))
    cand = torch.stack([
        torch.stack([a[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, a[:, 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, a[:, 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, a[:, 3] ** 2], -1)], -2)  # (N, 4 rows, 4)
    cand = cand / (2 * torch.clamp(a, min=0.1))[:, :, None]
    if branch is None:
        branch = a.detach().argmax(dim=-1)
    return cand.gather(1, branch[:, None, None].expand(-1, 1, 4))[:, 0], branch


def bound_gaussians_reference(verts, faces, bary, cplx, log_scales, thickness, branch=None):
    """(xyz, scaling, rotation, normals, branch) in verts.dtype; faces (F, 3) int64 in range, bary (G, 3)."""
    dt = verts.dtype
    bary = bary.to(device=verts.device, dtype=dt)
    G = bary.shape[0]
    fv = verts[faces]  # (F, 3, 3)
    p0, p1, p2 = fv[:, 0], fv[:, 1], fv[:, 2]
    n = F.normalize(torch.cross(p1 - p0, p2 - p0, dim=-1), eps=1e-6, dim=-1)
    R0 = F.normalize(n, eps=1e-12, dim=-1)
    b1 = F.normalize(p0 - p1, eps=1e-12, dim=-1)
    b2 = F.normalize(torch.cross(R0, b1, dim=-1), eps=1e-12, dim=-1)
    z = F.normalize(cplx, eps=1e-12, dim=-1).view(-1, G, 2)
    R1 = z[..., 0:1] * b1[:, None] + z[..., 1:2] * b2[:, None]
    R2 = -z[..., 1:2] * b1[:, None] + z[..., 0:1] * b2[:, None]
    R = torch.stack([R0[:, None].expand(-1, G, -1), R1, R2], dim=-1).reshape(-1, 3, 3)  # columns
    q, branch = matrix_to_quaternion(R, branch)
    rotation = F.normalize(q, eps=1e-12, dim=-1)
    xyz = (fv[:, None] * bary[None, :, :, None]).sum(dim=-2).reshape(-1, 3)
    thick = torch.full((len(cplx), 1), thickness, dtype=dt, device=verts.device)
    scaling = torch.cat([thick, torch.exp(log_scales)], dim=-1)
    normals = R0.repeat_interleave(G, dim=0)
    return xyz, scaling, rotation, normals, branch


OUTPUTS = ("xyz", "scaling", "rotation", "normals")
GRADS = ("verts", "complex", "log_scales")


def evaluate(dtype, verts, faces, bary, cplx, log_scales, thickness, ups, sign=None, branch=None):
    """Outputs and gradients of the restatement in `dtype`, as a dict over OUTPUTS + GRADS (+ "branch").  ups: the
    upstream gradients by output name (None or absent = zero).  sign (N,) multiplies the rotation's upstream
    gradient rows (the row-sign alignment of a comparison)."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in (verts, cplx, log_scales)]
    out = bound_gaussians_reference(leaves[0], faces.long(), bary, leaves[1], leaves[2], thickness, branch)
    res = {k: v.detach() for k, v in zip(OUTPUTS, out)}
    res["branch"] = out[4]
    loss = 0
    for k, v in zip(OUTPUTS, out):
        g = ups.get(k)
        if g is not None:
            g = g.to(dtype)
            if k == "rotation" and sign is not None:
                g = g * sign.to(dtype)[:, None]
            loss = loss + (v * g).sum()
    if torch.is_tensor(loss) and loss.requires_grad:
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    else:
        grads = (None, None, None)
    for k, g, leaf in zip(GRADS, grads, leaves):
        res[k] = torch.zeros_like(leaf) if g is None else g
    return res


def row_sign(got_rotation, ref_rotation):
    """+-1 per row: the sign of the dot product of a quaternion row with the reference's (+1 at 0)."""
    d = (got_rotation.double() * ref_rotation.double()).sum(-1)
    return torch.where(d < 0, -torch.ones_like(d), torch.ones_like(d))


# ---- the reference's own mesh-bound Gaussians: tests/golden/reference_mesh.npz ---------------------------------------
MESH_KEYS = OUTPUTS + GRADS


def mesh_fixture(z, G, tag):
    return {k: z[f"G{G}_{'d' if k in GRADS else ''}{k}_{tag}"] for k in MESH_KEYS}
