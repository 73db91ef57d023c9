"""A torch restatement of the reference's ARAP energy with given rotations (include/gsr.h gsr_sugar_arap_*),
differentiated by autograd: the checker of tests/test_sugar_arap.py and tests/test_gpu_sugar_arap.py.

It keeps the reference's composition (ARAPCoach, utils/arap_utils.py): a dense (V, V) weight matrix (small V only), a
padded (V, max valence) neighbour table, and per frame a padded (V, max valence, 3) edge matrix filled by
``index_put``, a ``bmm`` with the rotations, a norm and a weighted sum, in the dtype of its inputs (float64: the
reference; float32: the "fp32 null" the GPU bars are calibrated on).  Written from the formulas of the header, with
pypose's ``matrix()`` spelled out (``sugar_dynamic_reference.qmatrix``: no normalisation)."""
import torch

from sugar_cases import check_against_null
from sugar_dynamic_reference import qmatrix


def dense_cot_weights(verts, faces):
    """W + W^T, (V, V) in verts' dtype, with W[f[c], f[(c + 1) % 3]] = cot[c] / 8: the cotangent of the angle at corner
    c by Heron's area (clamped at 1e-12 before the root), assigned to the edge that leaves the corner."""
    V = verts.shape[0]
    faces = faces.long()
    fv = verts[faces]
    v0, v1, v2 = fv[:, 0], fv[:, 1], fv[:, 2]
    A = (v1 - v2).norm(dim=1)
    B = (v0 - v2).norm(dim=1)
    C = (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp_(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([(B2 + C2 - A2) / area, (A2 + C2 - B2) / area, (A2 + B2 - C2) / area], dim=1)
    cot /= 4.0
    W = torch.zeros((V, V), dtype=verts.dtype)
    W[faces.flatten(), faces[:, [1, 2, 0]].flatten()] = 0.5 * cot.flatten()
    return W + W.T


def one_rings(faces, V):
    """(ii, jj, nn): the directed one-ring edges (i, j), i ascending and j ascending within i, and j's slot nn in i's
    padded row.  A plain Python loop over the faces."""
    rings = [set() for _ in range(V)]
    for f in faces.tolist():
        for c in range(3):
            rings[f[c]].update((f[(c + 1) % 3], f[(c + 2) % 3]))
    ii, jj, nn = [], [], []
    for i, ring in enumerate(rings):
        for n, j in enumerate(sorted(ring)):
            ii.append(i), jj.append(j), nn.append(n)
    return torch.tensor(ii, dtype=torch.long), torch.tensor(jj, dtype=torch.long), torch.tensor(nn, dtype=torch.long)


def padded(values, ii, nn, V):
    """(V, max valence, ...) with values[e] at [ii[e], nn[e]] and zeros elsewhere, by index_put."""
    M = int(nn.max()) + 1 if nn.numel() else 1
    out = torch.zeros((V, M) + tuple(values.shape[1:]), dtype=values.dtype, device=values.device)
    return out.index_put((ii, nn), values)


def arap_energy_reference(vert_xyz, vert_rot, verts, ii, jj, nn, w):
    """(T,) energies.  vert_xyz (T, V, 3); vert_rot (T, V, 3, 3) matrices or (T, V, 4) xyzw quaternions; verts (V, 3)
    the rest vertices; (ii, jj, nn) of ``one_rings``; w (E,) the edge weights in that order (any dtype: constants)."""
    dt, V = vert_xyz.dtype, verts.shape[0]
    verts = verts.to(dt)
    R = qmatrix(vert_rot) if vert_rot.dim() == 3 else vert_rot
    Wn = padded(w.to(dt), ii, nn, V)
    P = padded(verts[ii] - verts[jj], ii, nn, V)
    out = []
    for t in range(vert_xyz.shape[0]):  # the reference's loop over the frames
        P_prime = padded(vert_xyz[t, ii] - vert_xyz[t, jj], ii, nn, V)
        rigid = torch.bmm(R[t], P.permute(0, 2, 1)).permute(0, 2, 1)
        stretch = torch.norm(P_prime - rigid, dim=2) ** 2
        out.append((Wn * stretch).sum())
    return torch.stack(out) if out else torch.zeros((0,), dtype=dt)


def evaluate(dtype, vert_xyz, vert_rot, verts, rings, w, up):
    """{"energy", "dvert_xyz", "dvert_rot"} of the restatement in `dtype`; up (T,): the upstream gradient."""
    x = vert_xyz.detach().to(dtype).clone().requires_grad_()
    r = vert_rot.detach().to(dtype).clone().requires_grad_()
    e = arap_energy_reference(x, r, verts, *rings, w)
    gx, gr = torch.autograd.grad((e * up.to(dtype)).sum(), [x, r], allow_unused=True)
    return {"energy": e.detach(), "dvert_xyz": torch.zeros_like(x) if gx is None else gx,
            "dvert_rot": torch.zeros_like(r) if gr is None else gr}


ARAP_MESHES = ("tetrahedron", "icosphere1", "fan40", "sliver")  # of tests/golden/reference_arap.npz
ENERGY_FLOOR = 2.0 ** -23


def check_arap(got, r64, r32, tag, grads=("dvert_xyz", "dvert_rot")):
    """The bar of the ARAP tests: sugar_cases.check_against_null on the gradients; the (T,) energy has too few elements
    for the null to be a stable sample, so per frame |got - ref64| / |ref64| <= max(2 x null, 2^-23), the second term
    being one float32 rounding of an fp64 result, doubled.  Prints its figures."""
    check_against_null(got, r64, r32, grads, tag)
    e, e64, e32 = got["energy"].double(), r64["energy"], r32["energy"].double()
    assert got["energy"].dtype == torch.float32 and e.shape == e64.shape, (tag, e.shape)
    for t in range(len(e64)):
        scale = abs(float(e64[t]))
        if scale == 0:
            assert float(e[t]) == 0, (tag, t)
            continue
        err, null = abs(float(e[t] - e64[t])) / scale, abs(float(e32[t] - e64[t])) / scale
        print(f"{tag} energy[{t}]: gpu {err:.3g}  fp32 null {null:.3g}")
        assert err <= max(2 * null, ENERGY_FLOOR), (tag, t, err, null)
