"""Plain-torch stand-ins for the small part of pypose and pytorch3d that the reference's SuGaR code calls, so that
tests/golden/make_golden.py can execute that code where neither library is installed.  The project's own code, written
from the libraries' documented conventions, dtype-generic (float32 and float64) and differentiable by autograd.
tests/test_reference_pins.py pins every function here to scipy.spatial.transform.Rotation at fp64 rounding.

pypose (injected as ``pp``): a LieTensor is a torch.Tensor subclass whose last dimension holds a quaternion
(x, y, z, w) (``SO3``) or a rotation vector (``so3``).  ``*`` and ``@`` between two SO3 are the Hamilton product; with a
number or a plain tensor ``*`` and ``/`` act elementwise (the reference scales and normalises quaternions that way).
``Log`` takes the plain arctangent of |v| / w, so w < 0 gives the same rotation vector as -q; ``Exp`` yields
w = cos(theta / 2) >= 0.  Both switch to their Taylor series near zero, below a threshold at which the first dropped
term is under half an ulp of the dtype.  ``matrix()`` is R = I + 2 w [v]x + 2 [v]x^2, the rotation of a unit
quaternion; what pypose does with a quaternion that is not unit is not known here, and the fixtures never ask.

pytorch3d: ``quaternion_to_matrix`` and ``matrix_to_quaternion`` in (w, x, y, z) order, the latter with the library's
choice among its four candidates (the largest of the four square roots, each candidate divided by twice that root
floored at 0.1) and no sign standardisation; ``Meshes`` with ``faces_normals_list`` (the cross product of the first two
edges, normalised with eps = 1e-6).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _hamilton(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    v = aw * bv + bw * av + torch.linalg.cross(av, bv, dim=-1)
    w = aw * bw - (av * bv).sum(-1, keepdim=True)
    return torch.cat([v, w], -1)


class LieTensor(torch.Tensor):
    """Base of SO3Tensor and so3Tensor.  Results of torch functions keep the subclass (torch's default)."""

    def tensor(self):
        return self.as_subclass(torch.Tensor)

    def __rmul__(self, other):
        return torch.mul(self.tensor(), other).as_subclass(type(self))

    def __truediv__(self, other):
        other = other.tensor() if isinstance(other, LieTensor) else other
        return torch.div(self.tensor(), other).as_subclass(type(self))


class SO3Tensor(LieTensor):
    def __mul__(self, other):
        if isinstance(other, SO3Tensor):
            return _hamilton(self.tensor(), other.tensor()).as_subclass(SO3Tensor)
        other = other.tensor() if isinstance(other, LieTensor) else other
        return torch.mul(self.tensor(), other).as_subclass(SO3Tensor)

    def __matmul__(self, other):
        if isinstance(other, SO3Tensor):
            return self * other
        raise NotImplementedError("the stand-in composes rotations only")

    def Inv(self):
        q = self.tensor()
        return torch.cat([-q[..., :3], q[..., 3:]], -1).as_subclass(SO3Tensor)

    def Log(self):
        q = self.tensor()
        v, w = q[..., :3], q[..., 3:]
        n2 = (v * v).sum(-1, keepdim=True)
        small = n2 < 0.1 * math.sqrt(torch.finfo(q.dtype).eps) * w * w
        one = torch.ones_like(w)
        n = torch.sqrt(torch.where(small, one, n2))
        w_zero = w == 0
        w_safe = torch.where(small | w_zero, one, w)
        direct = torch.where(w_zero, math.pi / n, 2 * torch.atan(n / w_safe) / n)
        w_series = torch.where(small, w, one)
        series = 2 / w_series - 2 * n2 / (3 * w_series ** 3)
        return (torch.where(small, series, direct) * v).as_subclass(so3Tensor)

    def matrix(self):
        x, y, z, w = self.tensor().unbind(-1)
        m = torch.stack([
            1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
        return m.reshape(self.shape[:-1] + (3, 3))


class so3Tensor(LieTensor):
    def __mul__(self, other):
        if isinstance(other, LieTensor):
            raise NotImplementedError("rotation vectors are scaled, not composed")
        return torch.mul(self.tensor(), other).as_subclass(so3Tensor)

    def Exp(self):
        phi = self.tensor()
        t2 = (phi * phi).sum(-1, keepdim=True)
        small = t2 < math.sqrt(torch.finfo(phi.dtype).eps)
        t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
        k = torch.where(small, 0.5 - t2 / 48, torch.sin(t / 2) / t)
        c = torch.where(small, 1 - t2 / 8, torch.cos(t / 2))
        return torch.cat([k * phi, c], -1).as_subclass(SO3Tensor)


def SO3(data):
    assert data.shape[-1] == 4, data.shape
    return torch.as_tensor(data).as_subclass(SO3Tensor)


def so3(data):
    assert data.shape[-1] == 3, data.shape
    return torch.as_tensor(data).as_subclass(so3Tensor)


def identity_SO3(*size, **kwargs):
    q = torch.zeros(*size, 4, **kwargs)
    q[..., 3] = 1
    return q.as_subclass(SO3Tensor)


def quaternion_to_matrix(quaternions):
    """(..., 4) (w, x, y, z) of any non-zero norm -> (..., 3, 3); the scale 2 / |q|^2 makes the result a rotation."""
    r, i, j, k = torch.unbind(quaternions, -1)
    two_s = 2.0 / (quaternions * quaternions).sum(-1)
    o = torch.stack([
        1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
        two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
        two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], -1)
    return o.reshape(quaternions.shape[:-1] + (3, 3))


def _sqrt_positive_part(x):
    """sqrt(max(0, x)) with a zero subgradient where x <= 0."""
    ret = torch.zeros_like(x)
    positive = x > 0
    ret[positive] = torch.sqrt(x[positive])
    return ret


def matrix_to_quaternion(matrix):
    """(..., 3, 3) rotations -> (..., 4) (w, x, y, z), the sign as the chosen candidate gives it."""
    batch = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp(min=0.1))
    pick = F.one_hot(q_abs.argmax(dim=-1), num_classes=4) > 0.5
    return cand[pick, :].reshape(batch + (4,))


class Meshes:
    """One mesh per list entry; only what the reference's SuGaR geometry reads."""

    def __init__(self, verts, faces, textures=None):
        self._verts, self._faces = list(verts), list(faces)

    def faces_normals_list(self):
        out = []
        for v, f in zip(self._verts, self._faces):
            fv = v[f.long()]
            n = torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)
            out.append(F.normalize(n, eps=1e-6, dim=-1))
        return out


class TexturesVertex:
    def __init__(self, verts_features=None):
        self.verts_features = verts_features
