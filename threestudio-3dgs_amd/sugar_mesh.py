"""The geometry of SuGaR Gaussians bound to a mesh over the C ABI (include/gsr.h gsr_sugar_mesh_*, csrc/gsr_mesh.hip).

In the reference's refine stage (configs/sugar_static_refine.yaml: 6 Gaussians per surface triangle, learnable
positions) a Gaussian has no position, normal axis or orientation of its own: ``SuGaRModel.points``, ``.scaling``,
``.quaternions`` and ``.get_gs_normals`` (geometry/sugar.py:449-536) rebuild them, at every property read, from the
mesh vertices, the face table, a 2-D "complex" in-plane rotation and two log-scales per Gaussian, through an (F, 3, 3)
vertex gather, a pytorch3d ``Meshes`` built for its face normals, three normalisations, two cross products, an
(N, 3, 3) concatenation and ``matrix_to_quaternion``; autograd keeps every intermediate and scatters the vertex
gradient with ``index_put`` atomics.  Here ``bound_gaussians`` is one fused kernel forward and two backward, which
recompute from the inputs and sum per vertex in a fixed order (no atomics: two calls give the same bits).

``MeshBinding`` is built once per mesh (in ``load_surface_mesh_to_bind``): it checks the faces, keeps an int32 copy
and the vertex incidence the backward sums by.  The four properties of the reference become views of one call
(INTEGRATION.md section 6).  GPU only, like ``sugar_field.neighbor_density``.
"""
from __future__ import annotations

import ctypes
import math

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import INT_DTYPES, Binding, aligned, float_tensor, incidence, on_gpu, ups, workspace

__all__ = ["MeshBinding", "bound_gaussians", "initial_log_scales", "REFERENCE_BARY", "REFERENCE_CIRCLE_RADIUS",
           "MESH_MAX_G"]

MESH_MAX_G = 8  # include/gsr.h GSR_MESH_MAX_G

# geometry/sugar.py:245-286: the barycentric coordinates of a triangle's Gaussians and the radius of the circle each
# one covers (in units of the triangle's shortest side), by n_gaussians_per_surface_triangle
REFERENCE_BARY = {
    1: ((1 / 3, 1 / 3, 1 / 3),),
    3: ((1 / 2, 1 / 4, 1 / 4), (1 / 4, 1 / 2, 1 / 4), (1 / 4, 1 / 4, 1 / 2)),
    4: ((1 / 3, 1 / 3, 1 / 3), (2 / 3, 1 / 6, 1 / 6), (1 / 6, 2 / 3, 1 / 6), (1 / 6, 1 / 6, 2 / 3)),
    6: ((2 / 3, 1 / 6, 1 / 6), (1 / 6, 2 / 3, 1 / 6), (1 / 6, 1 / 6, 2 / 3),
        (1 / 6, 5 / 12, 5 / 12), (5 / 12, 1 / 6, 5 / 12), (5 / 12, 5 / 12, 1 / 6)),
}
REFERENCE_CIRCLE_RADIUS = {
    1: 1. / 2. / math.sqrt(3.),
    3: 1. / 2. / (math.sqrt(3.) + 1.),
    4: 1. / (4. * math.sqrt(3.)),
    6: 1. / (4. + 2. * math.sqrt(3.)),
}

class MeshBinding(Binding):
    """What ``bound_gaussians`` needs of a mesh besides its vertices, built once.

    faces (F, 3), any integer dtype, every entry in [0, n_verts) (checked here: one host synchronisation);
    bary (G, 3), 1 <= G <= 8: the barycentric coordinates of a face's G Gaussians (Gaussian f G + g belongs to face f).
    Attributes: ``faces`` (F, 3) int32; ``corner_order`` (3F,) int32, the corners 3 f + c grouped by vertex, ascending
    within a vertex (a stable sort of ``faces.reshape(-1)``); ``vert_offsets`` (V + 1,) int32, vertex v owning
    ``corner_order[vert_offsets[v]:vert_offsets[v + 1]]``; ``bary`` (G, 3) float32 on the CPU (it travels in the kernel
    arguments); ``n_verts``, ``n_faces``, ``n_per_face``, ``n_gaussians``; ``circle_radius`` (None unless given).
    Works on CPU tensors too; ``to(device)`` moves the index tensors.
    """

    _TENSORS = ("faces", "corner_order", "vert_offsets")

    def __init__(self, faces, n_verts, bary, circle_radius=None):
        if not isinstance(faces, torch.Tensor) or faces.dtype not in INT_DTYPES:
            raise ValueError("faces must be an integer tensor")
        if faces.dim() != 2 or int(faces.shape[1]) != 3:
            raise ValueError(f"faces must have shape (*, 3), got {tuple(faces.shape)}")
        if isinstance(n_verts, bool) or not isinstance(n_verts, int) or n_verts < 0:
            raise ValueError("n_verts must be a non-negative integer")
        try:
            bary = torch.as_tensor(bary, dtype=torch.float32).detach().cpu().contiguous().clone()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("bary must be a (G, 3) array of numbers") from None
        if bary.dim() != 2 or int(bary.shape[1]) != 3 or not 1 <= int(bary.shape[0]) <= MESH_MAX_G:
            raise ValueError(f"bary must have shape (G, 3) with 1 <= G <= {MESH_MAX_G}, got {tuple(bary.shape)}")
        F = int(faces.shape[0])
        if F * int(bary.shape[0]) >= 2 ** 31 or n_verts >= 2 ** 31:
            raise ValueError("the mesh is too large: F x G and n_verts must stay below 2^31")
        flat = faces.reshape(-1).to(torch.int64)
        if F > 0 and (int(flat.min()) < 0 or int(flat.max()) >= n_verts):
            raise ValueError(f"faces has entries outside [0, {n_verts})")
        self.faces = faces.to(torch.int32).contiguous()
        self.corner_order, self.vert_offsets = incidence(flat, n_verts)
        self.bary = bary
        self.n_verts, self.n_faces, self.n_per_face = n_verts, F, int(bary.shape[0])
        self.n_gaussians = F * self.n_per_face
        self.circle_radius = None if circle_radius is None else float(circle_radius)

    @classmethod
    def from_reference_count(cls, faces, n_verts, n_gaussians_per_surface_triangle):
        """The binding with the reference's barycentric set and circle radius for 1, 3, 4 or 6 Gaussians per face."""
        G = n_gaussians_per_surface_triangle
        if G not in REFERENCE_BARY:
            raise ValueError(f"the reference places 1, 3, 4 or 6 Gaussians per triangle, not {G!r}")
        return cls(faces, n_verts, REFERENCE_BARY[G], REFERENCE_CIRCLE_RADIUS[G])


def initial_log_scales(verts, binding, circle_radius=None):
    """``initialize_learnable_radiuses`` (geometry/sugar.py:311-327): the initial ``_scales`` (N, 2) of the bound
    Gaussians, log of max(shortest side of the face x circle radius, 1e-7), the same for a face's G Gaussians and for
    both in-plane axes.  Init only, plain torch (CPU or GPU)."""
    verts = float_tensor(verts, "verts", (binding.n_verts, 3))
    radius = binding.circle_radius if circle_radius is None else circle_radius
    if radius is None:
        raise ValueError("this binding has no circle radius: give circle_radius")
    fv = verts[binding.faces.to(device=verts.device, dtype=torch.int64)]  # (F, 3, 3)
    scales = (fv - fv[:, [1, 2, 0]]).norm(dim=-1).min(dim=-1)[0] * radius
    scales = scales.clamp_min(0.0000001).reshape(-1, 1, 1).expand(-1, binding.n_per_face, 2)
    return torch.log(scales).reshape(-1, 2).contiguous()


def _bary_ptr(binding):
    return ctypes.c_void_p(binding.bary.data_ptr())


def _mesh_in(verts, cplx, log_scales, binding):
    """The gsr_sugar_mesh of these tensors (addresses only: the caller keeps the tensors)."""
    p = _gsr._ptr
    return _gsr.SugarMesh(V=binding.n_verts, F=binding.n_faces, G=binding.n_per_face, verts=p(verts),
                          faces=p(binding.faces), cplx=p(cplx), log_scales=p(log_scales))


class _BoundGaussians(torch.autograd.Function):
    """(verts, complex_numbers, log_scales) -> (xyz, scaling, rotation, normals)."""

    @staticmethod
    def forward(ctx, verts, cplx, log_scales, binding, thickness):
        dev = verts.device
        lib = _gsr.load_library()
        F, N = binding.n_faces, binding.n_gaussians
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(verts, cplx, log_scales)
        ctx.binding = binding
        fopt = dict(dtype=torch.float32, device=dev)
        xyz, scaling, normals = (torch.empty((N, 3), **fopt) for _ in range(3))
        rotation = torch.empty((N, 4), **fopt)
        if F > 0:
            _gsr._check(lib.gsr_sugar_mesh_forward(
                _mesh_in(verts, cplx, log_scales, binding), N, _bary_ptr(binding), thickness, _gsr._ptr(xyz),
                _gsr._ptr(scaling), _gsr._ptr(rotation), _gsr._ptr(normals), _gsr._stream(dev)))
        return xyz, scaling, rotation, normals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_scaling, g_rotation, g_normals):
        verts, cplx, log_scales = ctx.saved_tensors
        binding = ctx.binding
        dev = verts.device
        V, F, N = binding.n_verts, binding.n_faces, binding.n_gaussians
        if F == 0 or all(g is None for g in (g_xyz, g_scaling, g_rotation, g_normals)):
            return torch.zeros_like(verts), torch.zeros_like(cplx), torch.zeros_like(log_scales), None, None
        lib = _gsr.load_library()
        grads = ups((g_xyz, g_scaling, g_rotation, g_normals), dev)
        dverts, dcplx, dls = torch.empty_like(verts), torch.empty_like(cplx), torch.empty_like(log_scales)
        nbytes = int(lib.gsr_sugar_mesh_workspace_bytes(F, V))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_mesh_backward(
            _mesh_in(verts, cplx, log_scales, binding), N, _bary_ptr(binding), _gsr._ptr(binding.corner_order),
            _gsr._ptr(binding.vert_offsets), *(_gsr._ptr(g) for g in grads), _gsr._ptr(dverts), _gsr._ptr(dcplx),
            _gsr._ptr(dls), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return dverts, dcplx, dls, None, None


def bound_gaussians(verts, complex_numbers, log_scales, binding, thickness):
    """The mesh-bound Gaussians of ``SuGaRModel``: ``(xyz, scaling, rotation, normals)`` = its ``points`` (N, 3),
    ``scaling`` (N, 3), ``quaternions`` (N, 4) (w, x, y, z; unit) and ``get_gs_normals`` (N, 3), N = F G.

    verts (V, 3) = ``_points``; complex_numbers (N, 2) = ``_quaternions`` (the in-plane rotation, normalised here);
    log_scales (N, 2) = ``_scales``; all float32 on the GPU.  binding: the mesh's ``MeshBinding``; thickness =
    ``surface_mesh_thickness``.  Gaussian f G + g lies at sum_k bary[g, k] p_k of face f, has scales (thickness,
    exp(log_scales)), the face normal as its first axis and the face's first side, turned by the complex number in
    the face's plane, as its second (the formulas: include/gsr.h).  The quaternion's overall sign is that of
    ``matrix_to_quaternion``'s candidate row and may differ from the reference's where two candidates tie; every
    consumer is even in it.  Gradients flow to verts, complex_numbers and log_scales, bitwise reproducible; no double
    backward.
    """
    if not isinstance(binding, MeshBinding):
        raise ValueError("binding must be a MeshBinding")
    verts = float_tensor(verts, "verts", (binding.n_verts, 3))
    N = binding.n_gaussians
    try:
        cplx = float_tensor(complex_numbers, "complex_numbers", (N, 2))
        log_scales = float_tensor(log_scales, "log_scales", (N, 2))
    except ValueError as e:
        raise ValueError(f"{e} (N = F x G = {binding.n_faces} x {binding.n_per_face})") from None
    try:
        thickness = float(thickness)
    except (TypeError, ValueError):
        raise ValueError("thickness must be a number") from None
    on_gpu("bound_gaussians", verts, (("complex_numbers", cplx), ("log_scales", log_scales),
                                      ("the binding", binding.faces)))
    return _BoundGaussians.apply(verts.contiguous(), aligned(cplx), aligned(log_scales), binding, thickness)
