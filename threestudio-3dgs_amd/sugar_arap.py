"""The as-rigid-as-possible regulariser of dynamic SuGaR's motion stage over the C ABI (include/gsr.h gsr_sugar_arap_*,
csrc/gsr_arap.hip).

The reference's ``_compute_arap_energy`` (system/sugar_4dgen.py: the terms ``arap_reg_key_frame`` and
``arap_reg_inter_frame``) takes the timed vertices and their rotation matrices and calls
``ARAPCoach.compute_arap_energy`` (utils/arap_utils.py:148-189) once per frame in a Python loop: a padded (V, max
valence, 3) edge matrix scattered by ``index_put``, two ``bmm``, a norm and a weighted sum, every intermediate kept by
autograd and an atomic scatter in ``index_put``'s backward.  The coach itself forms a dense (V, V) weight matrix to
read about 6 V entries back.  Here it is one fused call for all T frames of a batch, on the outputs of
``sugar_dynamic.skin_vertices`` as they are:

    binding = ArapBinding(verts, faces)                       # once per mesh
    loss_arap = arap_energy(vert_xyz, vert_rot, binding).sum()

whose backward recomputes from the inputs and only gathers (no atomics: two calls give the same bits).  ``vert_rot``
is (T, V, 4) pypose (x, y, z, w) quaternions or (T, V, 3, 3) matrices.  The rest mesh is a constant (detached when the
binding is built), as in the motion stage.  GPU only, like ``sugar_dynamic``.
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import INT_DTYPES, Binding, aligned, float_tensor, on_gpu, row_offsets, ups, workspace

__all__ = ["ArapBinding", "arap_energy", "ARAP_ROT_FORMS"]

ARAP_ROT_FORMS = {"quat": 0, "matrix": 1}  # GSR_ARAP_QUAT, GSR_ARAP_MATRIX

class ArapBinding(Binding):
    """The one-rings of a rest mesh with the reference's edge weights, built once, in plain torch, without anything
    of size V x V.

    verts (V, 3) floating point (``get_xyz_verts``; detached, taken as float32), faces (F, 3) of any integer dtype
    (``get_faces``), every entry in [0, V), no face with a repeated vertex, no directed edge (a, b) = (f[c],
    f[(c + 1) % 3]) in two faces (there the reference's ``W[i, j] = ...`` has no defined winner): checked here, one
    host synchronisation.  Attributes, in CSR over the directed one-ring edges (i, j), i ascending and j ascending
    within a row (a vertex in no face has an empty row):
    ``offsets`` (V + 1,) int32; ``nbr`` (E,) int32, the j; ``w`` (E,) float32, w_ij = W[i, j] + W[j, i] with
    W[f[c], f[(c + 1) % 3]] = cot[c] / 8 of ``produce_cot_weights_nfmt(sparse=False)`` (arap_utils.py:77-116: the
    angle at v0 goes to edge (v0, v1); float32 Heron area clamped at 1e-12 before the root; op for op, so bitwise the
    reference's values; negative at obtuse corners); ``p`` (E, 3) float32 = verts[i] - verts[j], the entries of the
    reference's ``edge_matrix_nfmt`` (the kernels form p from ``verts`` in fp64 instead, exactly, see include/gsr.h);
    ``verts`` (V, 3) float32; ``n_verts``, ``n_faces``, ``n_edges``, ``max_valence``.  Works on CPU tensors too;
    ``to(device)`` moves it.
    """

    _TENSORS = ("nbr", "offsets", "w", "p", "verts")

    def __init__(self, verts, faces):
        if not isinstance(verts, torch.Tensor) or not verts.is_floating_point():
            raise ValueError("verts must be a floating-point tensor")
        if verts.dim() != 2 or int(verts.shape[1]) != 3:
            raise ValueError(f"verts must have shape (V, 3), got {tuple(verts.shape)}")
        if not isinstance(faces, torch.Tensor) or faces.dtype not in INT_DTYPES:
            raise ValueError("faces must be an integer tensor")
        if faces.dim() != 2 or int(faces.shape[1]) != 3:
            raise ValueError(f"faces must have shape (F, 3), got {tuple(faces.shape)}")
        if faces.device != verts.device:
            raise ValueError(f"faces is on {faces.device}, verts on {verts.device}")
        V, F = int(verts.shape[0]), int(faces.shape[0])
        if V >= 2 ** 31 or 6 * F >= 2 ** 31:
            raise ValueError("the mesh is too large: V and the 6 F directed edges must stay below 2^31")
        verts = verts.detach().to(torch.float32).contiguous()
        faces = faces.to(torch.int64)
        if F > 0 and (int(faces.min()) < 0 or int(faces.max()) >= V):
            raise ValueError(f"faces has entries outside [0, {V})")
        if F > 0 and bool(((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) |
                           (faces[:, 2] == faces[:, 0])).any()):
            raise ValueError("a face repeats a vertex")
        # the cotangents, op for op as arap_utils.py:77-98
        face_verts = verts[faces]
        v0, v1, v2 = face_verts[:, 0], face_verts[:, 1], face_verts[:, 2]
        A = (v1 - v2).norm(dim=1)
        B = (v0 - v2).norm(dim=1)
        C = (v0 - v1).norm(dim=1)
        s = 0.5 * (A + B + C)
        area = (s * (s - A) * (s - B) * (s - C)).clamp_(min=1e-12).sqrt()
        A2, B2, C2 = A * A, B * B, C * C
        cot = torch.stack([(B2 + C2 - A2) / area, (A2 + C2 - B2) / area, (A2 + B2 - C2) / area], dim=1)
        cot /= 4.0
        # W[i, j] = 0.5 cot, sparse: the directed edges as sorted keys i V + j
        key = faces.flatten() * V + faces[:, [1, 2, 0]].flatten()
        key, order = torch.sort(key)
        val = (0.5 * cot.flatten())[order]
        if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
            raise ValueError("a directed edge occurs in more than one face: the reference's weight is undefined")
        rev = (key % V) * V + key // V
        edges = torch.unique(torch.cat([key, rev]))  # sorted: i ascending, j ascending within i
        ii, jj = edges // V, edges % V

        def lookup(k):  # W at the keys k, 0 where no face has the directed edge
            if key.numel() == 0:
                return torch.zeros(k.shape, dtype=torch.float32, device=k.device)
            pos = torch.searchsorted(key, k).clamp_(max=key.numel() - 1)
            return torch.where(key[pos] == k, val[pos], torch.zeros_like(val[pos]))

        counts = torch.bincount(ii, minlength=V)
        self.offsets = row_offsets(counts)
        self.nbr = jj.to(torch.int32).contiguous()
        self.w = (lookup(edges) + lookup(jj * V + ii)).contiguous()
        self.p = (verts[ii] - verts[jj]).contiguous()
        self.verts = verts
        self.n_verts, self.n_faces, self.n_edges = V, F, int(edges.numel())
        self.max_valence = int(counts.max()) if V > 0 else 0


class _ArapEnergy(torch.autograd.Function):
    """(vert_xyz, vert_rot) -> energy (T,)."""

    @staticmethod
    def _in(vert_xyz, vert_rot, binding, form):
        """The gsr_sugar_arap of these tensors (addresses only: the caller keeps the tensors)."""
        p, b = _gsr._ptr, binding
        return _gsr.SugarArap(T=int(vert_xyz.shape[0]), V=b.n_verts, E=b.n_edges, rot_form=form, verts=p(b.verts),
                              w=p(b.w), vert_xyz=p(vert_xyz), vert_rot=p(vert_rot), offsets=p(b.offsets), nbr=p(b.nbr))

    @staticmethod
    def forward(ctx, vert_xyz, vert_rot, binding, form):
        dev = vert_xyz.device
        lib = _gsr.load_library()
        T, V = int(vert_xyz.shape[0]), binding.n_verts
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(vert_xyz, vert_rot)
        ctx.binding, ctx.form = binding, form
        energy = torch.zeros((T,), dtype=torch.float32, device=dev)
        if T > 0 and V > 0:
            nbytes = int(lib.gsr_sugar_arap_workspace_bytes(T, V))
            ws = workspace(nbytes, dev)
            _gsr._check(lib.gsr_sugar_arap_forward(_ArapEnergy._in(vert_xyz, vert_rot, binding, form),
                                                   _gsr._ptr(energy), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return energy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_energy):
        vert_xyz, vert_rot = ctx.saved_tensors
        dev = vert_xyz.device
        T, V = int(vert_xyz.shape[0]), ctx.binding.n_verts
        if T == 0 or V == 0 or g_energy is None:
            return torch.zeros_like(vert_xyz), torch.zeros_like(vert_rot), None, None
        lib = _gsr.load_library()
        (g,) = ups((g_energy,), dev)
        dxyz, drot = torch.empty_like(vert_xyz), torch.empty_like(vert_rot)
        _gsr._check(lib.gsr_sugar_arap_backward(_ArapEnergy._in(vert_xyz, vert_rot, ctx.binding, ctx.form),
                                                _gsr._ptr(g), _gsr._ptr(dxyz), _gsr._ptr(drot), _gsr._stream(dev)))
        return dxyz, drot, None, None


def arap_energy(vert_xyz, vert_rot, binding):
    """The ARAP energy of each of T deformed frames against the rest mesh, ``(T,)`` float32: what
    ``ARAPCoach.compute_arap_energy(xyz_prime=vert_xyz[t], vert_rotations=R[t])`` returns for t = 0 .. T-1 (the caller
    sums, as the reference's loop does).

    vert_xyz (T, V, 3) and vert_rot, float32 on the GPU: (T, V, 4) pypose (x, y, z, w) quaternions of any norm, e.g.
    ``skin_vertices``' ``vert_rot`` (R = I + 2 w [v]x + 2 [v]x^2, pypose's ``.matrix()``, no normalisation), or
    (T, V, 3, 3) matrices (``get_timed_vertex_rotation(return_matrix=True)``).  binding: the rest mesh's
    ``ArapBinding``.  E_t = sum_i sum_{j in N(i)} w_ij |(x'_i - x'_j) - R_i (x_i - x_j)|^2 over the directed one-ring
    edges (the formulas: include/gsr.h).  Gradients flow to vert_xyz and vert_rot (in the form given), bitwise
    reproducible; none to the rest mesh; no double backward.  vert_xyz equal to the rest vertices with identity
    rotations gives exactly 0.
    """
    if not isinstance(binding, ArapBinding):
        raise ValueError("binding must be an ArapBinding")
    V = binding.n_verts
    vert_xyz = float_tensor(vert_xyz, "vert_xyz", (None, V, 3))
    T = int(vert_xyz.shape[0])
    if isinstance(vert_rot, torch.Tensor) and vert_rot.dim() == 4:
        vert_rot = float_tensor(vert_rot, "vert_rot", (T, V, 3, 3))
        form = ARAP_ROT_FORMS["matrix"]
    else:
        try:
            vert_rot = float_tensor(vert_rot, "vert_rot", (T, V, 4))
        except ValueError as e:
            raise ValueError(f"{e} (quaternions) or (T, V, 3, 3) (matrices)") from None
        form = ARAP_ROT_FORMS["quat"]
    if T * V >= 2 ** 31:
        raise ValueError("the batch is too large: T x V must stay below 2^31")
    on_gpu("arap_energy", vert_xyz, (("vert_rot", vert_rot), ("the binding", binding.nbr)))
    return _ArapEnergy.apply(vert_xyz.contiguous(), aligned(vert_rot), binding, form)
