"""The time-batched geometry of dynamic SuGaR over the C ABI (include/gsr.h gsr_sugar_skin_*, gsr_sugar_timed_*,
csrc/gsr_dynamic.hip).

Every 4-D training step of the reference (system/sugar_4dgen.py with geometry/dynamic_sugar.py) first deforms the mesh
vertices with a deformation graph (``_get_timed_vertex_attributes_from_dg``: dual-quaternion skinning by default,
dynamic_sugar.py:505-575) and then rebuilds every Gaussian from the deformed vertices (``get_timed_gs_attributes``,
``fuse_rotations``, ``get_timed_gs_normals``, :329-346, :618-688): a (T, V, K, 4) gather of node quaternions, pypose's
``Log`` and ``Exp``, a dual-quaternion product, a (T, N, 3, 4) gather of vertex quaternions, a pytorch3d ``Meshes``
built for its face normals, with every intermediate kept by autograd and ``index_put`` scatters in its backward.  Here
the two stages are two fused calls for all T frames of a batch:

    vert_xyz, vert_rot, vert_scale = skin_vertices(verts, node_xyz, node_trans, node_rots, skin_binding, "dqs")
    xyz, rotation, normals, scaling = timed_gaussians(vert_xyz, vert_rot, rotation0, mesh_binding, ...)

whose backward recomputes from the inputs and adds in a fixed order (no atomics: two calls give the same bits).
``SkinBinding`` is built once per deformation graph, as ``sugar_mesh.MeshBinding`` is per mesh.  pypose quaternions
are (x, y, z, w): ``node_rots`` and ``vert_rot``; ``rotation0`` and ``rotation`` are this library's (w, x, y, z).
GPU only, like ``sugar_mesh.bound_gaussians``.
"""
from __future__ import annotations

import ctypes

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import INT_DTYPES, Binding, aligned, float_tensor, incidence, on_gpu, ups, workspace
from sugar_mesh import MeshBinding

__all__ = ["SkinBinding", "skin_vertices", "timed_gaussians", "SKIN_MAX_K", "SKIN_METHODS"]

SKIN_MAX_K = 32  # include/gsr.h GSR_SKIN_MAX_K
SKIN_METHODS = {"dqs": 0, "lbs": 1}  # GSR_SKIN_DQS, GSR_SKIN_LBS

class SkinBinding(Binding):
    """What ``skin_vertices`` needs of a deformation graph besides the node positions, built once.

    nbr (V, K), any integer dtype, 1 <= K <= 32, every entry in [0, n_nodes) (checked here: one host
    synchronisation): the nodes of each vertex (``_xyz_neighbor_node_idx``); weights (V, K) floating point
    (``_xyz_neighbor_nodes_weights``).  Attributes: ``nbr`` (V, K) int32; ``w`` (V, K) float32; ``item_order``
    (V K,) int32, the items v K + k grouped by node, ascending within a node (a stable sort of ``nbr.reshape(-1)``);
    ``node_offsets`` (P + 1,) int32, node j owning ``item_order[node_offsets[j]:node_offsets[j + 1]]``; ``n_verts``,
    ``n_nodes``, ``n_neighbors``.  Works on CPU tensors too; ``to(device)`` moves it.
    """

    _TENSORS = ("nbr", "w", "item_order", "node_offsets")

    def __init__(self, nbr, weights, n_nodes):
        if not isinstance(nbr, torch.Tensor) or nbr.dtype not in INT_DTYPES:
            raise ValueError("nbr must be an integer tensor")
        if nbr.dim() != 2 or not 1 <= int(nbr.shape[1]) <= SKIN_MAX_K:
            raise ValueError(f"nbr must have shape (V, K) with 1 <= K <= {SKIN_MAX_K}, got {tuple(nbr.shape)}")
        if not isinstance(weights, torch.Tensor) or not weights.is_floating_point():
            raise ValueError("weights must be a floating-point tensor")
        if weights.shape != nbr.shape:
            raise ValueError(f"weights must have nbr's shape {tuple(nbr.shape)}, got {tuple(weights.shape)}")
        if weights.device != nbr.device:
            raise ValueError(f"weights is on {weights.device}, nbr on {nbr.device}")
        if isinstance(n_nodes, bool) or not isinstance(n_nodes, int) or n_nodes < 0:
            raise ValueError("n_nodes must be a non-negative integer")
        V, K = int(nbr.shape[0]), int(nbr.shape[1])
        if V * K >= 2 ** 31 or n_nodes >= 2 ** 31:
            raise ValueError("the binding is too large: V x K and n_nodes must stay below 2^31")
        flat = nbr.reshape(-1).to(torch.int64)
        if V > 0 and (int(flat.min()) < 0 or int(flat.max()) >= n_nodes):
            raise ValueError(f"nbr has entries outside [0, {n_nodes})")
        self.nbr = nbr.to(torch.int32).contiguous()
        self.w = weights.detach().to(torch.float32).contiguous()
        self.item_order, self.node_offsets = incidence(flat, n_nodes)
        self.n_verts, self.n_nodes, self.n_neighbors = V, n_nodes, K

    @classmethod
    def from_euclidean(cls, verts, node_xyz, K, chunk=16384):
        """``build_deformation_graph(mode="eucdisc")`` (dynamic_sugar.py:719-730, 787-799): the K nearest nodes of
        each vertex, nearest first, and weight = distance / sum of the K distances (the square root of the squared
        distance, normalised, as the reference has it).  Init only, plain chunked torch (CPU or GPU)."""
        for name, t in (("verts", verts), ("node_xyz", node_xyz)):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.dim() != 2 or int(t.shape[1]) != 3:
                raise ValueError(f"{name} must be a floating-point tensor of shape (*, 3)")
        P = int(node_xyz.shape[0])
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= min(SKIN_MAX_K, P):
            raise ValueError(f"K must be an integer in 1..min({SKIN_MAX_K}, the number of nodes), got {K!r}")
        verts, node_xyz = verts.detach(), node_xyz.detach().to(verts.device)
        nbr, dist = [], []
        for s in range(0, int(verts.shape[0]), chunk):
            d2 = (verts[s:s + chunk, None, :] - node_xyz[None, :, :]).pow(2).sum(-1)
            val, idx = torch.topk(d2, K, dim=1, largest=False, sorted=True)
            nbr.append(idx)
            dist.append(val.sqrt())
        if not nbr:
            nbr, dist = [torch.zeros((0, K), dtype=torch.int64)], [torch.zeros((0, K), dtype=verts.dtype)]
        nbr, dist = torch.cat(nbr), torch.cat(dist)
        return cls(nbr, dist / dist.sum(dim=-1, keepdim=True), P)


def _skin_in(verts, node_trans, node_rots, node_scales, node_xyz, binding, method):
    """The gsr_sugar_skin of these tensors (addresses only: the caller keeps the tensors)."""
    p, b = _gsr._ptr, binding
    return _gsr.SugarSkin(T=int(node_trans.shape[0]), V=b.n_verts, P=b.n_nodes, K=b.n_neighbors, method=method,
                          verts=p(verts), node_xyz=p(node_xyz), node_trans=p(node_trans), node_rots=p(node_rots),
                          node_scales=p(node_scales), nbr=p(b.nbr), w=p(b.w))


def _timed_in(vert_xyz, vert_rot, rotation0, vert_scale, log_scales, binding, thickness):
    """The gsr_sugar_timed of these tensors (addresses only: the caller keeps the tensors)."""
    p, b = _gsr._ptr, binding
    return _gsr.SugarTimed(T=int(vert_xyz.shape[0]), V=b.n_verts, F=b.n_faces, G=b.n_per_face, vert_xyz=p(vert_xyz),
                           vert_rot=p(vert_rot), rotation0=p(rotation0), vert_scale=p(vert_scale),
                           log_scales=p(log_scales), faces=p(b.faces), thickness=thickness)


class _SkinVertices(torch.autograd.Function):
    """(verts, node_trans, node_rots, node_scales) -> (vert_xyz, vert_rot, vert_scale)."""

    @staticmethod
    def forward(ctx, verts, node_trans, node_rots, node_scales, node_xyz, binding, method):
        dev = verts.device
        lib = _gsr.load_library()
        T, P, V = int(node_trans.shape[0]), binding.n_nodes, binding.n_verts
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(verts, node_trans, node_rots, node_scales, node_xyz)
        ctx.binding, ctx.method = binding, method
        fopt = dict(dtype=torch.float32, device=dev)
        xyz, rot = torch.empty((T, V, 3), **fopt), torch.empty((T, V, 4), **fopt)
        scale = None if node_scales is None else torch.empty((T, V, 3), **fopt)
        if T > 0 and V > 0:
            nbytes = int(lib.gsr_sugar_skin_workspace_bytes(T, V, P))
            ws = workspace(nbytes, dev)
            _gsr._check(lib.gsr_sugar_skin_forward(
                _skin_in(verts, node_trans, node_rots, node_scales, node_xyz, binding, method), _gsr._ptr(xyz),
                _gsr._ptr(rot), _gsr._ptr(scale), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return xyz, rot, scale

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_rot, g_scale):
        verts, node_trans, node_rots, node_scales, node_xyz = ctx.saved_tensors
        binding, method = ctx.binding, ctx.method
        dev = verts.device
        T, P, V = int(node_trans.shape[0]), binding.n_nodes, binding.n_verts
        if node_scales is None:
            g_scale = None
        zeros = [torch.zeros_like(t) if t is not None else None for t in (verts, node_trans, node_rots, node_scales)]
        if T == 0 or V == 0 or all(g is None for g in (g_xyz, g_rot, g_scale)):
            return (*zeros, None, None, None)
        lib = _gsr.load_library()
        g_ups = ups((g_xyz, g_rot, g_scale), dev)
        grads = [torch.empty_like(t) if t is not None else None for t in (verts, node_trans, node_rots, node_scales)]
        nbytes = int(lib.gsr_sugar_skin_workspace_bytes(T, V, P))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_skin_backward(
            _skin_in(verts, node_trans, node_rots, node_scales, node_xyz, binding, method),
            _gsr._ptr(binding.item_order), _gsr._ptr(binding.node_offsets), *(_gsr._ptr(g) for g in g_ups),
            *(_gsr._ptr(g) for g in grads), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return (*grads, None, None, None)


def skin_vertices(verts, node_xyz, node_trans, node_rots, binding, method="dqs", node_scales=None):
    """The deformation-graph skinning of ``DynamicSuGaRModel._get_timed_vertex_attributes_from_dg`` for all T frames:
    ``(vert_xyz (T, V, 3), vert_rot (T, V, 4), vert_scale (T, V, 3) or None)``.

    verts (V, 3) = ``get_xyz_verts``; node_xyz (P, 3) = ``_deform_graph_node_xyz``; node_trans (T, P, 3) and
    node_rots (T, P, 4), (x, y, z, w) of any non-zero norm, the nodes' timed attributes; node_scales (T, P, 3) or
    None (``d_scale``); all float32 on the GPU.  binding: the graph's ``SkinBinding``; method "dqs" (dual-quaternion
    skinning, without an antipodal sign fix, as the reference) or "lbs" (``cfg.skinning_method``).  vert_rot =
    Exp(sum_k w_k Log(q_k)) is a unit (x, y, z, w) quaternion with w >= 0 (the formulas: include/gsr.h).  Gradients
    flow to verts, node_trans, node_rots (through the normalisation) and node_scales, bitwise reproducible; no
    double backward.
    """
    if not isinstance(binding, SkinBinding):
        raise ValueError("binding must be a SkinBinding")
    if method not in SKIN_METHODS:
        raise ValueError(f"method must be 'dqs' or 'lbs', got {method!r}")
    V, P = binding.n_verts, binding.n_nodes
    verts = float_tensor(verts, "verts", (V, 3))
    node_xyz = float_tensor(node_xyz, "node_xyz", (P, 3))
    node_trans = float_tensor(node_trans, "node_trans", (None, P, 3))
    T = int(node_trans.shape[0])
    node_rots = float_tensor(node_rots, "node_rots", (T, P, 4))
    if node_scales is not None:
        node_scales = float_tensor(node_scales, "node_scales", (T, P, 3))
    if T * max(V, P) >= 2 ** 31:
        raise ValueError("the batch is too large: T x V and T x P must stay below 2^31")
    if V > 0 and P == 0:
        raise ValueError("vertices without nodes")
    dev = on_gpu("skin_vertices", verts, (("node_xyz", node_xyz), ("node_trans", node_trans),
                                          ("node_rots", node_rots), ("node_scales", node_scales),
                                          ("the binding", binding.nbr)))
    out = _SkinVertices.apply(verts.contiguous(), node_trans.contiguous(), aligned(node_rots),
                              None if node_scales is None else node_scales.contiguous(),
                              node_xyz.detach().contiguous(), binding, SKIN_METHODS[method])
    return out[0], out[1], out[2]


class _TimedGaussians(torch.autograd.Function):
    """(vert_xyz, vert_rot, rotation0, vert_scale, log_scales) -> (xyz, rotation, normals, scaling)."""

    @staticmethod
    def forward(ctx, vert_xyz, vert_rot, rotation0, vert_scale, log_scales, binding, thickness):
        dev = vert_xyz.device
        lib = _gsr.load_library()
        T = int(vert_xyz.shape[0])
        F, N = binding.n_faces, binding.n_gaussians
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(vert_xyz, vert_rot, rotation0, vert_scale, log_scales)
        ctx.binding, ctx.thickness = binding, thickness
        fopt = dict(dtype=torch.float32, device=dev)
        xyz, normals = torch.empty((T, N, 3), **fopt), torch.empty((T, N, 3), **fopt)
        rotation = torch.empty((T, N, 4), **fopt)
        scaling = None if vert_scale is None else torch.empty((T, N, 3), **fopt)
        if T > 0 and F > 0:
            _gsr._check(lib.gsr_sugar_timed_forward(
                _timed_in(vert_xyz, vert_rot, rotation0, vert_scale, log_scales, binding, thickness), N,
                ctypes.c_void_p(binding.bary.data_ptr()), _gsr._ptr(xyz), _gsr._ptr(rotation), _gsr._ptr(normals),
                _gsr._ptr(scaling), _gsr._stream(dev)))
        return xyz, rotation, normals, scaling

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_xyz, g_rotation, g_normals, g_scaling):
        vert_xyz, vert_rot, rotation0, vert_scale, log_scales = ctx.saved_tensors
        binding = ctx.binding
        dev = vert_xyz.device
        T = int(vert_xyz.shape[0])
        F, N = binding.n_faces, binding.n_gaussians
        if vert_scale is None:
            g_scaling = None
        inputs = (vert_xyz, vert_rot, rotation0, vert_scale, log_scales)
        if T == 0 or F == 0 or all(g is None for g in (g_xyz, g_rotation, g_normals, g_scaling)):
            return (*(torch.zeros_like(t) if t is not None else None for t in inputs), None, None)
        lib = _gsr.load_library()
        g_ups = ups((g_xyz, g_rotation, g_normals, g_scaling), dev)
        grads = [torch.empty_like(t) if t is not None else None for t in inputs]
        nbytes = int(lib.gsr_sugar_timed_workspace_bytes(T, F))
        ws = workspace(nbytes, dev)
        _gsr._check(lib.gsr_sugar_timed_backward(
            _timed_in(*inputs, binding, ctx.thickness), N, ctypes.c_void_p(binding.bary.data_ptr()),
            _gsr._ptr(binding.corner_order), _gsr._ptr(binding.vert_offsets), *(_gsr._ptr(g) for g in g_ups),
            *(_gsr._ptr(g) for g in grads), _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
        return (*grads, None, None)


def timed_gaussians(vert_xyz, vert_rot, rotation0, binding, vert_scale=None, log_scales=None, thickness=None):
    """The Gaussians of the deformed mesh for all T frames: ``(xyz (T, N, 3), rotation (T, N, 4), normals (T, N, 3),
    scaling (T, N, 3) or None)`` = ``DynamicSuGaRModel.get_timed_gs_attributes``' "xyz", "rotation" and "scale" and
    ``get_timed_gs_normals``, N = F G.

    vert_xyz (T, V, 3) and vert_rot (T, V, 4) (x, y, z, w), e.g. of ``skin_vertices``; rotation0 (N, 4) (w, x, y, z)
    = the static ``get_rotation``; binding: the mesh's ``sugar_mesh.MeshBinding``; vert_scale (T, V, 3), log_scales
    (N, 2) = ``_scales`` and thickness = ``surface_mesh_thickness``: all three (``d_scale``) or none.  Gaussian
    f G + g lies at sum_c bary[g, c] vert_xyz[t, faces[f, c]], is turned by Exp(sum_c bary[g, c] Log(vert_rot)) from
    rotation0 (unit, (w, x, y, z)), has the deformed face's unit normal (the zero vector for a degenerate face) and
    scales (thickness, exp(log_scales + bary-mixed vert_scale[..., 1:])).  Gradients flow to vert_xyz, vert_rot,
    rotation0, vert_scale and log_scales, bitwise reproducible; no double backward.
    """
    if not isinstance(binding, MeshBinding):
        raise ValueError("binding must be a MeshBinding")
    V, N = binding.n_verts, binding.n_gaussians
    vert_xyz = float_tensor(vert_xyz, "vert_xyz", (None, V, 3))
    T = int(vert_xyz.shape[0])
    vert_rot = float_tensor(vert_rot, "vert_rot", (T, V, 4))
    given = [x is not None for x in (vert_scale, log_scales, thickness)]
    if any(given) and not all(given):
        raise ValueError("vert_scale, log_scales and thickness are given together or not at all")
    try:
        rotation0 = float_tensor(rotation0, "rotation0", (N, 4))
        if all(given):
            log_scales = float_tensor(log_scales, "log_scales", (N, 2))
    except ValueError as e:
        raise ValueError(f"{e} (N = F x G = {binding.n_faces} x {binding.n_per_face})") from None
    if all(given):
        vert_scale = float_tensor(vert_scale, "vert_scale", (T, V, 3))
        try:
            thickness = float(thickness)
        except (TypeError, ValueError):
            raise ValueError("thickness must be a number") from None
    else:
        thickness = 0.0
    if T * max(V, N) >= 2 ** 31:
        raise ValueError("the batch is too large: T x N and T x V must stay below 2^31")
    on_gpu("timed_gaussians", vert_xyz, (("vert_rot", vert_rot), ("rotation0", rotation0),
                                         ("vert_scale", vert_scale), ("log_scales", log_scales),
                                         ("the binding", binding.faces)))
    out = _TimedGaussians.apply(vert_xyz.contiguous(), aligned(vert_rot), aligned(rotation0),
                                None if vert_scale is None else vert_scale.contiguous(),
                                None if log_scales is None else aligned(log_scales), binding, thickness)
    return out[0], out[1], out[2], out[3]
