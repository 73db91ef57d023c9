"""The two mesh regularisers of the SuGaR surface over the C ABI (include/gsr.h gsr_sugar_normal_consistency_* and
gsr_sugar_laplacian_*, csrc/gsr_meshreg.hip).

The reference's SuGaR systems put ``pytorch3d.loss.mesh_normal_consistency(surface_meshes)`` and
``mesh_laplacian_smoothing(surface_meshes, "uniform")`` on the deformed surface every step
(system/sugar_static.py:286-297, system/sugar_4dgen.py:234-250), on a ``Meshes`` that ``surface_mesh`` /
``get_timed_surface_mesh`` rebuild every step (geometry/sugar.py:588-596, geometry/dynamic_sugar.py:312-327): the
unique edges (a sort over 3 F edges per frame), a second sort and a ``bincount``, the face-pair enumeration, a sparse
(V, V) Laplacian, and backwards that scatter atomically, all on a topology that never changes.  Here the topology is
derived once and each loss is one fused call for all T frames of a batch:

    topo = MeshTopology(faces, n_verts)                        # once per mesh
    nc = normal_consistency(vert_xyz, topo)                    # (T,)
    lap = laplacian_smoothing(vert_xyz, topo)                  # (T,)
    # mesh_normal_consistency(meshes) == nc.mean();  mesh_laplacian_smoothing(meshes, "uniform") == lap.mean()

whose backwards recompute from the inputs and only gather (no atomics: two calls give the same bits).  ``vert_xyz`` is
``sugar_dynamic.skin_vertices``' (T, V, 3) output, as ``sugar_arap.arap_energy`` takes it; the static stage passes
``_points[None]``.  GPU only, like ``sugar_arap``.

pytorch3d is a third-party package that is not part of the reference's tree: both losses are written from its
published algorithm, and the rule for a vertex in no face (below) could not be confirmed by running it.
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import _C as _gsr
from sugar_common import INT_DTYPES, Binding, float_tensor, incidence, on_gpu, row_offsets, ups, workspace

__all__ = ["MeshTopology", "normal_consistency", "laplacian_smoothing"]


class MeshTopology(Binding):
    """What the two losses need of a triangle mesh's connectivity, built once, in plain torch.

    faces (F, 3) of any integer dtype, every entry in [0, n_verts), no face with a repeated vertex: checked here, one
    host synchronisation.  Duplicated faces and edges in more than two faces are legal (unlike ``ArapBinding``).
    Attributes, all int32:
    ``edges`` (E, 2): the unique undirected edges (a, b), a < b, in lexicographic order (``Meshes.edges_packed()`` of
    one mesh);
    ``pairs`` (P, 4) = (a, b, c0, c1): for every edge every unordered pair of faces incident to it, c the face's third
    vertex; ordered by edge, then by (lower face index, higher face index).  A boundary edge has no pair, a manifold
    edge one, an edge in k faces k (k - 1) / 2;
    ``slot_offsets`` (V + 1,), ``slots`` (4 P,): per vertex the entries ``4 * pair + role`` (role 0..3 = a, b, c0, c1)
    at which it occurs in ``pairs``, ascending within a row;
    ``ring_offsets`` (V + 1,), ``ring`` (2 E,): per vertex its distinct neighbours j, ascending (a vertex in no face
    has an empty row);
    and the sizes ``n_verts``, ``n_faces``, ``n_edges``, ``n_pairs``, ``max_valence``, ``max_slots``.  Works on CPU
    tensors too; ``to(device)`` moves it.
    """

    _TENSORS = ("pairs", "edges", "slot_offsets", "slots", "ring_offsets", "ring")

    def __init__(self, faces, n_verts):
        if not isinstance(faces, torch.Tensor) or faces.dtype not in INT_DTYPES:
            raise ValueError("faces must be an integer tensor")
        if faces.dim() != 2 or int(faces.shape[1]) != 3:
            raise ValueError(f"faces must have shape (F, 3), got {tuple(faces.shape)}")
        V, F = int(n_verts), int(faces.shape[0])
        if V < 0:
            raise ValueError("n_verts must not be negative")
        if V >= 2 ** 31 or 6 * F >= 2 ** 31:
            raise ValueError("the mesh is too large: V and the 6 F directed edges must stay below 2^31")
        faces = faces.to(torch.int64)
        dev = faces.device
        if F > 0 and (int(faces.min()) < 0 or int(faces.max()) >= V):
            raise ValueError(f"faces has entries outside [0, {V})")
        if F > 0 and bool(((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) |
                           (faces[:, 2] == faces[:, 0])).any()):
            raise ValueError("a face repeats a vertex")
        # the 3 F half-edges (item 3 f + c: the edge that leaves corner c), as sorted keys a V + b with a < b
        v0, v1 = faces.flatten(), faces[:, [1, 2, 0]].flatten()
        lo, hi = torch.minimum(v0, v1), torch.maximum(v0, v1)
        third = faces.sum(1, keepdim=True).expand(F, 3).flatten() - lo - hi
        key, order = torch.sort(lo * V + hi, stable=True)  # (within an edge: ascending face index)
        third = third[order]
        ukey, count = torch.unique_consecutive(key, return_counts=True)
        ea, eb = ukey // max(V, 1), ukey % max(V, 1)
        E = int(ukey.numel())
        # every item pairs, as the lower face, with the items after it in its edge's group
        start = torch.cumsum(count, 0) - count
        rank = torch.arange(3 * F, device=dev) - torch.repeat_interleave(start, count)
        after = torch.repeat_interleave(count, count) - 1 - rank
        P = int(after.sum())
        if 4 * P >= 2 ** 31:
            raise ValueError("the mesh is too large: the 4 P pair slots must stay below 2^31")
        lower = torch.repeat_interleave(torch.arange(3 * F, device=dev), after)
        first = torch.cumsum(after, 0) - after
        upper = lower + 1 + torch.arange(P, device=dev) - first[lower]
        pairs = torch.stack([key[lower] // max(V, 1), key[lower] % max(V, 1), third[lower], third[upper]], 1)
        self.edges = torch.stack([ea, eb], 1).to(torch.int32).contiguous()
        self.pairs = pairs.to(torch.int32).contiguous()
        self.slots, self.slot_offsets = incidence(pairs.flatten(), V)
        # the one-rings: both directions of every edge, i ascending and j ascending within i
        directed = torch.sort(torch.cat([ukey, eb * V + ea]))[0]
        ii, jj = directed // max(V, 1), directed % max(V, 1)
        valence = torch.bincount(ii, minlength=V)
        self.ring_offsets = row_offsets(valence)
        self.ring = jj.to(torch.int32).contiguous()
        self.n_verts, self.n_faces, self.n_edges, self.n_pairs = V, F, E, P
        self.max_valence = int(valence.max()) if V > 0 else 0
        self.max_slots = int((self.slot_offsets[1:] - self.slot_offsets[:-1]).max()) if V > 0 else 0


def _in(vert_xyz, topo):
    """The gsr_sugar_meshreg of these tensors (addresses only: the caller keeps the tensors)."""
    p = _gsr._ptr
    return _gsr.SugarMeshReg(T=int(vert_xyz.shape[0]), V=topo.n_verts, E=topo.n_edges, P=topo.n_pairs,
                             vert_xyz=p(vert_xyz), pairs=p(topo.pairs), slot_offsets=p(topo.slot_offsets),
                             slots=p(topo.slots), ring_offsets=p(topo.ring_offsets), ring=p(topo.ring))


def _forward(entry, count, ctx, vert_xyz, topo):
    """vert_xyz -> loss (T,); `count` is what the loss averages over (nothing to launch at 0)."""
    dev = vert_xyz.device
    lib = _gsr.load_library()
    T = int(vert_xyz.shape[0])
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(vert_xyz)
    ctx.topo = topo
    out = torch.zeros((T,), dtype=torch.float32, device=dev)
    if T > 0 and count > 0:
        nbytes = int(lib.gsr_sugar_meshreg_workspace_bytes(T, topo.n_verts, topo.n_pairs, 0))
        ws = workspace(nbytes, dev)
        _gsr._check(getattr(lib, entry + "_forward")(_in(vert_xyz, topo), _gsr._ptr(out), _gsr._ptr(ws), nbytes,
                                                     _gsr._stream(dev)))
    return out


def _backward(entry, count, ws_pass, ctx, g_out):
    (vert_xyz,) = ctx.saved_tensors
    dev, topo = vert_xyz.device, ctx.topo
    T = int(vert_xyz.shape[0])
    if T == 0 or topo.n_verts == 0 or count == 0 or g_out is None:
        return torch.zeros_like(vert_xyz), None
    lib = _gsr.load_library()
    (g,) = ups((g_out,), dev)
    dxyz = torch.empty_like(vert_xyz)
    nbytes = int(lib.gsr_sugar_meshreg_workspace_bytes(T, topo.n_verts, topo.n_pairs, ws_pass))
    ws = workspace(nbytes, dev)
    _gsr._check(getattr(lib, entry + "_backward")(_in(vert_xyz, topo), _gsr._ptr(g), _gsr._ptr(dxyz), _gsr._ptr(ws),
                                                  nbytes, _gsr._stream(dev)))
    return dxyz, None


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vert_xyz, topo):
        return _forward("gsr_sugar_normal_consistency", topo.n_pairs, ctx, vert_xyz, topo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_nc):
        return _backward("gsr_sugar_normal_consistency", ctx.topo.n_pairs, 1, ctx, g_nc)  # GSR_MESHREG_NC_BACKWARD


class _Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vert_xyz, topo):
        return _forward("gsr_sugar_laplacian", topo.n_verts, ctx, vert_xyz, topo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lap):
        return _backward("gsr_sugar_laplacian", ctx.topo.n_verts, 2, ctx, g_lap)  # GSR_MESHREG_LAP_BACKWARD


def _checked(fn, vert_xyz, topo):
    if not isinstance(topo, MeshTopology):
        raise ValueError("topo must be a MeshTopology")
    vert_xyz = float_tensor(vert_xyz, "vert_xyz", (None, topo.n_verts, 3))
    if int(vert_xyz.shape[0]) * topo.n_verts >= 2 ** 31:
        raise ValueError("the batch is too large: T x V must stay below 2^31")
    on_gpu(fn, vert_xyz, (("the topology", topo.pairs),))
    return vert_xyz.contiguous()


def normal_consistency(vert_xyz, topo):
    """The normal consistency of each of T frames of one mesh, ``(T,)`` float32; its ``.mean()`` is
    ``mesh_normal_consistency`` of the T meshes.

    vert_xyz (T, V, 3) float32 on the GPU; topo: the mesh's ``MeshTopology``.  Per pair (a, b, c0, c1) of ``topo.pairs``
    n0 = (x_b - x_a) x (x_c0 - x_a), n1 = -(x_b - x_a) x (x_c1 - x_a), cos = n0 . n1 / (max(|n0|, 1e-8) max(|n1|,
    1e-8)) (``F.cosine_similarity``: each norm clamped on its own; as torch clamps the norm's value outside autograd,
    the norm's gradient n / |n| flows under the clamp too, 0 at n = 0), and nc_t = (1 / P) sum_p (1 - cos_p), 0 when
    P = 0.  The winding of the faces is not used, only the sorted edge (pytorch3d's
    convention): on a consistently wound mesh n0 and n1 are the two face normals.  fp64 arithmetic, one rounding per
    result.  Gradients flow to vert_xyz only, bitwise reproducible; a vertex in no pair gets exactly +0.0; no double
    backward.
    """
    return _NormalConsistency.apply(_checked("normal_consistency", vert_xyz, topo), topo)


def laplacian_smoothing(vert_xyz, topo):
    """The uniform Laplacian smoothing loss of each of T frames of one mesh, ``(T,)`` float32; its ``.mean()`` is
    ``mesh_laplacian_smoothing(meshes, "uniform")`` of the T meshes.

    d_i = (1 / deg_i) sum_{j in ring(i)} x_j - x_i with deg_i the number of distinct neighbours, and lap_t = (1 / V)
    sum_i |d_i|, 0 when V = 0; the gradient of |d_i| at d_i = 0 is 0 (torch's ``norm``).  A vertex in no face has deg 0
    and d_i = -x_i, so it adds |x_i|: pytorch3d subtracts the identity for every packed vertex.  That rule is stated
    from pytorch3d's published algorithm and was not confirmed by running it (it is not installed where this was
    written).  Arguments, precision and gradients as ``normal_consistency``.
    """
    return _Laplacian.apply(_checked("laplacian_smoothing", vert_xyz, topo), topo)
