"""Torch restatements of pytorch3d's ``mesh_normal_consistency`` and ``mesh_laplacian_smoothing(., "uniform")`` for T
frames of one topology (include/gsr.h gsr_sugar_normal_consistency_* / gsr_sugar_laplacian_*), differentiated by
autograd: the checker of tests/test_sugar_meshreg.py and tests/test_gpu_sugar_meshreg.py.

pytorch3d is not part of the reference's tree and is not installed, so there is no fixture made by its code: the
restatements are written from its published algorithm (they call ``F.cosine_similarity`` and ``torch.norm`` themselves,
so the edge cases at the eps clamp and at a zero vector are torch's), in the dtype of their inputs (float64: the
reference; float32: the "fp32 null" the GPU bars are calibrated on), and tests/test_sugar_meshreg.py pins them to
``brute_force`` below, the same definitions written differently (Python loops over a dict edge -> incident faces, numpy
float64), and to closed forms.  ``topology`` derives the edges and face pairs its own way (pytorch3d's: a sort by edge
index and the combinations of each edge's faces), not ``MeshTopology``'s."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from sugar_cases import check_against_null, mesh

OUT_FLOOR = 2.0 ** -23


def topology(faces, V):
    """(edges (E, 2), pairs (P, 4)) int64 of faces (F, 3): the unique sorted edges in lexicographic order, and per edge
    every combination of two of its faces (in face order) as (a, b, c0, c1)."""
    faces = faces.long()
    n_faces = len(faces)
    if n_faces == 0:
        return torch.zeros((0, 2), dtype=torch.long), torch.zeros((0, 4), dtype=torch.long)
    e = torch.cat([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]])  # edge k of face f at row k F + f
    opposite = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2]])
    e = torch.sort(e, dim=1)[0]
    ukey, edge_of = torch.unique(e[:, 0] * V + e[:, 1], return_inverse=True)
    edges = torch.stack([ukey // V, ukey % V], 1)
    face_of = torch.arange(n_faces).repeat(3)
    order = np.lexsort((face_of.numpy(), edge_of.numpy()))  # by edge, then by face
    count = torch.bincount(edge_of, minlength=len(edges)).tolist()
    rows, at = [], 0
    for k, n in enumerate(count):
        a, b = edges[k].tolist()
        for i, j in itertools.combinations(range(at, at + n), 2):
            rows.append((a, b, int(opposite[order[i]]), int(opposite[order[j]])))
        at += n
    return edges, torch.tensor(rows, dtype=torch.long).reshape(-1, 4)


def normal_consistency_reference(vert_xyz, pairs):
    """(T,): per frame the mean over the pairs of 1 - cos(n0, n1); zeros without pairs."""
    T = vert_xyz.shape[0]
    if len(pairs) == 0:
        return vert_xyz.new_zeros(T) + 0 * vert_xyz.sum((1, 2))
    a, b, c0, c1 = pairs.long().unbind(1)
    v0, v1 = vert_xyz[:, a], vert_xyz[:, b]
    n0 = torch.cross(v1 - v0, vert_xyz[:, c0] - v0, dim=-1)
    n1 = -torch.cross(v1 - v0, vert_xyz[:, c1] - v0, dim=-1)
    return (1 - F.cosine_similarity(n0, n1, dim=-1)).sum(-1) / len(pairs)


def laplacian_reference(vert_xyz, edges):
    """(T,): per frame the mean over the vertices of |L x|, L = A / deg - I over every vertex (a vertex without an edge
    keeps the -I row)."""
    T, V = vert_xyz.shape[:2]
    if V == 0:
        return vert_xyz.new_zeros(T)
    e0, e1 = edges.long().unbind(1)
    deg = torch.bincount(torch.cat([e0, e1]), minlength=V).to(vert_xyz.dtype)
    inv = torch.where(deg > 0, 1 / deg, deg)
    ii, jj = torch.cat([e0, e1]), torch.cat([e1, e0])
    lx = torch.zeros_like(vert_xyz).index_add(1, ii, inv[ii][None, :, None] * vert_xyz[:, jj]) - vert_xyz
    return torch.norm(lx, dim=-1).sum(-1) / V


def evaluate(dtype, vert_xyz, edges, pairs, ups):
    """{"nc", "lap", "dvert_xyz"} in `dtype`; ups: the (T,) upstream gradients by output name, those present."""
    x = vert_xyz.detach().to(dtype).clone().requires_grad_()
    out = {"nc": normal_consistency_reference(x, pairs), "lap": laplacian_reference(x, edges)}
    loss = sum((out[k] * ups[k].to(dtype)).sum() for k in ups)
    g = torch.autograd.grad(loss, x, allow_unused=True)[0] if torch.is_tensor(loss) and loss.requires_grad else None
    res = {k: v.detach() for k, v in out.items()}
    res["dvert_xyz"] = torch.zeros_like(x) if g is None else g
    return res


def brute_force(verts, faces):
    """One frame in numpy float64, written from the definitions: {"edges", "pairs", "nc", "lap", "deg"}."""
    x = np.asarray(verts, dtype=np.float64)
    faces = [tuple(int(i) for i in f) for f in np.asarray(faces).reshape(-1, 3)]
    incident = {}
    for k, f in enumerate(faces):
        for c in range(3):
            i, j = f[c], f[(c + 1) % 3]
            incident.setdefault((min(i, j), max(i, j)), []).append(k)
    edges = sorted(incident)
    pairs, total = [], 0.0
    for a, b in edges:
        fs = sorted(incident[(a, b)])
        for m in range(len(fs)):
            for n in range(m + 1, len(fs)):
                c0, c1 = (sum(faces[k]) - a - b for k in (fs[m], fs[n]))
                pairs.append((a, b, c0, c1))
                n0 = np.cross(x[b] - x[a], x[c0] - x[a])
                n1 = -np.cross(x[b] - x[a], x[c1] - x[a])
                l0, l1 = max(math.sqrt(n0 @ n0), 1e-8), max(math.sqrt(n1 @ n1), 1e-8)
                total += 1.0 - float(n0 @ n1) / (l0 * l1)
    ring = [set() for _ in range(len(x))]
    for a, b in edges:
        ring[a].add(b), ring[b].add(a)
    lap = 0.0
    for i, r in enumerate(ring):
        d = -x[i] if not r else sum(x[j] for j in sorted(r)) / len(r) - x[i]
        lap += math.sqrt(d @ d)
    return {"edges": edges, "pairs": pairs, "nc": total / len(pairs) if pairs else 0.0,
            "lap": lap / len(x) if len(x) else 0.0, "deg": [len(r) for r in ring], "ring": [sorted(r) for r in ring]}


# ---- the meshes of the GPU list ----------------------------------------------------------------------------------------
def book():
    """Three faces on the edge (0, 1), the pages at different angles: 3 pairs on one edge."""
    v = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.4, -0.3, 0.9], [0.6, -0.7, -0.5]]
    return torch.tensor(v), torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]])


def duplicated_face():
    """The tetrahedron's faces and face (0, 1, 2) once more, wound the other way: its pair with the original has c0 ==
    c1 (cos = -1)."""
    v, f = mesh("tetrahedron")
    return v, torch.cat([f, torch.tensor([[2, 1, 0]])])


def clamp_mesh():
    """sugar_cases' isolated_degenerate (vertex 12 in no face, a collinear face on vertices 13, 14, 15 of its own) and
    one more face (14, 13, 16) on the collinear face's first edge, so that the collinear face is in a pair."""
    v, f = mesh("isolated_degenerate")
    return torch.cat([v, torch.tensor([[1.005, 1.3, 1.1]])]), torch.cat([f, torch.tensor([[14, 13, 16]])])


def check_meshreg(got, r64, r32, tag, outs=("nc", "lap"), grads=("dvert_xyz",)):
    """The bar of the mesh-regulariser tests: sugar_cases.check_against_null on the gradients; a (T,) output has too
    few elements for the null to be a stable sample, so per frame |got - ref64| / |ref64| <= max(2 x null, 2^-23) (one
    float32 rounding of an fp64 result, doubled), and exactly 0 where ref64 is exactly 0.  Prints its figures."""
    check_against_null(got, r64, r32, grads, tag)
    for k in outs:
        e, e64, e32 = got[k].double(), r64[k], r32[k].double()
        assert got[k].dtype == torch.float32 and e.shape == e64.shape, (tag, k, e.shape)
        for t in range(len(e64)):
            scale = abs(float(e64[t]))
            if scale == 0:
                assert float(e[t]) == 0, (tag, k, t)
                continue
            err, null = abs(float(e[t] - e64[t])) / scale, abs(float(e32[t] - e64[t])) / scale
            print(f"{tag} {k}[{t}]: gpu {err:.3g}  fp32 null {null:.3g}")
            assert err <= max(2 * null, OUT_FLOOR), (tag, k, t, err, null)
