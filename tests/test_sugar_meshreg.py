"""sugar_meshreg (include/gsr.h gsr_sugar_normal_consistency_* / gsr_sugar_laplacian_*) without a GPU: the restatements
of tests/sugar_meshreg_reference.py (the checker of tests/test_gpu_sugar_meshreg.py) against the brute-force statement
of the same definitions and against closed forms, ``MeshTopology``'s tables against the brute force, the argument
checks, and the C entries' checks.  pytorch3d itself is not available: nothing here is pinned to its code."""
import ctypes
import math

import numpy as np
import pytest

from diff_gaussian_rasterization import _C

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_meshreg  # noqa: E402
import sugar_meshreg_reference as ref  # noqa: E402
from sugar_arap import ArapBinding  # noqa: E402
from sugar_cases import MESHES, jittered_icosphere, mesh  # noqa: E402
from sugar_meshreg import MeshTopology, laplacian_smoothing, normal_consistency  # noqa: E402

D = torch.float64
NAMES = ("gsr_sugar_meshreg_workspace_bytes", "gsr_sugar_normal_consistency_forward",
         "gsr_sugar_normal_consistency_backward", "gsr_sugar_laplacian_forward", "gsr_sugar_laplacian_backward")


def _ico(subdiv):
    v, f = jittered_icosphere(subdiv)
    return torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f)


# the meshes of the GPU list (tests/test_gpu_sugar_meshreg.py)
GPU_MESHES = dict({k: (lambda k=k: mesh(k)) for k in MESHES}, book=ref.book, duplicated_face=ref.duplicated_face,
                  clamp_mesh=ref.clamp_mesh, icosphere3=lambda: _ico(3), icosphere2=lambda: _ico(2))


def _both(verts, faces):
    """(restatement in fp64, brute force) of one frame."""
    V = len(verts)
    edges, pairs = ref.topology(faces, V)
    x = verts.to(D)[None]
    return ({"edges": edges, "pairs": pairs, "nc": float(ref.normal_consistency_reference(x, pairs)[0]),
             "lap": float(ref.laplacian_reference(x, edges)[0])}, ref.brute_force(verts.numpy(), faces.numpy()))


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GPU_MESHES))
def test_restatement_is_the_brute_force(name):
    verts, faces = GPU_MESHES[name]()
    got, want = _both(verts, faces)
    assert got["edges"].tolist() == [list(e) for e in want["edges"]]
    assert len(got["pairs"]) == len(want["pairs"]) and got["pairs"].tolist() == [list(p) for p in want["pairs"]]
    for k in ("nc", "lap"):
        print(f"{name} {k}: restatement {got[k]!r}  brute force {want[k]!r}")
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0 if want[k] else 1e-300)


def _nc_lap(verts, faces):
    verts = torch.as_tensor(verts, dtype=D)
    edges, pairs = ref.topology(torch.as_tensor(faces), len(verts))
    return (float(ref.normal_consistency_reference(verts[None], pairs)[0]),
            float(ref.laplacian_reference(verts[None], edges)[0]), len(pairs))


def test_closed_form_unit_cube():
    """12 outward-wound triangles: the 12 cube edges join faces at a right angle (1 - cos = 1), the 6 face diagonals
    coplanar triangles (0): P = 18, nc = 12 / 18."""
    v = [[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)]  # index 4 x + 2 y + z
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
         [1, 5, 7], [1, 7, 3]]
    vt = np.asarray(v)
    for a, b, c in f:  # outward: the normal points away from the centre
        assert np.cross(vt[b] - vt[a], vt[c] - vt[a]) @ (vt[a] - 0.5) > 0
    nc, _, P = _nc_lap(v, f)
    assert P == 18 and abs(nc - 2 / 3) <= 1e-15


def test_closed_form_regular_tetrahedron():
    """Centred at the origin: the dihedral angle has cos = 1/3 and the outward normals cos = -1/3, so nc = 4/3; the
    mean of the other three vertices is -x / 3, so d = -(4/3) x and lap = (4/3) |x|."""
    v = [[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]]
    f = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    nc, lap, P = _nc_lap(v, f)
    assert P == 6 and nc == pytest.approx(4 / 3, rel=1e-14) and lap == pytest.approx(4 / 3 * math.sqrt(3), rel=1e-14)


def test_closed_form_two_triangles_flat_and_folded():
    flat = [[0., 0., 0.], [1., 0., 0.], [0.3, 1., 0.], [0.6, -2., 0.]]
    f = [[0, 1, 2], [1, 0, 3]]
    nc, _, P = _nc_lap(flat, f)
    assert P == 1 and abs(nc) <= 1e-15
    folded = [[0., 0., 0.], [1., 0., 0.], [0.3, 1., 0.], [0.6, 2., 0.]]  # the second onto the first's side
    nc, _, P = _nc_lap(folded, f)
    assert P == 1 and nc == pytest.approx(2.0, abs=1e-15)


def test_closed_form_single_triangle():
    verts, faces = mesh("triangle")
    nc, lap, P = _nc_lap(verts, faces)
    want = ref.brute_force(verts.numpy(), faces.numpy())
    assert P == 0 and nc == 0.0 and want["deg"] == [2, 2, 2]
    x = verts.to(D)
    assert lap == pytest.approx(float(sum(((x.sum(0) - x[i]) / 2 - x[i]).norm() for i in range(3)) / 3), rel=1e-14)


def test_cosine_similarity_clamps_each_norm_on_its_own():
    """What the header states of the installed torch: two copies of (1e-9, 0, 0) give 1e-18 / (1e-8 1e-8) = 0.01, and
    the norm's gradient at the zero vector is 0."""
    a = torch.tensor([[1e-9, 0.0, 0.0]], dtype=D)
    assert float(torch.nn.functional.cosine_similarity(a, a.clone(), dim=1)) == pytest.approx(0.01, rel=1e-12)
    z = torch.zeros(1, 3, dtype=D, requires_grad=True)
    torch.norm(z, dim=1).sum().backward()
    assert not z.grad.any()


def test_isolated_vertex_adds_its_own_norm():
    verts, faces = mesh("fan200")
    with_it = ref.brute_force(verts.numpy(), faces.numpy())
    assert with_it["deg"][-1] == 0
    without = ref.brute_force(verts[:-1].numpy(), faces.numpy())
    V = len(verts)
    assert with_it["lap"] * V == pytest.approx(without["lap"] * (V - 1) + float(verts[-1].to(D).norm()), rel=1e-13)


# ---- MeshTopology ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GPU_MESHES))
def test_topology_is_the_brute_force(name):
    verts, faces = GPU_MESHES[name]()
    V = len(verts)
    t = MeshTopology(faces, V)
    want = ref.brute_force(verts.numpy(), faces.numpy())
    for k in MeshTopology._TENSORS:
        assert getattr(t, k).dtype == torch.int32, k
    assert (t.n_verts, t.n_faces, t.n_edges, t.n_pairs) == (V, len(faces), len(want["edges"]), len(want["pairs"]))
    assert t.edges.tolist() == [list(e) for e in want["edges"]]
    assert t.pairs.tolist() == [list(p) for p in want["pairs"]]
    # the slots: every (pair, role) once, in its vertex's row, rows ascending
    assert t.slot_offsets.shape == (V + 1,) and t.slots.shape == (4 * t.n_pairs,)
    assert sorted(t.slots.tolist()) == list(range(4 * t.n_pairs))
    flat = t.pairs.flatten()
    for i in range(V):
        row = t.slots[int(t.slot_offsets[i]):int(t.slot_offsets[i + 1])].long()
        assert bool((row[1:] > row[:-1]).all()) and bool((flat[row] == i).all())
    assert t.max_slots == max(int(torch.bincount(flat.long(), minlength=V).max()), 0)
    # the one-rings
    assert t.ring_offsets.shape == (V + 1,) and t.ring.shape == (2 * t.n_edges,)
    assert [t.ring[int(t.ring_offsets[i]):int(t.ring_offsets[i + 1])].tolist() for i in range(V)] == want["ring"]
    assert t.max_valence == max(want["deg"])
    moved = t.to("cpu")
    assert moved is not t and torch.equal(moved.pairs, t.pairs) and t.device.type == "cpu"


@pytest.mark.parametrize("name", sorted(MESHES))
def test_ring_is_the_arap_bindings(name):
    verts, faces = mesh(name)
    t, b = MeshTopology(faces, len(verts)), ArapBinding(verts, faces)
    assert torch.equal(t.ring, b.nbr) and torch.equal(t.ring_offsets, b.offsets) and t.max_valence == b.max_valence


def test_book_and_duplicated_face():
    verts, faces = ref.book()
    t = MeshTopology(faces, len(verts))
    assert t.n_pairs == 3 and t.pairs.tolist() == [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4]] and t.n_edges == 7
    verts, faces = ref.duplicated_face()
    t = MeshTopology(faces, len(verts))
    same = t.pairs[t.pairs[:, 2] == t.pairs[:, 3]]
    assert len(same) == 3 and t.n_pairs == 3 * 3 + 3  # the three edges of face (0, 1, 2) are in three faces each
    x = verts.to(D)[None]
    per_pair = 1 - torch.nn.functional.cosine_similarity(
        *(s * torch.cross(x[0, same[:, 1].long()] - x[0, same[:, 0].long()],
                          x[0, same[:, 2].long()] - x[0, same[:, 0].long()], dim=-1) for s in (1, -1)), dim=-1)
    assert torch.allclose(per_pair, torch.full((3,), 2.0, dtype=D), rtol=0, atol=1e-15)


def test_sizes_at_the_shipped_mesh_formulas():
    """icosphere(3): V = 642, F = 1280, E = 1920 = P (closed and manifold), every slot row 2 x valence."""
    v, f = gs.icosphere(3)
    t = MeshTopology(torch.as_tensor(f), len(v))
    assert (t.n_verts, t.n_faces, t.n_edges, t.n_pairs, t.max_valence, t.max_slots) == (642, 1280, 1920, 1920, 6, 12)
    e = MeshTopology(torch.zeros((0, 3), dtype=torch.int64), 3)
    assert (e.n_edges, e.n_pairs, e.max_valence, e.max_slots) == (0, 0, 0, 0)
    assert e.ring_offsets.tolist() == [0, 0, 0, 0] and e.slot_offsets.tolist() == [0, 0, 0, 0]
    none = MeshTopology(torch.zeros((0, 3), dtype=torch.int64), 0)
    assert none.ring_offsets.tolist() == [0] and none.pairs.shape == (0, 4)


def test_topology_argument_checks():
    _, faces = mesh("tetrahedron")
    with pytest.raises(ValueError, match="integer"):
        MeshTopology(faces.float(), 4)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        MeshTopology(faces[:, :2], 4)
    with pytest.raises(ValueError, match="outside"):
        MeshTopology(torch.tensor([[0, 1, 4]]), 4)
    with pytest.raises(ValueError, match="outside"):
        MeshTopology(torch.tensor([[0, 1, -1]]), 4)
    with pytest.raises(ValueError, match="repeats a vertex"):
        MeshTopology(torch.tensor([[0, 1, 1]]), 4)
    with pytest.raises(ValueError, match="too large"):
        MeshTopology(torch.zeros((1, 3), dtype=torch.int64).expand(2 ** 31 // 6 + 1, 3), 4)
    with pytest.raises(ValueError, match="too large"):
        MeshTopology(faces, 2 ** 31)
    assert MeshTopology(torch.tensor([[0, 1, 2], [0, 1, 3]]), 4).n_pairs == 1  # a directed edge twice: legal here
    assert MeshTopology(faces.int(), 4).pairs.dtype == torch.int32


def test_loss_argument_checks():
    _, faces = mesh("tetrahedron")
    t = MeshTopology(faces, 4)
    x = torch.zeros(2, 4, 3)
    for fn in (normal_consistency, laplacian_smoothing):
        with pytest.raises(ValueError, match="MeshTopology"):
            fn(x, None)
        with pytest.raises(ValueError, match="vert_xyz must be a float32"):
            fn(x.double(), t)
        with pytest.raises(ValueError, match="vert_xyz must have shape"):
            fn(x[:, :3], t)
        with pytest.raises(ValueError, match="vert_xyz must have shape"):
            fn(x[0], t)
        with pytest.raises(ValueError, match="no CPU path"):
            fn(x, t)


# ---- the C entries -----------------------------------------------------------------------------------------------------
def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES
    assert "gsr_sugar_meshreg" in _C.STRUCTS
    assert set(sugar_meshreg.__all__) == {"MeshTopology", "normal_consistency", "laplacian_smoothing"}


def test_workspace_bytes_grow_as_documented():
    size = _C.load_library().gsr_sugar_meshreg_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    T, V, P = 8, 163842, 491520
    assert int(size(T, V, P, 0)) == up(8 * T * 1920)  # 8 T ceil(max(P, V) / 256)
    assert int(size(T, V, 0, 0)) == up(8 * T * 641)
    assert int(size(T, V, P, 1)) == up(96 * T * P)  # the normal consistency's backward: four fp64 rows per (t, pair)
    assert int(size(T, V, P, 2)) == up(24 * T * V)  # the Laplacian's backward: one fp64 row per (t, vertex)
    assert int(size(2 * T, V, P, 1)) == 2 * int(size(T, V, P, 1))
    assert int(size(0, 0, 0, 0)) == 256 and int(size(-1, -1, -1, 1)) == 256 and int(size(-1, -1, -1, 2)) == 256
    assert int(size(T, V, P, 3)) == 0 and int(size(T, V, P, -1)) == 0  # an unknown pass


def test_c_entries_check_before_any_device_work():
    lib = _C.load_library()
    null, v = None, ctypes.c_void_p(256)  # (never dereferenced: every call here fails, or has nothing to do, first)
    fields = ("vert_xyz", "pairs", "slot_offsets", "slots", "ring_offsets", "ring")

    def reg(T, V, E, P, **missing):
        return _C.SugarMeshReg(T=T, V=V, E=E, P=P, **{k: missing.get(k, v) for k in fields})

    calls = {"nc_fwd": lambda s, out=v, ws=v, n=1 << 40: lib.gsr_sugar_normal_consistency_forward(s, out, ws, n, null),
             "nc_bwd": lambda s, out=v, ws=v, n=1 << 40, g=v: lib.gsr_sugar_normal_consistency_backward(s, g, out, ws, n,
                                                                                                      null),
             "lap_fwd": lambda s, out=v, ws=v, n=1 << 40: lib.gsr_sugar_laplacian_forward(s, out, ws, n, null),
             "lap_bwd": lambda s, out=v, ws=v, n=1 << 40, g=v: lib.gsr_sugar_laplacian_backward(s, g, out, ws, n, null)}

    def fails(rc, msg):
        assert rc == 1 and msg in lib.gsr_last_error().decode(), (rc, msg, lib.gsr_last_error())

    for name, call in calls.items():
        nc = name.startswith("nc")
        assert call(reg(0, 4, 6, 6)) == 0  # nothing to do: T = 0
        assert call(reg(2, 4, 6, 0) if nc else reg(2, 0, 0, 0)) == 0  # ... and no pair / no vertex
        fails(call(None), "null pointer")
        fails(call(reg(-1, 4, 6, 6)), "negative")
        fails(call(reg(1, 4, 6, -6)), "negative")
        fails(call(reg(2 ** 16, 2 ** 15, 6, 6)), "2^31")
        fails(call(reg(1, 4, 6, 2 ** 29)), "2^31")
        for field in ("vert_xyz",) + (("pairs",) if nc else ("ring_offsets", "ring")):
            fails(call(reg(1, 4, 6, 6, **{field: null})), "null pointer argument: " + field)
        if name == "nc_bwd":
            for field in ("slot_offsets", "slots"):
                fails(call(reg(1, 4, 6, 6, **{field: null})), "null pointer argument: " + field)
        out_name = "dL_dvert_xyz" if name.endswith("bwd") else name[:-4]
        fails(call(reg(1, 4, 6, 6), out=null), "null pointer argument: " + out_name)
        fails(call(reg(1, 4, 6, 6), ws=null), "null pointer argument: workspace")
        fails(call(reg(1, 4, 6, 6), ws=ctypes.c_void_p(260)), "workspace must be 8-byte aligned")
        fails(call(reg(1, 4, 6, 6), n=255), "workspace too small")
        if nc:
            fails(call(reg(1, 4, 6, 6, pairs=ctypes.c_void_p(264))), "pairs must be 16-byte aligned")
        if name.endswith("bwd"):
            fails(call(reg(1, 4, 6, 6), g=null), "null pointer argument: dL_d" + name[:-4])
