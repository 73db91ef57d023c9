"""sugar_arap (include/gsr.h gsr_sugar_arap_*) without a GPU: the binding's CSR one-rings and weights against the dense
(V, V) restatement of tests/sugar_arap_reference.py (bitwise: both sides run the same torch float32 ops on this
machine), the argument checks, and the properties that pin the energy restatement (the checker of the GPU tests in
tests/test_gpu_sugar_arap.py)."""
import ctypes

import pytest

from diff_gaussian_rasterization import _C

torch = pytest.importorskip("torch")

import sugar_arap  # noqa: E402
import sugar_arap_reference as ref  # noqa: E402
from sugar_arap import ArapBinding, arap_energy  # noqa: E402
from sugar_cases import MESHES, mesh, random_quats  # noqa: E402

NAMES = ("gsr_sugar_arap_workspace_bytes", "gsr_sugar_arap_forward", "gsr_sugar_arap_backward")
D = torch.float64

def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES
    assert set(sugar_arap.__all__) >= {"ArapBinding", "arap_energy"}
    assert int(lib.gsr_sugar_arap_workspace_bytes(8, 163842)) == 8 * 8 * 641 + 192  # 8 T ceil(V / 256), to 256 bytes


@pytest.mark.parametrize("name", sorted(MESHES))
def test_binding_is_the_dense_restatement(name):
    verts, faces = mesh(name)
    V = len(verts)
    b = ArapBinding(verts, faces)
    ii, jj, nn = ref.one_rings(faces, V)
    assert b.offsets.dtype == torch.int32 and b.nbr.dtype == torch.int32 and b.offsets.shape == (V + 1,)
    assert b.w.dtype == torch.float32 and b.p.dtype == torch.float32 and b.p.shape == (b.n_edges, 3)
    assert (b.n_verts, b.n_faces, b.n_edges) == (V, len(faces), len(ii))
    counts = torch.bincount(ii, minlength=V)
    assert torch.equal(b.offsets.long(), torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]))
    assert b.max_valence == int(counts.max())
    assert torch.equal(b.nbr.long(), jj)  # ascending within a row, as one_rings lists them
    for i in range(V):
        row = b.nbr[int(b.offsets[i]):int(b.offsets[i + 1])]
        assert bool((row[1:] > row[:-1]).all())
    W = ref.dense_cot_weights(verts, faces)
    assert torch.equal(b.w, W[ii, jj])  # bitwise
    assert torch.equal(b.p, verts[ii] - verts[jj])
    assert torch.isfinite(b.w).all()
    # symmetric across reverse edges, bitwise
    where = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(ii, jj))}
    back = torch.tensor([where[(int(j), int(i))] for i, j in zip(ii, jj)], dtype=torch.long)
    assert torch.equal(b.w, b.w[back]) and torch.equal(b.p, -b.p[back])
    assert bool((b.w < 0).any()), "no obtuse corner in " + name
    moved = b.to("cpu")
    assert moved is not b and torch.equal(moved.w, b.w)


def test_valences():
    assert ArapBinding(*mesh("triangle")).max_valence == 2
    assert ArapBinding(*mesh("tetrahedron")).max_valence == 3
    b = ArapBinding(*mesh("icosphere1"))
    assert sorted(set((b.offsets[1:] - b.offsets[:-1]).tolist())) == [5, 6] and b.n_verts == 42
    assert ArapBinding(*mesh("fan200")).max_valence == 200
    b = ArapBinding(*mesh("isolated_degenerate"))
    assert int(b.offsets[12]) == int(b.offsets[13])  # the vertex in no face: an empty row
    e = ArapBinding(torch.zeros(3, 3), torch.zeros((0, 3), dtype=torch.int64))
    assert (e.n_edges, e.max_valence) == (0, 0) and e.offsets.tolist() == [0, 0, 0, 0]


def test_degenerate_face_takes_the_clamp():
    verts, faces = mesh("isolated_degenerate")
    b = ArapBinding(verts, faces)
    rows = slice(int(b.offsets[13]), int(b.offsets[16]))
    assert b.w[rows].numel() == 6 and torch.isfinite(b.w[rows]).all()
    # area = sqrt(1e-12) = 1e-6: the weights are the squared-length sums over 8e-6
    v = verts[13:16]
    A2, B2, C2 = [float(x) for x in ((v[1] - v[2]).norm() ** 2, (v[0] - v[2]).norm() ** 2, (v[0] - v[1]).norm() ** 2)]
    k = int(b.offsets[13])  # edge (13, 14): the corner at 13 alone (no reverse edge in a face)
    assert int(b.nbr[k]) == 14 and float(b.w[k]) == pytest.approx((B2 + C2 - A2) / 8e-6, rel=1e-4)


def test_binding_argument_checks():
    verts, faces = mesh("tetrahedron")
    with pytest.raises(ValueError, match="floating-point"):
        ArapBinding(verts.long(), faces)
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        ArapBinding(verts[:, :2], faces)
    with pytest.raises(ValueError, match="integer"):
        ArapBinding(verts, faces.float())
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        ArapBinding(verts, faces[:, :2])
    with pytest.raises(ValueError, match="outside"):
        ArapBinding(verts, torch.tensor([[0, 1, 4]]))
    with pytest.raises(ValueError, match="outside"):
        ArapBinding(verts, torch.tensor([[0, 1, -1]]))
    with pytest.raises(ValueError, match="repeats a vertex"):
        ArapBinding(verts, torch.tensor([[0, 1, 1]]))
    with pytest.raises(ValueError, match="more than one face"):
        ArapBinding(verts, torch.tensor([[0, 1, 2], [0, 1, 3]]))  # the directed edge (0, 1) twice
    with pytest.raises(ValueError, match="too large"):
        ArapBinding(verts, torch.zeros((1, 3), dtype=torch.int64).expand(2 ** 31 // 6 + 1, 3))
    assert ArapBinding(verts.double(), faces.int()).w.dtype == torch.float32


def test_energy_argument_checks():
    verts, faces = mesh("tetrahedron")
    b = ArapBinding(verts, faces)
    x, q = torch.zeros(2, 4, 3), torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="ArapBinding"):
        arap_energy(x, q, None)
    with pytest.raises(ValueError, match="vert_xyz must be a float32"):
        arap_energy(x.double(), q, b)
    with pytest.raises(ValueError, match="vert_xyz must have shape"):
        arap_energy(x[:, :3], q, b)
    with pytest.raises(ValueError, match="vert_rot must have shape"):
        arap_energy(x, q[:1], b)
    with pytest.raises(ValueError, match="vert_rot must have shape"):
        arap_energy(x, torch.zeros(2, 4, 3, 2), b)
    with pytest.raises(ValueError, match="vert_rot must be a float32"):
        arap_energy(x, torch.zeros(2, 4, 3, 3, dtype=D), b)
    with pytest.raises(ValueError, match="no CPU path"):
        arap_energy(x, q, b)


def test_c_entries_check_before_any_device_work():
    lib = _C.load_library()
    null = None

    def arap(T, V, E, rot_form):  # (every pointer of the struct null)
        return _C.SugarArap(T=T, V=V, E=E, rot_form=rot_form)

    assert lib.gsr_sugar_arap_forward(arap(0, 0, 0, 0), null, null, 0, null) == 0  # nothing to do
    assert lib.gsr_sugar_arap_backward(arap(0, 4, 0, 1), null, null, null, null) == 0
    for args, msg in (((1, 4, 6, 2), "rot_form"), ((-1, 4, 6, 0), "negative"), ((2 ** 16, 2 ** 15, 6, 0), "2^31"),
                      ((1, 4, 6, 0), "null pointer")):
        assert lib.gsr_sugar_arap_forward(arap(*args), null, null, 0, null) == 1
        assert msg in lib.gsr_last_error().decode()
        assert lib.gsr_sugar_arap_backward(arap(*args), null, null, null, null) == 1
        assert msg in lib.gsr_last_error().decode()
    v = ctypes.c_void_p(16)  # never dereferenced: a null struct fails first
    assert lib.gsr_sugar_arap_forward(null, v, v, 1 << 40, null) == 1 and b"null pointer" in lib.gsr_last_error()
    assert lib.gsr_sugar_arap_backward(null, v, v, v, null) == 1 and b"null pointer" in lib.gsr_last_error()


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_is_the_double_loop_on_the_tetrahedron():
    verts, faces = mesh("tetrahedron")
    verts = verts.to(D)
    gen = torch.Generator().manual_seed(0)
    x = verts + 0.2 * torch.randn(4, 3, generator=gen, dtype=D)
    R = torch.randn(4, 3, 3, generator=gen, dtype=D)
    W = ref.dense_cot_weights(verts, faces)
    ii, jj, nn = ref.one_rings(faces, 4)
    got = ref.arap_energy_reference(x[None], R[None], verts, ii, jj, nn, W[ii, jj])
    want = 0.0
    for i in range(4):
        for j in range(4):
            if i != j:  # closed: every pair is an edge
                want = want + W[i, j] * ((x[i] - x[j]) - R[i] @ (verts[i] - verts[j])).pow(2).sum()
    assert got.shape == (1,) and float(got[0]) == pytest.approx(float(want), rel=1e-13)


@pytest.mark.parametrize("form", ["quat", "matrix"])
@pytest.mark.parametrize("name", ["tetrahedron", "icosphere1", "fan200"])
def test_restatement_vanishes_under_a_rigid_motion(name, form):
    """x' = Q x + t with every R_i = Q: E < 1e-24 sum |w| |p|^2 (float64 rounding)."""
    verts, faces = mesh(name)
    verts = verts.to(D)
    V = len(verts)
    b = ArapBinding(verts, faces)
    rings = ref.one_rings(faces, V)
    gen = torch.Generator().manual_seed(1)
    q = torch.nn.functional.normalize(random_quats(gen, (1,), dtype=D, identity_every=0), dim=-1)
    Q = ref.qmatrix(q)[0]
    x = verts @ Q.T + torch.tensor([0.3, -0.2, 0.5], dtype=D)
    rot = q.expand(V, 4) if form == "quat" else Q.expand(V, 3, 3)
    e = ref.arap_energy_reference(x[None], rot[None].contiguous(), verts, *rings, b.w)
    scale = float((b.w.to(D).abs() * (verts[rings[0]] - verts[rings[1]]).pow(2).sum(-1)).sum())
    assert abs(float(e[0])) < 1e-24 * scale, (float(e[0]), scale)


def test_restatement_takes_unnormalised_quaternions_as_pypose_does():
    gen = torch.Generator().manual_seed(2)
    q = random_quats(gen, (5,), dtype=D)
    x, y, z, w = q.unbind(-1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(5, 3, 3)
    want = torch.eye(3, dtype=D) + 2 * w[:, None, None] * K + 2 * K @ K  # I + 2 w [v]x + 2 [v]x^2
    assert torch.allclose(ref.qmatrix(q), want, rtol=0, atol=1e-15)
