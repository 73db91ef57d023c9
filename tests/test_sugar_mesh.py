"""sugar_mesh (include/gsr.h gsr_sugar_mesh_*) without a GPU: the mesh binding's incidence, the reference's barycentric
tables, initial_log_scales, the argument checks of the Python wrapper and of the C entries (which precede any device
work), and the fp64 restatement of tests/sugar_mesh_reference.py itself against the synthetic SuGaR scene.  The
kernels' numerics are checked on the GPU in tests/test_gpu_sugar_mesh.py."""
import ctypes
import math

import numpy as np
import pytest

from diff_gaussian_rasterization import _C
from kernel_budget import assert_kernel_budget, needs_hipcc

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_mesh  # noqa: E402
import sugar_mesh_reference as ref  # noqa: E402
from sugar_mesh import MeshBinding, bound_gaussians, initial_log_scales  # noqa: E402

NAMES = ("gsr_sugar_mesh_workspace_bytes", "gsr_sugar_mesh_forward", "gsr_sugar_mesh_backward")


def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES


def _check_incidence(binding, faces):
    flat = faces.reshape(-1).long()
    V, F = binding.n_verts, binding.n_faces
    assert binding.faces.dtype == torch.int32 and torch.equal(binding.faces.long(), faces.long())
    assert binding.corner_order.dtype == torch.int32 and binding.corner_order.shape == (3 * F,)
    assert binding.vert_offsets.dtype == torch.int32 and binding.vert_offsets.shape == (V + 1,)
    assert sorted(binding.corner_order.tolist()) == list(range(3 * F))  # every corner once
    counts = torch.bincount(flat, minlength=V)
    assert torch.equal(binding.vert_offsets.long(), torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]))
    for v in range(V):
        own = binding.corner_order[int(binding.vert_offsets[v]):int(binding.vert_offsets[v + 1])].long()
        assert (flat[own] == v).all() and (own[1:] > own[:-1]).all(), v  # its corners, ascending


def test_binding_of_two_triangles():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    b = MeshBinding(faces, 5, [[0.5, 0.25, 0.25], [0.25, 0.5, 0.25]])  # vertex 4: no face
    assert (b.n_verts, b.n_faces, b.n_per_face, b.n_gaussians) == (5, 2, 2, 4) and b.circle_radius is None
    assert b.corner_order.tolist() == [0, 1, 4, 2, 3, 5]
    assert b.vert_offsets.tolist() == [0, 1, 3, 5, 6, 6]
    assert b.bary.dtype == torch.float32 and b.bary.device.type == "cpu" and b.bary.shape == (2, 3)
    _check_incidence(b, faces)
    for dtype in (torch.int32, torch.int16, torch.uint8):
        assert torch.equal(MeshBinding(faces.to(dtype), 4, [[1., 0., 0.]]).corner_order, b.corner_order)
    empty = MeshBinding(torch.zeros(0, 3, dtype=torch.int64), 3, [[1., 0., 0.]])
    assert empty.n_gaussians == 0 and empty.vert_offsets.tolist() == [0, 0, 0, 0]
    moved = b.to("cpu")
    assert moved is not b and torch.equal(moved.faces, b.faces) and moved.bary is b.bary


def test_binding_of_an_icosphere():
    v, f = gs.icosphere(1)
    faces = torch.tensor(f)
    b = MeshBinding.from_reference_count(faces, len(v), 6)
    assert (b.n_verts, b.n_faces, b.n_gaussians) == (42, 80, 480)
    _check_incidence(b, faces)


def test_reference_tables():
    """geometry/sugar.py:245-286: each set is symmetric under the triangle's corner permutations, sums to 1 per
    Gaussian and has the centroid as its mean; the radii by their closed forms."""
    assert set(sugar_mesh.REFERENCE_BARY) == set(sugar_mesh.REFERENCE_CIRCLE_RADIUS) == {1, 3, 4, 6}
    for G, rows in sugar_mesh.REFERENCE_BARY.items():
        t = np.asarray(rows, np.float64)
        assert t.shape == (G, 3) and np.allclose(t.sum(1), 1, atol=1e-15) and np.allclose(t.mean(0), 1 / 3, atol=1e-15)
        have = sorted(map(tuple, np.round(t, 12)))
        for perm in ((1, 2, 0), (1, 0, 2)):
            assert sorted(map(tuple, np.round(t[:, perm], 12))) == have
    assert sugar_mesh.REFERENCE_BARY[3][0] == (0.5, 0.25, 0.25)
    assert sugar_mesh.REFERENCE_BARY[4][0] == (1 / 3, 1 / 3, 1 / 3) and sugar_mesh.REFERENCE_BARY[4][1][0] == 2 / 3
    assert sugar_mesh.REFERENCE_BARY[6][0] == (2 / 3, 1 / 6, 1 / 6)
    assert sugar_mesh.REFERENCE_BARY[6][3] == (1 / 6, 5 / 12, 5 / 12)
    r = sugar_mesh.REFERENCE_CIRCLE_RADIUS
    assert r[1] == pytest.approx(0.28867513459481287, rel=1e-15)  # the incircle of the unit triangle
    assert r[3] == pytest.approx(0.18301270189221933, rel=1e-15)
    assert r[4] == pytest.approx(0.14433756729740643, rel=1e-15)
    assert r[6] == pytest.approx(0.13397459621556135, rel=1e-15)
    faces = torch.tensor([[0, 1, 2]])
    for G in (1, 3, 4, 6):
        b = MeshBinding.from_reference_count(faces, 3, G)
        assert b.n_per_face == G and b.circle_radius == r[G]
        assert torch.equal(b.bary, torch.tensor(sugar_mesh.REFERENCE_BARY[G], dtype=torch.float32))
    for G in (0, 2, 5, 7, "6"):
        with pytest.raises(ValueError):
            MeshBinding.from_reference_count(faces, 3, G)


def test_initial_log_scales():
    v, f = gs.icosphere(1)
    verts = torch.tensor(v, dtype=torch.float32)
    faces = torch.tensor(f)
    b = MeshBinding.from_reference_count(faces, len(v), 6)
    got = initial_log_scales(verts, b)
    fv = verts.numpy().astype(np.float64)[f]
    side = np.linalg.norm(fv - fv[:, [1, 2, 0]], axis=-1).min(-1)
    want = np.log(np.maximum(side / (4 + 2 * math.sqrt(3)), 1e-7))
    assert got.dtype == torch.float32 and got.shape == (480, 2)
    assert np.abs(got.numpy().astype(np.float64) - np.repeat(want, 6)[:, None]).max() < 1e-6
    # a collapsed face: the 1e-7 floor
    flat = MeshBinding.from_reference_count(torch.tensor([[0, 0, 1]]), 2, 3)
    assert torch.allclose(initial_log_scales(verts[:2], flat), torch.full((3, 2), math.log(1e-7)))
    custom = MeshBinding(faces, len(v), [[1 / 3, 1 / 3, 1 / 3]])
    with pytest.raises(ValueError, match="circle"):
        initial_log_scales(verts, custom)
    assert torch.equal(initial_log_scales(verts, custom, 1 / (4 + 2 * math.sqrt(3)))[:, 0], got[::6, 0])
    with pytest.raises(ValueError):
        initial_log_scales(verts[:10], b)


def test_binding_argument_errors():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    bary = [[1 / 3, 1 / 3, 1 / 3]]
    bad = [
        (faces.float(), 4, bary), (faces.tolist(), 4, bary), (faces.bool(), 4, bary),  # not an integer tensor
        (faces[:, :2], 4, bary), (faces.reshape(-1), 4, bary), (faces[None], 4, bary),  # not (F, 3)
        (faces, 3, bary), (torch.tensor([[0, -1, 2]]), 4, bary),  # an entry out of range
        (faces, -1, bary), (faces, 4.0, bary), (faces, True, bary),
        (faces, 4, torch.zeros(0, 3)), (faces, 4, torch.zeros(9, 3)),  # G = 0, G = 9
        (faces, 4, torch.zeros(3)), (faces, 4, torch.zeros(2, 2)), (faces, 4, "bary"),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            MeshBinding(*args)
    assert MeshBinding(faces, 4, torch.zeros(8, 3)).n_per_face == 8


def test_bound_gaussians_argument_errors():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    b = MeshBinding.from_reference_count(faces, 4, 3)
    ok = dict(verts=torch.zeros(4, 3), complex_numbers=torch.zeros(6, 2), log_scales=torch.zeros(6, 2))
    bad = [
        dict(ok, verts=torch.zeros(4, 3, dtype=torch.float64)), dict(ok, verts=torch.zeros(5, 3)),
        dict(ok, verts=torch.zeros(4, 2)), dict(ok, verts=[[0., 0., 0.]] * 4),
        dict(ok, complex_numbers=torch.zeros(5, 2)), dict(ok, complex_numbers=torch.zeros(8, 2)),  # N != F x G
        dict(ok, complex_numbers=torch.zeros(6, 3)), dict(ok, complex_numbers=torch.zeros(6, 2, dtype=torch.float16)),
        dict(ok, log_scales=torch.zeros(2, 2)), dict(ok, log_scales=torch.zeros(6)),
        dict(ok, log_scales=torch.zeros(6, 2, dtype=torch.int64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            bound_gaussians(kw["verts"], kw["complex_numbers"], kw["log_scales"], b, 1e-3)
    with pytest.raises(ValueError, match="F x G"):
        bound_gaussians(ok["verts"], torch.zeros(7, 2), ok["log_scales"], b, 1e-3)
    with pytest.raises(ValueError, match="MeshBinding"):
        bound_gaussians(*ok.values(), faces, 1e-3)
    with pytest.raises(ValueError, match="thickness"):
        bound_gaussians(*ok.values(), b, "thin")
    with pytest.raises(ValueError, match="no CPU path"):  # well-formed CPU tensors
        bound_gaussians(*ok.values(), b, 1e-3)


def test_c_entries_check_their_arguments_without_gpu():
    lib = _C.load_library()
    assert lib.gsr_sugar_mesh_workspace_bytes(0, 0) > 0  # valid for an empty mesh
    assert lib.gsr_sugar_mesh_workspace_bytes(0, 100) > 0
    for F in (1, 7, 327_680):
        assert 36 * F <= lib.gsr_sugar_mesh_workspace_bytes(F, 3 * F) <= 36 * F + 256
    v = ctypes.c_void_p(16)  # never dereferenced: the calls fail validation first
    bary = (ctypes.c_float * 24)(*([1 / 3] * 24))
    big = 1 << 40

    def mesh(V, F, G, verts, faces, cplx, ls):
        return _C.SugarMesh(V=V, F=F, G=G, verts=verts, faces=faces, cplx=cplx, log_scales=ls)

    def fwd(V=4, F=2, G=3, N=6, verts=v, faces=v, bary=bary, cplx=v, ls=v, xyz=v, sc=v, rot=v, nrm=v):
        return lib.gsr_sugar_mesh_forward(mesh(V, F, G, verts, faces, cplx, ls), N, bary, 1e-3, xyz, sc, rot, nrm, None)

    def bwd(V=4, F=2, G=3, N=6, verts=v, faces=v, bary=bary, cplx=v, ls=v, co=v, vo=v, g=(v, v, v, v), dv=v, dc=v,
            dl=v, ws=v, nbytes=big):
        return lib.gsr_sugar_mesh_backward(mesh(V, F, G, verts, faces, cplx, ls), N, bary, co, vo, *g, dv, dc, dl, ws,
                                           nbytes, None)

    assert lib.gsr_sugar_mesh_forward(None, 6, bary, 1e-3, v, v, v, v, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_mesh_backward(None, 6, bary, v, v, v, v, v, v, v, v, v, v, big, None) == 1
    assert b"null" in lib.gsr_last_error()
    # N != F x G: rejected with code 1 before the (null) device pointers are looked at
    for call in (fwd, bwd):
        assert call(N=7, verts=None, faces=None, cplx=None, ls=None) == 1 and b"F x G" in lib.gsr_last_error()
    assert fwd(N=5, verts=None, faces=None, cplx=None, ls=None, xyz=None, sc=None, rot=None, nrm=None) == 1
    assert b"F x G" in lib.gsr_last_error()
    for call in (fwd, bwd):
        for G in (0, 9):
            assert call(G=G, N=2 * G) == 1 and b"G must" in lib.gsr_last_error()
        assert call(V=-1) == 1 and call(F=-1, N=-3) == 1
        assert call(F=1 << 30, N=3 << 30) == 1  # (N as an int wraps: not F x G)
        for name in ("verts", "faces", "bary", "cplx", "ls"):
            assert call(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
        assert call(cplx=ctypes.c_void_p(20)) == 1 and b"aligned" in lib.gsr_last_error()
        assert call(F=0, N=0) == 0  # nothing to launch
        assert call(F=0, N=0, verts=None, faces=None, cplx=None, ls=None) == 0
    for name in ("xyz", "sc", "rot", "nrm"):
        assert fwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert fwd(rot=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()
    for name in ("co", "vo", "dv", "dc", "dl", "ws"):
        assert bwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert bwd(g=(v, v, ctypes.c_void_p(24), v)) == 1 and b"aligned" in lib.gsr_last_error()
    assert bwd(dc=ctypes.c_void_p(20)) == 1 and b"aligned" in lib.gsr_last_error()
    assert bwd(nbytes=lib.gsr_sugar_mesh_workspace_bytes(2, 4) - 1) == 1 and b"workspace" in lib.gsr_last_error()


def test_restatement_against_the_synthetic_scene():
    """make_sugar_scene builds the same Gaussians in numpy from its own formulas (fp64, rounded to fp32), with
    complex = (1, 0) and scales = shortest side / (4 + 2 sqrt 3): means, scales and normals agree with the fp64
    restatement to fp32 rounding, rotations up to each row's sign."""
    scene = gs.make_sugar_scene(subdiv=2, sh_degree=0)
    v, f = gs.icosphere(2)
    verts, faces = torch.tensor(v, dtype=torch.float64), torch.tensor(f)
    b = MeshBinding.from_reference_count(faces, len(v), 6)
    N = b.n_gaussians
    cplx = torch.tensor([[1.0, 0.0]], dtype=torch.float64).expand(N, 2)
    s = torch.tensor(scene["scales"][:, 1:].astype(np.float64))
    xyz, scaling, rotation, normals, branch = ref.bound_gaussians_reference(
        verts, faces, torch.tensor(sugar_mesh.REFERENCE_BARY[6], dtype=torch.float64), cplx, torch.log(s), 3.5e-6)
    assert len(torch.unique(branch)) == 4  # every candidate row of matrix_to_quaternion is taken somewhere
    eps = 2.0 ** -24

    def close(a, name, tol=eps):
        want = torch.tensor(scene[name].astype(np.float64))
        assert a.shape == want.shape and float((a - want).abs().max()) <= tol * float(want.abs().max()), name

    close(xyz, "means3D")
    close(scaling, "scales", 2 * eps)  # (the scene's fp32 scale through log and exp)
    close(normals, "normals")
    want_q = torch.tensor(scene["rotations"].astype(np.float64))
    sign = ref.row_sign(rotation, want_q)
    assert float((rotation * sign[:, None] - want_q).abs().max()) <= 2 * eps
    assert float((rotation.norm(dim=-1) - 1).abs().max()) < 1e-12
    # the restatement in fp32 (the GPU tests' null) is that close to itself in fp64
    verts32 = verts.float()
    ups = {k: None for k in ref.OUTPUTS}
    a = ref.evaluate(torch.float32, verts32, faces, b.bary, cplx.float(), torch.log(s).float(), 3.5e-6, ups)
    c = ref.evaluate(torch.float64, verts32, faces, b.bary, cplx.float(), torch.log(s).float(), 3.5e-6, ups)
    for k in ("xyz", "scaling", "normals"):
        assert float((a[k].double() - c[k]).abs().max()) <= 8 * eps * float(c[k].abs().max()), k


def test_restatement_gradient_does_not_depend_on_the_candidate_row():
    """The composite gradient with the second-largest candidate row forced equals the one with the largest (up to
    the row's sign, aligned through the upstream gradient): a branch flip between the kernel and the reference needs
    no allowance."""
    v, f = gs.icosphere(1)
    verts, faces = torch.tensor(v, dtype=torch.float32), torch.tensor(f)
    b = MeshBinding.from_reference_count(faces, len(v), 6)
    gen = torch.Generator().manual_seed(0)
    N = b.n_gaussians
    cplx, ls = torch.randn(N, 2, generator=gen), torch.randn(N, 2, generator=gen) * 0.3 - 4
    ups = {"rotation": torch.randn(N, 4, generator=gen), "normals": torch.randn(N, 3, generator=gen)}
    first = ref.evaluate(torch.float64, verts, faces, b.bary, cplx, ls, 1e-3, ups)
    # the second-largest a_i, read off the reference rotation (a_i = 2 |q_i| for a rotation matrix)
    second = first["rotation"].abs().argsort(dim=-1, descending=True)[:, 1]
    forced = ref.evaluate(torch.float64, verts, faces, b.bary, cplx, ls, 1e-3, ups, branch=second)
    sign = ref.row_sign(forced["rotation"], first["rotation"])
    aligned = ref.evaluate(torch.float64, verts, faces, b.bary, cplx, ls, 1e-3, ups, sign=sign, branch=second)
    assert float((forced["rotation"] * sign[:, None] - first["rotation"]).abs().max()) < 1e-12
    for k in ref.GRADS:
        scale = float(first[k].abs().max())
        assert float((aligned[k] - first[k]).abs().max()) <= 1e-9 * max(scale, 1.0), k


@needs_hipcc
def test_mesh_kernels_do_not_spill(tmp_path):
    kernels = ("k_mesh_forwardE", "k_mesh_faceE", "k_mesh_vertexE")
    res = assert_kernel_budget("gsr_mesh.hip", tmp_path, "k_mesh", dict.fromkeys(kernels, 0), sgpr_too=True)
    for name, r in res.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
