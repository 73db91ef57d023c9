"""Pin the torch restatements of the SuGaR stages (tests/sugar_arap_reference.py, tests/sugar_dynamic_reference.py,
tests/sugar_mesh_reference.py, the field and normal checkers of tests/sugar_cases.py), and the ArapBinding's weights, to
fixtures computed by the reference's own code (read by ``fixture`` of tests/sugar_cases.py, which also holds the bars).

tests/golden/make_golden.py lifts ARAPCoach (utils/arap_utils.py), the skinning / timed-Gaussian methods of
geometry/dynamic_sugar.py with the DualQuaternion class (utils/dual_quaternions.py), and the mesh-bound property bodies
of SuGaRModel (geometry/sugar.py) out of the reference's source with ``ast`` and runs them on the CPU, once in float32
(``*_f32``: the reference as it really runs, the "fp32 null" of tests/test_gpu_reference_pins.py) and once in float64
(``*_f64``: the value to match), with autograd gradients for stored upstream gradients.  Only inputs and outputs are in
the ``.npz`` files; nothing here reads the reference.  pypose and pytorch3d are replaced by
tests/golden/standins.py, which this file pins to scipy.

Bars, as the shading pin of tests/test_golden.py: max |restatement - fixture| <= 1e-12 max |fixture| on outputs, 1e-10
on gradients, both in float64.  No tensor needed more (the measured gaps are in each test's docstring).

What the fixtures keep away from, on purpose: quaternions off the unit sphere (all stored node, vertex and rest
rotations are float64 and unit to fp64 rounding), because what pypose's ``Log()`` and ``matrix()`` do there cannot be
checked without pypose; see ``test_skin_restatement`` for the one place where that shows in a gradient.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sugar_arap_reference as arap_ref  # noqa: E402
import sugar_dynamic_reference as dyn_ref  # noqa: E402
import sugar_mesh_reference as mesh_ref  # noqa: E402
from sugar_arap_reference import ARAP_MESHES  # noqa: E402
from sugar_cases import (FIELD_RUNS, GRAD_BAR, OUT_BAR, D, _compose64, _field, _mask, _normal,  # noqa: E402
                         _quat_to_matrix, _run, close, field_keys, fixture, null_is_usable)
from sugar_cases import _rel as rel  # noqa: E402
from sugar_dynamic_reference import SKIN_KEYS, TIMED_KEYS, tangent  # noqa: E402
from sugar_mesh_reference import MESH_KEYS, mesh_fixture  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# the stand-ins against scipy


def _standin_quats():
    """Unit (x, y, z, w), float64: angles 1e-9 .. just under pi (log-spaced, then linear), both signs of w."""
    rng = np.random.default_rng(5)
    angle = np.concatenate([np.logspace(-9, 0, 60), np.linspace(1.0, np.pi - 1e-6, 40)])
    axis = rng.normal(size=(len(angle), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    q = np.concatenate([np.sin(angle / 2)[:, None] * axis, np.cos(angle / 2)[:, None]], 1)
    q[1::2] *= -1  # w < 0
    return q, angle[:, None] * axis


def test_standins_match_scipy():
    """product, inverse, matrix, Log, Exp of the pypose stand-in and the two pytorch3d conversions against
    scipy.spatial.transform.Rotation (scalar-last quaternions), at fp64 rounding (1e-12).  Measured: 7.8e-16 at the
    most (matrix); Log 4.4e-16."""
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    from golden import standins as pp

    q, rotvec = _standin_quats()
    assert (q[:, 3] > 0).any() and (q[:, 3] < 0).any()
    p = np.roll(q, 17, axis=0).copy()
    a, b = pp.SO3(torch.tensor(q)), pp.SO3(torch.tensor(p))
    ra, rb = Rotation.from_quat(q), Rotation.from_quat(p)

    def same_rotation(got, want, tag):  # quaternions up to sign
        got, want = got.tensor().numpy(), want.as_quat()
        s = np.sign((got * want).sum(-1, keepdims=True))
        err = np.abs(got - s * want).max()
        print(f"{tag}: {err:.3g}")
        assert err <= 1e-12, (tag, err)

    def same(got, want, tag):
        err = np.abs(np.asarray(got) - want).max()
        print(f"{tag}: {err:.3g}")
        assert err <= 1e-12, (tag, err)

    same_rotation(a * b, ra * rb, "product")
    same_rotation(a @ b, ra * rb, "matmul")
    # not only the same rotation: the Hamilton product itself, (x, y, z, w), sign and all
    x1, y1, z1, w1 = q.T
    x2, y2, z2, w2 = p.T
    ham = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                    w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], 1)
    same((a * b).tensor().numpy(), ham, "Hamilton product")
    same_rotation(a.Inv(), ra.inv(), "inverse")
    same(a.matrix().numpy(), ra.as_matrix(), "matrix")
    same(a.Log().tensor().numpy(), ra.as_rotvec(), "Log")
    same(a.Log().tensor().numpy(), rotvec, "Log against the angles drawn")
    same_rotation(pp.so3(torch.tensor(rotvec)).Exp(), Rotation.from_rotvec(rotvec), "Exp")
    assert bool((pp.so3(torch.tensor(rotvec)).Exp().tensor()[:, 3] >= 0).all())
    same((0.5 * a).tensor().numpy(), 0.5 * q, "scalar *")
    same((a / 2.0).tensor().numpy(), q / 2.0, "scalar /")
    same(pp.identity_SO3(3, 2).numpy(), np.broadcast_to([0.0, 0, 0, 1], (3, 2, 4)), "identity")
    assert isinstance(a[3:5], pp.LieTensor) and isinstance(a, pp.LieTensor) and type(a.Log()) is pp.so3Tensor
    # pytorch3d: (w, x, y, z)
    wxyz = torch.tensor(q[:, [3, 0, 1, 2]])
    same(pp.quaternion_to_matrix(wxyz).numpy(), ra.as_matrix(), "quaternion_to_matrix")
    same(pp.quaternion_to_matrix(3.0 * wxyz).numpy(), ra.as_matrix(), "quaternion_to_matrix of 3 q")
    back = pp.matrix_to_quaternion(torch.tensor(ra.as_matrix()))
    same_rotation(pp.SO3(back[:, [1, 2, 3, 0]]), ra, "matrix_to_quaternion")
    # the sign is the chosen candidate's: its own squared component is the positive one
    which = torch.tensor(np.abs(q[:, [3, 0, 1, 2]])).argmax(-1)
    assert bool((back.gather(1, which[:, None]) > 0).all())
    # faces_normals_list
    v = torch.tensor(np.random.default_rng(6).normal(size=(5, 3)))
    f = torch.tensor([[0, 1, 2], [2, 1, 3], [4, 0, 3]])
    n = pp.Meshes(verts=[v], faces=[f]).faces_normals_list()[0].numpy()
    vn = v.numpy()
    want = np.cross(vn[f[:, 1]] - vn[f[:, 0]], vn[f[:, 2]] - vn[f[:, 0]])
    same(n, want / np.linalg.norm(want, axis=1, keepdims=True), "faces_normals_list")


def test_standins_in_float32():
    """dtype-generic: float32 in, float32 out, within float32 rounding of the float64 result."""
    from golden import standins as pp

    q, rotvec = _standin_quats()
    a64, a32 = pp.SO3(torch.tensor(q)), pp.SO3(torch.tensor(q).float())
    for name, f in (("Log", lambda a: a.Log().tensor()), ("matrix", lambda a: a.matrix()),
                    ("product", lambda a: (a * a.Inv() * a).tensor())):
        got = f(a32)
        assert got.dtype == torch.float32 and rel(got, f(a64)) < 1e-6, name
    e = pp.so3(torch.tensor(rotvec).float()).Exp().tensor()
    assert e.dtype == torch.float32 and rel(e, pp.so3(torch.tensor(rotvec)).Exp().tensor()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# ARAP


@pytest.mark.parametrize("name", ARAP_MESHES)
def test_arap_fixture_shapes_what_it_should(name):
    z = fixture("arap")
    verts, faces = z[f"{name}_verts"], z[f"{name}_faces"]
    ii, jj, nn = (z[f"{name}_{k}"] for k in ("ii", "jj", "nn"))
    counts = torch.bincount(ii, minlength=len(verts))
    assert int(counts.min()) > 0  # no isolated vertex
    directed = faces.flatten() * len(verts) + faces[:, [1, 2, 0]].flatten()
    assert len(torch.unique(directed)) == len(directed)  # no repeated directed edge
    w = z[f"{name}_weights_f32"][ii, nn]
    if name != "tetrahedron":
        assert bool((w < 0).any())  # an obtuse corner
    if name == "icosphere1":
        assert sorted(set(counts.tolist())) == [5, 6] and len(verts) == 42
    if name == "fan40":
        assert int(counts[0]) == 40 and int(counts.max()) == 40
    if name == "sliver":
        fv = verts[faces[-1]].double()
        A, B, C = (fv[1] - fv[2]).norm(), (fv[0] - fv[2]).norm(), (fv[0] - fv[1]).norm()
        s = 0.5 * (A + B + C)
        assert 0 <= float(s * (s - A) * (s - B) * (s - C)) < 1e-12  # under the clamp
    # the rotations are rotations, and rot_q is matrix_to_quaternion of them up to sign and float32 rounding
    R, q = z[f"{name}_rot"], z[f"{name}_rot_q"]
    assert rel(R @ R.transpose(-1, -2), torch.eye(3, dtype=D).expand_as(R)) < 1e-6
    back, _ = mesh_ref.matrix_to_quaternion(R.reshape(-1, 3, 3))
    back = back[:, [1, 2, 3, 0]].reshape(q.shape)
    sign = torch.sign((back * q).sum(-1, keepdim=True))
    assert rel(sign * back, q.double()) < 1e-6
    assert torch.equal(dyn_ref.qmatrix(q.double()), R)
    null_is_usable(z, f"{name}_", ("energy", "dvert_xyz", "dvert_rot", "dvert_rot_q", "weights"))


@pytest.mark.parametrize("name", ARAP_MESHES)
def test_arap_restatement(name):
    """dense_cot_weights, one_rings and arap_energy_reference in float64 against ARAPCoach in float64: the weights
    per directed edge (the reference's ring order is a Python set's, the restatement's is sorted: matched by (i, j)),
    the energies and both gradients.  Measured: weights 0 (bitwise), energy <= 1.9e-16, gradients <= 1.6e-16."""
    z = fixture("arap")
    verts, faces = z[f"{name}_verts"], z[f"{name}_faces"]
    V = len(verts)
    ii, jj, nn = (z[f"{name}_{k}"] for k in ("ii", "jj", "nn"))
    rings = arap_ref.one_rings(faces, V)
    mine = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(rings[0], rings[1]))}
    theirs = {(int(i), int(j)) for i, j in zip(ii, jj)}
    assert set(mine) == theirs and len(ii) == len(rings[0])
    order = torch.tensor([mine[(int(i), int(j))] for i, j in zip(ii, jj)])
    W = arap_ref.dense_cot_weights(verts.double(), faces)
    w_ref = z[f"{name}_weights_f64"][ii, nn]
    close(W[ii, jj], w_ref, OUT_BAR, f"{name} weights")
    w = W[rings[0], rings[1]]
    assert torch.equal(w[order], W[ii, jj])
    got = arap_ref.evaluate(D, z[f"{name}_xyz"], z[f"{name}_rot"], verts, rings, w, z[f"{name}_up"])
    close(got["energy"], z[f"{name}_energy_f64"], OUT_BAR, f"{name} energy")
    for k in ("dvert_xyz", "dvert_rot"):
        close(got[k], z[f"{name}_{k}_f64"], GRAD_BAR, f"{name} {k}")
    # the quaternion form of the restatement is the same function of the same rotations
    gq = arap_ref.evaluate(D, z[f"{name}_xyz"], z[f"{name}_rot_q"], verts, rings, w, z[f"{name}_up"])
    close(gq["energy"], z[f"{name}_energy_f64"], OUT_BAR, f"{name} energy (quaternions)")
    close(gq["dvert_xyz"], z[f"{name}_dvert_xyz_f64"], GRAD_BAR, f"{name} dvert_xyz (quaternions)")
    close(gq["dvert_rot"], z[f"{name}_dvert_rot_q_f64"], GRAD_BAR, f"{name} dvert_rot (quaternions)")


@pytest.mark.parametrize("name", ARAP_MESHES)
def test_arap_binding_weights_are_bitwise_the_reference_dense_branch(name):
    """ArapBinding(verts, faces) on the CPU: the same directed edges as ARAPCoach's (ii, jj), and for every one bitwise
    the float32 ``edge_cot_weights[ii, nn]`` that ``produce_cot_weights_nfmt(sparse=False)`` itself computed."""
    from sugar_arap import ArapBinding

    z = fixture("arap")
    verts, faces = z[f"{name}_verts"], z[f"{name}_faces"]
    b = ArapBinding(verts, faces)
    ii, jj, nn = (z[f"{name}_{k}"] for k in ("ii", "jj", "nn"))
    row = torch.repeat_interleave(torch.arange(b.n_verts), (b.offsets[1:] - b.offsets[:-1]).long())
    mine = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(row, b.nbr))}
    assert len(mine) == b.n_edges == len(ii) and set(mine) == {(int(i), int(j)) for i, j in zip(ii, jj)}
    order = torch.tensor([mine[(int(i), int(j))] for i, j in zip(ii, jj)])
    want = z[f"{name}_weights_f32"][ii, nn]
    assert b.w.dtype == want.dtype == torch.float32
    assert torch.equal(b.w[order], want)  # bitwise
    assert b.max_valence == z[f"{name}_weights_f32"].shape[1]
    # the padding of the reference's table is zero
    pad = torch.ones_like(z[f"{name}_weights_f32"], dtype=torch.bool)
    pad[ii, nn] = False
    assert not z[f"{name}_weights_f32"][pad].any()


@pytest.mark.parametrize("name", ARAP_MESHES)
def test_arap_energy_at_rest_is_exactly_zero(name):
    z = fixture("arap")
    assert float(z[f"{name}_rest_energy_f64"]) == 0.0 and float(z[f"{name}_rest_energy_f32"]) == 0.0
    verts, faces = z[f"{name}_verts"], z[f"{name}_faces"]
    V = len(verts)
    rings = arap_ref.one_rings(faces, V)
    w = arap_ref.dense_cot_weights(verts.double(), faces)[rings[0], rings[1]]
    for rot in (torch.eye(3, dtype=D).expand(1, V, 3, 3), torch.tensor([0.0, 0, 0, 1], dtype=D).expand(1, V, 4)):
        e = arap_ref.arap_energy_reference(verts.double()[None], rot, verts, *rings, w)
        assert e.shape == (1,) and float(e) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# skinning and timed Gaussians


def skin_restated(dtype, z, K, method):
    ups = {k: z[f"skin_K{K}_up_{n}"] for k, n in (("xyz", "xyz"), ("rot", "rotation"), ("scale", "scale"))}
    inputs = dict(verts=z["skin_verts"], node_trans=z["skin_node_trans"], node_rots=z["skin_node_rots"],
                  node_scales=z["skin_node_scales"])
    r = dyn_ref.evaluate_skin(dtype, inputs, z["skin_node_xyz"], z[f"skin_K{K}_nbr"], z[f"skin_K{K}_w"], method, ups)
    r["rotation"] = r.pop("rot")
    return r


def test_skin_fixture_shapes_what_it_should():
    z = fixture("dynamic")
    assert z["skin_verts"].shape == (42, 3) and z["skin_node_rots"].shape == (3, 7, 4)
    q = z["skin_node_rots"]
    assert q.dtype == D and rel(q.norm(dim=-1), torch.ones(3, 7, dtype=D)) < 1e-15
    angle = 2 * torch.atan2(q[..., :3].norm(dim=-1), q[..., 3].abs())
    assert float(angle.max()) > 2.5 and float(angle.max()) <= 3.0 and (q[..., 3] > 0).any() and (q[..., 3] < 0).any()
    assert float(z["skin_node_trans"].abs().max()) > 1.0  # of the mesh's size
    nbr = z["skin_K4_nbr"]
    assert bool((nbr == 0).any(-1).all()) and not (nbr == 5).any() and not (z["skin_K1_nbr"] == 5).any()
    for K in (1, 4):
        for method in ("lbs", "dqs"):
            null_is_usable(z, f"skin_K{K}_{method}_", SKIN_KEYS)


@pytest.mark.parametrize("method", ["lbs", "dqs"])
@pytest.mark.parametrize("K", [1, 4])
def test_skin_restatement(K, method):
    """skin_vertices_reference in float64 against _get_timed_vertex_attributes_from_dg in float64.

    Quaternions compare as tests/test_gpu_sugar_dynamic.py compares them: exactly, no sign alignment (Exp gives
    w = cos(theta / 2) on both sides).  Measured: outputs 0 (bitwise); gradients <= 3.6e-16 (dnode_rots after the
    projection below).

    dnode_rots is compared after removing its component along the quaternion.  The reference's LBS branch feeds
    ``neighbor_nodes_rots.matrix()`` the quaternion as it is, the header (and the restatement, and the kernel)
    normalises it first (``qhat``); on unit quaternions the values agree, but the derivative along the quaternion's
    norm is 0 for the header's formula and 2 (R - I) p for an unnormalised ``matrix()``.  That component is exactly the
    behaviour off the unit sphere, which is pinned to the header alone: the stand-in's ``matrix()``
    cannot speak for pypose there.  Measured without the projection: lbs 0.66 (K = 1), 0.67 (K = 4); dqs, whose
    from_quat_pose_array normalises by plain division, agrees unprojected to 2.1e-16 -- asserted."""
    z = fixture("dynamic")
    got = skin_restated(D, z, K, method)
    q = z["skin_node_rots"]
    for k in SKIN_KEYS:
        want, have = z[f"skin_K{K}_{method}_{k}_f64"], got[k]
        if k == "dnode_rots":
            print(f"K={K} {method} dnode_rots before the projection: {rel(have, want):.3g}")
            if method == "dqs":
                close(have, want, GRAD_BAR, f"K={K} {method} {k} unprojected")
            want, have = tangent(want, q), tangent(have, q)
        close(have, want, GRAD_BAR if k.startswith("d") else OUT_BAR, f"K={K} {method} {k}")


def timed_restated(dtype, z, G):
    ups = {k: z[f"timed_G{G}_up_{n}"] for k, n in (("xyz", "xyz"), ("rotation", "rotation"), ("scaling", "scale"))}
    inputs = dict(vert_xyz=z["timed_vert_xyz"], vert_rot=z["timed_vert_rot"], rotation0=z[f"timed_G{G}_rotation0"],
                  vert_scale=z["timed_vert_scale"], log_scales=z[f"timed_G{G}_log_scales"])
    r = dyn_ref.evaluate_timed(dtype, inputs, z["timed_faces"], z[f"timed_G{G}_bary"], float(z["timed_thickness"]), ups)
    r["scale"] = r.pop("scaling")
    return r


def test_timed_fixture_shapes_what_it_should():
    z = fixture("dynamic")
    assert z["timed_faces"].shape == (20, 3) and z["timed_vert_rot"].shape == (3, 12, 4)
    for q in (z["timed_vert_rot"], z["timed_G1_rotation0"], z["timed_G3_rotation0"]):
        assert q.dtype == D and rel(q.norm(dim=-1), torch.ones(q.shape[:-1], dtype=D)) < 1e-15
    q = z["timed_vert_rot"]
    assert (q[..., 3] > 0).any() and (q[..., 3] < 0).any()
    for G in (1, 3):
        assert z[f"timed_G{G}_rotation0"].shape == (20 * G, 4)
        null_is_usable(z, f"timed_G{G}_", TIMED_KEYS)


@pytest.mark.parametrize("G", [1, 3])
def test_timed_restatement(G):
    """timed_gaussians_reference in float64 against get_timed_gs_attributes (with fuse_rotations and
    _get_gs_xyz_from_vertex) in float64: positions, (w, x, y, z) rotations compared exactly as
    tests/test_gpu_sugar_dynamic.py compares them, scales, and the five gradients.  The gradients to vert_rot and
    rotation0 are whole: Log does not depend on the norm, and the product's result is normalised on both sides.
    Measured: outputs 0 (bitwise), gradients <= 3.9e-16."""
    z = fixture("dynamic")
    got = timed_restated(D, z, G)
    for k in TIMED_KEYS:
        close(got[k], z[f"timed_G{G}_{k}_f64"], GRAD_BAR if k.startswith("d") else OUT_BAR, f"G={G} {k}")


# ---------------------------------------------------------------------------------------------------------------------
# mesh-bound Gaussians


def mesh_restated(dtype, z, G, sign=None):
    ups = {k: z[f"G{G}_up_{k}"] for k in mesh_ref.OUTPUTS}
    return mesh_ref.evaluate(dtype, z["verts"], z["faces"], z[f"G{G}_bary"], z[f"G{G}_complex"], z[f"G{G}_log_scales"],
                             float(z["thickness"]), ups, sign=sign)


@pytest.mark.parametrize("G", [1, 3])
def test_mesh_fixture_shapes_what_it_should(G):
    z = fixture("mesh")
    assert z["faces"].shape == (20, 3) and z[f"G{G}_complex"].shape == (20 * G, 2)
    null_is_usable(z, f"G{G}_", mesh_ref.OUTPUTS + tuple("d" + k for k in mesh_ref.GRADS))
    # scaling's thickness column is a constant on both sides; its other columns carry the null
    assert rel(z[f"G{G}_scaling_f32"][:, 1:], z[f"G{G}_scaling_f64"][:, 1:]) > 0
    assert float(z[f"G{G}_log_scales"].std()) > 0.1 and float(z["thickness"]) == 3.5e-6


@pytest.mark.parametrize("G", [1, 3])
def test_mesh_restatement(G):
    """bound_gaussians_reference in float64 against the points, scaling, quaternions and get_gs_normals property
    bodies of SuGaRModel in float64 (bound branch).  The quaternion rows compare as tests/test_gpu_sugar_mesh.py
    compares them, through ``row_sign``; here every sign is +1 (asserted): the restatement takes pytorch3d's candidate.
    Measured: outputs 0 (bitwise), gradients <= 3.9e-16.

    A deliberate deviation that the fixture stays off: the header normalises the face normal twice (eps 1e-6, then
    1e-12) where pytorch3d's faces_normals_list and the reference's F.normalize do the same; and where the reference's
    ``normalize(cross(R_0, base_R_1))`` has no ``dim`` (so dim=1, the same axis for (F, 3)).  Every face of the
    fixture has an area far above 1e-6 (asserted), so no clamp acts."""
    z = fixture("mesh")
    fv = z["verts"][z["faces"]].double()
    assert float(torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]).norm(dim=-1).min()) > 1e-2
    want = mesh_fixture(z, G, "f64")
    got = mesh_restated(D, z, G)
    s = mesh_ref.row_sign(got["rotation"], want["rotation"])
    assert bool((s > 0).all())
    for k in MESH_KEYS:
        close(got[k], want[k], GRAD_BAR if k in mesh_ref.GRADS else OUT_BAR, f"G={G} {k}")


# ---------------------------------------------------------------------------------------------------------------------
# density field and neighbour-normal loss


def field_inputs(z, K, run):
    """The float32 tensors get_field_values was run on: Gaussians' inv_sr is the reference's own float32 one."""
    s = z[f"K{K}_strengths_w"] if run == "w" else z["strengths"]
    return dict(x=z["x"], centers=z["points"], inv_sr=z["inv_sr_f32"], strengths=s[:, 0],
                min_scale=z["scaling"].min(-1)[0])


def test_field_fixture_shapes_what_it_should():
    z = fixture("field")
    assert z["points"].shape == (200, 3) and z["x"].shape == (65, 3) and z["knn_idx"].shape == (200, 16)
    sc = z["scaling"]
    assert float(sc.max() / sc.min()) > 60  # two decades
    assert rel(z["quaternions"].norm(dim=-1), torch.ones(200)) > 0.1  # quaternion_to_matrix normalises: not unit
    for K in (1, 16):
        d = z[f"K{K}_a_density_f64"]
        assert int((d >= 1).sum()) >= 5 and int((d < 1e-16).sum()) >= 1 and int((d == 0).sum()) == 1  # both branches
        if K == 1:  # under the clamp without being 0 (at K = 16 the far samples still see a wide neighbour)
            assert int(((d > 0) & (d < 1e-16)).sum()) == 4
        assert bool(((z[f"K{K}_a_density_f32"] >= 1) == (d >= 1)).all())
        assert float(z[f"K{K}_w_density_f64"].max()) < 1 and float(z[f"K{K}_w_density_f32"].max()) < 1
        assert int((z[f"K{K}_w_density_f64"] < 1e-16).sum()) >= 1
        for run in FIELD_RUNS:
            keys = [k for k in field_keys(run) if not (K == 1 and run == "a" and k == "beta")]
            null_is_usable(z, f"K{K}_{run}_", keys)
        # K = 1, average: beta is a copy of one float32 scale, the null is exactly 0 and the kernel must be exact
        null_is_usable(z, f"K{K}_normal_", ("loss", "dnormals"))
    assert torch.equal(z["K1_a_beta_f32"].double(), z["K1_a_beta_f64"])
    null_is_usable(z, "", ("inv_sr", "cov_full", "normals"))
    assert z["cov6_f64"].dtype == torch.float32  # the reference's torch.zeros(..., dtype=torch.float)


def test_covariance_and_smallest_axis_restated():
    """get_covariance (the inverse scaled rotation R(q) diag(1 / clamp(s, 1e-8)), the full matrix L L^T and its six
    upper entries) and get_smallest_axis against the short restatements the field and normal tests build their scenes
    with (sugar_cases._quat_to_matrix) and sugar_field.smallest_axis.  cov6 is float32 in the reference
    whatever the dtype of its inputs (``torch.zeros(..., dtype=torch.float)`` in get_covariance): the float64 run's
    cov6 is the float64 matrix rounded to float32, one float32 rounding: measured gap 3.0e-8 of the largest entry
    (2^-25); the bar is 4 x 2^-24, four times the format's bound for one rounding."""
    import sugar_field

    z = fixture("field")
    Rm = _quat_to_matrix(z["quaternions"].double())
    sc = z["scaling"].double()
    close(Rm * (1 / sc.clamp(min=1e-8))[:, None], z["inv_sr_f64"], OUT_BAR, "inv_sr")
    L = Rm * sc[:, None]
    cov = L @ L.transpose(-1, -2)
    close(cov, z["cov_full_f64"], OUT_BAR, "cov_full")
    six = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], -1)
    gap = rel(six, z["cov6_f64"])
    print(f"cov6: {gap:.3g}")
    assert gap <= 4 * 2.0 ** -24
    idx = sc.min(dim=-1)[1][..., None, None].expand(-1, 3, -1)
    close(Rm.gather(2, idx).squeeze(2), z["normals_f64"], OUT_BAR, "smallest axis")
    lib = sugar_field.smallest_axis(z["quaternions"], z["scaling"])  # the library's, float32 only
    err, null = rel(lib, z["normals_f64"]), rel(z["normals_f32"], z["normals_f64"])
    print(f"sugar_field.smallest_axis: {err:.3g}  fp32 null {null:.3g}")
    assert lib.dtype == torch.float32 and err <= 2 * null
    assert torch.equal(z["normals_idx_f64"], sc.min(-1)[1]) and torch.equal(z["normals_idx_f32"], sc.min(-1)[1])


@pytest.mark.parametrize("run", sorted(FIELD_RUNS))
@pytest.mark.parametrize("K", [1, 16])
def test_field_restatement(K, run):
    """The field checker ``_field`` and the composition ``_compose64`` of tests/sugar_cases.py in float64
    against get_field_values + get_beta in float64, on the same float32 inputs.  Outputs of all three runs; for run
    "l" (density and the learnable beta) also the gradients to x, points, inv_sr and strengths by ``_run``.  The
    gradients of run "w" pass through sdf and the weighted beta, for which the project has no differentiable CPU
    restatement (``_compose64`` is forward only): they are pinned on the GPU side only.
    Measured: every output and gradient 0 (bitwise: the checker runs the reference's operations in its order)."""
    z = fixture("field")
    mode, df, sdf_on, want_op = FIELD_RUNS[run]
    inp = field_inputs(z, K, run)
    idx = z["knn_idx"][z["gaussian_idx"]][:, :K]
    ok = _mask(idx, 200)
    i64 = {k: v.double() for k, v in inp.items()}
    op, den, beta_avg = _field(i64["x"], idx, ok, i64["centers"], i64["inv_sr"], i64["strengths"], i64["min_scale"], df)
    dens, beta, t, sdf = _compose64(den, op, beta_avg, i64["min_scale"][idx], mode, z["log_beta"], 0.7, 1e-16)
    want = {k: z[f"K{K}_{run}_{k}_f64"] for k in field_keys(run)}
    close(den, want["density"], OUT_BAR, f"K={K} {run} density")
    close(beta.contiguous(), want["beta"], OUT_BAR, f"K={K} {run} beta")
    if want_op:
        close(op, want["closest_gaussian_opacities"], OUT_BAR, f"K={K} {run} opacities")
    if sdf_on:
        close(sdf, want["sdf"], OUT_BAR, f"K={K} {run} sdf")
    if run == "l":
        res = _run(D, inp, idx, ok, df, (None, z[f"K{K}_up_density"], None))
        for k, g in zip(("x", "points", "inv_sr", "strengths"), res[3:7]):
            g = g[:, None] if k == "strengths" else g
            close(g, want["d" + k], GRAD_BAR, f"K={K} {run} d{k}")
        assert not want["dscaling"].any() and want["dlog_beta"].any()
        up = z[f"K{K}_up_beta"]
        close((torch.exp(z["log_beta"].double()) * up.sum()), want["dlog_beta"], GRAD_BAR, f"K={K} l dlog_beta")


@pytest.mark.parametrize("K", [1, 16])
def test_normal_restatement(K):
    """The normal checker ``_normal`` of tests/sugar_cases.py in float64, in both of its arrangements,
    against the body of ``if use_sdf_better_normal_loss:`` in float64: the per-sample loss and the gradient to the
    normals (run a's float32 opacities, the reference's float32 smallest axes).  Measured: 0 (bitwise) as the
    reference writes the sum, 2.1e-16 in the checker's other arrangement."""
    z = fixture("field")
    own = z["gaussian_idx"]
    idx = z["knn_idx"][own][:, :K]
    inp = dict(x=z["x"], centers=z["points"], normals=z["normals_f32"], min_scale=z["scaling"].min(-1)[0],
               op=z[f"K{K}_a_closest_gaussian_opacities_f32"])
    for literal in (True, False):
        got = _normal(D, inp, idx, own, _mask(idx, 200), torch.ones(65, dtype=torch.bool), z[f"K{K}_up_normal"],
                      literal=literal)
        close(got["loss"], z[f"K{K}_normal_loss_f64"], OUT_BAR, f"K={K} normal loss (literal={literal})")
        close(got["dnormals"], z[f"K{K}_normal_dnormals_f64"], GRAD_BAR, f"K={K} dnormals (literal={literal})")
    close(z[f"K{K}_normal_loss_f64"].mean(), z[f"K{K}_normal_mean_f64"], OUT_BAR, "mean")
