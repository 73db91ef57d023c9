"""The fused SuGaR kernels on the GPU against fixtures computed by the reference's own code (tests/golden/*.npz, made by
tests/golden/make_golden.py and read by ``fixture`` of tests/sugar_cases.py; what is lifted and how:
tests/test_reference_pins.py, which pins the torch restatements to the same fixtures on the CPU).

Bar, the one of the geometry stages' own GPU tests (``_rel`` and ``check_against_null`` of tests/sugar_cases.py and the
energy rule, ``check_arap`` of tests/sugar_arap_reference.py, are imported, not copied): per tensor
max |gpu - ref_f64| / max |ref_f64| <= 2 x the same figure of ``*_f32`` against ``*_f64``, both read from the fixture,
so the null is the reference's own float32 run; exact zeros where the reference tensor is all zero; per frame of the
ARAP energy max(2 x null, 2^-23).  Each check prints its two figures.
Inputs stored in float64 (the unit quaternions) reach the kernels rounded to float32, as they reached the reference's
float32 run.
"""
import pytest

torch = pytest.importorskip("torch")

import sugar_mesh_reference as mesh_ref  # noqa: E402
from sugar_arap_reference import ARAP_MESHES, check_arap  # noqa: E402
from sugar_cases import (FIELD_LEAVES, FIELD_RUNS, _rel, backprop, check_against_null, field_keys,  # noqa: E402
                         fixture)
from sugar_dynamic_reference import SKIN_KEYS, TIMED_KEYS, tangent  # noqa: E402
from sugar_mesh_reference import MESH_KEYS, mesh_fixture  # noqa: E402

F32 = torch.float32


def _leaf(t):
    return t.to(F32).cuda().requires_grad_()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["matrix", "quat"])
@pytest.mark.parametrize("name", ARAP_MESHES)
def test_arap_energy(name, form):
    """arap_energy with the binding's own weights against ARAPCoach.compute_arap_energy with its own.  The quaternion
    form is fed ``rot_q``, the float32 quaternions whose matrices (pypose's formula, float64) the reference was given;
    its rotation gradient is the fixture's ``dvert_rot_q``: autograd through the stand-in's ``matrix()`` into the
    reference's energy, in make_golden.py."""
    from sugar_arap import ArapBinding, arap_energy

    z = fixture("arap")
    refs = [{k: z[f"{name}_{k}_{tag}"] for k in ("energy", "dvert_xyz", "dvert_rot")} for tag in ("f64", "f32")]
    if form == "quat":
        for r, tag in zip(refs, ("f64", "f32")):
            r["dvert_rot"] = z[f"{name}_dvert_rot_q_{tag}"]
    x = _leaf(z[f"{name}_xyz"])
    r = _leaf(z[f"{name}_rot"] if form == "matrix" else z[f"{name}_rot_q"])
    e = arap_energy(x, r, ArapBinding(z[f"{name}_verts"], z[f"{name}_faces"]).to("cuda"))
    got = backprop([e], ["energy"], [x, r], ["dvert_xyz", "dvert_rot"], {"energy": z[f"{name}_up"].to(F32)}, ["energy"])
    check_arap(got, *refs, f"{name} {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lbs", "dqs"])
@pytest.mark.parametrize("K", [1, 4])
def test_skin_vertices(K, method):
    """For "lbs", dnode_rots is compared without its component along the quaternion, on all three sides: see
    tests/test_reference_pins.py::test_skin_restatement."""
    from sugar_dynamic import SkinBinding, skin_vertices

    z = fixture("dynamic")
    binding = SkinBinding(z[f"skin_K{K}_nbr"], z[f"skin_K{K}_w"], 7).to("cuda")
    leaves = [_leaf(z[k]) for k in ("skin_verts", "skin_node_trans", "skin_node_rots", "skin_node_scales")]
    out = skin_vertices(leaves[0], z["skin_node_xyz"].cuda(), leaves[1], leaves[2], binding, method, leaves[3])
    names = SKIN_KEYS[:3]
    got = backprop(out, names, leaves, SKIN_KEYS[3:], {k: z[f"skin_K{K}_up_{k}"].to(F32) for k in names}, names)
    r64, r32 = ({k: z[f"skin_K{K}_{method}_{k}_{tag}"] for k in SKIN_KEYS} for tag in ("f64", "f32"))
    if method == "lbs":
        for d in (got, r64, r32):
            d["dnode_rots"] = tangent(d["dnode_rots"], z["skin_node_rots"])
    check_against_null(got, r64, r32, SKIN_KEYS, f"skin K={K} {method}")


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3])
def test_timed_gaussians(G):
    from sugar_dynamic import timed_gaussians
    from sugar_mesh import MeshBinding

    z = fixture("dynamic")
    binding = MeshBinding(z["timed_faces"], 12, z[f"timed_G{G}_bary"]).to("cuda")
    leaves = [_leaf(z[k]) for k in ("timed_vert_xyz", "timed_vert_rot", f"timed_G{G}_rotation0", "timed_vert_scale",
                                    f"timed_G{G}_log_scales")]
    thickness = float(z["timed_thickness"])
    xyz, rotation, normals, scaling = timed_gaussians(leaves[0], leaves[1], leaves[2], binding, leaves[3], leaves[4],
                                                      thickness)
    names = TIMED_KEYS[:3]
    got = backprop((xyz, rotation, scaling), names, leaves, TIMED_KEYS[3:],
                   {k: z[f"timed_G{G}_up_{k}"].to(F32) for k in names}, names)
    r64, r32 = ({k: z[f"timed_G{G}_{k}_{tag}"] for k in TIMED_KEYS} for tag in ("f64", "f32"))
    check_against_null(got, r64, r32, TIMED_KEYS, f"timed G={G}")
    assert torch.equal(got["scale"][..., 0], torch.full(got["scale"].shape[:2], thickness, dtype=F32))
    assert torch.isfinite(normals).all()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3])
def test_bound_gaussians(G):
    """The quaternion rows are compared as they are: no row of the fixture sits at a tie between two candidates of
    matrix_to_quaternion, so the kernel must take the reference's (asserted through ``row_sign``)."""
    from sugar_mesh import MeshBinding, bound_gaussians

    z = fixture("mesh")
    binding = MeshBinding(z["faces"], len(z["verts"]), z[f"G{G}_bary"]).to("cuda")
    leaves = [_leaf(z[k]) for k in ("verts", f"G{G}_complex", f"G{G}_log_scales")]
    thickness = float(z["thickness"])
    out = bound_gaussians(*leaves, binding, thickness)
    ups = {k: z[f"G{G}_up_{k}"].to(F32) for k in mesh_ref.OUTPUTS}
    got = backprop(out, mesh_ref.OUTPUTS, leaves, mesh_ref.GRADS, ups, mesh_ref.OUTPUTS)
    r64, r32 = mesh_fixture(z, G, "f64"), mesh_fixture(z, G, "f32")
    for d in (got, r32):
        assert bool((mesh_ref.row_sign(d["rotation"], r64["rotation"]) > 0).all())
    check_against_null(got, r64, r32, MESH_KEYS, f"bound G={G}")
    assert torch.equal(got["scaling"][:, 0], torch.full((20 * G,), thickness, dtype=F32))
    assert _rel(got["xyz"], r64["xyz"]) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("run", sorted(FIELD_RUNS))
@pytest.mark.parametrize("K", [1, 16])
def test_field_values(K, run):
    """neighbor_density and get_field_values against SuGaRRegularizer.get_field_values + get_beta: the three runs of
    the fixture (tests/golden/make_golden.py make_field_reference: every beta mode, return_sdf on and off, opacities on
    and off, density_factor 1 and 1.3, samples in the normalisation branch and under the clamp), outputs, and for runs
    "w" and "l" the gradients to x, points, inv_scaled_rotation, strengths, scaling and log_beta.  K = 1, run "a":
    beta copies one float32 scale, the null is 0 and the result must be exact."""
    from sugar_field import get_field_values, neighbor_density

    z = fixture("field")
    mode, df, sdf_on, want_op = FIELD_RUNS[run]
    arrays = dict(x=z["x"], points=z["points"], inv_sr=z["inv_sr_f32"],
                  strengths=z[f"K{K}_strengths_w"] if run == "w" else z["strengths"], scaling=z["scaling"],
                  log_beta=z["log_beta"])
    leaves = {k: _leaf(arrays[k]) for k in FIELD_LEAVES}
    index = dict(knn_idx=z["knn_idx"][:, :K].contiguous().cuda(), gaussian_idx=z["gaussian_idx"].cuda())
    fields = get_field_values(
        leaves["x"], points=leaves["points"], inv_scaled_rotation=leaves["inv_sr"], strengths=leaves["strengths"],
        scaling=leaves["scaling"], beta_mode=mode, log_beta=leaves["log_beta"], return_sdf=sdf_on,
        density_threshold=float(z["density_threshold"]), density_factor=df,
        return_closest_gaussian_opacities=want_op, return_beta=True, **index)
    keys = field_keys(run)
    assert set(fields) == set(field_keys(run, grads=False))
    got = {k: fields[k].detach().cpu() for k in fields}
    if run != "a":
        loss = sum((fields[k] * z[f"K{K}_up_{k}"].to(F32).cuda()).sum() for k in fields)
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        got.update({"d" + k: (torch.zeros_like(l) if g is None else g).cpu()
                    for (k, l), g in zip(leaves.items(), grads)})
    r64, r32 = ({k: z[f"K{K}_{run}_{k}_{tag}"] for k in keys} for tag in ("f64", "f32"))
    check_against_null(got, r64, r32, keys, f"field K={K} {run}")
    if run == "a":  # the fused op by itself
        den, beta_avg, op = neighbor_density(leaves["x"], leaves["points"], leaves["inv_sr"], leaves["strengths"],
                                             leaves["scaling"].min(dim=-1)[0], density_factor=df,
                                             return_opacities=True, **index)
        direct = {"density": den.detach().cpu(), "beta": beta_avg.detach().cpu(),
                  "closest_gaussian_opacities": op.detach().cpu()}
        check_against_null(direct, r64, r32, tuple(direct), f"neighbor_density K={K}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 16])
def test_neighbor_normal_loss(K):
    """neighbor_normal_loss against the body of ``if use_sdf_better_normal_loss:``: the per-sample loss and the
    gradient to the normals, in both forms of the neighbour table."""
    from sugar_field import neighbor_normal_loss

    z = fixture("field")
    r64, r32 = ({"loss": z[f"K{K}_normal_loss_{tag}"], "dnormals": z[f"K{K}_normal_dnormals_{tag}"]}
                for tag in ("f64", "f32"))
    own = z["gaussian_idx"].cuda()
    tables = (dict(knn_idx=z["knn_idx"][:, :K].contiguous().cuda()),
              dict(closest_gaussians_idx=z["knn_idx"][z["gaussian_idx"]][:, :K].contiguous().cuda()))
    for table in tables:
        normals = _leaf(z["normals_f32"])
        loss = neighbor_normal_loss(z["x"].cuda(), z["points"].cuda(), normals, z["scaling"].min(-1)[0].cuda(),
                                    z[f"K{K}_a_closest_gaussian_opacities_f32"].cuda(), gaussian_idx=own, **table)
        (g,) = torch.autograd.grad((loss * z[f"K{K}_up_normal"].to(F32).cuda()).sum(), normals)
        check_against_null({"loss": loss.detach().cpu(), "dnormals": g.cpu()}, r64, r32, ("loss", "dnormals"),
                           f"normal K={K} {next(iter(table))}")
