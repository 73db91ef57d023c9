"""Generate the golden vectors under tests/golden/ (run in the build container, where /root/reference exists).

Two kinds of fixtures:

1. reference_*.npz — outputs of the reference's OWN pure-torch functions, lifted from the source text
   with `ast` and executed on CPU (the reference package as a whole is not importable: it needs
   threestudio/plyfile/simple_knn, absent here; these functions need only torch/numpy/math):
     eval_sh, C0..C3                 geometry/sugar.py:743-830
     build_rotation, build_scaling_rotation, strip_lowerdiag/strip_symmetric
                                     geometry/gaussian_base.py:47-134   (device="cuda" rewritten to "cpu")
     getProjectionMatrix, getWorld2View2
                                     utils/sugar_utils.py:796-829
     camera construction             geometry/sugar.py:891-896 (world_view, full_proj, camera_center)
     Depth2Normal                    renderer/diff_gaussian_rasterizer_shading.py:22-51
     GaussianDiffuseWithPointLightMaterial.forward
                                     material/gaussian_material.py:41-104 (method body; threestudio's dot
                                     supplied), composed as the shading renderer does (:169-208)
   They pin the CPU restatement's SH, covariance and projection pieces (tests/test_golden.py).
   Only inputs and outputs are written; no reference source is stored.
   The SuGaR stages likewise, each run in float32 (*_f32) and in float64 (*_f64, torch's default dtype
   switched around the run), with autograd gradients for stored upstream gradients (tests/test_reference_pins.py,
   tests/test_gpu_reference_pins.py); pypose and pytorch3d come from tests/golden/standins.py:
     ARAPCoach (whole class)         utils/arap_utils.py:16-189          -> reference_arap.npz
     _get_timed_vertex_attributes_from_dg, get_timed_gs_attributes, _get_gs_xyz_from_vertex, fuse_rotations
                                     geometry/dynamic_sugar.py:505-575, 618-688, 856-868
     DualQuaternion (whole class)    utils/dual_quaternions.py:19-252    -> reference_dynamic.npz
     SuGaRModel.points, scaling, quaternions, get_face_normals, get_gs_normals (bound branch)
                                     geometry/sugar.py:449-536           -> reference_mesh.npz
     SuGaRRegularizer (whole class: get_covariance, get_field_values, get_beta, get_smallest_axis) and the body of
     `if use_sdf_better_normal_loss:` in coarse_density_regulation
                                     utils/sugar_utils.py:79-474, 725-757 -> reference_field.npz

2. oracle_scene.npz — a small seeded scene + camera with the CPU restatement's fp64 forward outputs and
   gradients (oracle/gsr_oracle.c).  Regression fixture for the oracle and a committed target for the
   GPU parity tests.  (The reference has no rasterizer, so no reference-generated fixture exists for
   the full path: parity of the full rasterizer is unpinned by the reference)

Usage:  python tests/golden/make_golden.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def lift(path: str, names: list[str], extra_globals: dict) -> dict:
    """Execute the top-level definitions `names` from a reference source file; return its namespace."""
    src = open(path).read()
    tree = ast.parse(src)
    keep = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            keep.append(node)
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in node.targets):
            keep.append(node)
    code = ast.unparse(ast.Module(body=keep, type_ignores=[]))
    code = code.replace('device="cuda"', 'device="cpu"').replace("device='cuda'", "device='cpu'")
    ns = dict(extra_globals)
    exec(compile(code, path, "exec"), ns)  # noqa: S102 — reference pure functions, CPU only
    missing = [n for n in names if n not in ns]
    if missing:
        raise RuntimeError(f"could not lift {missing} from {path}")
    return ns


def make_reference(ref: str):
    g = {"torch": torch, "np": np, "math": math}
    sugar = lift(os.path.join(ref, "geometry/sugar.py"), ["C0", "C1", "C2", "C3", "C4", "eval_sh"], g)
    base = lift(os.path.join(ref, "geometry/gaussian_base.py"),
                ["C0", "RGB2SH", "SH2RGB", "strip_lowerdiag", "strip_symmetric", "build_rotation",
                 "build_scaling_rotation"], g)
    utils = lift(os.path.join(ref, "utils/sugar_utils.py"), ["getWorld2View2", "getProjectionMatrix", "fov2focal"], g)

    rng = np.random.default_rng(2024)
    # --- SH: eval_sh(deg, sh[..., C, coeff], dirs) at dirs = normalize(pos - campos)
    n = 64
    sh = rng.normal(0, 0.5, size=(n, 16, 3))
    pos = rng.normal(0, 1, size=(n, 3))
    campos = np.array([2.5, -0.3, 0.7])
    d = pos - campos
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = {"sh": sh, "pos": pos, "campos": campos}
    for deg in range(4):
        res = sugar["eval_sh"](deg, torch.tensor(sh).transpose(1, 2), torch.tensor(d))
        out[f"eval_sh_deg{deg}"] = res.numpy()
    rgb = rng.random((n, 3))
    out["rgb"] = rgb
    out["rgb2sh"] = base["RGB2SH"](torch.tensor(rgb)).numpy()
    np.savez_compressed(os.path.join(HERE, "reference_sh.npz"), **out)

    # --- covariance: L = R(q) S, Sigma = L L^T, upper triangle (strip_symmetric)
    scales = np.exp(rng.normal(-3, 1, size=(n, 3)))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    L = base["build_scaling_rotation"](torch.tensor(scales, dtype=torch.float32), torch.tensor(q, dtype=torch.float32))
    cov = base["strip_symmetric"](L @ L.transpose(1, 2))
    R = base["build_rotation"](torch.tensor(q, dtype=torch.float32))
    np.savez_compressed(os.path.join(HERE, "reference_cov.npz"), scales=scales, rotations=q,
                        cov3D=cov.double().numpy(), R=R.double().numpy())

    # --- projection + camera construction (geometry/sugar.py:891-896)
    cams = []
    for i in range(8):
        fovx = math.radians(rng.uniform(30, 90))
        fovy = math.radians(rng.uniform(30, 90))
        znear, zfar = 0.01 if i % 2 else 0.1, 100.0
        A = rng.normal(size=(3, 3))
        Qm, _ = np.linalg.qr(A)
        if np.linalg.det(Qm) < 0:
            Qm[:, 0] *= -1
        Rm, T = Qm, rng.normal(0, 2, size=3)
        P = utils["getProjectionMatrix"](znear=znear, zfar=zfar, fovX=fovx, fovY=fovy)
        wv = torch.tensor(utils["getWorld2View2"](Rm, T)).transpose(0, 1)
        full = (wv.unsqueeze(0).bmm(P.transpose(0, 1).unsqueeze(0))).squeeze(0)
        center = wv.inverse()[3, :3]
        # the same camera as an OpenGL camera-to-world (threestudio convention fed to get_cam_info_gaussian)
        c2w = np.linalg.inv(utils["getWorld2View2"](Rm, T).astype(np.float64))
        c2w[:3, 1:3] *= -1
        cams.append(dict(fovx=fovx, fovy=fovy, znear=znear, zfar=zfar, P=P.double().numpy(),
                         world_view=wv.double().numpy(), full_proj=full.double().numpy(),
                         center=center.double().numpy(), c2w_gl=c2w))
    np.savez_compressed(os.path.join(HERE, "reference_camera.npz"),
                        **{f"{k}_{i}": np.asarray(v) for i, c in enumerate(cams) for k, v in c.items()})


def lift_method(path: str, cls: str, method: str, extra_globals: dict):
    """One method of a reference class as a plain function (annotations stripped: the class itself needs
    threestudio; the method body needs only torch)."""
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == method)
    fn.decorator_list = []
    fn.returns = None
    for a in fn.args.args + fn.args.kwonlyargs:
        a.annotation = None
    code = ast.unparse(ast.Module(body=[fn], type_ignores=[]))
    ns = dict(extra_globals)
    exec(compile(code, path, "exec"), ns)  # noqa: S102 — reference pure method body, CPU only
    return ns[method]


def make_shading_reference(ref: str):
    """The shading renderer's post-raster epilogue from the reference's own code: Depth2Normal
    (renderer/diff_gaussian_rasterizer_shading.py:22-51) and GaussianDiffuseWithPointLightMaterial.forward
    (material/gaussian_material.py:41-104), composed as the renderer does (:169-208); threestudio's
    dot(x, y) = sum(x * y, -1, keepdim=True) is supplied.  fp64, CPU; outputs and gradients for seeded
    upstream gradients."""
    from types import SimpleNamespace

    import random

    F = torch.nn.functional
    g = {"torch": torch, "F": F, "random": random, "dot": lambda x, y: torch.sum(x * y, -1, keepdim=True)}
    d2n = lift(os.path.join(ref, "renderer/diff_gaussian_rasterizer_shading.py"), ["Depth2Normal"], g)["Depth2Normal"]()
    # its stencil weights (0, +-1) as fp64 so the fixture is computed in fp64 (the values are exact)
    d2n.delzdelxkernel = d2n.delzdelxkernel.double()
    d2n.delzdelykernel = d2n.delzdelykernel.double()
    material_forward = lift_method(os.path.join(ref, "material/gaussian_material.py"),
                                   "GaussianDiffuseWithPointLightMaterial", "forward", g)
    rng = np.random.default_rng(77)
    out = {}
    H, W = 20, 28
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = (2.0 + 0.3 * np.sin(xs / 5.0) * np.cos(ys / 4.0) + 0.01 * rng.random((H, W)))[None]
    f = 0.5 * H / math.tan(math.radians(30))
    rays_d = np.stack([(xs + 0.5 - W / 2) / f, -(ys + 0.5 - H / 2) / f, -np.ones_like(xs)], -1)
    Qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    rays_d = rays_d @ Qm.T
    rays_o = np.broadcast_to(rng.normal(size=3), (H, W, 3)).copy()
    alpha = rng.random((1, H, W))
    alpha[:, : H // 2, : W // 2] = 1.0
    color = rng.random((3, H, W)) * alpha * 1.2 - 0.05
    bg = rng.random((H, W, 3))
    light = rng.normal(size=3) * 3
    ups = [rng.normal(size=(3, H, W)), rng.normal(size=(3, H, W)), rng.normal(size=(1, H, W))]
    out.update(color=color, depth=depth, alpha=alpha, rays_o=rays_o, rays_d=rays_d, bg=bg, light=light,
               up_render=ups[0], up_normal=ups[1], up_depth=ups[2])
    for shading in ("diffuse", "albedo", "textureless"):
        t = {k: torch.tensor(v, requires_grad=True) for k, v in (("color", color), ("depth", depth), ("alpha", alpha),
                                                                 ("bg", bg))}
        ro, rd = torch.tensor(rays_o), torch.tensor(rays_d)
        mat = SimpleNamespace(training=False, ambient_only=False,
                              cfg=SimpleNamespace(soft_shading=False, diffuse_prob=0.75, textureless_prob=0.5),
                              diffuse_light_color=torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64),
                              ambient_light_color=torch.tensor([0.1, 0.2, 0.15], dtype=torch.float64))
        # renderer/diff_gaussian_rasterizer_shading.py:172-208 (pred_normal off, comp_rgb_bg = bg)
        rendered_depth = t["depth"].clone()
        xyz_map = ro + rendered_depth.permute(1, 2, 0) * rd
        normal_map = d2n(xyz_map.permute(2, 0, 1).unsqueeze(0))[0]
        normal_map = F.normalize(normal_map, dim=0)
        light_positions = torch.tensor(light)[None, None, :].expand(H, W, -1)
        shading_normal = normal_map.permute(1, 2, 0)
        rgb_fg = material_forward(mat, positions=xyz_map, shading_normal=shading_normal,
                                  albedo=(t["color"] / (t["alpha"] + 1e-6)).permute(1, 2, 0),
                                  light_positions=light_positions, shading=shading).permute(2, 0, 1)
        rendered_image = rgb_fg * t["alpha"] + (1 - t["alpha"]) * t["bg"].reshape(H, W, 3).permute(2, 0, 1)
        normal_map = normal_map * 0.5 * t["alpha"] + 0.5
        mask = t["alpha"] > 0.99
        normal_mask = mask.repeat(3, 1, 1)
        normal_map = torch.where(normal_mask, normal_map, normal_map.detach())
        rendered_depth = torch.where(mask, rendered_depth, rendered_depth.detach())
        render = rendered_image.clamp(0, 1)
        torch.autograd.backward([render, normal_map, rendered_depth],
                                [torch.tensor(ups[0]), torch.tensor(ups[1]), torch.tensor(ups[2])])
        out[f"{shading}_render"] = render.detach().numpy()
        out[f"{shading}_normal"] = normal_map.detach().numpy()
        out[f"{shading}_depth"] = rendered_depth.detach().numpy()
        for k, v in t.items():
            out[f"{shading}_grad_{k}"] = v.grad.numpy()
    out["ambient"] = np.array([0.1, 0.2, 0.15])
    out["diffuse"] = np.array([0.9, 0.8, 0.7])
    np.savez_compressed(os.path.join(HERE, "reference_shading.npz"), **out)


class _Annotation:
    """Stands for every threestudio.utils.typing name: ``Float[Tensor, "N 3"]`` in a lifted signature evaluates."""

    def __class_getitem__(cls, item):
        return cls


TYPING = {k: _Annotation for k in ("Float", "Int", "Tensor", "ndarray", "Dict", "List", "Union", "Optional", "Tuple",
                                   "Quaternion")}
DTYPES = (("f32", torch.float32), ("f64", torch.float64))


class default_dtype:
    """The reference's ``torch.zeros`` / ``torch.ones`` follow torch's default dtype: float64 for the value to match."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)


def _unit_quats(rng, shape, max_angle):
    """float64 unit quaternions (x, y, z, w), angles uniform in (0, max_angle], every second one negated (w < 0)."""
    axis = rng.normal(size=shape + (3,))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rng.uniform(0.02, max_angle, size=shape + (1,))
    q = np.concatenate([np.sin(half) * axis, np.cos(half)], -1)
    sign = np.where(np.arange(q[..., 0].size).reshape(shape) % 2 == 0, 1.0, -1.0)[..., None]
    q = q * sign
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _jittered_icosphere(subdiv, seed, amount=0.45):
    sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
    import gsr_synthetic as gs

    v, f = gs.icosphere(subdiv)
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    return v + amount * edge * np.random.default_rng(seed).uniform(-1, 1, v.shape), np.asarray(f, np.int64)


def _arap_meshes():
    """No vertex outside every face (the reference's get_indices raises) and no directed edge in two faces."""
    tet = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.8, 0.4, 0.0], [0.1, 0.4, 1.0]]),
           np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64))
    n = 40  # a closed, crumpled fan: the hub's row has 40 entries
    ang = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7 * ang)], 1)
    fan = (np.concatenate([[[0.0, 0.0, 0.3]], ring]),
           np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1))
    v, f = _jittered_icosphere(0, seed=3)
    sliver = (np.concatenate([v, [[1.0, 1.0, 1.0], [1.01, 1.0, 1.0], [1.02, 1.000001, 1.0]]]),
              np.concatenate([f, [[12, 13, 14]]]))  # Heron's product ~1e-16, under the 1e-12 clamp
    return {"tetrahedron": tet, "icosphere1": _jittered_icosphere(1, seed=0), "fan40": fan, "sliver": sliver}


def make_arap_reference(ref: str):
    """ARAPCoach (utils/arap_utils.py), the whole class, on the CPU: its one-ring indices, its dense-branch cotangent
    weights and compute_arap_energy with given rotation matrices, per frame, with the gradients of a seeded weight per
    frame.  The rotations are the matrices (float64, by pypose's unnormalised formula) of stored float32 quaternions
    ``rot_q``, so that the quaternion form of the kernel can be fed the same rotations exactly."""
    import standins

    g = {"torch": torch, "np": np, "defaultdict": __import__("collections").defaultdict, "batch_svd": torch.svd, **TYPING}
    Coach = lift(os.path.join(ref, "utils/arap_utils.py"), ["ARAPCoach"], g)["ARAPCoach"]
    rng = np.random.default_rng(31)
    out, T = {}, 2
    for name, (v, f) in _arap_meshes().items():
        verts = np.asarray(v, np.float32)
        V = len(verts)
        edge = np.linalg.norm(verts[f[:, 0]] - verts[f[:, 1]], axis=1).mean()
        xyz = (verts[None] + 0.3 * edge * rng.normal(size=(T, V, 3))).astype(np.float32)
        rot_q = _unit_quats(rng, (T, V), 3.0).astype(np.float32)
        rot = standins.SO3(torch.tensor(rot_q, dtype=torch.float64)).matrix().numpy()
        up = rng.normal(size=T)
        out.update({f"{name}_verts": verts, f"{name}_faces": f, f"{name}_xyz": xyz, f"{name}_rot_q": rot_q,
                    f"{name}_rot": rot, f"{name}_up": up})
        for tag, dt in DTYPES:
            with default_dtype(dt):
                coach = Coach(torch.tensor(verts).to(dt), f, "cpu")
                ii, jj, nn = coach._indices_for_nfmt
                energies, gx, gr, gq = [], [], [], []
                for t in range(T):
                    x = torch.tensor(xyz[t]).to(dt).requires_grad_()
                    R = torch.tensor(rot[t]).to(dt).requires_grad_()
                    e = coach.compute_arap_energy(x, R)
                    a, b = torch.autograd.grad(e * float(up[t]), [x, R])
                    energies.append(e.detach()), gx.append(a), gr.append(b)
                    # the same frame with the matrices formed from rot_q inside the graph: the quaternion form's gradient
                    q = torch.tensor(rot_q[t]).to(dt).requires_grad_()
                    e = coach.compute_arap_energy(x, standins.SO3(q).matrix())
                    gq.append(torch.autograd.grad(e * float(up[t]), q)[0])
                rest = coach.compute_arap_energy(coach.verts.clone(), torch.eye(3).expand(V, 3, 3).contiguous())
            assert coach.edge_cot_weights.dtype == dt and energies[0].dtype == dt
            out.update({f"{name}_ii": ii.numpy(), f"{name}_jj": jj.numpy(), f"{name}_nn": nn.numpy(),
                        f"{name}_weights_{tag}": coach.edge_cot_weights.numpy(),
                        f"{name}_energy_{tag}": torch.stack(energies).numpy(),
                        f"{name}_dvert_xyz_{tag}": torch.stack(gx).numpy(),
                        f"{name}_dvert_rot_{tag}": torch.stack(gr).numpy(),
                        f"{name}_dvert_rot_q_{tag}": torch.stack(gq).numpy(),
                        f"{name}_rest_energy_{tag}": rest.numpy()})
    np.savez_compressed(os.path.join(HERE, "reference_arap.npz"), **out)


def _grads(outs, ups, leaves):
    """{"d" + name: gradient} of sum_k <outs[k], ups[k]> to the leaves (zeros where nothing flows)."""
    loss = sum((outs[k] * torch.as_tensor(ups[k]).to(outs[k].dtype)).sum() for k in ups)
    gs_ = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return {"d" + k: (torch.zeros_like(l) if g_ is None else g_).detach().as_subclass(torch.Tensor).numpy()
            for (k, l), g_ in zip(leaves.items(), gs_)}


def make_dynamic_reference(ref: str):
    """geometry/dynamic_sugar.py: _get_timed_vertex_attributes_from_dg ("lbs" and "dqs", d_scale on and off),
    fuse_rotations, get_timed_gs_attributes and _get_gs_xyz_from_vertex, with the whole DualQuaternion class of
    utils/dual_quaternions.py; pypose and einops' rearrange as tests/golden/standins.py and a reshape.  ``self`` is a
    SimpleNamespace with exactly what those bodies read.  Quaternion inputs are float64 and unit to fp64 rounding (the
    float32 run and the kernels get them rounded to float32): what pypose does off the unit sphere is not pinned."""
    from types import SimpleNamespace

    import standins as pp

    F = torch.nn.functional
    g = {"torch": torch, "pp": pp, "json": None, "F": F, **TYPING}
    DQ = lift(os.path.join(ref, "utils/dual_quaternions.py"), ["quat_norm", "quat_conjugate", "DualQuaternion"], g)
    path = os.path.join(ref, "geometry/dynamic_sugar.py")
    g = {**g, "DualQuaternion": DQ["DualQuaternion"],
         "rearrange": __import__("einops").rearrange}
    fuse = lift(path, ["fuse_rotations"], g)["fuse_rotations"]
    g["fuse_rotations"] = fuse
    skin, timed, gs_xyz = (lift_method(path, "DynamicSuGaRModel", m, g) for m in
                           ("_get_timed_vertex_attributes_from_dg", "get_timed_gs_attributes",
                            "_get_gs_xyz_from_vertex"))
    rng = np.random.default_rng(53)
    out = {}

    # --- skinning: V = 42, 7 nodes, T = 3
    v, _ = _jittered_icosphere(1, seed=1)
    verts = np.asarray(v, np.float32)
    V, P, T = len(verts), 7, 3
    node_xyz = (verts[rng.permutation(V)[:P]] + 0.05 * rng.normal(size=(P, 3))).astype(np.float32)
    node_trans = rng.normal(size=(T, P, 3)).astype(np.float32)  # of the mesh's size (radius 1)
    node_rots = _unit_quats(rng, (T, P), 3.0)  # float64
    node_scales = (0.1 * rng.normal(size=(T, P, 3))).astype(np.float32)
    out.update(skin_verts=verts, skin_node_xyz=node_xyz, skin_node_trans=node_trans, skin_node_rots=node_rots,
               skin_node_scales=node_scales)
    others = np.array([1, 2, 3, 4, 6])  # node 5 is used by no vertex
    for K in (1, 4):
        if K == 1:  # one node each, so node 0 cannot be everybody's
            nbr = others[rng.integers(0, 5, size=(V, 1))]
            nbr[::6, 0] = 0
        else:  # node 0 is used by every vertex
            nbr = np.stack([np.concatenate([[0], rng.permutation(others)[:K - 1]]) for _ in range(V)])
        w = rng.uniform(0.1, 1.1, size=(V, K))
        # K = 1: a weight of exactly 1 would make the scale output a copy; the reference does not ask for sum 1
        w = (w / w.sum(-1, keepdims=True) if K > 1 else 0.5 + w).astype(np.float32)
        ups = {"xyz": rng.normal(size=(T, V, 3)), "rotation": rng.normal(size=(T, V, 4)),
               "scale": rng.normal(size=(T, V, 3))}
        out.update({f"skin_K{K}_nbr": nbr.astype(np.int64), f"skin_K{K}_w": w})
        out.update({f"skin_K{K}_up_{k}": u for k, u in ups.items()})
        for method in ("lbs", "dqs"):
            for tag, dt in DTYPES:
                res = {}
                for d_scale in (True, False):
                    leaves = {k: torch.tensor(a).to(dt).requires_grad_() for k, a in
                              (("verts", verts), ("node_trans", node_trans), ("node_rots", node_rots),
                               ("node_scales", node_scales))}
                    me = SimpleNamespace(
                        _deform_graph_node_xyz=torch.tensor(node_xyz).to(dt), _xyz_neighbor_node_idx=torch.tensor(nbr),
                        _xyz_neighbor_nodes_weights=torch.tensor(w).to(dt), get_xyz_verts=leaves["verts"],
                        cfg=SimpleNamespace(skinning_method=method, d_scale=d_scale),
                        get_timed_dg_attributes=lambda timestamp, frame_idx: {
                            "xyz": leaves["node_trans"], "rotation": pp.SO3(leaves["node_rots"]),
                            "scale": leaves["node_scales"]})
                    with default_dtype(dt):
                        outs = skin(me, None, torch.arange(T))
                    assert ("scale" in outs) == d_scale and outs["xyz"].dtype == dt
                    outs = {k: o.as_subclass(torch.Tensor) for k, o in outs.items()}
                    res[d_scale] = {k: o.detach().numpy() for k, o in outs.items()}
                    res[d_scale].update(_grads(outs, {k: ups[k] for k in outs}, leaves))
                for k in res[False]:  # d_scale only adds the scale output and its gradient
                    if k != "dnode_scales":
                        assert np.array_equal(res[False][k], res[True][k]), (K, method, tag, k)
                assert not res[False]["dnode_scales"].any()
                out.update({f"skin_K{K}_{method}_{k}_{tag}": a for k, a in res[True].items()})

    # --- timed Gaussians on a jittered icosphere(0), G = 1 and 3 (geometry/sugar.py:245-262: the reference's float32
    #     barycentric sets), T = 3
    v, f = _jittered_icosphere(0, seed=2)
    verts = np.asarray(v, np.float32)
    V, Fn = len(verts), len(f)
    vert_xyz = (verts[None] + 0.1 * rng.normal(size=(T, V, 3))).astype(np.float32)
    vert_rot = _unit_quats(rng, (T, V), 3.0)  # float64
    vert_scale = (0.1 * rng.normal(size=(T, V, 3))).astype(np.float32)
    thickness = 3.5e-6
    out.update(timed_faces=f, timed_vert_xyz=vert_xyz, timed_vert_rot=vert_rot, timed_vert_scale=vert_scale,
               timed_thickness=np.float64(thickness))
    barys = {1: [[1 / 3, 1 / 3, 1 / 3]], 3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]]}
    for G, bary in barys.items():
        N = Fn * G
        bary = np.asarray(bary, np.float32)
        q0 = rng.normal(size=(N, 4))
        rotation0 = q0 / np.linalg.norm(q0, axis=-1, keepdims=True)  # float64 unit (w, x, y, z)
        log_scales = (0.3 * rng.normal(size=(N, 2)) - 4).astype(np.float32)
        ups = {"xyz": rng.normal(size=(T, N, 3)), "rotation": rng.normal(size=(T, N, 4)),
               "scale": rng.normal(size=(T, N, 3))}
        out.update({f"timed_G{G}_bary": bary, f"timed_G{G}_rotation0": rotation0, f"timed_G{G}_log_scales": log_scales})
        out.update({f"timed_G{G}_up_{k}": u for k, u in ups.items()})
        for tag, dt in DTYPES:
            leaves = {k: torch.tensor(a).to(dt).requires_grad_() for k, a in
                      (("vert_xyz", vert_xyz), ("vert_rot", vert_rot), ("rotation0", rotation0),
                       ("vert_scale", vert_scale), ("log_scales", log_scales))}
            faces = torch.tensor(f)
            coords = torch.tensor(bary).to(dt)[..., None]
            me = SimpleNamespace(
                get_timed_vertex_attributes=lambda timestamp, frame_idx: {
                    "xyz": leaves["vert_xyz"], "rotation": pp.SO3(leaves["vert_rot"]), "scale": leaves["vert_scale"]},
                _gs_vert_connections=faces.repeat_interleave(G, dim=0), _gs_bary_weights=torch.cat([coords] * Fn, dim=0),
                get_rotation=leaves["rotation0"], cfg=SimpleNamespace(d_scale=True), _scales=leaves["log_scales"],
                device="cpu", surface_mesh_thickness=thickness, scale_activation=torch.exp,
                binded_to_surface_mesh=True, _surface_mesh_faces=faces, surface_triangle_bary_coords=coords,
                _points=None)
            me._get_gs_xyz_from_vertex = lambda xyz_vert=None: gs_xyz(me, xyz_vert)
            with default_dtype(dt):
                outs = timed(me, None, torch.arange(T))
            outs = {k: o.as_subclass(torch.Tensor) for k, o in outs.items()}
            assert all(o.dtype == dt for o in outs.values())
            out.update({f"timed_G{G}_{k}_{tag}": o.detach().numpy() for k, o in outs.items()})
            out.update({f"timed_G{G}_{k}_{tag}": a for k, a in _grads(outs, ups, leaves).items()})
    np.savez_compressed(os.path.join(HERE, "reference_dynamic.npz"), **out)


def make_mesh_reference(ref: str):
    """geometry/sugar.py, SuGaRModel: the bodies of the points, scaling, quaternions, get_face_normals and
    get_gs_normals properties in their mesh-bound branch, on a jittered icosphere(0) with G = 1 and 3; pytorch3d's
    Meshes and matrix_to_quaternion as tests/golden/standins.py."""
    from types import SimpleNamespace

    import standins

    F = torch.nn.functional
    g = {"torch": torch, "F": F, "matrix_to_quaternion": standins.matrix_to_quaternion, **TYPING}
    path = os.path.join(ref, "geometry/sugar.py")
    props = {m: lift_method(path, "SuGaRModel", m, g) for m in
             ("points", "scaling", "quaternions", "get_face_normals", "get_gs_normals")}
    rng = np.random.default_rng(67)
    v, f = _jittered_icosphere(0, seed=4)
    verts = np.asarray(v, np.float32)
    Fn, thickness = len(f), 3.5e-6
    out = dict(verts=verts, faces=f, thickness=np.float64(thickness))
    barys = {1: [[1 / 3, 1 / 3, 1 / 3]], 3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]]}
    for G, bary in barys.items():
        N = Fn * G
        bary = np.asarray(bary, np.float32)
        cplx = rng.normal(size=(N, 2)).astype(np.float32)
        log_scales = (0.3 * rng.normal(size=(N, 2)) - 4).astype(np.float32)
        ups = {"xyz": rng.normal(size=(N, 3)), "scaling": rng.normal(size=(N, 3)), "rotation": rng.normal(size=(N, 4)),
               "normals": rng.normal(size=(N, 3))}
        out.update({f"G{G}_bary": bary, f"G{G}_complex": cplx, f"G{G}_log_scales": log_scales})
        out.update({f"G{G}_up_{k}": u for k, u in ups.items()})
        for tag, dt in DTYPES:
            leaves = {k: torch.tensor(a).to(dt).requires_grad_() for k, a in
                      (("verts", verts), ("complex", cplx), ("log_scales", log_scales))}
            faces = torch.tensor(f)

            class Model:  # the lifted property bodies read each other through self
                binded_to_surface_mesh = True
                _points, _quaternions, _scales = leaves["verts"], leaves["complex"], leaves["log_scales"]
                _surface_mesh_faces, _n_points, device = faces, N, "cpu"
                surface_triangle_bary_coords = torch.tensor(bary).to(dt)[..., None]
                surface_mesh_thickness, scale_activation = thickness, staticmethod(torch.exp)
                cfg = SimpleNamespace(n_gaussians_per_surface_triangle=G)
                surface_mesh = property(lambda self: standins.Meshes(verts=[self._points], faces=[self._surface_mesh_faces]))
                points, scaling, quaternions = (property(props[m]) for m in ("points", "scaling", "quaternions"))
                get_face_normals, get_gs_normals = (property(props[m]) for m in ("get_face_normals", "get_gs_normals"))

            me = Model()
            with default_dtype(dt):
                outs = {"xyz": me.points, "scaling": me.scaling, "rotation": me.quaternions,
                        "normals": me.get_gs_normals}
            assert all(o.dtype == dt for o in outs.values())
            out.update({f"G{G}_{k}_{tag}": o.detach().numpy() for k, o in outs.items()})
            out.update({f"G{G}_{k}_{tag}": a for k, a in _grads(outs, ups, leaves).items()})
    np.savez_compressed(os.path.join(HERE, "reference_mesh.npz"), **out)


def _if_body(path: str, cls: str, method: str, test_name: str, extra_globals: dict):
    """The body of the statement ``if <test_name>:`` inside a reference method, compiled: exec it in a namespace that
    holds the local names it reads."""
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == method)
    found = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Name) and n.test.id == test_name]
    assert len(found) == 1, (test_name, len(found))
    code = compile(ast.unparse(ast.Module(body=found[0].body, type_ignores=[])), path, "exec")
    return lambda local_names: exec(code, dict(extra_globals), local_names)  # noqa: S102 -- reference code, CPU only


def make_field_reference(ref: str):
    """utils/sugar_utils.py, the whole SuGaRRegularizer class: get_covariance, get_field_values with get_beta (three
    modes) and get_smallest_axis; and the body of ``if use_sdf_better_normal_loss:`` in coarse_density_regulation, fed
    stored samples and the lifted get_field_values' opacities.  N = 200 Gaussians, M = 65 samples, K = 1 and 16.

    Three runs of get_field_values per K ("a", "w", "l"; all with return_beta):
      a  beta_mode average, density_factor 1, return_sdf, opacities; outputs only.  Samples 0-4 sit on the centres of
         Gaussians of strength exactly 1 (density >= 1: the normalisation branch), samples 5-8 are 9 to 11.5 sigma
         away (density under opacity_min_clamp, yet a normal float32 number, so that float32 and float64 take the
         same branches) and sample 9 is so far that every opacity is exactly 0 in both.  In float32 a normalised density is exactly 1 and the root's derivative at 0 is
         infinite, so this run stores no gradients;
      w  weighted_average, density_factor 1.3, return_sdf, opacities, with gradients, on strengths scaled down so that
         no density reaches 1;
      l  learnable, return_sdf off, no opacities, with gradients (strengths as in a)."""
    from types import SimpleNamespace

    import standins

    path = os.path.join(ref, "utils/sugar_utils.py")
    g = {"torch": torch, "np": np, "quaternion_to_matrix": standins.quaternion_to_matrix, "GaussianBaseModel": None}
    Reg = lift(path, ["SuGaRRegularizer"], g)["SuGaRRegularizer"]
    normal_block = _if_body(path, "SuGaRRegularizer", "coarse_density_regulation", "use_sdf_better_normal_loss", g)
    rng = np.random.default_rng(89)
    N, M = 200, 65
    points = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    scaling = (10 ** rng.uniform(-2.3, -0.3, size=(N, 3))).astype(np.float32)  # two decades
    quats = rng.normal(size=(N, 4))
    quats = (quats / np.linalg.norm(quats, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, size=(N, 1))).astype(np.float32)
    strengths = (1 / (1 + np.exp(-2 * rng.normal(size=(N, 1))))).astype(np.float32)
    strengths[:5] = 1.0
    d2 = ((points[:, None].astype(np.float64) - points[None]) ** 2).sum(-1)
    knn = np.argsort(d2, axis=1, kind="stable")[:, :16].astype(np.int64)  # column 0 is the Gaussian itself
    own = rng.integers(5, N, size=M).astype(np.int64)
    own[:5] = np.arange(5)
    R = standins.quaternion_to_matrix(torch.tensor(quats, dtype=torch.float64)).numpy()
    x = points[own] + np.einsum("mij,mj->mi", R[own], 1.5 * scaling[own] * rng.normal(size=(M, 3)))
    x[:5] = points[:5]
    x[5:9] = points[own[5:9]] + R[own[5:9], :, 0] * scaling[own[5:9], :1] * np.array([[9.0], [9.5], [10.5], [11.5]])
    x[9] = [50.0, 50.0, 50.0]
    x = x.astype(np.float32)
    log_beta = np.array([-3.0], np.float32)
    out = dict(points=points, scaling=scaling, quaternions=quats, strengths=strengths, knn_idx=knn, gaussian_idx=own,
               x=x, log_beta=log_beta, density_threshold=np.float64(0.7))

    def regulariser(dt, leaves, K, mode):
        me = object.__new__(Reg)
        me.gaussians = SimpleNamespace(get_xyz=leaves["points"], get_scaling=leaves["scaling"], device="cpu",
                                       get_opacity=leaves["strengths"], get_rotation=torch.tensor(quats).to(dt))
        me.binded_to_surface_mesh, me.beta_mode, me.knn_idx = False, mode, torch.tensor(knn[:, :K])
        if "log_beta" in leaves:
            me._log_beta = leaves["log_beta"]
        return me

    def tensors(dt, **arrays):
        return {k: torch.tensor(a).to(dt).requires_grad_() for k, a in arrays.items()}

    for tag, dt in DTYPES:
        with default_dtype(dt):
            me = regulariser(dt, tensors(dt, points=points, scaling=scaling, strengths=strengths), 16, "average")
            out[f"inv_sr_{tag}"] = me.get_covariance(return_full_matrix=True, return_sqrt=True,
                                                     inverse_scales=True).detach().numpy()
            out[f"cov_full_{tag}"] = me.get_covariance(return_full_matrix=True).detach().numpy()
            out[f"cov6_{tag}"] = me.get_covariance().detach().numpy()  # the reference makes this one float32 always
            axis, axis_idx = me.get_smallest_axis(return_idx=True)
            out[f"normals_{tag}"], out[f"normals_idx_{tag}"] = axis.detach().numpy(), axis_idx.numpy()
    inv_sr, normals = out["inv_sr_f32"], out["normals_f32"]  # what the kernels are fed; both runs start from them

    for K in (1, 16):
        ups = {"density": rng.normal(size=M), "closest_gaussian_opacities": rng.normal(size=(M, K)),
               "beta": rng.normal(size=M), "sdf": rng.normal(size=M), "normal": rng.normal(size=M)}
        out.update({f"K{K}_up_{k}": u for k, u in ups.items()})
        dens = None
        for tag, dt in reversed(DTYPES):  # float64 first: it sets the scaled-down strengths
            for run, mode, df, sdf_on, want_op in (("a", "average", 1.0, True, True),
                                                   ("w", "weighted_average", 1.3, True, True),
                                                   ("l", "learnable", 1.0, False, False)):
                s = strengths if run != "w" else out.get(f"K{K}_strengths_w")
                if s is None:
                    s = out[f"K{K}_strengths_w"] = (strengths * np.float32(0.8 / 1.3 / float(dens.max()))).astype(np.float32)
                leaves = tensors(dt, x=x, points=points, inv_sr=inv_sr, strengths=s, scaling=scaling, log_beta=log_beta)
                me = regulariser(dt, leaves, K, mode)
                with default_dtype(dt):
                    fields = me.get_field_values(
                        leaves["x"], torch.tensor(own), gaussian_inv_scaled_rotation=leaves["inv_sr"], return_sdf=sdf_on,
                        density_threshold=0.7, density_factor=df, return_closest_gaussian_opacities=want_op,
                        return_beta=True)
                assert set(fields) == {"density", "beta"} | ({"sdf"} if sdf_on else set()) | (
                    {"closest_gaussian_opacities"} if want_op else set())
                assert all(f.dtype == dt for f in fields.values())
                if run == "a" and tag == "f64":
                    dens = fields["density"].detach().numpy()
                out.update({f"K{K}_{run}_{k}_{tag}": f.detach().numpy() for k, f in fields.items()})
                if run != "a":
                    out.update({f"K{K}_{run}_{k}_{tag}": a for k, a in
                                _grads(fields, {k: ups[k] for k in fields}, leaves).items()})
        for tag, dt in DTYPES:  # the neighbour-normal block, on this dtype's copy of run a's float32 opacities
            op = torch.tensor(out[f"K{K}_a_closest_gaussian_opacities_f32"]).to(dt)
            leaves = tensors(dt, normals=normals)
            me = regulariser(dt, tensors(dt, points=points, scaling=scaling, strengths=strengths), K, "average")
            me.get_normals = lambda estimate_from_points=False: leaves["normals"]
            names = dict(self=me, sdf_gaussian_idx=torch.tensor(own), sdf_samples=torch.tensor(x).to(dt),
                         fields={"closest_gaussian_opacities": op}, loss={"normal_regulation": 0},
                         sdf_better_normal_gradient_through_normal_only=True)
            with default_dtype(dt):
                normal_block(names)
            loss = names["sdf_better_normal_loss"]
            assert loss.dtype == dt and loss.shape == (M,)
            out[f"K{K}_normal_loss_{tag}"] = loss.detach().numpy()
            out[f"K{K}_normal_mean_{tag}"] = names["loss"]["normal_regulation"].detach().numpy()
            out[f"K{K}_normal_dnormals_{tag}"] = _grads({"normal": loss}, {"normal": ups["normal"]}, leaves)["dnormals"]
    np.savez_compressed(os.path.join(HERE, "reference_field.npz"), **out)


def make_oracle_scene():
    sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle
    from gsr_testutil import make_camera, oracle_cam

    import gsr_synthetic as gs

    scene = gs.make_scene(600, sh_degree=3, seed=42)
    cam = make_camera(48, 40, fovy_deg=55.0, elevation=20.0, azimuth=35.0, distance=2.2)
    bg = np.array([0.3, 0.6, 0.9], np.float32)
    gc, gd, ga = gs.upstream_grads(40, 48, seed=5)
    f = oracle.forward(scene, oracle_cam(cam), bg, "f64")
    b = oracle.backward(scene, oracle_cam(cam), bg, gc, gd, ga, prec="f64")
    out = {f"scene_{k}": v for k, v in scene.items() if isinstance(v, np.ndarray)}
    out.update({f"cam_{k}": np.asarray(v) for k, v in cam.items()})
    out.update(bg=bg, dL_dcolor=gc, dL_ddepth=gd, dL_dalpha=ga, sh_degree=np.int64(scene["sh_degree"]))
    out.update({f"out_{k}": np.asarray(v) for k, v in f.items()})
    out.update({f"grad_{k}": v for k, v in b.items()})
    np.savez_compressed(os.path.join(HERE, "oracle_scene.npz"), **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--skip-reference", action="store_true")
    a = ap.parse_args()
    if not a.skip_reference:
        make_reference(a.reference)
        make_shading_reference(a.reference)
        make_arap_reference(a.reference)
        make_dynamic_reference(a.reference)
        make_mesh_reference(a.reference)
        make_field_reference(a.reference)
    make_oracle_scene()
    print("golden vectors written to", HERE)
