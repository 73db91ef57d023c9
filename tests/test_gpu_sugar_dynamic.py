"""sugar_dynamic.skin_vertices and timed_gaussians (include/gsr.h gsr_sugar_skin_*, gsr_sugar_timed_*,
csrc/gsr_dynamic.hip) on the GPU against the fp64 torch restatement of the same formulas
(tests/sugar_dynamic_reference.py), differentiated by autograd on the CPU.

Bar (``check_against_null`` of tests/sugar_cases.py), as in tests/test_gpu_sugar_mesh.py.  Per tensor (the outputs, the
gradients): max |gpu - ref64| / max |ref64| <= 2 x the same figure of the restatement in float32 on the CPU (the "fp32 null", computed here on the same inputs):
the kernels may not be less exact than twice what they replace; the factor 2 is there because the null is itself a few
ulps of one rounding sample.  Where the reference tensor is all zero the result must be exactly zero.  No quaternion
sign alignment: Exp yields w >= 0 and the product is deterministic.  Each check prints its figures.
Inputs keep the null itself away from Log's branch at theta = +-pi: rotation angles within +-2.6 rad (|w| / |q| >=
0.25), both signs of w, norms in [0.5, 1.5], some rows exactly the identity.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_dynamic_reference as ref  # noqa: E402
from sugar_cases import NullCase, _fan, _rel, backprop, random_quats  # noqa: E402

THICKNESS = 3.5e-6


class _Skin(NullCase):
    """A deformation graph with random node attributes and upstream gradients; reference and null computed once."""

    def __init__(self, T, verts, P, K, method, scales, seed=0, nbr=None, identity=False):
        from sugar_dynamic import SkinBinding

        gen = torch.Generator().manual_seed(seed)
        self.verts = torch.as_tensor(np.asarray(verts), dtype=torch.float32)
        V = len(self.verts)
        self.node_xyz = self.verts[torch.randint(0, V, (P,), generator=gen)] + 0.05 * torch.randn(P, 3, generator=gen)
        if nbr is None:
            self.binding = SkinBinding.from_euclidean(self.verts, self.node_xyz, K)
        else:
            w = torch.rand(V, K, generator=gen) + 0.1
            self.binding = SkinBinding(nbr, w / w.sum(-1, keepdim=True), P)
        self.method = method
        if identity:  # the training start
            self.trans = torch.zeros(T, P, 3)
            self.rots = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(T, P, 4).contiguous()
        else:
            self.trans = 0.3 * torch.randn(T, P, 3, generator=gen)
            self.rots = random_quats(gen, (T, P))
        self.scales = 0.1 * torch.randn(T, P, 3, generator=gen) if scales else None
        self.ups = {"xyz": torch.randn(T, V, 3, generator=gen), "rot": torch.randn(T, V, 4, generator=gen)}
        if scales:
            self.ups["scale"] = torch.randn(T, V, 3, generator=gen)
        self.keys = self.outputs + ("dverts", "dnode_trans", "dnode_rots") + (("dnode_scales",) if scales else ())

    def evaluate(self, dtype, ups):
        inputs = dict(verts=self.verts, node_trans=self.trans, node_rots=self.rots, node_scales=self.scales)
        return ref.evaluate_skin(dtype, inputs, self.node_xyz, self.binding.nbr, self.binding.w, self.method, ups)

    def gpu(self, which=None):
        from sugar_dynamic import skin_vertices

        leaves = [None if t is None else t.cuda().requires_grad_()
                  for t in (self.verts, self.trans, self.rots, self.scales)]
        out = skin_vertices(leaves[0], self.node_xyz.cuda(), leaves[1], leaves[2], self.binding.to("cuda"),
                            self.method, leaves[3])
        assert (out[2] is None) == (self.scales is None)
        return backprop(out, ref.SKIN_OUTPUTS, leaves, ["d" + k for k in ref.SKIN_INPUTS], self.ups,
                        which or self.outputs)


@functools.lru_cache(maxsize=None)
def _cloud(V, seed=0):
    return torch.randn(V, 3, generator=torch.Generator().manual_seed(seed)).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_skin_one_of_everything(method):
    case = _Skin(1, [[0.3, -0.2, 0.5]], 1, 1, method, True, seed=1)
    case.check(case.gpu(), tag=f"T=V=P=K=1 {method}")


@pytest.mark.gpu
@pytest.mark.parametrize("scales", [False, True])
@pytest.mark.parametrize("method", ["dqs", "lbs"])
@pytest.mark.parametrize("K", [1, 8, 16, 32])
def test_skin_cloud(K, method, scales):
    case = _Skin(3, _cloud(200), 40, K, method, scales, seed=K)
    case.check(case.gpu(), tag=f"T=3 V=200 P=40 K={K} {method} scales={scales}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_skin_identity_nodes(method):
    """The training start: every node rotation the identity, no translation.  The outputs are exact."""
    case = _Skin(3, _cloud(200), 40, 8, method, False, seed=3, identity=True)
    got = case.gpu()
    assert torch.equal(got["rot"], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(3, 200, 4))
    if method == "dqs":
        assert torch.equal(got["xyz"], case.verts[None].expand(3, 200, 3))
    for k in case.keys:
        assert torch.isfinite(got[k]).all(), k
    case.check(got, tag=f"identity nodes {method}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_skin_unused_node_and_a_node_of_every_vertex(method):
    """Node 0 is used by all V = 700 vertices (a list of 700 items: eleven rounds of the wave), node 5 by none."""
    V, P, K = 700, 9, 3
    gen = torch.Generator().manual_seed(11)
    nbr = torch.stack([torch.zeros(V, dtype=torch.int64), torch.randint(1, 5, (V,), generator=gen),
                       torch.randint(6, 9, (V,), generator=gen)], 1)
    case = _Skin(2, _cloud(V, 1), P, K, method, True, seed=4, nbr=nbr)
    assert int(case.binding.node_offsets[1]) == V
    assert int(case.binding.node_offsets[5]) == int(case.binding.node_offsets[6])
    got = case.gpu()
    case.check(got, tag=f"V=700 {method}")
    for k in ("dnode_trans", "dnode_rots", "dnode_scales"):
        assert not got[k][:, 5].any() and not torch.signbit(got[k][:, 5]).any(), k  # exactly 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_skin_icosphere3(method):
    """V = 642, P = 37, K = 16: no size a multiple of 64."""
    v, _ = gs.icosphere(3)
    case = _Skin(2, v, 37, 16, method, True, seed=5)
    case.check(case.gpu(), tag=f"icosphere(3) P=37 K=16 {method}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("xyz",), ("rot",)])
def test_skin_partial_upstream_gradients(which):
    case = _Skin(3, _cloud(200), 40, 8, "dqs", True, seed=6)
    got = case.gpu(which)
    case.check(got, which, tag=f"skin only {which[0]}")
    assert not got["dnode_scales"].any()
    if which == ("rot",):
        assert not got["dverts"].any() and not got["dnode_trans"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_skin_bitwise_repeatable(method):
    case = _Skin(3, _cloud(200), 40, 16, method, True, seed=7)
    a, b = case.gpu(), case.gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


class _Timed(NullCase):
    """A mesh with random deformed vertices, vertex rotations and upstream gradients."""

    def __init__(self, T, verts, faces, G, scales, seed=0):
        from sugar_mesh import MeshBinding

        gen = torch.Generator().manual_seed(seed)
        self.faces = torch.as_tensor(np.asarray(faces), dtype=torch.int64)
        base = torch.as_tensor(np.asarray(verts), dtype=torch.float32)
        V = len(base)
        self.binding = MeshBinding.from_reference_count(self.faces, V, G)
        N = self.binding.n_gaussians
        self.inputs = dict(vert_xyz=base[None] + 0.03 * torch.randn(T, V, 3, generator=gen),
                           vert_rot=random_quats(gen, (T, V)),
                           rotation0=torch.nn.functional.normalize(torch.randn(N, 4, generator=gen), dim=-1),
                           vert_scale=0.1 * torch.randn(T, V, 3, generator=gen) if scales else None,
                           log_scales=0.3 * torch.randn(N, 2, generator=gen) - 4 if scales else None)
        self.ups = {"xyz": torch.randn(T, N, 3, generator=gen), "rotation": torch.randn(T, N, 4, generator=gen),
                    "normals": torch.randn(T, N, 3, generator=gen)}
        if scales:
            self.ups["scaling"] = torch.randn(T, N, 3, generator=gen)
        self.scales = scales
        self.keys = self.outputs + tuple("d" + k for k in ref.TIMED_INPUTS if self.inputs[k] is not None)

    def evaluate(self, dtype, ups):
        return ref.evaluate_timed(dtype, self.inputs, self.faces, self.binding.bary, THICKNESS, ups)

    def gpu(self, which=None):
        from sugar_dynamic import timed_gaussians

        leaves = {k: None if t is None else t.cuda().requires_grad_() for k, t in self.inputs.items()}
        opt = dict(vert_scale=leaves["vert_scale"], log_scales=leaves["log_scales"], thickness=THICKNESS)
        out = timed_gaussians(leaves["vert_xyz"], leaves["vert_rot"], leaves["rotation0"], self.binding.to("cuda"),
                              **(opt if self.scales else {}))
        assert (out[3] is None) == (not self.scales)
        return backprop(out, ref.TIMED_OUTPUTS, [leaves[k] for k in ref.TIMED_INPUTS],
                        ["d" + k for k in ref.TIMED_INPUTS], self.ups, which or self.outputs)

    def check(self, got, which=None, tag=""):
        super().check(got, which, tag)
        if self.scales:
            T, N = got["scaling"].shape[:2]
            assert torch.equal(got["scaling"][..., 0], torch.full((T, N), THICKNESS, dtype=torch.float32)), tag
            assert not got["dvert_scale"][..., 0].any(), tag  # component 0 is discarded: exactly zero


@pytest.mark.gpu
def test_timed_one_face_one_gaussian():
    case = _Timed(1, [[0.1, 0.2, 0.3], [0.9, 0.1, 0.2], [0.3, 0.8, 0.5]], [[0, 1, 2]], 1, True, seed=1)
    assert case.binding.n_gaussians == 1
    case.check(case.gpu(), tag="F=1 G=1")


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 4, 6])
def test_timed_icosphere0(G):
    v, f = gs.icosphere(0)
    case = _Timed(2, v, f, G, True, seed=10 + G)
    case.check(case.gpu(), tag=f"icosphere(0) G={G}")


@pytest.mark.gpu
@pytest.mark.parametrize("scales", [False, True])
def test_timed_icosphere3(scales):
    """T = 3, V = 642, F = 1280, N = 7680: several blocks of (t, face), (t, vertex) and Gaussian lanes, none whole."""
    v, f = gs.icosphere(3)
    case = _Timed(3, v, f, 6, scales, seed=20)
    assert (case.binding.n_verts, case.binding.n_faces, case.binding.n_gaussians) == (642, 1280, 7680)
    case.check(case.gpu(), tag=f"icosphere(3) G=6 scales={scales}")


@pytest.mark.gpu
def test_timed_fan_of_200_faces_and_an_unused_vertex():
    verts, faces = _fan(200)
    case = _Timed(2, verts, faces, 3, True, seed=3)
    assert int(case.binding.vert_offsets[1]) == 200 and int(case.binding.vert_offsets[-1]) == 600
    got = case.gpu()
    case.check(got, tag="fan")
    for k in ("dvert_xyz", "dvert_rot", "dvert_scale"):
        assert not got[k][:, -1].any() and not torch.signbit(got[k][:, -1]).any(), k  # exactly 0.0


@pytest.mark.gpu
def test_timed_degenerate_face():
    """A face with two equal corners appended to icosphere(0): everything finite, and nothing else changes."""
    v, f = gs.icosphere(0)
    G = 6
    clean = _Timed(2, v, f, G, True, seed=4)
    full = _Timed(2, v, np.concatenate([f, [[0, 0, 5]]]), G, True, seed=4)
    n = clean.binding.n_gaussians
    for name in ("vert_xyz", "vert_rot", "vert_scale"):
        full.inputs[name] = clean.inputs[name]
    for name in ("rotation0", "log_scales"):
        full.inputs[name][:n] = clean.inputs[name]
    for k in full.ups:
        full.ups[k][:, :n] = clean.ups[k]
    a, b = clean.gpu(), full.gpu()
    for k in full.keys:
        assert torch.isfinite(b[k]).all(), k
    for k in clean.outputs:
        assert torch.equal(a[k], b[k][:, :n]), k
    for k in ("drotation0", "dlog_scales"):
        assert torch.equal(a[k], b[k][:n]), k
    untouched = [i for i in range(12) if i not in (0, 5)]
    for k in ("dvert_xyz", "dvert_rot", "dvert_scale"):
        assert torch.equal(a[k][:, untouched], b[k][:, untouched]), k
    assert not b["normals"][:, n:].any()  # no normal: the zero vector


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("xyz",), ("rotation",)])
def test_timed_partial_upstream_gradients(which):
    v, f = gs.icosphere(1)
    case = _Timed(2, v, f, 6, True, seed=5)
    got = case.gpu(which)
    case.check(got, which, tag=f"timed only {which[0]}")
    assert not got["dlog_scales"].any() and not got["dvert_scale"].any()
    if which == ("xyz",):
        assert not got["dvert_rot"].any() and not got["drotation0"].any() and got["dvert_xyz"].any()
    else:
        assert not got["dvert_xyz"].any()


@pytest.mark.gpu
def test_timed_bitwise_repeatable():
    v, f = gs.icosphere(2)
    case = _Timed(3, v, f, 6, True, seed=6)
    a, b = case.gpu(), case.gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_identity_nodes_reproduce_the_static_mesh():
    """T = 1 with identity nodes: timed_gaussians(skin_vertices(...)) has bound_gaussians' xyz and normals, both
    within the bar of the static restatement (tests/sugar_mesh_reference.py: fp64, and its float32 null)."""
    import sugar_mesh_reference as mesh_ref
    from sugar_dynamic import SkinBinding, skin_vertices, timed_gaussians
    from sugar_mesh import MeshBinding, bound_gaussians

    v, f = gs.icosphere(2)
    verts, faces = torch.tensor(v, dtype=torch.float32), torch.tensor(f)
    mb = MeshBinding.from_reference_count(faces, len(v), 6)
    N, P = mb.n_gaussians, 20
    gen = torch.Generator().manual_seed(9)
    node_xyz = verts[torch.randperm(len(v), generator=gen)[:P]]
    sb = SkinBinding.from_euclidean(verts, node_xyz, 8)
    rots = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(1, P, 4).contiguous()
    cplx, ls = torch.randn(N, 2, generator=gen), torch.randn(N, 2, generator=gen) - 4
    r64 = mesh_ref.evaluate(torch.float64, verts, faces, mb.bary, cplx, ls, THICKNESS, {})
    r32 = mesh_ref.evaluate(torch.float32, verts, faces, mb.bary, cplx, ls, THICKNESS, {})
    static = bound_gaussians(verts.cuda(), cplx.cuda(), ls.cuda(), mb.to("cuda"), THICKNESS)
    vx, vr, _ = skin_vertices(verts.cuda(), node_xyz.cuda(), torch.zeros(1, P, 3).cuda(), rots.cuda(), sb.to("cuda"))
    xyz, rotation, normals, scaling = timed_gaussians(vx, vr, static[2], mb.to("cuda"))
    assert scaling is None and xyz.shape == (1, N, 3)
    for name, a, b in (("xyz", xyz[0], static[0]), ("normals", normals[0], static[3])):
        bar = 2 * _rel(r32[name], r64[name])
        err, err_static = _rel(a.cpu(), r64[name]), _rel(b.cpu(), r64[name])
        print(f"static {name}: timed {err:.3g}  bound_gaussians {err_static:.3g}  fp32 null {bar / 2:.3g}")
        assert err <= bar and err_static <= bar, (name, err, err_static, bar)


@pytest.mark.gpu
def test_chain_feeds_the_rasterizer():
    """skin_vertices -> timed_gaussians -> rasterize_views on icosphere(3): two frames as two 64 x 64 views, each view
    given its frame's Gaussians, the normals as the second colour set.  It renders, and finite non-zero gradients
    reach node_trans and node_rots."""
    from diff_gaussian_rasterization.batched import rasterize_views
    from gsr_testutil import _settings, make_camera
    from sugar_dynamic import SkinBinding, skin_vertices, timed_gaussians
    from sugar_mesh import MeshBinding, bound_gaussians, initial_log_scales

    dev = "cuda"
    v, f = gs.icosphere(3)
    verts = torch.tensor(v, dtype=torch.float32, device=dev)
    mb = MeshBinding.from_reference_count(torch.tensor(f), len(v), 6).to(dev)
    gen = torch.Generator().manual_seed(5)
    T, P, N = 2, 30, mb.n_gaussians
    node_xyz = verts[torch.randperm(len(v), generator=gen)[:P].to(dev)]
    sb = SkinBinding.from_euclidean(verts, node_xyz, 8)
    trans = (0.05 * torch.randn(T, P, 3, generator=gen)).to(dev).requires_grad_()
    rots = random_quats(gen, (T, P), max_angle=0.3).to(dev).requires_grad_()
    cplx = torch.randn(N, 2, generator=gen).to(dev)
    log_scales = initial_log_scales(verts, mb)
    rotation0 = bound_gaussians(verts, cplx, log_scales, mb, THICKNESS)[2]
    vx, vr, _ = skin_vertices(verts, node_xyz, trans, rots, sb, "dqs")
    xyz, rotation, normals, _ = timed_gaussians(vx, vr, rotation0, mb)
    scaling = torch.cat([torch.full((N, 1), THICKNESS, device=dev), torch.exp(log_scales)], -1)
    colors = torch.rand(N, 3, generator=gen).to(dev)
    opacities = (torch.rand(N, 1, generator=gen) * 0.39 + 0.6).to(dev)
    loss = 0
    for t in range(T):  # each view is given its frame's Gaussians
        m2 = torch.zeros((N, 3), device=dev, requires_grad=True)
        c, r, d, a, c2 = rasterize_views([_settings(make_camera(64, 64), [0.0, 0.0, 0.0], 0)], xyz[t], [m2], opacities,
                                         colors_precomp=colors, scales=scaling, rotations=rotation[t],
                                         colors2=normals[t])
        assert c.shape == (1, 3, 64, 64) and c2.shape == (1, 3, 64, 64) and float(a.detach().max()) > 0.5
        u = [torch.randn(x.shape, generator=gen).to(dev) for x in (c, d, a, c2)]
        loss = loss + (c * u[0]).sum() + (d * u[1]).sum() + (a * u[2]).sum() + (c2 * u[3]).sum()
    loss.backward()
    for name, x in (("node_trans", trans), ("node_rots", rots)):
        assert x.grad is not None and torch.isfinite(x.grad).all(), name
        assert all(x.grad[t].any() for t in range(T)), name
