"""sugar_arap.arap_energy (include/gsr.h gsr_sugar_arap_*, csrc/gsr_arap.hip) on the GPU against the fp64 torch
restatement of the reference's padded per-frame computation (tests/sugar_arap_reference.py), differentiated by
autograd on the CPU.

Bar (``check_arap`` of tests/sugar_arap_reference.py).  Per gradient tensor the project's rule (``check_against_null``
of tests/sugar_cases.py): at most twice the error of the restatement in float32 on the CPU (the "fp32 null", computed
here on the same inputs), exact zeros where the reference is all zero.  The (T,) energy has too few elements for the
null to be a stable sample: per frame |gpu - ref64| / |ref64| <= max(2 x null, 2^-23), the second term being one float32 rounding
of an fp64 result, doubled.  Each check prints its figures.  The upstream gradient is a random weight per frame.
Rest meshes have obtuse corners (negative weights: asserted); the deformed vertices are the rest vertices plus noise
of the edge-length scale; quaternions have norms in [0.5, 1.5] and both signs of w (the matrix formula is not
normalised); matrices are random, not rotations.
"""
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_arap_reference as ref  # noqa: E402
import sugar_dynamic_reference as dyn_ref  # noqa: E402
from sugar_cases import NullCase, backprop, jittered_icosphere, mesh, random_quats  # noqa: E402

FORMS = ("quat", "matrix")


class _Case(NullCase):
    """A rest mesh with random deformed vertices, rotations and upstream weights; reference and null computed once."""

    def __init__(self, name, T, form, seed=0):
        from sugar_arap import ArapBinding

        gen = torch.Generator().manual_seed(seed)
        self.verts, self.faces = mesh(name) if isinstance(name, str) else name
        V = len(self.verts)
        self.binding = ArapBinding(self.verts, self.faces)
        self.rings = ref.one_rings(self.faces, V)
        assert torch.equal(self.binding.nbr.long(), self.rings[1])
        assert bool((self.binding.w < 0).any())  # an obtuse corner
        edge = float(self.binding.p.norm(dim=-1).mean())
        self.xyz = self.verts[None] + 0.3 * edge * torch.randn(T, V, 3, generator=gen)
        self.rot = random_quats(gen, (T, V)) if form == "quat" else (
            torch.eye(3) + 0.4 * torch.randn(T, V, 3, 3, generator=gen))
        self.up = torch.randn(T, generator=gen)
        self.ups = {"energy": self.up}

    def evaluate(self, dtype, ups):
        return ref.evaluate(dtype, self.xyz, self.rot, self.verts, self.rings, self.binding.w, ups["energy"])

    def gpu(self, up=None):
        from sugar_arap import arap_energy

        x, r = self.xyz.cuda().requires_grad_(), self.rot.cuda().requires_grad_()
        e = arap_energy(x, r, self.binding.to("cuda"))
        ups = self.ups if up is None else {"energy": up}
        return backprop([e], ["energy"], [x, r], ["dvert_xyz", "dvert_rot"], ups, ["energy"])

    def check(self, got, tag):
        ref.check_arap(got, *self.reference(self.outputs), tag)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,T", [("triangle", 1), ("tetrahedron", 3), ("icosphere1", 2)])
def test_small_meshes(name, T, form):
    """One triangle: every edge a boundary edge, W has one term each.  The tetrahedron is closed.  icosphere(1) has
    valences 5 and 6."""
    case = _Case(name, T, form, seed=1)
    case.check(case.gpu(), f"{name} T={T} {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_icosphere3_has_several_block_sums(form):
    """V = 642: three blocks per frame, the last not whole."""
    verts, faces = jittered_icosphere(3)
    case = _Case((torch.as_tensor(verts, dtype=torch.float32), torch.as_tensor(faces)), 2, form, seed=2)
    assert case.binding.n_verts == 642
    case.check(case.gpu(), f"icosphere(3) {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fan_of_200_faces(form):
    """One row of valence 200 (the wave's path) among rows of 3, and a vertex no face uses."""
    case = _Case("fan200", 2, form, seed=3)
    off = case.binding.offsets
    assert int(off[1] - off[0]) == 200 and case.binding.max_valence == 200 and int(off[-1] - off[-2]) == 0
    got = case.gpu()
    case.check(got, f"fan {form}")
    for k in ("dvert_xyz", "dvert_rot"):
        assert not got[k][:, -1].any() and not torch.signbit(got[k][:, -1]).any(), k  # exactly 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_isolated_vertex_and_degenerate_face(form):
    case = _Case("isolated_degenerate", 2, form, seed=4)
    got = case.gpu()
    case.check(got, f"isolated + degenerate {form}")
    for k in ("dvert_xyz", "dvert_rot"):
        assert not got[k][:, 12].any() and not torch.signbit(got[k][:, 12]).any(), k  # the empty row: exactly 0.0
        assert got[k][:, 13:].any(), k  # the clamped face's weights are finite and act


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["icosphere1", "fan200"])
def test_rest_pose_is_exactly_zero(name, form):
    from sugar_arap import ArapBinding, arap_energy

    verts, faces = mesh(name)
    T, V = 2, len(verts)
    b = ArapBinding(verts, faces).to("cuda")
    x = verts[None].expand(T, V, 3).contiguous().cuda().requires_grad_()
    ident = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(T, V, 4) if form == "quat" else torch.eye(3).expand(T, V, 3, 3)
    r = ident.contiguous().cuda().requires_grad_()
    e = arap_energy(x, r, b)
    gx, gr = torch.autograd.grad((e * torch.tensor([0.7, -1.3]).cuda()).sum(), [x, r])
    assert e.shape == (T,) and not e.any() and not gx.any() and not gr.any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_bitwise_repeatable(form):
    case = _Case("fan200", 3, form, seed=5)
    a, b = case.gpu(), case.gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_frame_without_upstream_gradient_gets_exact_zeros(form):
    case = _Case("icosphere1", 3, form, seed=6)
    up = case.up.clone()
    up[1] = 0.0
    got = case.gpu(up)
    full = case.gpu()
    for k in ("dvert_xyz", "dvert_rot"):
        assert not got[k][1].any(), k
        assert torch.equal(got[k][0], full[k][0]) and torch.equal(got[k][2], full[k][2]) and full[k][1].any(), k


@pytest.mark.gpu
def test_empty_batches_launch_nothing():
    from sugar_arap import ArapBinding, arap_energy

    b = ArapBinding(*mesh("tetrahedron")).to("cuda")
    x = torch.zeros(0, 4, 3, device="cuda", requires_grad=True)
    e = arap_energy(x, torch.zeros(0, 4, 4, device="cuda"), b)
    assert e.shape == (0,)
    e.sum().backward()
    assert x.grad.shape == (0, 4, 3)
    none = ArapBinding(torch.zeros(0, 3), torch.zeros((0, 3), dtype=torch.int64)).to("cuda")
    assert arap_energy(torch.zeros(2, 0, 3, device="cuda"), torch.zeros(2, 0, 3, 3, device="cuda"), none).tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_chain_from_the_skinning(method):
    """skin_vertices -> arap_energy(vert_xyz, vert_rot) on icosphere(2) under a 20-node graph: the gradients that reach
    node_trans and node_rots against the chained fp64 restatements, and their float32 null."""
    from sugar_arap import ArapBinding, arap_energy
    from sugar_dynamic import SkinBinding, skin_vertices

    v, f = jittered_icosphere(2, seed=7)
    verts, faces = torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f)
    T, V, P, K = 3, len(verts), 20, 8
    gen = torch.Generator().manual_seed(8)
    node_xyz = verts[torch.randperm(V, generator=gen)[:P]].clone()
    sb, ab = SkinBinding.from_euclidean(verts, node_xyz, K), ArapBinding(verts, faces)
    rings = ref.one_rings(faces, V)
    trans, rots = 0.1 * torch.randn(T, P, 3, generator=gen), random_quats(gen, (T, P), max_angle=0.8)
    up = torch.randn(T, generator=gen)

    def restated(dt):
        t, q = trans.to(dt).requires_grad_(), rots.to(dt).requires_grad_()
        xyz, rot, _ = dyn_ref.skin_vertices_reference(verts.to(dt), node_xyz.to(dt), t, q, sb.nbr.long(), sb.w, method)
        e = ref.arap_energy_reference(xyz, rot, verts, *rings, ab.w)
        gt, gq = torch.autograd.grad((e * up.to(dt)).sum(), [t, q])
        return {"energy": e.detach(), "dnode_trans": gt, "dnode_rots": gq}

    r64, r32 = restated(torch.float64), restated(torch.float32)
    t, q = trans.cuda().requires_grad_(), rots.cuda().requires_grad_()
    xyz, rot, _ = skin_vertices(verts.cuda(), node_xyz.cuda(), t, q, sb.to("cuda"), method)
    e = arap_energy(xyz, rot, ab.to("cuda"))
    gt, gq = torch.autograd.grad((e * up.cuda()).sum(), [t, q])
    got = {"energy": e.detach().cpu(), "dnode_trans": gt.cpu(), "dnode_rots": gq.cpu()}
    assert r64["dnode_trans"].any() and r64["dnode_rots"].any()
    ref.check_arap(got, r64, r32, f"chain {method}", grads=("dnode_trans", "dnode_rots"))
