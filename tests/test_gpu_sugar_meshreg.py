"""sugar_meshreg.normal_consistency / laplacian_smoothing (include/gsr.h gsr_sugar_normal_consistency_* /
gsr_sugar_laplacian_*, csrc/gsr_meshreg.hip) on the GPU against the fp64 torch restatements of
tests/sugar_meshreg_reference.py, differentiated by autograd on the CPU (tests/test_sugar_meshreg.py pins them to a
brute-force statement and to closed forms: pytorch3d itself is not available).

Bar (``check_meshreg`` of tests/sugar_meshreg_reference.py).  dvert_xyz under the project's rule
(``check_against_null`` of tests/sugar_cases.py): at most twice the error of the restatement in float32 on the CPU (the
"fp32 null", computed here on the same inputs), exact zeros where the reference is all zero.  The (T,) outputs have too
few elements for the null to be a stable sample: per frame |gpu - ref64| / |ref64| <= max(2 x null, 2^-23), the second
term being one float32 rounding of an fp64 result, doubled; exactly 0 where the reference is exactly 0.  Each check
prints its figures.  The upstream gradient is a random weight per frame; the vertices are the mesh's own plus noise of
0.3 of the mean edge length, except where stated.  Each loss is differentiated on its own and both together.
"""
import pytest

torch = pytest.importorskip("torch")

import sugar_dynamic_reference as dyn_ref  # noqa: E402
import sugar_meshreg_reference as ref  # noqa: E402
from sugar_cases import NullCase, backprop, jittered_icosphere, mesh, random_quats  # noqa: E402

WHICH = (("nc",), ("lap",), ("nc", "lap"))


def _ico(subdiv, seed=0):
    v, f = jittered_icosphere(subdiv, seed=seed)
    return torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f)


class _Case(NullCase):
    """A mesh with noisy vertices and random upstream weights; reference and null computed once per `which`."""

    keys = ("dvert_xyz",)

    def __init__(self, name, T, seed=0, noise=0.3):
        from sugar_meshreg import MeshTopology

        gen = torch.Generator().manual_seed(seed)
        self.verts, self.faces = mesh(name) if isinstance(name, str) else name
        V = len(self.verts)
        self.topo = MeshTopology(self.faces, V)
        self.edges, self.pairs = ref.topology(self.faces, V)
        assert torch.equal(self.topo.pairs.long(), self.pairs) and torch.equal(self.topo.edges.long(), self.edges)
        e = self.edges
        self.edge = float((self.verts[e[:, 0]] - self.verts[e[:, 1]]).norm(dim=-1).mean()) if len(e) else 1.0
        self.xyz = self.verts[None] + noise * self.edge * torch.randn(T, V, 3, generator=gen)
        self.ups = {"nc": torch.randn(T, generator=gen), "lap": torch.randn(T, generator=gen)}

    def evaluate(self, dtype, ups):
        return ref.evaluate(dtype, self.xyz, self.edges, self.pairs, ups)

    def gpu(self, which=("nc", "lap"), ups=None):
        from sugar_meshreg import laplacian_smoothing, normal_consistency

        x, topo = self.xyz.cuda().requires_grad_(), self.topo.to("cuda")
        out = [normal_consistency(x, topo), laplacian_smoothing(x, topo)]
        return backprop(out, ["nc", "lap"], [x], ["dvert_xyz"], self.ups if ups is None else ups, which)

    def check_all(self, tag):
        """Each loss alone and both together; returns what the GPU gave per `which`."""
        got = {}
        for which in WHICH:
            got[which] = self.gpu(which)
            ref.check_meshreg(got[which], *self.reference(which), f"{tag} d({'+'.join(which)})")
        return got


def _positive_zero(t):
    return not t.any() and not torch.signbit(t).any()


@pytest.mark.gpu
def test_single_triangle_has_no_pair():
    """P = 0: nc is exactly 0 with an exactly zero gradient (nothing is launched); every vertex has deg 2."""
    case = _Case("triangle", 1, seed=1)
    assert case.topo.n_pairs == 0 and case.topo.max_valence == 2
    got = case.check_all("triangle")
    assert _positive_zero(got[("nc",)]["nc"]) and _positive_zero(got[("nc",)]["dvert_xyz"])
    assert got[("lap",)]["dvert_xyz"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("tetrahedron", 3), ("icosphere1", 2), ("open_fan", 2)])
def test_small_meshes(name, T):
    """The tetrahedron is closed: every edge has its pair and every vertex occurs as an edge end and as a third vertex.
    icosphere(1) has valences 5 and 6.  The open fan has boundary edges without a pair and rim ends of valence 2."""
    case = _Case(name, T, seed=2)
    if name == "tetrahedron":
        assert case.topo.n_pairs == case.topo.n_edges == 6
        ends, thirds = (set(case.topo.pairs[:, c].flatten().tolist()) for c in (slice(0, 2), slice(2, 4)))
        assert ends == thirds == {0, 1, 2, 3}
    if name == "open_fan":
        deg = (case.topo.ring_offsets[1:] - case.topo.ring_offsets[:-1]).tolist()
        assert case.topo.n_pairs < case.topo.n_edges and deg[1] == 2 and deg[-1] == 2
    case.check_all(f"{name} T={T}")


@pytest.mark.gpu
def test_fan_of_200_faces():
    """The hub's slot row and ring row (200 entries each: it is the first end of the 200 spokes, the rim edges are
    boundary edges) take the wave's path.  The vertex no face uses gets exactly
    +0.0 from nc and, from lap, the isolated vertex's own term: d = -x, |d| = |x|, so the gradient is g / V x / |x|."""
    case = _Case("fan200", 2, seed=3)
    t = case.topo
    assert int(t.slot_offsets[1] - t.slot_offsets[0]) == 200 == t.max_slots and t.max_valence == 200
    assert int(t.slot_offsets[-1] - t.slot_offsets[-2]) == 0 == int(t.ring_offsets[-1] - t.ring_offsets[-2])
    got = case.check_all("fan200")
    last = got[("nc",)]["dvert_xyz"][:, -1]
    assert _positive_zero(last), last
    x = case.xyz[:, -1].double()
    want = case.ups["lap"].double()[:, None] / t.n_verts * x / x.norm(dim=-1, keepdim=True)
    lone = got[("lap",)]["dvert_xyz"][:, -1].double()
    print("fan200 isolated vertex: lap gradient", lone.tolist(), "closed form", want.tolist())
    assert float((lone - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())


@pytest.mark.gpu
def test_eps_clamp_and_zero_laplacian():
    """ref.clamp_mesh: vertex 12 is in no face; the face (13, 14, 15) is in a pair and is kept collinear, so its normal
    is under cosine_similarity's 1e-8 clamp and the gradients through it (~1e8 times the others) are torch's own.  Frame
    0: vertex 15 is one float32 step off the line (0 < |n| < 1e-8).  Frame 1: vertex 15 is exactly the mean of its ring
    (13, 14), so the normal is exactly 0 and d_15 = 0, whose gradient contribution is 0.  The vertices of the collinear
    face carry no noise.  The clamped pair's corners (13 .. 16) and the rest are held to the bar separately, as the bar
    is relative to a tensor's largest entry."""
    case = _Case(ref.clamp_mesh(), 2, seed=4)
    x = case.xyz
    x[:, 13:16] = case.verts[13:16]
    x[0, 15, 1] += 2.0 ** -23
    x[1, 13:15] = (x[1, 13:15] + 0.05 * torch.randn(2, 3, generator=torch.Generator().manual_seed(5))
                   ).mul(4096).round().div(4096)
    x[1, 15] = (x[1, 13] + x[1, 14]) / 2
    assert torch.equal(x[1, 15].double(), (x[1, 13].double() + x[1, 14].double()) / 2)
    assert case.topo.ring[int(case.topo.ring_offsets[15]):int(case.topo.ring_offsets[16])].tolist() == [13, 14]
    p = [i for i, row in enumerate(case.pairs.tolist()) if row[:2] == [13, 14]]
    assert len(p) == 1 and sorted(case.pairs[p[0], 2:].tolist()) == [15, 16]
    xd = x.double()
    n = torch.cross(xd[:, 14] - xd[:, 13], xd[:, 15] - xd[:, 13], dim=-1).norm(dim=-1)
    assert 0 < float(n[0]) < 1e-8 and float(n[1]) == 0
    for which in WHICH:
        got = case.gpu(which)
        r64, r32 = case.reference(which)
        tag = f"clamp d({'+'.join(which)})"
        ref.check_meshreg(got, r64, r32, tag, grads=())
        for part, rows in (("clamped pair", slice(13, 17)), ("rest", slice(0, 13))):
            ref.check_against_null(*({"dvert_xyz": d["dvert_xyz"][:, rows]} for d in (got, r64, r32)), ("dvert_xyz",),
                                   f"{tag} {part}")
        if "nc" in which:
            assert float(r64["dvert_xyz"][:, 13:17].abs().max()) > 1e4  # the clamp's 1 / eps acts
    # d_15 = 0 in frame 1: vertex 15 gets only what its neighbours' terms send it, and no NaN
    r64, _ = case.reference(("lap",))
    assert torch.isfinite(r64["dvert_xyz"]).all() and r64["dvert_xyz"][1, 15].any()
    got = case.gpu(("nc",))["dvert_xyz"]
    assert _positive_zero(got[:, 12])  # the vertex in no face: exactly +0.0 from nc


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["book", "duplicated_face"])
def test_non_manifold(name):
    """Three faces on one edge give three pairs; a duplicated face gives pairs with c0 == c1, whose two rows go to one
    vertex."""
    case = _Case(getattr(ref, name)(), 1, seed=6)
    if name == "book":
        assert case.topo.n_pairs == 3
    else:
        assert int((case.topo.pairs[:, 2] == case.topo.pairs[:, 3]).sum()) == 3
    case.check_all(name)


@pytest.mark.gpu
def test_icosphere3_has_several_block_sums():
    """V = 642, P = 1920: three and eight blocks per frame, the last not whole."""
    case = _Case(_ico(3), 2, seed=7)
    assert (case.topo.n_verts, case.topo.n_pairs) == (642, 1920)
    case.check_all("icosphere(3)")


@pytest.mark.gpu
def test_bitwise_repeatable():
    case = _Case("fan200", 3, seed=8)
    a, b = case.gpu(), case.gpu()
    assert set(a) == {"nc", "lap", "dvert_xyz"}
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("which", WHICH[:2])
def test_a_frame_without_upstream_gradient_gets_exact_zeros(which):
    case = _Case("icosphere1", 3, seed=9)
    ups = {k: v.clone() for k, v in case.ups.items()}
    for v in ups.values():
        v[1] = 0.0
    got, full = case.gpu(which, ups)["dvert_xyz"], case.gpu(which)["dvert_xyz"]
    assert _positive_zero(got[1]) and full[1].any()
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])


@pytest.mark.gpu
def test_empty_batches_launch_nothing():
    from sugar_meshreg import MeshTopology, laplacian_smoothing, normal_consistency

    topo = MeshTopology(mesh("tetrahedron")[1], 4).to("cuda")
    none = MeshTopology(torch.zeros((0, 3), dtype=torch.int64), 0).to("cuda")
    for fn in (normal_consistency, laplacian_smoothing):
        x = torch.zeros(0, 4, 3, device="cuda", requires_grad=True)
        out = fn(x, topo)
        assert out.shape == (0,)
        out.sum().backward()
        assert x.grad.shape == (0, 4, 3)
        x = torch.zeros(2, 0, 3, device="cuda", requires_grad=True)
        out = fn(x, none)
        assert out.tolist() == [0, 0]
        out.sum().backward()
        assert x.grad.shape == (2, 0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_chain_from_the_skinning(method):
    """skin_vertices -> normal_consistency + laplacian_smoothing on icosphere(2) under a 20-node graph: the gradients
    that reach node_trans and node_rots against the chained fp64 restatements, and their float32 null."""
    from sugar_dynamic import SkinBinding, skin_vertices
    from sugar_meshreg import MeshTopology, laplacian_smoothing, normal_consistency

    verts, faces = _ico(2, seed=7)
    T, V, P, K = 3, len(verts), 20, 8
    gen = torch.Generator().manual_seed(10)
    node_xyz = verts[torch.randperm(V, generator=gen)[:P]].clone()
    sb, topo = SkinBinding.from_euclidean(verts, node_xyz, K), MeshTopology(faces, V)
    edges, pairs = ref.topology(faces, V)
    trans, rots = 0.1 * torch.randn(T, P, 3, generator=gen), random_quats(gen, (T, P), max_angle=0.8)
    up_nc, up_lap = torch.randn(T, generator=gen), torch.randn(T, generator=gen)

    def restated(dt):
        t, q = trans.to(dt).requires_grad_(), rots.to(dt).requires_grad_()
        xyz, _, _ = dyn_ref.skin_vertices_reference(verts.to(dt), node_xyz.to(dt), t, q, sb.nbr.long(), sb.w, method)
        nc, lap = ref.normal_consistency_reference(xyz, pairs), ref.laplacian_reference(xyz, edges)
        gt, gq = torch.autograd.grad((nc * up_nc.to(dt)).sum() + (lap * up_lap.to(dt)).sum(), [t, q])
        return {"nc": nc.detach(), "lap": lap.detach(), "dnode_trans": gt, "dnode_rots": gq}

    r64, r32 = restated(torch.float64), restated(torch.float32)
    t, q = trans.cuda().requires_grad_(), rots.cuda().requires_grad_()
    xyz, _, _ = skin_vertices(verts.cuda(), node_xyz.cuda(), t, q, sb.to("cuda"), method)
    nc, lap = normal_consistency(xyz, topo.to("cuda")), laplacian_smoothing(xyz, topo.to("cuda"))
    gt, gq = torch.autograd.grad((nc * up_nc.cuda()).sum() + (lap * up_lap.cuda()).sum(), [t, q])
    got = {"nc": nc.detach().cpu(), "lap": lap.detach().cpu(), "dnode_trans": gt.cpu(), "dnode_rots": gq.cpu()}
    assert r64["dnode_trans"].any() and r64["dnode_rots"].any()
    ref.check_meshreg(got, r64, r32, f"chain {method}", grads=("dnode_trans", "dnode_rots"))
