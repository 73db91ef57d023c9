"""sugar_deform.deformation_knots (include/gsr.h gsr_sugar_deform_*, csrc/gsr_deform.hip) on the GPU against the fp64
torch restatement of the same formulas (tests/sugar_deform_reference.py, pinned to the reference's own
DeformationNetwork by tests/test_sugar_deform.py), differentiated by autograd on the CPU, and against the reference's
fixture itself.

Bar, the project's rule (``check_against_null`` of tests/sugar_cases.py, which states it): at most twice the error of
the restatement in float32 on the CPU (the "fp32 null", computed here on the same inputs).  Every check prints both.
Small planes (resolution (4, 5, 6, 3), multires (1, 2)) unless stated; random planes, MLP and upstream gradients.
"""
import pytest

torch = pytest.importorskip("torch")

import sugar_deform_reference as ref  # noqa: E402
from sugar_cases import NullCase, backprop, check_against_null  # noqa: E402

F32 = torch.float32
RESOLUTION, MULTIRES = (4, 5, 6, 3), (1, 2)
AABB = torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])


def random_weights(gen, resolution=RESOLUTION, multires=MULTIRES, d_scale=True):
    """The reference's shapes with every tensor random: planes U(0.1, 1.5), the MLP N(0, 0.3)."""
    from sugar_deform import DeformationWeights

    w = DeformationWeights.init_like_reference(gen, resolution, multires, d_scale)
    with torch.no_grad():
        for p in w.planes:
            p.copy_(torch.rand(p.shape, generator=gen) * 1.4 + 0.1)
        for t in w.mlp:
            t.copy_(torch.randn(t.shape, generator=gen) * 0.3)
    return w


class _Deform(NullCase):
    """Points, ticks, weights and upstream gradients; reference and null computed once per set of gradients."""

    def __init__(self, points, ticks, weights, normalize=True, d_scale=True, seed=0, resolution=RESOLUTION,
                 multires=MULTIRES):
        gen = torch.Generator().manual_seed(1000 + seed)
        self.points, self.ticks = torch.as_tensor(points, dtype=F32), torch.as_tensor(ticks, dtype=F32)
        self.w, self.normalize, self.d_scale = weights, normalize, d_scale
        self.resolution, self.multires = resolution, multires
        self.mlp = weights.mlp[:14 if d_scale else 10]
        T, P = len(self.ticks), len(self.points)
        self.ups = {"xyz": torch.randn(T, P, 3, generator=gen), "rot": torch.randn(T, P, 4, generator=gen)}
        if d_scale:
            self.ups["scale"] = torch.randn(T, P, 3, generator=gen)
        self.keys = ref.keys(len(weights.planes), len(self.mlp))

    def evaluate(self, dtype, ups):
        return ref.evaluate(dtype, self.points, self.ticks, AABB, self.w.planes, self.mlp, ups, self.normalize)

    def gpu(self, which=None):
        from sugar_deform import HexPlaneBinding, deformation_knots

        binding = HexPlaneBinding(self.points, self.ticks, AABB, self.resolution, self.multires).to("cuda")
        w = self.w.to("cuda").requires_grad_()
        out = deformation_knots(binding, w, self.normalize, self.d_scale)
        assert (out[2] is None) == (not self.d_scale)
        return backprop(out, ref.OUTPUTS, w.planes + w.mlp[:len(self.mlp)], self.keys[len(self.ups):], self.ups,
                        which or self.outputs)


def _points(P, gen, spread=1.3):
    return torch.rand(P, 3, generator=gen) * 2 * spread - spread


TICKS = [-0.1, 0.0, 0.45, 1.0, 1.2]  # below 0, on the first and the last time texel, above 1


@pytest.mark.gpu
def test_one_of_everything():
    gen = torch.Generator().manual_seed(1)
    case = _Deform(_points(1, gen, 0.9), [0.3], random_weights(gen), seed=1)
    case.check(case.gpu(), tag="T=P=1")


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("d_scale", [True, False])
def test_across_a_wave_and_a_block(d_scale, normalize):
    """(T, P) = (5, 257): more points than a wave, than the 8 waves of a block and than one round of 32 blocks."""
    gen = torch.Generator().manual_seed(2)
    case = _Deform(_points(257, gen), TICKS, random_weights(gen), normalize, d_scale, seed=2)
    case.check(case.gpu(), tag=f"T=5 P=257 d_scale={d_scale} normalize={normalize}")


@pytest.mark.gpu
def test_border_and_corners():
    gen = torch.Generator().manual_seed(3)
    points = _points(40, gen)
    points[0] = torch.tensor([0.3, 0.5, -0.2])  # y: n = -0.5, exactly texel 1 of the first level's 5
    points[1] = -1.0  # n = +1: the upper edge of every axis
    points[2] = 1.0   # n = -1: the lower edge
    case = _Deform(points, TICKS, random_weights(gen), seed=3)
    n = ref.normalize_aabb(case.points.double(), AABB.double())
    for d in range(3):
        assert (n[:, d] < -1).any() and (n[:, d] > 1).any()  # beyond the box on both sides of every axis
    assert float((n[0, 1] + 1) / 2 * 4) == 1.0 and (n[1] == 1).all()
    assert (case.ticks < 0).any() and (case.ticks > 1).any()
    case.check(case.gpu(), tag="border and corners")


@pytest.mark.gpu
def test_crowded_and_empty_texels():
    """70 points inside one cell of the coarsest level: rows longer than a wave; most texels untouched."""
    gen = torch.Generator().manual_seed(4)
    points = torch.rand(70, 3, generator=gen) * 0.1 + torch.tensor([0.05, 0.05, 0.05])
    case = _Deform(points, [0.2, 0.3], random_weights(gen), seed=4)
    from sugar_deform import HexPlaneBinding

    b = HexPlaneBinding(case.points, case.ticks, AABB, RESOLUTION, MULTIRES)
    assert all(len(set(b.cell[0, d].tolist())) == 1 for d in range(3))
    assert int((b.sp_offsets[1:] - b.sp_offsets[:-1]).max()) >= 70
    got = case.gpu()
    case.check(got, tag="70 points in one cell")
    r64 = case.reference(tuple(case.ups))[0]
    empty = 0
    for i in range(12):
        g, want = got[f"dplane{i}"], r64[f"dplane{i}"]
        untouched = want == 0
        empty += int(untouched.sum())
        assert not g[untouched].any() and not torch.signbit(g[untouched]).any(), i  # exactly +0.0
        assert (g[~untouched] != 0).all(), i
    assert empty > 1000


@pytest.mark.gpu
def test_training_start():
    """init_like_reference: zero heads.  The knots are exact and only the final layers get a gradient."""
    from sugar_deform import DeformationWeights

    gen = torch.Generator().manual_seed(5)
    w = DeformationWeights.init_like_reference(gen, RESOLUTION, MULTIRES)
    case = _Deform(_points(257, gen), TICKS, w, seed=5)
    got = case.gpu()
    assert not got["xyz"].any() and not got["scale"].any()
    assert torch.equal(got["rot"], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(5, 257, 4))
    final = {"dmlp4", "dmlp5", "dmlp8", "dmlp9", "dmlp12", "dmlp13"}
    for k in case.keys[3:]:
        assert got[k].any() == (k in final), k
    case.check(got, tag="training start")


@pytest.mark.gpu
def test_dead_hidden_units():
    """A feature_out bias that keeps hidden units 0..9 negative for every sample: relu' = 0 there."""
    gen = torch.Generator().manual_seed(6)
    w = random_weights(gen)
    with torch.no_grad():
        w.mlp[1][:10] = -1e4
    case = _Deform(_points(257, gen), TICKS, w, seed=6)
    got = case.gpu()
    case.check(got, tag="dead units")
    assert not got["dmlp0"][:10].any() and not got["dmlp1"][:10].any() and got["dmlp0"][10:].any()
    for i in (2, 6, 10):  # the residual layers read relu(h): the dead units' columns
        assert not got[f"dmlp{i}"][:, :10].any() and got[f"dmlp{i}"][:, 10:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("xyz",), ("rot",)])
def test_partial_upstream_gradients(which):
    gen = torch.Generator().manual_seed(7)
    case = _Deform(_points(257, gen), TICKS, random_weights(gen), seed=7)
    got = case.gpu(which)
    case.check(got, which, tag=f"only {which[0]}")
    mine, other = ((2, 6), (6, 2)) if which == ("xyz",) else ((6, 2), (2, 6))
    for i in range(4):
        assert not got[f"dmlp{other[0] + i}"].any() and not got[f"dmlp{10 + i}"].any()
        assert got[f"dmlp{mine[0] + i}"].any()


@pytest.mark.gpu
def test_bitwise_repeatable():
    gen = torch.Generator().manual_seed(8)
    case = _Deform(_points(257, gen), TICKS, random_weights(gen), seed=8)
    a, b = case.gpu(), case.gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dg", "dg_noscale", "vert"])
def test_reference_fixture(case):
    """The reference's own DeformationNetwork (tests/golden/reference_deform.npz): the null is its float32 run."""
    from sugar_deform import HexPlaneBinding, deformation_knots

    z = ref.fixture()
    normalize, d_scale = ref.CASES[case]
    w = ref.fixture_weights(z, d_scale)
    r64, r32 = (ref.fixture_reference(z, case, tag, w) for tag in ("f64", "f32"))
    binding = HexPlaneBinding(z["points"], z["ticks"], z["aabb"], RESOLUTION, MULTIRES).to("cuda")
    wg = w.to("cuda").requires_grad_()
    out = deformation_knots(binding, wg, normalize, d_scale)
    ups = {k: up.to(F32) for k, up in ref.fixture_ups(z, d_scale).items()}
    got = backprop(out, ref.OUTPUTS, wg.parameters(), ref.keys(12, len(w.mlp))[len(ups):], ups, tuple(ups))
    keys = tuple(k for k in got if k in r64)
    assert len(keys) == {"dg": 29, "dg_noscale": 11, "vert": 15}[case]
    check_against_null(got, r64, r32, keys, f"fixture {case}")


@pytest.mark.gpu
def test_shipped_resolution():
    """(64, 64, 64, 25) x (1, 2, 4, 8) at (T, P) = (5, 257): the 512^2 planes and the offsets of four levels."""
    gen = torch.Generator().manual_seed(10)
    res, mul = (64, 64, 64, 25), (1, 2, 4, 8)
    case = _Deform(_points(257, gen, 1.1), TICKS, random_weights(gen, res, mul), seed=10, resolution=res, multires=mul)
    case.check(case.gpu(), tag="shipped resolution")


@pytest.mark.gpu
def test_chain_to_the_skinned_vertices():
    """deformation_knots -> spline_attributes -> skin_vertices on icosphere(0) with 5 nodes, against the composed
    restatements under the same rule."""
    import gsr_synthetic as gs
    import sugar_dynamic_reference as dyn_ref
    import sugar_spline_reference as spline_ref
    from sugar_deform import HexPlaneBinding, deformation_knots
    from sugar_dynamic import SkinBinding, skin_vertices
    from sugar_spline import SplineGrid, spline_attributes

    v, _ = gs.icosphere(0)
    verts = torch.tensor(v, dtype=F32) * 0.8
    gen = torch.Generator().manual_seed(11)
    P, n = 5, 8
    grid = SplineGrid.for_frames(n)
    ticks = torch.linspace(float(grid.start_time), float(grid.end_time), n)
    t = torch.tensor([0.0, 0.37, 0.41, 1.0])
    node_xyz = verts[torch.randperm(len(v), generator=gen)[:P]].contiguous()
    sb = SkinBinding.from_euclidean(verts, node_xyz, 3)
    w = random_weights(gen)
    with torch.no_grad():  # small deformations: the knots' rotations stay near the identity
        for i in (4, 5, 8, 9, 12, 13):
            w.mlp[i].mul_(0.1)
    names = ("xyz", "rot", "scale")
    ups = {k: torch.randn(len(t), len(v), 4 if k == "rot" else 3, generator=gen) for k in names}
    keys = names + ref.keys(12, 14)[3:]

    def composed(dtype):
        pl = [x.detach().to(dtype).requires_grad_() for x in w.planes]
        ml = [x.detach().to(dtype).requires_grad_() for x in w.mlp]
        kx, kr, ks = ref.deformation_reference(node_xyz.to(dtype), ticks.to(dtype), AABB.to(dtype), pl, ml, True)
        nt, nr, ns = spline_ref.spline_reference(t, kx, kr, grid, ks)
        out = dyn_ref.skin_vertices_reference(verts.to(dtype), node_xyz.to(dtype), nt, nr, sb.nbr.long(), sb.w, "dqs",
                                              ns)
        loss = sum((o * ups[k].to(dtype)).sum() for k, o in zip(names, out))
        grads = torch.autograd.grad(loss, pl + ml)
        res = {k: o.detach() for k, o in zip(names, out)}
        res.update({k: g for k, g in zip(keys[3:], grads)})
        return res

    r64, r32 = composed(torch.float64), composed(F32)
    wg = w.to("cuda").requires_grad_()
    binding = HexPlaneBinding(node_xyz, ticks, AABB, RESOLUTION, MULTIRES).to("cuda")
    kx, kr, ks = deformation_knots(binding, wg)
    nt, nr, ns = spline_attributes(t.cuda(), kx, kr, grid, ks)
    out = skin_vertices(verts.cuda(), node_xyz.cuda(), nt, nr, sb.to("cuda"), "dqs", ns)
    got = backprop(out, names, wg.parameters(), keys[3:], ups, names)
    check_against_null(got, r64, r32, keys, "deform -> spline -> skin")
