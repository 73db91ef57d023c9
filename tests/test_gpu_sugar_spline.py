"""sugar_spline.spline_attributes (include/gsr.h gsr_sugar_spline_*, csrc/gsr_spline.hip) on the GPU against the fp64
torch restatement of the same formulas (tests/sugar_spline_reference.py, pinned to the reference's own Spline by
tests/test_sugar_spline.py), differentiated by autograd on the CPU, and against the reference's fixture itself.

Bar, the project's rule (``check_against_null`` of tests/sugar_cases.py, which states it): at most twice the error of
the restatement in float32 on the CPU (the "fp32 null", computed here on the same inputs).  Every check prints both.
Knot rotations keep the null itself away from Log's branch at theta = +-pi: angles within +-1.2 rad, so two adjacent
knots are at most 2.4 rad apart; both signs of w, norms in [0.5, 1.5], some rows exactly the identity.
"""
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_dynamic_reference as dyn_ref  # noqa: E402
import sugar_spline_reference as ref  # noqa: E402
from sugar_cases import NullCase, backprop, check_against_null, random_quats  # noqa: E402

F32 = torch.float32
IDENTITY = [0.0, 0.0, 0.0, 1.0]


class _Spline(NullCase):
    """Random knots, timestamps and upstream gradients; reference and null computed once per set of gradients."""

    def __init__(self, grid, timestamps, P, scales, seed=0, identity=False):
        gen = torch.Generator().manual_seed(seed)
        self.grid, n = grid, grid.n_knots
        self.t = torch.as_tensor(timestamps, dtype=F32)
        T = len(self.t)
        if identity:  # the training start
            self.inputs = dict(knots_xyz=torch.zeros(n, P, 3), knots_rot=torch.tensor(IDENTITY).expand(n, P, 4).clone())
        else:
            self.inputs = dict(knots_xyz=torch.randn(n, P, 3, generator=gen),
                               knots_rot=random_quats(gen, (n, P), max_angle=1.2))
        self.inputs["knots_scale"] = 0.1 * torch.randn(n, P, 3, generator=gen) if scales else None
        self.ups = {"xyz": torch.randn(T, P, 3, generator=gen), "rot": torch.randn(T, P, 4, generator=gen)}
        if scales:
            self.ups["scale"] = torch.randn(T, P, 3, generator=gen)
        self.keys = self.outputs + tuple("d" + k for k in ref.SPLINE_INPUTS if self.inputs[k] is not None)

    def evaluate(self, dtype, ups):
        return ref.evaluate(dtype, self.inputs, self.grid, self.t, ups)

    def gpu(self, which=None):
        from sugar_spline import spline_attributes

        leaves = [None if self.inputs[k] is None else self.inputs[k].cuda().requires_grad_() for k in ref.SPLINE_INPUTS]
        out = spline_attributes(self.t.cuda(), leaves[0], leaves[1], self.grid, leaves[2])
        assert (out[2] is None) == (self.inputs["knots_scale"] is None)
        return backprop(out, ref.SPLINE_OUTPUTS, leaves, ["d" + k for k in ref.SPLINE_INPUTS], self.ups,
                        which or self.outputs)


def _grid(degree, n_knots=7):
    from sugar_spline import SplineGrid

    return SplineGrid(degree, 0.3, -0.3, n_knots)  # knots at -0.3, 0, 0.3, ...


# below the range, in three segments (two in one), on a knot time, above the range
TIMES = [-0.5, 0.35, 0.5, 0.6, 2.0]


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 3])
def test_one_of_everything(degree):
    """(T, P, n_knots) = (1, 1, degree + 1): the only segment there is."""
    case = _Spline(_grid(degree, degree + 1), [0.1], 1, True, seed=1)
    case.check(case.gpu(), tag=f"T=P=1 degree {degree}")


@pytest.mark.gpu
@pytest.mark.parametrize("scales", [False, True])
@pytest.mark.parametrize("degree", [1, 3])
def test_across_a_wave_and_a_block(degree, scales):
    """(T, P, n_knots) = (5, 257, 7): P crosses a wave and a block of 256; timestamps outside the range on both sides
    (clamped), two in one segment and one on a knot time; knots with w < 0 and of non-unit norm."""
    case = _Spline(_grid(degree), TIMES, 257, scales, seed=10 * degree + scales)
    q = case.inputs["knots_rot"]
    assert (q[..., 3] < 0).any() and float((q.norm(dim=-1) - 1).abs().max()) > 0.3
    first = ref.segments(case.grid, case.t)[0].tolist()
    assert first[1] == first[2] and len(set(first)) >= 3
    case.check(case.gpu(), tag=f"T=5 P=257 degree {degree} scales={scales}")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 3])
def test_uncovered_knots_get_exactly_zero(degree):
    """Five timestamps in one segment: the knots outside it get exactly 0.0."""
    case = _Spline(_grid(degree), [0.31, 0.35, 0.4, 0.5, 0.59], 257, True, seed=3)
    first = ref.segments(case.grid, case.t)[0]
    assert len(set(first.tolist())) == 1
    covered = set(range(int(first[0]), int(first[0]) + degree + 1))
    got = case.gpu()
    case.check(got, tag=f"one segment degree {degree}")
    for k in ("dknots_xyz", "dknots_rot", "dknots_scale"):
        for j in range(7):
            if j in covered:
                assert got[k][j].any(), (k, j)
            else:
                assert not got[k][j].any() and not torch.signbit(got[k][j]).any(), (k, j)  # exactly 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 3])
def test_identity_knots(degree):
    """The training start: every knot rotation the identity, no translation.  The outputs are exact."""
    case = _Spline(_grid(degree), TIMES, 257, False, seed=4, identity=True)
    got = case.gpu()
    assert torch.equal(got["rot"], torch.tensor(IDENTITY).expand(5, 257, 4)) and not got["xyz"].any()
    for k in case.keys:
        assert torch.isfinite(got[k]).all(), k
    case.check(got, tag=f"identity knots degree {degree}")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 3])
def test_many_timestamps_per_knot(degree):
    """T = 70 timestamps over the 32 knots of SplineGrid.for_frames(32): the second pass adds many rows per knot."""
    from sugar_spline import SplineGrid

    gen = torch.Generator().manual_seed(5)
    t = torch.rand(70, generator=gen) * 1.2 - 0.1  # some beyond [0, 1]
    case = _Spline(SplineGrid.for_frames(32, degree), t, 33, True, seed=6)
    case.check(case.gpu(), tag=f"T=70 n_knots=32 degree {degree}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("xyz",), ("rot",)])
def test_partial_upstream_gradients(which):
    case = _Spline(_grid(3), TIMES, 257, True, seed=7)
    got = case.gpu(which)
    case.check(got, which, tag=f"spline only {which[0]}")
    assert not got["dknots_scale"].any()
    other = "dknots_rot" if which == ("xyz",) else "dknots_xyz"
    assert not got[other].any() and got["dknots_xyz" if which == ("xyz",) else "dknots_rot"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 3])
def test_bitwise_repeatable(degree):
    case = _Spline(_grid(degree), TIMES, 257, True, seed=8)
    a, b = case.gpu(), case.gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("degree", [1, 3])
def test_reference_fixture(degree, scale):
    """The reference's own Spline (tests/golden/reference_spline.npz), as tests/test_gpu_reference_pins.py compares the
    other stages: the null is the reference's float32 run.  The float64 unit quaternions reach the kernel rounded to
    float32, as they reached that run."""
    from sugar_cases import fixture
    from sugar_spline import spline_attributes

    z = fixture("spline")
    leaves = [z[k].to(F32).cuda().requires_grad_() if scale or k != "knots_scale" else None for k in ref.SPLINE_INPUTS]
    out = spline_attributes(z["timestamps"].cuda(), leaves[0], leaves[1], ref.fixture_grid(z, degree), leaves[2])
    assert (out[2] is None) == (not scale)
    names = ("xyz", "rotation", "scale")[:3 if scale else 2]
    got = backprop(out, names, leaves, ["d" + k for k in ref.SPLINE_INPUTS], {k: z[f"up_{k}"].to(F32) for k in names},
                   names)
    keys = tuple(k for k in ref.SPLINE_KEYS if k in got)
    assert len(keys) == (6 if scale else 4)
    r64, r32 = ({k: z[f"deg{degree}_{k}_{tag}"] for k in keys} for tag in ("f64", "f32"))
    check_against_null(got, r64, r32, keys, f"fixture degree {degree} scale={scale}")


@pytest.mark.gpu
def test_chain_to_the_timed_gaussians():
    """spline_attributes -> skin_vertices -> timed_gaussians on icosphere(0): the outputs and the gradients to the
    knots against the composed restatements, under the same rule."""
    from sugar_dynamic import SkinBinding, skin_vertices, timed_gaussians
    from sugar_mesh import MeshBinding
    from sugar_spline import SplineGrid, spline_attributes

    v, f = gs.icosphere(0)
    verts, faces = torch.tensor(v, dtype=F32), torch.tensor(f)
    mb = MeshBinding.from_reference_count(faces, len(v), 3)
    gen = torch.Generator().manual_seed(9)
    P, N, n = 5, mb.n_gaussians, 8
    grid = SplineGrid.for_frames(n)
    t = torch.tensor([0.0, 0.37, 0.41, 1.0])
    T = len(t)
    node_xyz = verts[torch.randperm(len(v), generator=gen)[:P]]
    sb = SkinBinding.from_euclidean(verts, node_xyz, 3)
    knots = dict(knots_xyz=0.2 * torch.randn(n, P, 3, generator=gen),
                 knots_rot=random_quats(gen, (n, P), max_angle=0.8),
                 knots_scale=0.1 * torch.randn(n, P, 3, generator=gen))
    rotation0 = torch.nn.functional.normalize(torch.randn(N, 4, generator=gen), dim=-1)
    log_scales = 0.3 * torch.randn(N, 2, generator=gen) - 4
    thickness = 3.5e-6
    names = ("xyz", "rotation", "normals", "scaling")
    ups = {k: torch.randn(T, N, 4 if k == "rotation" else 3, generator=gen) for k in names}

    def composed(dtype):
        leaves = {k: x.to(dtype).requires_grad_() for k, x in knots.items()}
        nt, nr, ns = ref.spline_reference(t, leaves["knots_xyz"], leaves["knots_rot"], grid, leaves["knots_scale"])
        vx, vr, vs = dyn_ref.skin_vertices_reference(verts.to(dtype), node_xyz.to(dtype), nt, nr, sb.nbr.long(), sb.w,
                                                     "dqs", ns)
        out = dyn_ref.timed_gaussians_reference(vx, vr, rotation0.to(dtype), faces, mb.bary, vs, log_scales.to(dtype),
                                                thickness)
        loss = sum((o * ups[k].to(dtype)).sum() for k, o in zip(names, out))
        grads = torch.autograd.grad(loss, list(leaves.values()))
        res = {k: o.detach() for k, o in zip(names, out)}
        res.update({"d" + k: g for k, g in zip(leaves, grads)})
        return res

    r64, r32 = composed(torch.float64), composed(F32)
    leaves = {k: x.cuda().requires_grad_() for k, x in knots.items()}
    nt, nr, ns = spline_attributes(t.cuda(), leaves["knots_xyz"], leaves["knots_rot"], grid, leaves["knots_scale"])
    vx, vr, vs = skin_vertices(verts.cuda(), node_xyz.cuda(), nt, nr, sb.to("cuda"), "dqs", ns)
    out = timed_gaussians(vx, vr, rotation0.cuda(), mb.to("cuda"), vs, log_scales.cuda(), thickness)
    got = backprop(out, names, leaves.values(), ["d" + k for k in leaves], ups, names)
    check_against_null(got, r64, r32, tuple(got), "spline -> skin -> timed")
