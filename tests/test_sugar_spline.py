"""sugar_spline (include/gsr.h gsr_sugar_spline_*) without a GPU: the fp64 restatement of
tests/sugar_spline_reference.py (the checker of the GPU tests) against the fixture computed by the reference's own
``Spline`` (tests/golden/reference_spline.npz, made by tests/golden/make_golden_spline.py) and its properties,
``SplineGrid`` against the reference's float32 bounds, and the argument checks of the Python wrapper and of the C
entries (which precede any device work).  The kernels' numerics are checked on the GPU in
tests/test_gpu_sugar_spline.py.

Bars of the fixture comparison, those of tests/sugar_cases.py for every pinned stage: max |restatement -
fixture| <= 1e-12 max |fixture| on outputs, 1e-10 on gradients, in float64."""
import ctypes

import numpy as np
import pytest

from diff_gaussian_rasterization import _C

torch = pytest.importorskip("torch")

import sugar_spline_reference as ref  # noqa: E402
from sugar_cases import GRAD_BAR, OUT_BAR, close, fixture, null_is_usable, random_quats  # noqa: E402
from sugar_spline import SplineGrid, spline_attributes  # noqa: E402
from sugar_spline_reference import SPLINE_KEYS, fixture_grid  # noqa: E402

NAMES = ("gsr_sugar_spline_workspace_bytes", "gsr_sugar_spline_forward", "gsr_sugar_spline_backward")
D = torch.float64
IDENTITY = [0.0, 0.0, 0.0, 1.0]


def restated(dtype, z, degree, scale=True):
    ups = {k: z[f"up_{n}"] for k, n in (("xyz", "xyz"), ("rot", "rotation"), ("scale", "scale"))}
    inputs = dict(knots_xyz=z["knots_xyz"], knots_rot=z["knots_rot"], knots_scale=z["knots_scale"] if scale else None)
    r = ref.evaluate(dtype, inputs, fixture_grid(z, degree), z["timestamps"], ups)
    r["rotation"] = r.pop("rot")
    return r


def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES


# ---- the grid -------------------------------------------------------------------------------------------------------
def _bits(grid):
    return np.array([grid.start_time, grid.sampling_interval, grid.end_time, grid.t_lower, grid.t_upper, grid.clamp_lo,
                     grid.clamp_hi])


def test_spline_grid_has_the_bits_of_the_reference():
    """start_time, sampling_interval, end_time, t_lower_bound, t_upper_bound and the two clamp bounds of the reference's
    0-dim float32 tensors: the fixture's two grids and init_cubic_spliner's for 14 and 32 frames."""
    z = fixture("spline")
    for degree in (1, 3):
        got = _bits(fixture_grid(z, degree))
        assert got.dtype == np.float32 and np.array_equal(got, z[f"deg{degree}_grid"].numpy()), degree
    for n in (14, 32):
        got = _bits(SplineGrid.for_frames(n))
        assert got.dtype == np.float32 and np.array_equal(got, z[f"frames{n}_grid"].numpy()), n
    lin = SplineGrid.for_frames(14, degree=1)
    assert lin.t_lower == lin.start_time and lin.t_upper == lin.end_time and lin.n_knots == 14
    # a tensor is taken as its number
    g = SplineGrid(3, torch.tensor(0.3), -torch.tensor(0.3), 7)
    assert np.array_equal(_bits(g), z["deg3_grid"].numpy())


def test_for_frames_keeps_the_unit_interval_inside_the_knots():
    """t = 0 and t = 1 (and the clamped values beyond them) fall into segments whose four knots exist, before the
    kernels' own clamp of the index."""
    for n in (4, 14, 32):
        grid = SplineGrid.for_frames(n)
        t = torch.tensor([0.0, 1.0, -3.0, 7.0, 0.5])
        first, u = ref.segments(grid, t, clamp_index=False)
        assert int(first.min()) >= 0 and int(first.max()) + 3 <= n - 1, (n, first)
        assert float(u.min()) >= 0 and float(u.max()) < 1
        assert int(first[0]) == 0 and int(first[1]) == n - 4
        assert torch.equal(ref.segments(grid, t)[0], first)


def test_spline_grid_argument_errors():
    bad = [(2, 0.1, 0.0, 8), (3.0, 0.1, 0.0, 8), (True, 0.1, 0.0, 8), ("3", 0.1, 0.0, 8),  # degree
           (3, 0.1, 0.0, 3), (1, 0.1, 0.0, 1), (3, 0.1, 0.0, 8.0), (3, 0.1, 0.0, True), (3, 0.1, 0.0, 2 ** 31),
           (3, 0.0, 0.0, 8), (3, -0.1, 0.0, 8), (3, float("nan"), 0.0, 8), (3, float("inf"), 0.0, 8),
           (3, "x", 0.0, 8), (3, None, 0.0, 8), (3, torch.zeros(2), 0.0, 8), (3, True, 0.0, 8),
           (3, 0.1, float("inf"), 8), (3, 0.1, None, 8), (3, 0.1, [0.0], 8)]
    for args in bad:
        with pytest.raises(ValueError):
            SplineGrid(*args)
    for n in (3, 0, 4.0, True, None):
        with pytest.raises(ValueError):
            SplineGrid.for_frames(n)
    assert SplineGrid(3, 0.1, 0.0, 4).n_knots == 4 and SplineGrid(1, 0.1, 0.0, 2).n_knots == 2
    assert "degree=3" in repr(SplineGrid.for_frames(8))


# ---- the restatement against the reference's own code ----------------------------------------------------------------
def test_fixture_shapes_what_it_should():
    z = fixture("spline")
    assert z["knots_xyz"].shape == (7, 5, 3) and z["knots_rot"].shape == (7, 5, 4) and z["timestamps"].shape == (6,)
    q = z["knots_rot"]
    assert q.dtype == D and float((q.norm(dim=-1) - 1).abs().max()) < 1e-15
    assert (q[..., 3] > 0).any() and (q[..., 3] < 0).any()
    for degree in (1, 3):
        grid = fixture_grid(z, degree)
        t = z["timestamps"]
        assert (t < float(grid.t_lower)).any() and (t > float(grid.t_upper)).any()  # both clamps act
        first, u = ref.segments(grid, t, clamp_index=False)
        assert int(first.min()) >= 0 and int(first.max()) + degree <= 6  # the reference read no knot out of range
        assert len(set(first.tolist())) < len(first)  # two timestamps share a segment
        knot_times = float(grid.start_time) + float(grid.sampling_interval) * np.arange(1, 6)
        assert any(abs(float(x) - k) < 1e-6 for x in t for k in knot_times)  # one on an interior knot time
        null_is_usable(z, f"deg{degree}_", SPLINE_KEYS)


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("degree", [1, 3])
def test_spline_restatement(degree, scale):
    """spline_reference in float64 against Spline.forward in float64, outputs and the gradients to the knots.  Without
    the scale attribute the reference's other tensors are bitwise the same (asserted by make_golden_spline.py), so the
    same fixture serves.  Measured: outputs <= 2.8e-17 (degree 3: bitwise), gradients <= 1.9e-16."""
    z = fixture("spline")
    got = restated(D, z, degree, scale)
    for k in SPLINE_KEYS:
        if not scale and k in ("scale", "dknots_scale"):
            assert got.get(k) is None
            continue
        close(got[k], z[f"deg{degree}_{k}_f64"], GRAD_BAR if k.startswith("d") else OUT_BAR, f"degree {degree} {k}")


@pytest.mark.parametrize("degree", [1, 3])
def test_float32_restatement_is_the_reference_float32_run_within_rounding(degree):
    """The fp32 null of the GPU tests is what the reference gives in float32, up to float32 rounding: both evaluate the
    same few dozen operations in float32, in different groupings (lerp, bvv and sum against plain expressions), so
    they may differ by some ulps of the largest element; the bar is 2e-6, 17 ulps.  Measured: 1.1e-7 at the most."""
    z = fixture("spline")
    got = restated(torch.float32, z, degree)
    for k in SPLINE_KEYS:
        want = z[f"deg{degree}_{k}_f32"]
        assert got[k].dtype == torch.float32
        err = float((got[k] - want).abs().max()) / float(want.abs().max())
        assert err < 2e-6, (degree, k, err)


@pytest.mark.parametrize("degree", [1, 3])
def test_gradcheck_of_the_restatement(degree):
    gen = torch.Generator().manual_seed(degree)
    n, P = 6, 3
    grid = SplineGrid(degree, 0.3, -0.3, n)
    t = torch.tensor([-1.0, 0.1, 0.17, 0.6, 0.77, 1.1, 5.0])
    xyz = torch.randn(n, P, 3, generator=gen, dtype=D).requires_grad_()
    rot = random_quats(gen, (n, P), D, max_angle=1.2, identity_every=4).requires_grad_()
    scale = torch.randn(n, P, 3, generator=gen, dtype=D).requires_grad_()
    fn = lambda a, b, c: ref.spline_reference(t, a, b, grid, c)
    assert torch.autograd.gradcheck(fn, (xyz, rot, scale), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 3])
def test_equal_knots_give_that_knot(degree):
    gen = torch.Generator().manual_seed(10)
    n, P = 7, 4
    grid = SplineGrid(degree, 0.3, -0.3, n)
    t = torch.tensor([-1.0, 0.05, 0.31, 0.6, 0.9, 4.0])
    k_xyz = torch.randn(1, P, 3, generator=gen, dtype=D).expand(n, P, 3)
    k_scale = torch.randn(1, P, 3, generator=gen, dtype=D).expand(n, P, 3)
    q = random_quats(gen, (1, P), D, max_angle=2.0, identity_every=0)
    q = q / q.norm(dim=-1, keepdim=True) * torch.where(q[..., 3:] < 0, -1.0, 1.0)  # unit, w > 0: Exp(Log(q)) = q
    xyz, rot, scale = ref.spline_reference(t, k_xyz, q.expand(n, P, 4), grid, k_scale)
    assert float((xyz - k_xyz[:1]).abs().max()) < 1e-14 and float((scale - k_scale[:1]).abs().max()) < 1e-14
    assert float((rot - q).abs().max()) < 1e-14  # up to the rounding of Exp o Log


@pytest.mark.parametrize("degree", [1, 3])
def test_identity_knots_give_identity_and_zero_with_finite_gradients(degree):
    """The training start: every knot rotation the identity, no translation."""
    n, P = 7, 3
    grid = SplineGrid(degree, 0.3, -0.3, n)
    t = torch.tensor([0.0, 0.31, 0.6, 1.2])
    k_xyz = torch.zeros(n, P, 3, dtype=D, requires_grad=True)
    k_rot = torch.tensor(IDENTITY, dtype=D).expand(n, P, 4).clone().requires_grad_()
    xyz, rot, _ = ref.spline_reference(t, k_xyz, k_rot, grid)
    assert not xyz.any() and torch.equal(rot, torch.tensor(IDENTITY, dtype=D).expand(4, P, 4))
    gen = torch.Generator().manual_seed(11)
    loss = (xyz * torch.randn(xyz.shape, generator=gen, dtype=D)).sum() + \
        (rot * torch.randn(rot.shape, generator=gen, dtype=D)).sum()
    gx, gr = torch.autograd.grad(loss, [k_xyz, k_rot])
    assert torch.isfinite(gx).all() and torch.isfinite(gr).all() and gx.any() and gr.any()


def test_linear_spline_at_a_knot_time_reproduces_the_knot():
    gen = torch.Generator().manual_seed(12)
    n, P = 6, 4
    grid = SplineGrid(1, 0.25, 0.0, n)  # exact in float32: t = 0.25 i has u = 0
    t = torch.tensor([0.25, 0.5, 1.0])
    assert ref.segments(grid, t)[0].tolist() == [1, 2, 4] and not ref.segments(grid, t)[1].any()
    k_xyz = torch.randn(n, P, 3, generator=gen, dtype=D)
    q = random_quats(gen, (n, P), D, max_angle=2.0)
    xyz, rot, _ = ref.spline_reference(t, k_xyz, q, grid)
    assert torch.equal(xyz, k_xyz[[1, 2, 4]])
    unit = q / q.norm(dim=-1, keepdim=True) * torch.where(q[..., 3:] < 0, -1.0, 1.0)
    assert float((rot - unit[[1, 2, 4]]).abs().max()) < 1e-14


def test_cubic_rotation_keeps_the_norm_of_its_first_knot():
    gen = torch.Generator().manual_seed(13)
    n, P = 7, 5
    grid = SplineGrid(3, 0.3, -0.3, n)
    t = torch.tensor([0.1, 0.7])
    q = random_quats(gen, (n, P), D, max_angle=1.2)
    _, rot, _ = ref.spline_reference(t, torch.zeros(n, P, 3, dtype=D), q, grid)
    first = ref.segments(grid, t)[0]
    assert float((rot.norm(dim=-1) - q[first].norm(dim=-1)).abs().max()) < 1e-14


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_spline_attributes_argument_errors():
    grid = SplineGrid(3, 0.3, -0.3, 7)
    ok = dict(timestamps=torch.zeros(2), knots_xyz=torch.zeros(7, 5, 3), knots_rot=torch.zeros(7, 5, 4),
              knots_scale=None)
    bad = [
        dict(ok, timestamps=torch.zeros(2, 1)), dict(ok, timestamps=torch.zeros(2, dtype=D)),
        dict(ok, timestamps=[0.0, 0.1]), dict(ok, knots_xyz=torch.zeros(6, 5, 3)), dict(ok, knots_xyz=torch.zeros(7, 5, 4)),
        dict(ok, knots_xyz=torch.zeros(5, 7, 3)), dict(ok, knots_xyz=torch.zeros(7, 5, 3, dtype=torch.float16)),
        dict(ok, knots_rot=torch.zeros(7, 5, 3)), dict(ok, knots_rot=torch.zeros(7, 4, 4)),
        dict(ok, knots_rot=torch.zeros(7, 5, 4, dtype=D)), dict(ok, knots_scale=torch.zeros(7, 5, 4)),
        dict(ok, knots_scale=torch.zeros(6, 5, 3)), dict(ok, knots_scale=torch.zeros(7, 5, 3, dtype=D)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            spline_attributes(kw["timestamps"], kw["knots_xyz"], kw["knots_rot"], grid, kw["knots_scale"])
    with pytest.raises(ValueError, match="n_knots = 7"):
        spline_attributes(ok["timestamps"], torch.zeros(8, 5, 3), torch.zeros(8, 5, 4), grid)
    with pytest.raises(ValueError, match="SplineGrid"):
        spline_attributes(ok["timestamps"], ok["knots_xyz"], ok["knots_rot"], (3, 0.3, -0.3, 7))
    for scale in (None, torch.zeros(7, 5, 3)):
        with pytest.raises(ValueError, match="no CPU path"):  # well-formed CPU tensors
            spline_attributes(ok["timestamps"], ok["knots_xyz"], ok["knots_rot"], grid, scale)


def test_c_entries_check_their_arguments_without_gpu():
    lib = _C.load_library()
    assert lib.gsr_sugar_spline_workspace_bytes(0, 0, 3) > 0 and lib.gsr_sugar_spline_workspace_bytes(0, 0, 1) > 0
    for T, P in ((1, 1), (5, 257), (8, 1000), (8, 163_842)):
        for degree in (1, 3):
            want = 80 * (degree + 1) * T * P
            assert want <= lib.gsr_sugar_spline_workspace_bytes(T, P, degree) <= want + 256
    v = ctypes.c_void_p(16)  # never dereferenced: the calls fail validation first
    odd = ctypes.c_void_p(24)
    big = 1 << 40

    def spline(T, P, n, degree, start, interval, lo, hi, ts, kx, kr, ks):
        return _C.SugarSpline(T=T, P=P, n_knots=n, degree=degree, start=start, interval=interval, lo=lo, hi=hi,
                              timestamps=ts, knots_xyz=kx, knots_rot=kr, knots_scale=ks)

    def fwd(T=2, P=5, n=7, degree=3, start=-0.3, interval=0.3, lo=0.0, hi=1.2, ts=v, kx=v, kr=v, ks=None, xyz=v,
            rot=v, sc=None):
        return lib.gsr_sugar_spline_forward(spline(T, P, n, degree, start, interval, lo, hi, ts, kx, kr, ks), xyz, rot,
                                            sc, None)

    def bwd(T=2, P=5, n=7, degree=3, start=-0.3, interval=0.3, lo=0.0, hi=1.2, ts=v, kx=v, kr=v, ks=None,
            g=(v, v, None), dx=v, dr=v, ds=None, ws=v, nbytes=big):
        return lib.gsr_sugar_spline_backward(spline(T, P, n, degree, start, interval, lo, hi, ts, kx, kr, ks), *g, dx,
                                             dr, ds, ws, nbytes, None)

    assert lib.gsr_sugar_spline_forward(None, v, v, None, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_spline_backward(None, v, v, None, v, v, None, v, big, None) == 1
    assert b"null" in lib.gsr_last_error()
    for call in (fwd, bwd):
        for degree in (0, 2, 4, -1):
            assert call(degree=degree) == 1 and b"degree must" in lib.gsr_last_error()
        assert call(n=3) == 1 and b"n_knots" in lib.gsr_last_error()
        assert call(degree=1, n=1) == 1 and b"n_knots" in lib.gsr_last_error()
        assert call(T=-1) == 1 and call(P=-1) == 1 and b"negative" in lib.gsr_last_error()
        for interval in (0.0, -0.3, float("nan")):
            assert call(interval=interval) == 1 and b"interval" in lib.gsr_last_error()
        assert call(T=1 << 16, P=1 << 15) == 1 and b"2^31" in lib.gsr_last_error()
        assert call(n=1 << 16, P=1 << 15) == 1 and b"2^31" in lib.gsr_last_error()
        for name in ("ts", "kx", "kr"):
            assert call(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
        assert call(kr=odd) == 1 and b"aligned" in lib.gsr_last_error()
        assert call(T=0) == 0 and call(P=0) == 0  # nothing to launch
        assert call(T=0, ts=None, kx=None, kr=None) == 0
    for name in ("xyz", "rot"):
        assert fwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert fwd(ks=v, sc=None) == 1 and b"null" in lib.gsr_last_error()  # knots_scale without a scale output
    assert fwd(rot=odd) == 1 and b"aligned" in lib.gsr_last_error()
    for name in ("dx", "dr", "ws"):
        assert bwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert bwd(ks=v, ds=None) == 1 and b"null" in lib.gsr_last_error()
    assert bwd(g=(v, odd, None)) == 1 and b"aligned" in lib.gsr_last_error()
    assert bwd(dr=odd) == 1 and b"aligned" in lib.gsr_last_error()
    assert bwd(ws=ctypes.c_void_p(20)) == 1 and b"aligned" in lib.gsr_last_error()
    for degree in (1, 3):
        assert bwd(degree=degree, nbytes=lib.gsr_sugar_spline_workspace_bytes(2, 5, degree) - 1) == 1
        assert b"workspace" in lib.gsr_last_error()
