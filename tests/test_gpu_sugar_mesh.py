"""sugar_mesh.bound_gaussians (include/gsr.h gsr_sugar_mesh_*, csrc/gsr_mesh.hip) on the GPU against the fp64 torch
restatement of the same formulas (tests/sugar_mesh_reference.py), differentiated by autograd on the CPU.

Bar (``check_against_null`` of tests/sugar_cases.py).  Per tensor (the four outputs, the three gradients):
max |gpu - ref64| / max |ref64| <= 2 x the same figure of the restatement in float32 on the CPU (the "fp32 null",
computed here on the same inputs): the kernel may not be less exact than twice what it replaces.  The factor 2 is there
because the null is itself a few ulps of one rounding sample.  An all-zero reference tensor wants exact zeros.  Before
comparing, each quaternion row's sign is aligned with the sign of its dot product with the reference row (the kernel
and the reference may take different candidate rows of matrix_to_quaternion where two tie), and that row's upstream
gradient is multiplied by the same sign, on the null's side too.  The thickness column of `scaling` and the gradients
of outputs without an upstream gradient are exact.  Each check prints its figures.
Measured on the CPU (icosphere(3), G = 6), the null: 1e-7 to 1.7e-7 for all outputs and gradients.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_mesh_reference as ref  # noqa: E402
from sugar_cases import NullCase, _fan, backprop, check_against_null  # noqa: E402

THICKNESS = 3.5e-6


class _Case(NullCase):
    """A mesh with random per-Gaussian parameters and upstream gradients; the reference and the null computed once."""

    def __init__(self, verts, faces, G, seed=0, bary=None):
        from sugar_mesh import MeshBinding

        self.verts = torch.as_tensor(np.asarray(verts), dtype=torch.float32)
        self.faces = torch.as_tensor(np.asarray(faces), dtype=torch.int64)
        if bary is None:
            self.binding = MeshBinding.from_reference_count(self.faces, len(self.verts), G)
        else:
            self.binding = MeshBinding(self.faces, len(self.verts), bary)
        gen = torch.Generator().manual_seed(seed)
        N = self.binding.n_gaussians
        self.cplx = torch.randn(N, 2, generator=gen)
        self.log_scales = torch.randn(N, 2, generator=gen) * 0.3 - 4
        self.ups = {k: torch.randn(N, 4 if k == "rotation" else 3, generator=gen) for k in ref.OUTPUTS}
        self.keys = ref.OUTPUTS + ref.GRADS

    def evaluate(self, dtype, ups, sign=None):
        return ref.evaluate(dtype, self.verts, self.faces, self.binding.bary, self.cplx, self.log_scales, THICKNESS,
                            ups, sign=sign)

    def aligned(self, r0, got, ups):
        """(row signs s of got's quaternions against r0's, the fp64 reference for them, its rows times s).  `got` had
        the plain upstream gradient: a flipped row's reference gradient is that of -q, i.e. the reference with that
        row's upstream gradient negated.  |got - s r| = |s got - r|, and the bar sees `got` as the kernel wrote it."""
        s = ref.row_sign(got["rotation"], r0["rotation"])
        r = r0 if bool((s > 0).all()) else self.evaluate(torch.float64, ups, sign=s)
        return s, dict(r, rotation=r["rotation"] * s[:, None])

    def references(self, ups):
        """(fp64 reference without alignment, fp32 null, the reference aligned to the null)."""
        r0, null = super().references(ups)
        return r0, null, self.aligned(r0, null, ups)[1]

    def gpu(self, which=ref.OUTPUTS, binding=None):
        from sugar_mesh import bound_gaussians

        leaves = [t.cuda().requires_grad_() for t in (self.verts, self.cplx, self.log_scales)]
        out = bound_gaussians(*leaves, (binding or self.binding).to("cuda"), THICKNESS)
        return backprop(out, ref.OUTPUTS, leaves, ref.GRADS, self.ups, which)

    def check(self, got, which=ref.OUTPUTS, tag=""):
        r0, null, rn = self.reference(tuple(which))
        s, r = self.aligned(r0, got, {k: self.ups[k] for k in which})
        N = self.binding.n_gaussians
        assert torch.equal(got["scaling"][:, 0], torch.full((N,), THICKNESS, dtype=torch.float32)), tag
        check_against_null(got, r, null, self.keys, tag, null_ref=rn, note=f"  flipped rows {int((s < 0).sum())}")


def _icosphere_case(subdiv, G):
    v, f = gs.icosphere(subdiv)
    return _Case(v, f, G, seed=10 * subdiv + G)


@functools.lru_cache(maxsize=None)
def _ico3():
    return _icosphere_case(3, 6)


@functools.lru_cache(maxsize=None)
def _ico3_gpu():
    return _ico3().gpu()


@pytest.mark.gpu
def test_one_face_one_gaussian():
    case = _Case([[0.1, 0.2, 0.3], [0.9, 0.1, 0.2], [0.3, 0.8, 0.5]], [[0, 1, 2]], 1, seed=1)
    assert case.binding.n_gaussians == 1
    case.check(case.gpu(), tag="F=1 G=1")


@pytest.mark.gpu
def test_two_triangles_sharing_an_edge():
    case = _Case([[0., 0., 0.], [1., 0., 0.1], [0., 1., 0.2], [1.1, 0.9, -0.3]], [[0, 1, 2], [2, 1, 3]], 3, seed=2)
    case.check(case.gpu(), tag="two triangles G=3")


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 4, 6])
def test_icosphere0(G):
    """12 vertices of valence 5, every barycentric set of the reference."""
    case = _icosphere_case(0, G)
    assert case.binding.n_verts == 12 and case.binding.n_faces == 20
    case.check(case.gpu(), tag=f"icosphere(0) G={G}")


@pytest.mark.gpu
def test_icosphere3_all_outputs():
    """V = 642, F = 1280, N = 7680: 30 blocks of Gaussians, 5 of faces, 3 of vertices, none a whole number of faces;
    the four candidate rows of matrix_to_quaternion are each taken by about a quarter of the Gaussians."""
    case = _ico3()
    assert (case.binding.n_verts, case.binding.n_faces, case.binding.n_gaussians) == (642, 1280, 7680)
    counts = torch.bincount(case.reference(ref.OUTPUTS)[0]["branch"], minlength=4)
    assert int(counts.min()) > 1500, counts.tolist()
    case.check(_ico3_gpu(), tag="icosphere(3) G=6")


@pytest.mark.gpu
def test_custom_barycentric_set_of_eight():
    """G = 8, the largest, with weights that are not the reference's."""
    gen = torch.Generator().manual_seed(8)
    bary = torch.rand(8, 3, generator=gen) + 0.05
    bary = bary / bary.sum(-1, keepdim=True)
    v, f = gs.icosphere(1)
    case = _Case(v, f, 8, seed=18, bary=bary)
    case.check(case.gpu(), tag="icosphere(1) G=8")


@pytest.mark.gpu
def test_fan_of_200_faces_and_an_unused_vertex():
    verts, faces = _fan(200)
    case = _Case(verts, faces, 3, seed=3)
    assert int(case.binding.vert_offsets[1]) == 200 and int(case.binding.vert_offsets[-1]) == 600
    got = case.gpu()
    case.check(got, tag="fan")
    assert torch.equal(got["verts"][-1], torch.zeros(3))  # the vertex no face uses: exactly 0.0
    assert not torch.signbit(got["verts"][-1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("xyz",), ("rotation",)])
def test_partial_upstream_gradients(which):
    """Only one output carries a gradient (the others arrive as None): the restatement with the others zeroed."""
    case = _icosphere_case(1, 6)
    got = case.gpu(which)
    case.check(got, which, tag=f"only {which[0]}")
    assert not got["log_scales"].any()  # scaling has no upstream gradient: exactly zero
    if which == ("xyz",):
        assert not got["complex"].any()
        assert got["verts"].any()


@pytest.mark.gpu
def test_degenerate_face():
    """A face with two equal corners appended to icosphere(0): everything finite, and nothing else changes."""
    v, f = gs.icosphere(0)
    G = 6
    clean = _Case(v, f, G, seed=4)
    full = _Case(v, np.concatenate([f, [[0, 0, 5]]]), G, seed=4)
    n = clean.binding.n_gaussians
    for name in ("cplx", "log_scales"):  # the same parameters for the shared Gaussians
        getattr(full, name)[:n] = getattr(clean, name)
    for k in ref.OUTPUTS:
        full.ups[k][:n] = clean.ups[k]
    a, b = clean.gpu(), full.gpu()
    for k in ref.OUTPUTS + ref.GRADS:
        assert torch.isfinite(b[k]).all(), k
    for k in ref.OUTPUTS + ("complex", "log_scales"):
        assert torch.equal(a[k], b[k][:n]), k
    untouched = [i for i in range(12) if i not in (0, 5)]
    assert torch.equal(a["verts"][untouched], b["verts"][untouched])
    assert not b["normals"][n:].any()  # no normal: the zero vector
    assert torch.equal(b["rotation"][n:], torch.tensor([[1., 0., 0., 0.]]).expand(G, 4))


@pytest.mark.gpu
def test_face_entry_out_of_range_is_not_dereferenced():
    """A binding whose face table was damaged after its check: that face gives zeros, the others are unchanged."""
    case = _icosphere_case(1, 6)
    good = case.gpu()
    bad = case.binding.to("cpu")
    bad.faces = bad.faces.clone()
    bad.faces[3, 1] = case.binding.n_verts + 7
    bad.faces[9, 2] = -1
    got = case.gpu(binding=bad)
    hit = torch.zeros(case.binding.n_gaussians, dtype=torch.bool)
    hit[3 * 6:4 * 6] = True
    hit[9 * 6:10 * 6] = True
    for k in ref.OUTPUTS + ("complex", "log_scales"):
        assert not got[k][hit].any(), k
        assert torch.equal(got[k][~hit], good[k][~hit]), k
    assert torch.isfinite(got["verts"]).all()
    far = torch.ones(case.binding.n_verts, dtype=torch.bool)
    far[case.faces[[3, 9]].reshape(-1)] = False
    assert torch.equal(got["verts"][far], good["verts"][far])


@pytest.mark.gpu
def test_bitwise_repeatable():
    a, b = _ico3_gpu(), _ico3().gpu()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_outputs_feed_the_sugar_normal_render():
    """icosphere(3)'s bound Gaussians through rasterize_views in the SuGaR normal renderer's form (the face normals
    as the second colour set), one 64 x 64 view: it renders, and the gradient reaches the vertices."""
    from diff_gaussian_rasterization.batched import rasterize_views
    from gsr_testutil import _settings, make_camera
    from sugar_mesh import bound_gaussians, initial_log_scales

    case = _ico3()
    dev = "cuda"
    binding = case.binding.to(dev)
    verts = case.verts.to(dev).requires_grad_()
    cplx = case.cplx.to(dev).requires_grad_()
    log_scales = initial_log_scales(verts.detach(), binding).requires_grad_()
    xyz, scaling, rotation, normals = bound_gaussians(verts, cplx, log_scales, binding, THICKNESS)
    P = binding.n_gaussians
    gen = torch.Generator().manual_seed(5)
    colors = torch.rand(P, 3, generator=gen).to(dev)
    opacities = (torch.rand(P, 1, generator=gen) * 0.39 + 0.6).to(dev)
    m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
    c, r, d, a, c2 = rasterize_views([_settings(make_camera(64, 64), [0.0, 0.0, 0.0], 0)], xyz, [m2], opacities,
                                     colors_precomp=colors, scales=scaling, rotations=rotation, colors2=normals)
    assert c.shape == (1, 3, 64, 64) and c2.shape == (1, 3, 64, 64) and float(a.detach().max()) > 0.5
    u = [torch.randn(t.shape, generator=gen).to(dev) for t in (c, d, a, c2)]
    ((c * u[0]).sum() + (d * u[1]).sum() + (a * u[2]).sum() + (c2 * u[3]).sum()).backward()
    for name, t in (("verts", verts), ("complex", cplx), ("log_scales", log_scales)):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.any(), name
