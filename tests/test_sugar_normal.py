"""sugar_field.neighbor_normal_loss and the regulariser step around it (include/gsr.h gsr_sugar_normal_*) without a
GPU: the library's entry points and their argument checks, which precede any device work, the Python wrappers'
validation, and the N- and M-sized torch parts (smallest_axis, sample_points_in_gaussians) against restatements
written here.  The kernels' numerics are checked on the GPU in tests/test_gpu_sugar_normal.py."""
import ctypes

import pytest

from diff_gaussian_rasterization import _C
from kernel_budget import assert_kernel_budget, needs_hipcc

NAMES = ("gsr_sugar_normal_workspace_bytes", "gsr_sugar_normal_forward", "gsr_sugar_normal_backward")


def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES


def test_workspace_bound():
    """Backward workspace <= 24 M (K + 1) + 80 N + 8192 bytes, and at least the double-buffered sort of M (K + 1)
    terms; the forward's share is O(N): the 32-byte records only."""
    lib = _C.load_library()
    for M, K, N in ((500_000, 16, 1_000_000), (8192, 32, 2100), (1, 1, 1), (100, 16, 0)):
        b = lib.gsr_sugar_normal_workspace_bytes(M, K, N)
        assert 16 * M * (K + 1) <= b <= 24 * M * (K + 1) + 80 * N + 8192, (M, K, N, b)
        assert b < 3 * 4 * M * K + 16 * M * (K + 1) + 80 * N + 8192  # no room for an (M, K, 3) float array beside it
        f = lib.gsr_sugar_normal_workspace_bytes(0, K, N)
        assert 32 * N <= f <= 32 * max(N, 1) + 256
    assert lib.gsr_sugar_normal_workspace_bytes(10, 0, 10) == 0
    assert lib.gsr_sugar_normal_workspace_bytes(10, 33, 10) == 0


def test_argument_errors_without_gpu():
    lib = _C.load_library()
    v = ctypes.c_void_p(16)  # never dereferenced: the calls fail validation first
    big = 1 << 40

    def fwd(M=10, K=4, N=5, R=5, x=v, own=v, nbr=v, per_sample=0, centers=v, normals=v, op=v, loss=v, ws=v,
            nbytes=big, rec=None):
        s = _C.SugarNormal(M=M, K=K, N=N, R=R, x=x, own=own, nbr=nbr, per_sample=per_sample, centers=centers,
                           normals=normals, min_scale=v, op=op)
        return lib.gsr_sugar_normal_forward(s, loss, rec, ws, nbytes, None)

    def bwd(M=10, K=4, N=5, R=5, x=v, own=v, nbr=v, per_sample=0, centers=v, normals=v, op=v, rec=v, g=v, dn=v, ws=v,
            nbytes=big):
        s = _C.SugarNormal(M=M, K=K, N=N, R=R, x=x, own=own, nbr=nbr, per_sample=per_sample, centers=centers,
                           normals=normals, min_scale=v, op=op)
        return lib.gsr_sugar_normal_backward(s, rec, g, dn, ws, nbytes, None)

    assert lib.gsr_sugar_normal_forward(None, v, None, v, big, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_normal_backward(None, v, v, v, v, big, None) == 1 and b"null" in lib.gsr_last_error()
    for call in (fwd, bwd):
        for K in (0, 33):
            assert call(K=K) == 1 and b"K" in lib.gsr_last_error()
        assert call(M=-1) == 1 and call(N=-1) == 1 and call(R=-1) == 1
        assert call(per_sample=1, R=9) == 1 and b"rows" in lib.gsr_last_error()  # a per-sample table has M rows
        # M (K + 1) < 2^31: 2^27 x 15 is at the limit (2^27 x 16 terms)
        assert call(M=1 << 27, K=15) == 1 and b"2^31" in lib.gsr_last_error()
        assert call(M=1 << 27, K=15, nbytes=16) == 1 and b"2^31" in lib.gsr_last_error()  # before the workspace
        assert call(nbytes=16) == 1 and b"workspace" in lib.gsr_last_error()
        assert call(M=0) == 0 and call(M=0, per_sample=1, R=0) == 0  # nothing to launch
        for name in ("x", "own", "nbr", "centers", "normals", "op", "ws"):
            assert call(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert fwd(loss=None) == 1
    odd = ctypes.c_void_p(24)  # rec is read and written as float4
    assert bwd(rec=odd) == 1 and b"aligned" in lib.gsr_last_error()
    assert fwd(rec=odd) == 1 and b"aligned" in lib.gsr_last_error()
    assert bwd(rec=None) == 1 and bwd(g=None) == 1 and bwd(dn=None) == 1
    assert fwd(nbytes=lib.gsr_sugar_normal_workspace_bytes(0, 4, 5) - 1) == 1
    assert bwd(nbytes=lib.gsr_sugar_normal_workspace_bytes(10, 4, 5) - 1) == 1


def _args(torch, M=6, K=4, N=5):
    return dict(x=torch.zeros(M, 3), centers=torch.zeros(N, 3), normals=torch.zeros(N, 3),
                min_scaling=torch.zeros(N), opacities=torch.zeros(M, K)), torch.zeros(M, K, dtype=torch.int64)


def test_python_argument_errors():
    torch = pytest.importorskip("torch")
    from sugar_field import neighbor_normal_loss

    a, idx = _args(torch)
    knn, gi = torch.zeros(5, 4, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)
    bad = [
        dict(a, x=torch.zeros(6, 2)), dict(a, x=torch.zeros(6, 3, dtype=torch.float64)), dict(a, x=[[0., 0., 0.]]),
        dict(a, centers=torch.zeros(5, 4)), dict(a, normals=torch.zeros(4, 3)), dict(a, normals=torch.zeros(5, 4)),
        dict(a, normals=torch.zeros(5, 3, dtype=torch.float16)), dict(a, min_scaling=torch.zeros(5, 1)),
        dict(a, opacities=torch.zeros(6, 5)), dict(a, opacities=torch.zeros(5, 4)),
        dict(a, opacities=torch.zeros(6, 4, dtype=torch.float64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            neighbor_normal_loss(**kw, gaussian_idx=gi, closest_gaussians_idx=idx)
    index_forms = [
        dict(gaussian_idx=gi), dict(gaussian_idx=gi, knn_idx=knn, closest_gaussians_idx=idx),
        dict(gaussian_idx=gi.int(), knn_idx=knn), dict(gaussian_idx=gi[:5], knn_idx=knn),
        dict(gaussian_idx=gi[:, None], closest_gaussians_idx=idx), dict(gaussian_idx=gi, knn_idx=knn.float()),
        dict(gaussian_idx=gi, closest_gaussians_idx=idx[:5]), dict(gaussian_idx=gi, closest_gaussians_idx=idx[0]),
        dict(gaussian_idx=gi, closest_gaussians_idx=idx.int()),
    ]
    for kw in index_forms:
        with pytest.raises(ValueError):
            neighbor_normal_loss(**a, **kw)
    for K in (0, 33):  # the K range
        wide = dict(a, opacities=torch.zeros(6, K))
        with pytest.raises(ValueError):
            neighbor_normal_loss(**wide, gaussian_idx=gi, closest_gaussians_idx=torch.zeros(6, K, dtype=torch.int64))
    with pytest.raises(TypeError):
        neighbor_normal_loss(**a, closest_gaussians_idx=idx)  # gaussian_idx is required
    with pytest.raises(TypeError):
        neighbor_normal_loss(*a.values(), gi, idx)  # the index forms are keyword-only
    with pytest.raises(NotImplementedError, match="gradient_through_normal_only"):
        neighbor_normal_loss(**a, gaussian_idx=gi, knn_idx=knn, gradient_through_normal_only=False)
    # well-formed CPU tensors: no CPU path, as neighbor_density
    for kw in (dict(closest_gaussians_idx=idx), dict(knn_idx=knn)):
        with pytest.raises(_C.GSRError):
            neighbor_normal_loss(**a, gaussian_idx=gi, **kw)


def _rotation_columns(torch, q):
    """The three columns of the rotation matrix of a unit quaternion (w, x, y, z), as the images of the basis vectors
    under v -> v + 2 w (u x v) + 2 u x (u x v), u = (x, y, z)."""
    w, u = q[:, :1], q[:, 1:]
    cols = []
    for a in range(3):
        e = torch.zeros_like(u)
        e[:, a] = 1
        cols.append(e + 2 * w * torch.cross(u, e, dim=-1) + 2 * torch.cross(u, torch.cross(u, e, dim=-1), dim=-1))
    return cols


def test_smallest_axis():
    torch = pytest.importorskip("torch")
    from sugar_field import smallest_axis

    g = torch.Generator().manual_seed(5)
    q = torch.randn(200, 4, generator=g) * 3  # not unit: normalised inside
    sc = torch.rand(200, 3, generator=g) + 0.01
    sc[:3] = torch.tensor([[3., 2., 1.], [1., 3., 2.], [2., 1., 3.]])
    got = smallest_axis(q, sc)
    cols = _rotation_columns(torch, (q / q.norm(dim=-1, keepdim=True)).double())
    am = sc.argmin(-1)
    assert am[:3].tolist() == [2, 0, 1]
    want = torch.stack([cols[int(am[n])][n] for n in range(200)])
    assert got.dtype == torch.float32 and got.shape == (200, 3)
    assert (got.double() - want).abs().max() < 1e-6
    assert ((got.norm(dim=-1) - 1).abs() < 1e-6).all()
    # the identity and a quarter turn about z, exactly
    q2 = torch.tensor([[2., 0., 0., 0.], [1., 0., 0., 1.]])
    s2 = torch.tensor([[1., 0.5, 2.], [0.1, 1., 2.]])
    assert torch.allclose(smallest_axis(q2, s2), torch.tensor([[0., 1., 0.], [0., 1., 0.]]), atol=1e-7)
    leaf = q.clone().requires_grad_()
    smallest_axis(leaf, sc).sum().backward()
    assert torch.isfinite(leaf.grad).all() and leaf.grad.any()
    with pytest.raises(ValueError):
        smallest_axis(q[:, :3], sc)
    with pytest.raises(ValueError):
        smallest_axis(q, sc[:10])


def _sample_restated(torch, points, quats, scaling, strengths, num, factor, mask, by_opacity, by_volume, seed):
    """utils/sugar_utils.py:183-230 line by line, with the rotation of the noise written as the Hamilton products
    q (0, v) q* in components."""
    g = torch.Generator().manual_seed(seed)
    sc = scaling if mask is None else scaling[mask]
    areas = sc[:, 0] * sc[:, 1] * sc[:, 2] if by_volume else torch.ones_like(sc[:, 0])
    if by_opacity:
        areas = areas * (strengths if mask is None else strengths[mask]).view(-1)
    areas = areas.abs()
    cum_probs = areas.cumsum(dim=-1) / areas.sum(dim=-1, keepdim=True)
    idx = torch.multinomial(cum_probs, num_samples=num, replacement=True, generator=g)  # the cumulative ones
    if mask is not None:
        idx = torch.arange(len(points))[mask][idx]
    noise = torch.randn(num, 3, generator=g)
    v = factor * scaling[idx] * noise
    q = torch.nn.functional.normalize(quats, dim=-1)[idx]
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    vw, vx, vy, vz = torch.zeros_like(qw), v[:, 0], v[:, 1], v[:, 2]
    tw = qw * vw - qx * vx - qy * vy - qz * vz  # t = q (0, v)
    tx = qw * vx + qx * vw + qy * vz - qz * vy
    ty = qw * vy - qx * vz + qy * vw + qz * vx
    tz = qw * vz + qx * vy - qy * vx + qz * vw
    cw, cx, cy, cz = qw * 1., qx * -1., qy * -1., qz * -1.  # q*
    rx = tw * cx + tx * cw + ty * cz - tz * cy  # the vector part of t q*
    ry = tw * cy - tx * cz + ty * cw + tz * cx
    rz = tw * cz + tx * cy - ty * cx + tz * cw
    return points[idx] + torch.stack([rx, ry, rz], -1), idx


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("by_opacity,by_volume", [(False, True), (False, False), (True, True), (True, False)])
def test_sample_points_in_gaussians(masked, by_opacity, by_volume):
    torch = pytest.importorskip("torch")
    from sugar_field import sample_points_in_gaussians

    g = torch.Generator().manual_seed(9)
    n, num = 300, 4000
    points = torch.randn(n, 3, generator=g)
    quats = torch.randn(n, 4, generator=g)
    scaling = torch.exp(torch.randn(n, 3, generator=g) * 0.5) * 0.1
    strengths = torch.sigmoid(torch.randn(n, 1, generator=g))
    mask = (torch.rand(n, generator=g) < 0.6) if masked else None
    want_x, want_i = _sample_restated(torch, points, quats, scaling, strengths, num, 1.5, mask, by_opacity, by_volume, 4)
    got_x, got_i = sample_points_in_gaussians(
        points, quats, scaling, num, 1.5, strengths=strengths, mask=mask,
        probabilities_proportional_to_opacity=by_opacity, probabilities_proportional_to_volume=by_volume,
        generator=torch.Generator().manual_seed(4))
    assert got_i.dtype == torch.int64 and torch.equal(got_i, want_i)
    assert torch.equal(got_x, want_x)
    if masked:
        assert mask[got_i].all()
    if not by_opacity and not by_volume and not masked:
        # the cumulative probabilities as weights: index n is drawn in proportion to n + 1, not uniformly
        assert got_i.double().mean() > 0.6 * n
    # the noise is a rotation of the scaled normal draw: its length is the scaled draw's
    noise = torch.randn(num, 3, generator=_after_multinomial(torch, points, scaling, strengths, num, mask,
                                                              by_opacity, by_volume))
    want_len = (1.5 * scaling[got_i] * noise).norm(dim=-1)
    assert torch.allclose((got_x - points[got_i]).norm(dim=-1), want_len, rtol=1e-4, atol=1e-6)


def _after_multinomial(torch, points, scaling, strengths, num, mask, by_opacity, by_volume):
    """A generator in the state the index draw leaves it in."""
    g = torch.Generator().manual_seed(4)
    sc = scaling if mask is None else scaling[mask]
    areas = sc.prod(-1) if by_volume else torch.ones_like(sc[:, 0])
    if by_opacity:
        areas = areas * (strengths if mask is None else strengths[mask]).view(-1)
    torch.multinomial(areas.abs().cumsum(-1) / areas.abs().sum(), num, replacement=True, generator=g)
    return g


def test_sample_points_argument_errors_and_gradients():
    torch = pytest.importorskip("torch")
    from sugar_field import sample_points_in_gaussians

    points, quats, scaling = torch.randn(10, 3), torch.randn(10, 4), torch.rand(10, 3) + 0.1
    with pytest.raises(ValueError):
        sample_points_in_gaussians(points, quats[:, :3], scaling, 5)
    with pytest.raises(ValueError):
        sample_points_in_gaussians(points, quats, scaling[:5], 5)
    with pytest.raises(ValueError, match="strengths"):
        sample_points_in_gaussians(points, quats, scaling, 5, probabilities_proportional_to_opacity=True)
    leaves = [t.clone().requires_grad_() for t in (points, quats, scaling)]
    x, idx = sample_points_in_gaussians(*leaves, 64, 1.5, generator=torch.Generator().manual_seed(0))
    x.square().sum().backward()
    for t in leaves:
        assert torch.isfinite(t.grad).all() and t.grad.any()


def test_coarse_density_regulation_needs_a_gpu():
    torch = pytest.importorskip("torch")
    from sugar_field import coarse_density_regulation

    n = 20
    args = (torch.randn(n, 3), torch.randn(n, 4), torch.rand(n, 3) + 0.1, torch.rand(n, 1),
            torch.zeros(n, 4, dtype=torch.int64))
    with pytest.raises(_C.GSRError):
        coarse_density_regulation(*args, n_samples=16, use_sdf_better_normal_loss=True)
    empty = coarse_density_regulation(torch.zeros(0, 3), torch.zeros(0, 4), torch.zeros(0, 3), torch.zeros(0, 1),
                                      torch.zeros(0, 4, dtype=torch.int64), n_samples=16,
                                      use_sdf_better_normal_loss=True)
    assert empty == {"density_regulation": 0, "normal_regulation": 0}
    with pytest.raises(TypeError):
        coarse_density_regulation(*args, 16, True)  # the options are keyword-only


@needs_hipcc
def test_normal_kernels_do_not_spill(tmp_path):
    kernels = ("k_normal_packE", "k_normal_sampleILb0E", "k_normal_sampleILb1E", "k_normal_gaussILi64E",
               "k_normal_gaussILi16E")
    assert_kernel_budget("gsr_normal.hip", tmp_path, "k_normal", dict.fromkeys(kernels, 0), sgpr_too=True)
