"""sugar_field (include/gsr.h gsr_sugar_field_*) without a GPU: the library's new entry points and their argument
checks, which precede any device work, and the Python wrappers' validation.  The numerics are checked on the GPU in
tests/test_gpu_sugar_field.py."""
import ctypes

import pytest

from diff_gaussian_rasterization import _C
from kernel_budget import assert_kernel_budget, needs_hipcc


def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in ("gsr_sugar_field_workspace_bytes", "gsr_sugar_field_forward", "gsr_sugar_field_backward"):
        assert hasattr(lib, name) and name in _C.SIGNATURES


def test_workspace_bound():
    """Backward workspace <= 24 M K bytes + O(M + N): nothing of size 9 M K floats; the forward's share is the
    64-byte records only."""
    lib = _C.load_library()
    for M, K, N in ((500_000, 16, 1_000_000), (500_000, 16, 100_000), (8192, 32, 2100), (1, 1, 1), (100, 16, 0)):
        b = lib.gsr_sugar_field_workspace_bytes(M, K, N)
        assert 16 * M * K <= b <= 24 * M * K + 80 * N + 8192, (M, K, N, b)
        f = lib.gsr_sugar_field_workspace_bytes(0, K, N)
        assert 64 * N <= f <= 64 * max(N, 1) + 256
    assert lib.gsr_sugar_field_workspace_bytes(10, 0, 10) == 0 and lib.gsr_sugar_field_workspace_bytes(10, 33, 10) == 0


def test_argument_errors_without_gpu():
    lib = _C.load_library()
    v = ctypes.c_void_p(16)  # never dereferenced: the calls fail validation first
    big = 1 << 40

    def field(M, K, N, R, x, nbr, row, centers):
        return _C.SugarField(M=M, K=K, N=N, R=R, x=x, nbr=nbr, row=row, centers=centers, inv_sr=v, strengths=v,
                             min_scale=v, density_factor=1.0)

    def fwd(M=10, K=4, N=5, R=10, x=v, nbr=v, row=None, centers=v, density=v, ws=v, nbytes=big):
        return lib.gsr_sugar_field_forward(field(M, K, N, R, x, nbr, row, centers), density, v, None, ws, nbytes, None)

    def bwd(M=10, K=4, N=5, R=10, row=None, dx=v, dcenters=v, nbytes=big):
        return lib.gsr_sugar_field_backward(field(M, K, N, R, v, v, row, v), v, None, None, dx, dcenters, v, v, v, v,
                                            nbytes, None)

    assert lib.gsr_sugar_field_forward(None, v, v, None, v, big, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_field_backward(None, v, None, None, v, v, v, v, v, v, big, None) == 1
    assert b"null" in lib.gsr_last_error()
    for call in (fwd, bwd):
        for K in (0, 33):
            assert call(K=K) == 1 and b"K" in lib.gsr_last_error()
        assert call(M=-1) == 1 and call(N=-1) == 1
        assert call(R=9) == 1 and b"rows" in lib.gsr_last_error()  # no row: the table has M rows
        assert call(M=1 << 27, K=16, R=1 << 27) == 1 and b"2^31" in lib.gsr_last_error()
        assert call(nbytes=16) == 1 and b"workspace" in lib.gsr_last_error()
        assert call(M=0, R=0) == 0  # nothing to launch
    assert fwd(x=None) == 1 and fwd(nbr=None) == 1 and fwd(centers=None) == 1 and fwd(density=None) == 1
    assert fwd(ws=None) == 1
    assert bwd(dx=None) == 1 and bwd(dcenters=None) == 1
    assert fwd(nbytes=lib.gsr_sugar_field_workspace_bytes(0, 4, 5) - 1) == 1
    assert bwd(nbytes=lib.gsr_sugar_field_workspace_bytes(10, 4, 5) - 1) == 1


def _args(torch, M=6, K=4, N=5):
    return dict(x=torch.zeros(M, 3), centers=torch.zeros(N, 3), inv_scaled_rotation=torch.zeros(N, 3, 3),
                strengths=torch.zeros(N), min_scaling=torch.zeros(N)), torch.zeros(M, K, dtype=torch.int64)


def test_python_argument_errors():
    torch = pytest.importorskip("torch")
    from sugar_field import FIELD_MAX_K, neighbor_density

    assert FIELD_MAX_K == 32
    a, idx = _args(torch)
    knn, gi = torch.zeros(5, 4, dtype=torch.int64), torch.zeros(6, dtype=torch.int64)
    bad = [
        dict(a, x=torch.zeros(6, 2)), dict(a, x=torch.zeros(6, 3, dtype=torch.float64)), dict(a, x=[[0., 0., 0.]]),
        dict(a, centers=torch.zeros(5, 4)), dict(a, inv_scaled_rotation=torch.zeros(5, 9)),
        dict(a, inv_scaled_rotation=torch.zeros(4, 3, 3)), dict(a, strengths=torch.zeros(4)),
        dict(a, strengths=torch.zeros(5, 2)), dict(a, strengths=torch.zeros(5, dtype=torch.float16)),
        dict(a, min_scaling=torch.zeros(5, 1)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            neighbor_density(**kw, closest_gaussians_idx=idx)
    index_forms = [
        dict(), dict(knn_idx=knn), dict(gaussian_idx=gi), dict(knn_idx=knn, gaussian_idx=gi, closest_gaussians_idx=idx),
        dict(knn_idx=knn, closest_gaussians_idx=idx), dict(closest_gaussians_idx=idx.int()),
        dict(closest_gaussians_idx=idx[:5]), dict(closest_gaussians_idx=idx[:, :0]),
        dict(closest_gaussians_idx=torch.zeros(6, 33, dtype=torch.int64)), dict(closest_gaussians_idx=idx[0]),
        dict(knn_idx=knn, gaussian_idx=gi[:5]), dict(knn_idx=knn.float(), gaussian_idx=gi),
        dict(knn_idx=knn, gaussian_idx=gi[:, None]),
    ]
    for kw in index_forms:
        with pytest.raises(ValueError):
            neighbor_density(**a, **kw)
    with pytest.raises(ValueError):
        neighbor_density(**a, closest_gaussians_idx=idx, density_factor="x")
    # well-formed CPU tensors: no CPU path, as knn_points
    for kw in (dict(closest_gaussians_idx=idx), dict(knn_idx=knn, gaussian_idx=gi),
               dict(closest_gaussians_idx=idx, return_opacities=True)):
        with pytest.raises(_C.GSRError):
            neighbor_density(**a, **kw)
    with pytest.raises(_C.GSRError):
        neighbor_density(**dict(a, strengths=torch.zeros(5, 1)), closest_gaussians_idx=idx)
    with pytest.raises(TypeError):
        neighbor_density(*a.values(), idx)  # the index forms are keyword-only


def test_get_field_values_argument_errors():
    torch = pytest.importorskip("torch")
    from sugar_field import get_field_values

    a, idx = _args(torch)
    kw = dict(points=a["centers"], inv_scaled_rotation=a["inv_scaled_rotation"], strengths=a["strengths"][:, None],
              scaling=torch.ones(5, 3), closest_gaussians_idx=idx)
    with pytest.raises(NotImplementedError, match="sdf_grad"):
        get_field_values(a["x"], **kw, return_sdf_grad=True)
    with pytest.raises(ValueError, match="beta_mode"):
        get_field_values(a["x"], **kw, beta_mode="median")
    with pytest.raises(ValueError, match="log_beta"):
        get_field_values(a["x"], **kw, beta_mode="learnable")
    with pytest.raises(ValueError):
        get_field_values(a["x"], **dict(kw, scaling=torch.ones(5)))
    with pytest.raises(ValueError):
        get_field_values(a["x"], **dict(kw, closest_gaussians_idx=None))
    with pytest.raises(_C.GSRError):
        get_field_values(a["x"], **kw)  # CPU tensors
    with pytest.raises(TypeError):
        get_field_values(a["x"], a["centers"])  # everything but x is keyword-only


@needs_hipcc
def test_field_kernels_do_not_spill(tmp_path):
    kernels = ("k_field_packE", "k_field_sampleILb0E", "k_field_sampleILb1E", "k_field_gaussILi64E",
               "k_field_gaussILi16E")
    assert_kernel_budget("gsr_field.hip", tmp_path, "k_field", dict.fromkeys(kernels, 0), sgpr_too=True)
