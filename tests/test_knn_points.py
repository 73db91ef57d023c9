"""knn_points (simple_knn.knn_points, include/gsr.h gsr_knn_points): the K nearest points of every point of a
cloud within that cloud, the self-search form of pytorch3d.ops.knn_points that the reference's SuGaR geometry
uses (geometry/sugar.py:646, utils/sugar_utils.py:41,248).

The oracle has no K-NN, so the checker lives here: an fp64 search over the fp32-rounded points (scipy's cKDTree,
or a numpy brute force sorted by (distance, index) where exact ties are the point of the test).

Distance bar, rtol = 1e-6 and atol = 0: the kernel forms fma(dz, dz, fma(dy, dy, dx * dx)) in fp32 — two rounded
subtractions feed each square and three roundings accumulate, under 6 * 2^-24 = 3.6e-7 relative; exact duplicates
give exactly 0 on both sides.  Distances do not depend on tie-breaking, so no cloud is exempt from any check."""
import ctypes
import functools

import numpy as np
import pytest

from diff_gaussian_rasterization import _C
from kernel_budget import assert_kernel_budget, needs_hipcc

RTOL = 1e-6
KS = [1, 4, 16, 32]


def _clouds():
    """The six clouds of tests/test_knn.py (same seed, same order)."""
    rng = np.random.default_rng(0)
    yield "uniform-5k", rng.uniform(-1, 1, (5000, 3))
    c = rng.normal(size=(40, 3)) * 2
    yield "clusters-8k", c[rng.integers(0, 40, 8000)] + rng.normal(size=(8000, 3)) * 0.01
    pts = rng.uniform(-1, 1, (3000, 3))
    pts[1000:1100] = pts[0:100]  # exact duplicates: distance 0 counts
    yield "duplicates-3k", pts
    plane = rng.uniform(-1, 1, (4000, 3))
    plane[:, 2] = 0.25  # flat bbox axis
    yield "plane-4k", plane
    grid = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.1  # equal distances
    yield "grid-1728", grid
    yield "ball-20k", rng.normal(size=(20000, 3)) * np.cbrt(rng.uniform(0, 1, (20000, 1)))


CLOUDS = {name: pts.astype(np.float32) for name, pts in _clouds()}


def _ref_dists(pts32, K, queries=None):
    """fp64 squared distances to the K nearest points (self included), ascending; +inf where P < K."""
    from scipy.spatial import cKDTree

    p = pts32.astype(np.float64)
    q = p if queries is None else p[queries]
    d, _ = cKDTree(p).query(q, k=K)
    return d.reshape(len(q), K) ** 2


@functools.lru_cache(maxsize=None)
def _cloud_ref(name):
    """(P, 32) reference distances of a cloud, computed once: the K nearest are its first K columns."""
    ref = _ref_dists(CLOUDS[name], 32)
    ref.setflags(write=False)
    return ref


def _brute_sorted(pts32, K):
    """Brute force in fp64 over an integer lattice, each row sorted by (distance, index): the defined order, ties
    included.  The distances are integers, so distance * P + index is one exact sort key."""
    p = pts32.astype(np.float64)
    P = len(p)
    d2 = sum((p[:, None, k] - p[None, :, k]) ** 2 for k in range(3))
    assert (d2 == np.rint(d2)).all() and d2.max() < 2 ** 20
    key = d2.astype(np.int64) * P + np.arange(P)[None, :]
    best = np.sort(np.partition(key, K - 1, axis=1)[:, :K], axis=1)
    return (best // P).astype(np.float64), best % P


def _gpu_knn(pts32, K):
    import torch
    from simple_knn import knn_points

    out = knn_points(torch.from_numpy(pts32).cuda(), K=K)
    assert out.knn is None and out.dists.dtype == torch.float32 and out.idx.dtype == torch.int64
    assert not out.dists.requires_grad
    return out.dists.cpu().numpy(), out.idx.cpu().numpy()


def _check_rows(pts32, d, idx, ref, queries=None, tag=""):
    """Checks 1-3 of a (Q, K) result against the reference distances `ref` (Q, K)."""
    P, K = len(pts32), d.shape[1]
    Q = len(d)
    assert d.shape == idx.shape == ref.shape == (Q, K), tag
    n = min(P, K)  # columns that hold a neighbour
    # 1. distances
    np.testing.assert_allclose(d.astype(np.float64), ref, rtol=RTOL, atol=0, err_msg=tag)
    if n < K:
        assert np.isposinf(d[:, n:]).all() and (idx[:, n:] == -1).all(), tag
    # 2. indices: in range, distinct, and the distance recomputed from them
    v = idx[:, :n]
    assert ((v >= 0) & (v < P)).all(), tag
    s = np.sort(v, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), tag + ": repeated index in a row"
    p = pts32.astype(np.float64)
    q = p if queries is None else p[queries]
    again = ((p[v] - q[:, None, :]) ** 2).sum(-1)
    np.testing.assert_allclose(d[:, :n].astype(np.float64), again, rtol=RTOL, atol=0, err_msg=tag)
    # 3. order: distances ascend, equal bits ascend by index
    assert (d[:, 1:] >= d[:, :-1]).all(), tag
    tie = d[:, 1:n] == d[:, : n - 1]
    assert (v[:, 1:][tie] > v[:, :-1][tie]).all(), tag + ": tie not broken by the lower index"


def _mean3(d):
    """distCUDA2's mean over columns 1..3 of a knn_points row, formed the same way in fp32."""
    d = d.astype(np.float32)
    return (d[:, 1] + d[:, 2] + d[:, 3]) / np.float32(3)


# ---------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("P", [0, 1, 1000])
@pytest.mark.parametrize("K", [1, 16, 32])
def test_workspace_covers_the_tree(P, K):
    lib = _C.load_library()
    assert lib.gsr_knn_points_workspace_bytes(P, K) >= lib.gsr_knn_workspace_bytes(P)


def test_argument_errors_without_gpu():
    """Validation precedes any device work (pointers never dereferenced)."""
    lib = _C.load_library()
    v = ctypes.c_void_p(16)
    big = 1 << 30
    for K in (0, 33):
        assert lib.gsr_knn_points(10, K, v, v, v, v, big, None) == 1
        assert b"K" in lib.gsr_last_error()
    assert lib.gsr_knn_points(-1, 4, v, v, v, v, big, None) == 1
    assert lib.gsr_knn_points(10, 4, None, v, v, v, big, None) == 1
    assert lib.gsr_knn_points(10, 4, v, v, None, v, big, None) == 1
    small = lib.gsr_knn_points_workspace_bytes(1000, 4) - 1
    assert lib.gsr_knn_points(1000, 4, v, v, v, v, small, None) == 1
    assert b"workspace" in lib.gsr_last_error()
    assert lib.gsr_knn_points(0, 4, None, None, None, None, 0, None) == 0  # nothing to launch


def test_python_argument_errors():
    torch = pytest.importorskip("torch")
    import simple_knn
    from simple_knn._C import KNN, knn_points

    assert simple_knn.knn_points is knn_points and KNN._fields == ("dists", "idx", "knn")
    with pytest.raises(ValueError):
        knn_points(torch.zeros((10, 2)), K=4)
    for K in (0, 33):
        with pytest.raises(ValueError):
            knn_points(torch.zeros((10, 3)), K=K)
    p = torch.zeros((10, 3))
    with pytest.raises(NotImplementedError, match="itself"):
        knn_points(p, torch.zeros((10, 3)), K=4)
    with pytest.raises(NotImplementedError):
        knn_points(p, p[:5], K=4)
    with pytest.raises(_C.GSRError):
        knn_points(p, p, K=4)  # a CPU tensor: no CPU path
    with pytest.raises(TypeError):
        knn_points(p, K=4, return_nn=True)
    with pytest.raises(TypeError):
        knn_points(p, K=4, lengths1=None)


@needs_hipcc
def test_knn_kernels_do_not_spill(tmp_path):
    """Every list capacity (4, 8, 16, 32) keeps its list in registers (compiler resource remarks only)."""
    kernels = ("k_knn_bboxE", "k_knn_mortonE", "k_knn_gatherE", "k_knn_box_aabbE", "k_knn_aabbE", "k_knn_queryE",
               "k_knn_pointsILi4E", "k_knn_pointsILi8E", "k_knn_pointsILi16E", "k_knn_pointsILi32E")
    assert_kernel_budget("gsr_knn.hip", tmp_path, "k_knn", dict.fromkeys(kernels, 0))


# ---------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(CLOUDS))
def test_clouds(name, K):
    """Checks 1-3 on the six clouds, and (K >= 4) the bitwise tie to distCUDA2."""
    import torch
    from simple_knn._C import distCUDA2

    pts = CLOUDS[name]
    d, idx = _gpu_knn(pts, K)
    _check_rows(pts, d, idx, _cloud_ref(name)[:, :K], tag=f"{name} K={K}")
    if K >= 4:
        # one zero (the point itself) removed from the list leaves the 3 nearest others
        mean = distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()
        np.testing.assert_array_equal(_mean3(d), mean, err_msg=f"{name} K={K}")


def _lattices():
    grid = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    yield "grid-1728-int", grid.astype(np.float32)
    yield "int8-4096", np.random.default_rng(11).integers(0, 8, (4096, 3)).astype(np.float32)  # heavy duplication


@pytest.mark.gpu
@pytest.mark.parametrize("name,pts", list(_lattices()))
def test_exact_ties(name, pts):
    """Integer lattices: every distance is an exact small integer in fp32 and fp64, so the whole result equals the
    brute force sorted by (distance, index) — the <= pruning and the index tie rule."""
    ref_d, ref_i = _brute_sorted(pts, 32)
    for K in KS:
        d, idx = _gpu_knn(pts, K)
        np.testing.assert_array_equal(d.astype(np.float64), ref_d[:, :K], err_msg=f"{name} K={K}")
        np.testing.assert_array_equal(idx, ref_i[:, :K], err_msg=f"{name} K={K}")


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 1023, 1025, 32769])
def test_ragged_sizes(P):
    pts = np.random.default_rng(P).uniform(-3, 3, (P, 3)).astype(np.float32)
    d, idx = _gpu_knn(pts, 16)
    _check_rows(pts, d, idx, _ref_dists(pts, 16), tag=f"P={P}")


@pytest.mark.gpu
def test_wrapper_behaviour():
    import torch
    from simple_knn import knn_points

    empty = knn_points(torch.zeros((0, 3), device="cuda"), K=5)
    assert empty.dists.shape == (0, 5) and empty.idx.shape == (0, 5)
    assert empty.dists.dtype == torch.float32 and empty.idx.dtype == torch.int64
    a, b = (torch.from_numpy(CLOUDS[n][:3000]).cuda() for n in ("uniform-5k", "duplicates-3k"))
    both = torch.stack([a, b])
    out = knn_points(both, both, K=8)
    assert out.dists.shape == (2, 3000, 8) and out.idx.shape == (2, 3000, 8)
    for k, one in enumerate((a, b)):
        single = knn_points(one, K=8)
        assert torch.equal(out.dists[k], single.dists) and torch.equal(out.idx[k], single.idx)
        again = knn_points(one, one, K=8)
        assert torch.equal(again.dists, single.dists) and torch.equal(again.idx, single.idx)
    # non-contiguous and float64 inputs, as distCUDA2 accepts them
    single = knn_points(a, K=8)
    wide = torch.zeros((3000, 5), device="cuda")
    wide[:, 1:4] = a
    nc = knn_points(wide[:, 1:4], K=8)
    f64 = knn_points(a.double(), K=8)
    for o in (nc, f64):
        assert torch.equal(o.dists, single.dists) and torch.equal(o.idx, single.idx)
    grad = knn_points(a.clone().requires_grad_(True), K=8)
    assert not grad.dists.requires_grad and torch.equal(grad.idx, single.idx)


@pytest.mark.gpu
def test_second_top_level_pass():
    """2,100,000 points: more than 64 top nodes of 32,768 points, so the outer loop of the walk runs twice (the
    smallest such cloud has 64 * 32768 + 1 points; the C5 scene's 1.97M stays under it).  2000 sampled queries
    against cKDTree, and the distCUDA2 tie on the same samples."""
    import torch
    from scipy.spatial import cKDTree
    from simple_knn import knn_points
    from simple_knn._C import distCUDA2

    rng = np.random.default_rng(5)
    n = 2_100_000
    pts = (rng.normal(size=(n, 3)) * np.cbrt(rng.uniform(0, 1, (n, 1))) * 0.8).astype(np.float32)
    q = rng.choice(n, 2000, replace=False)
    g = torch.from_numpy(pts).cuda()
    out = knn_points(g, K=16)
    assert out.dists.shape == (n, 16) and out.idx.shape == (n, 16)
    qi = torch.from_numpy(q).cuda()
    d, idx = out.dists[qi].cpu().numpy(), out.idx[qi].cpu().numpy()
    mean = distCUDA2(g)[qi].cpu().numpy()
    p = pts.astype(np.float64)
    ref, _ = cKDTree(p).query(p[q], k=16)
    _check_rows(pts, d, idx, ref ** 2, queries=q, tag="2.1M")
    np.testing.assert_array_equal(_mean3(d), mean)


@pytest.mark.gpu
def test_reference_call_sites():
    """reset_neighbors (geometry/sugar.py:646, utils/sugar_utils.py:248) and the K = 4 radius initialisation
    (utils/sugar_utils.py:41-54), restated on 20k points."""
    import torch
    from simple_knn import knn_points

    name = "ball-20k"
    points = torch.from_numpy(CLOUDS[name]).cuda()
    n = len(points)
    ref = _cloud_ref(name)
    with torch.no_grad():
        knns = knn_points(points[None], points[None], K=16)
        knn_dists, knn_idx = knns.dists[0], knns.idx[0]
    assert knn_dists.shape == (n, 16) and knn_idx.shape == (n, 16)
    assert torch.isfinite(knn_dists).all()
    np.testing.assert_allclose(knn_dists.cpu().numpy().astype(np.float64), ref[:, :16], rtol=RTOL, atol=0)

    knn = knn_points(points[None], points[None], K=4)
    radiuses = torch.sqrt(knn.dists[..., 1:]).min(-1, keepdim=True)[0].clamp_min(0.0000001) * 1.0
    assert radiuses.shape == (1, n, 1) and torch.isfinite(radiuses).all()
    want = np.maximum(np.sqrt(ref[:, 1:4]).min(-1, keepdims=True), 0.0000001)
    np.testing.assert_allclose(radiuses[0].cpu().numpy().astype(np.float64), want, rtol=RTOL, atol=0)
