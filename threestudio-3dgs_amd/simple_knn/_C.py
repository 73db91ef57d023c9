"""``simple_knn._C.distCUDA2`` over the C ABI (include/gsr.h gsr_knn_mean_dist, csrc/gsr_knn.hip).

The reference initialises Gaussian scales from the point cloud (geometry/gaussian_base.py:434-438):

    dist2 = torch.clamp_min(distCUDA2(torch.from_numpy(np.asarray(pcd.points)).float().cuda()), 0.0000001)

``distCUDA2(points)`` takes a float (P, 3) GPU tensor and returns the (P,) float tensor of mean squared
distances to each point's 3 nearest other points, like the external graphdeco-inria/simple-knn
extension.  The workspace comes from the PyTorch caching allocator; the kernels run on the current
stream.  No CPU path: a CPU tensor or a missing library raises.

``knn_points`` (include/gsr.h gsr_knn_points) stands in for ``pytorch3d.ops.knn_points`` where the reference's
SuGaR geometry searches a cloud against itself (geometry/sugar.py:646 and utils/sugar_utils.py:248
``reset_neighbors``, utils/sugar_utils.py:41 radius initialisation).
"""
from __future__ import annotations

import collections
import operator

import torch

from diff_gaussian_rasterization import _C as _gsr

__all__ = ["distCUDA2", "knn_points", "KNN", "KNN_MAX_K"]

KNN = collections.namedtuple("KNN", "dists idx knn")  # pytorch3d.ops.knn_points's result type
KNN_MAX_K = 32  # include/gsr.h GSR_KNN_MAX_K


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("distCUDA2 expects a (P, 3) tensor")
    dev = points.device
    _gsr._require_gpu(dev)
    lib = _gsr.load_library()
    pts = _gsr._f32(points, "points", dev)
    P = points.shape[0]
    out = torch.empty((P,), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    nbytes = int(lib.gsr_knn_workspace_bytes(P))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _gsr._check(lib.gsr_knn_mean_dist(P, _gsr._ptr(pts), _gsr._ptr(out), _gsr._ptr(ws), nbytes,
                                      _gsr._stream(dev)))
    return out


def knn_points(p1: torch.Tensor, p2: torch.Tensor | None = None, K: int = 1, return_sorted: bool = True) -> KNN:
    """The K nearest points of every point of a cloud within that cloud: ``pytorch3d.ops.knn_points(p, p, K=K)``.

    p1: (P, 3), or the reference's batched (B, P, 3) (the clouds are searched one after the other).  p2 must be
    None or p1 itself: searching another cloud is not built (NotImplementedError).  1 <= K <= 32.  Lengths
    arguments and ``return_nn`` are not accepted.  Returns ``KNN(dists, idx, knn)``: squared Euclidean distances
    (P, K) float32 and input indices (P, K) int64 (with a leading B for batched input); ``knn`` is always None.

    - The search is exact.  A point is its own neighbour, at distance 0.
    - Each row ascends by (distance, index): exact fp32 ties go to the lower index, so column 0 is the point
      itself unless an exact duplicate has a lower index, and two calls give the same bits.  ``return_sorted``
      is accepted for the signature's sake; rows are always sorted.
    - P < K: the missing columns hold dists = +inf and idx = -1.  This padding is this package's own definition
      (pytorch3d pads with 0 for clouds of unequal lengths in a batch; there is no such batch here).
    - NaN or infinite coordinates: unspecified.
    - No autograd (the reference calls it under ``torch.no_grad()``): the outputs never require grad.
    """
    if not isinstance(p1, torch.Tensor) or p1.dim() not in (2, 3) or p1.shape[-1] != 3:
        raise ValueError("knn_points expects a (P, 3) or (B, P, 3) tensor")
    try:
        K = operator.index(K)
    except TypeError:
        K = 0
    if not 1 <= K <= KNN_MAX_K:
        raise ValueError(f"knn_points: K must be an integer in 1..{KNN_MAX_K}, got {K!r}")
    if p2 is not None and not (isinstance(p2, torch.Tensor) and p2.data_ptr() == p1.data_ptr()
                               and p2.shape == p1.shape and p2.stride() == p1.stride()):
        raise NotImplementedError("knn_points: only the search of a cloud against itself is supported "
                                  "(p2 must be None or p1)")
    dev = p1.device
    _gsr._require_gpu(dev)
    lib = _gsr.load_library()
    pts = p1.detach()
    pts = pts if pts.numel() == 0 else _gsr._f32(pts, "points", dev)
    B, P = (1 if p1.dim() == 2 else int(p1.shape[0])), int(p1.shape[-2])
    clouds = pts.reshape(B, P, 3)
    dists = torch.empty((B, P, K), dtype=torch.float32, device=dev)
    idx = torch.empty((B, P, K), dtype=torch.int64, device=dev)
    if B * P > 0:
        nbytes = int(lib.gsr_knn_points_workspace_bytes(P, K))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)  # clouds run in stream order: one workspace
        for b in range(B):
            _gsr._check(lib.gsr_knn_points(P, K, _gsr._ptr(clouds[b]), _gsr._ptr(dists[b]), _gsr._ptr(idx[b]),
                                           _gsr._ptr(ws), nbytes, _gsr._stream(dev)))
    if p1.dim() == 2:
        return KNN(dists[0], idx[0], None)
    return KNN(dists, idx, None)
