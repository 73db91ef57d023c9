"""Diagnostic: time of simple_knn.knn_points (csrc/gsr_knn.hip k_knn_points) on the benchmark's ball of points
(gsr_synthetic.make_scene's positions: uniform in a ball of radius 0.8) at the C3 (1M) and C5-class (2M) sizes for
K = 4 and K = 16, beside distCUDA2 on the same points (the same tree with a 3-entry list) and a brute-force
baseline on the same GPU at 100k points (chunked torch.cdist(...)**2 + topk, K = 16).  HIP events on the current
stream, warm-up, median of the timed runs.  Prints one JSON object (committed as profiles/knn_points.json).
Usage (GPU box): python profiles/diag_knn_points.py [--runs 15]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
from diff_gaussian_rasterization import _C  # noqa: E402
from simple_knn._C import distCUDA2, knn_points  # noqa: E402


def ball(n, seed=0, radius=0.8):
    """Positions of gsr_synthetic.make_scene (without its host-side scale initialisation)."""
    rng = np.random.default_rng(seed)
    phis = rng.random(n) * 2 * np.pi
    thetas = np.arccos(rng.random(n) * 2 - 1)
    r = radius * np.cbrt(rng.random(n))
    xyz = np.stack([r * np.sin(thetas) * np.cos(phis), r * np.sin(thetas) * np.sin(phis), r * np.cos(thetas)], axis=1)
    return torch.from_numpy(xyz.astype(np.float32)).cuda()


def time_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def brute_force(points, K, chunk=4096):
    """Exact K-NN by distance matrix: (chunk, P) squared distances, K smallest per row."""
    d, i = [], []
    for s in range(0, points.shape[0], chunk):
        dd, ii = torch.topk(torch.cdist(points[s:s + chunk], points) ** 2, K, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _C.load_library()
    res = {"library": lib.gsr_version().decode(), "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "warmup": args.warmup, "sizes": {}}
    for n in (1_000_000, 2_000_000):
        pts = ball(n)
        row = {"distCUDA2": time_ms(lambda: distCUDA2(pts), args.warmup, args.runs)}
        for K in (4, 16):
            row[f"knn_points_K{K}"] = time_ms(lambda: knn_points(pts, K=K), args.warmup, args.runs)
            row[f"knn_points_K{K}_over_distCUDA2"] = round(
                row[f"knn_points_K{K}"]["median_ms"] / row["distCUDA2"]["median_ms"], 2)
        res["sizes"][str(n)] = row
    n = 100_000
    pts = ball(n)
    ours = knn_points(pts, K=16)
    bd, _ = brute_force(pts, 16)
    # the baseline finds the same neighbours (cdist's distances differ in the last bits, and near 0 by cancellation)
    res["brute_force_max_abs_diff"] = float((bd - ours.dists).abs().max())
    row = {"knn_points_K16": time_ms(lambda: knn_points(pts, K=16), args.warmup, args.runs),
           "brute_force_cdist_topk_K16": time_ms(lambda: brute_force(pts, 16), args.warmup, args.runs)}
    row["brute_force_over_knn_points"] = round(
        row["brute_force_cdist_topk_K16"]["median_ms"] / row["knn_points_K16"]["median_ms"], 1)
    res["sizes"][str(n)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
