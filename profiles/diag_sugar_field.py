"""Diagnostic: the fused SuGaR neighbour density field (sugar_field.neighbor_density, csrc/gsr_field.hip) against the
reference's formula as a torch composition on the same GPU, at the regulariser's size: M = 500 000 samples, K = 16,
N = 100k and 1M Gaussians, forward + backward with all three upstream gradients.  Gaussians: points of a ball with
16-NN from simple_knn.knn_points, scales from the neighbour distances with a flat third axis, random rotations;
samples drawn inside random Gaussians as sample_points_in_gaussians does.  HIP events on the current stream, warm-up,
the two paths alternated run by run, medians.  Per path: ms per step (forward + backward), ms of the forward alone,
peak allocated bytes above the inputs, and the forward's effective gather bandwidth (M K neighbours x (56 B of
Gaussian + 8 B of index) / forward time).  Prints one JSON object (committed as profiles/sugar_field.json).
Usage (GPU box): python profiles/diag_sugar_field.py [--runs 15] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
from diff_gaussian_rasterization import _C  # noqa: E402
from simple_knn import knn_points  # noqa: E402
from sugar_field import neighbor_density  # noqa: E402


def quat_to_matrix(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def make_scene(n, m, k, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = dict(device="cuda", generator=g)
    pts = torch.randn(n, 3, **r)
    pts = pts / pts.norm(dim=-1, keepdim=True) * 0.8 * torch.rand(n, 1, **r) ** (1 / 3)
    knn = knn_points(pts, K=k)
    radius = knn.dists[:, 1:4].mean(-1).sqrt().clamp_min(1e-7)
    scales = radius[:, None] * torch.exp(0.3 * torch.randn(n, 3, **r))
    scales[:, 2] *= 0.05
    rot = quat_to_matrix(torch.randn(n, 4, **r))
    gi = torch.randint(0, n, (m,), **r)
    x = pts[gi] + (rot[gi] @ (1.5 * scales[gi] * torch.randn(m, 3, **r))[..., None])[..., 0]
    return dict(x=x, centers=pts, inv_sr=(rot * (1 / scales.clamp(min=1e-8))[:, None]).contiguous(),
                strengths=torch.sigmoid(2 * torch.randn(n, **r)), min_scale=scales.min(-1)[0], knn=knn.idx, gi=gi,
                ups=(torch.randn(m, **r), torch.randn(m, **r), torch.randn(m, k, **r)))


def composition(x, centers, inv_sr, strengths, min_scale, idx):
    """utils/sugar_utils.py:296-310 and :423 as written there."""
    shift = x[:, None] - centers[idx]
    warped = inv_sr[idx].transpose(-1, -2) @ shift[..., None]
    q = (warped[..., 0] * warped[..., 0]).sum(dim=-1).clamp(min=0., max=1e8)
    op = strengths[idx] * torch.exp(-1. / 2 * q)
    return op.sum(dim=-1), min_scale[idx].mean(dim=1), op


def paths(sc):
    names = ("x", "centers", "inv_sr", "strengths", "min_scale")

    def leaves():
        return [sc[k].detach().requires_grad_() for k in names]

    def fused(backward=True):
        lv = leaves()
        den, beta, op = neighbor_density(*lv, knn_idx=sc["knn"], gaussian_idx=sc["gi"], return_opacities=True)
        return torch.autograd.grad((den, beta, op), lv, sc["ups"]) if backward else (den, beta, op)

    def torch_composition(backward=True):
        lv = leaves()
        out = composition(*lv, sc["knn"][sc["gi"]])
        return torch.autograd.grad(out, lv, sc["ups"]) if backward else out

    return {"fused": fused, "torch": torch_composition}


def timed(fn, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(**kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    M, K = 500_000, 16
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "M": M, "K": K, "sizes": {}}
    for n in (100_000, 1_000_000):
        sc = make_scene(n, M, K)
        fns = paths(sc)
        ms = {name: {"step": [], "forward": []} for name in fns}
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():  # alternated: both paths see the same clocks and cache state drift
                step, fwd = timed(fn), timed(fn, backward=False)
                if it >= args.warmup:
                    ms[name]["step"].append(step)
                    ms[name]["forward"].append(fwd)
        row = {}
        for name, fn in fns.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            fwd = statistics.median(ms[name]["forward"])
            row[name] = {"step_ms": round(statistics.median(ms[name]["step"]), 4),
                         "step_min_ms": round(min(ms[name]["step"]), 4),
                         "step_max_ms": round(max(ms[name]["step"]), 4), "forward_ms": round(fwd, 4),
                         "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base),
                         "forward_gather_GBps": round(M * K * 64 / (fwd * 1e-3) / 1e9, 1)}
        row["torch_over_fused_step"] = round(row["torch"]["step_ms"] / row["fused"]["step_ms"], 2)
        a, b = fns["fused"](), fns["torch"]()
        row["max_abs_grad_diff"] = [float((p - q).abs().max()) for p, q in zip(a, b)]
        res["sizes"][str(n)] = row
        del sc, fns, a, b
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
