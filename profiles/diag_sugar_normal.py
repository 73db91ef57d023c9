"""Diagnostic: the fused SuGaR neighbour-normal loss (sugar_field.neighbor_normal_loss, csrc/gsr_normal.hip) against
the reference's formula (utils/sugar_utils.py:725-757) as a torch composition on the same GPU, at the regulariser's
size: M = 500 000 samples, K = 16, N = 100k and 1M Gaussians, forward + backward to the normals from the mean loss.
Scene as profiles/diag_sugar_field.py (points of a ball, 16-NN from simple_knn.knn_points, flat third axis, random
rotations, samples drawn inside random Gaussians); normals = each Gaussian's flat axis, opacities = the fused field's.
HIP events on the current stream, warm-up, the two paths alternated run by run, medians.  Per path: ms per step
(forward + backward), ms of the forward alone, peak allocated bytes above the inputs.  Prints one JSON object
(committed as profiles/sugar_normal.json).
Usage (GPU box): python profiles/diag_sugar_normal.py [--runs 15] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from diag_sugar_field import make_scene, timed  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from sugar_field import neighbor_density, neighbor_normal_loss  # noqa: E402


def composition(x, centers, normals, min_scale, op, knn_idx, gaussian_idx):
    """utils/sugar_utils.py:726-756 as written there."""
    closest_gaussians_idx = knn_idx[gaussian_idx]
    closest_min_scaling = min_scale[closest_gaussians_idx].detach().view(len(x), -1)
    closest_gaussian_normals = normals[closest_gaussians_idx]
    samples_gaussian_normals = normals[gaussian_idx]
    closest_gaussian_normals = closest_gaussian_normals * torch.sign(
        (closest_gaussian_normals * samples_gaussian_normals[:, None]).sum(dim=-1, keepdim=True)).detach()
    normal_weights = ((x[:, None] - centers[closest_gaussians_idx]) * closest_gaussian_normals).sum(dim=-1).abs()
    normal_weights = normal_weights.detach()
    normal_weights = op.detach() * normal_weights / closest_min_scaling.clamp(min=1e-6) ** 2
    normal_weights_sum = normal_weights.sum(dim=-1).detach()
    normal_weights = normal_weights / normal_weights_sum.unsqueeze(-1).clamp(min=1e-6)
    return (samples_gaussian_normals - (normal_weights[..., None] * closest_gaussian_normals).sum(dim=-2)
            ).pow(2).sum(dim=-1)


def paths(sc):
    def fused(backward=True):
        n = sc["normals"].detach().requires_grad_()
        loss = neighbor_normal_loss(sc["x"], sc["centers"], n, sc["min_scale"], sc["op"], gaussian_idx=sc["gi"],
                                    knn_idx=sc["knn"])
        return torch.autograd.grad(loss.mean(), n)[0] if backward else loss

    def torch_composition(backward=True):
        n = sc["normals"].detach().requires_grad_()
        loss = composition(sc["x"], sc["centers"], n, sc["min_scale"], sc["op"], sc["knn"], sc["gi"])
        return torch.autograd.grad(loss.mean(), n)[0] if backward else loss

    return {"fused": fused, "torch": torch_composition}


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
        with torch.no_grad():
            flat = (sc["inv_sr"] * sc["min_scale"][:, None, None])[:, :, 2]  # column 2: the axis of the 0.05 scale
            sc["normals"] = (flat / flat.norm(dim=-1, keepdim=True)).contiguous()
            sc["op"] = neighbor_density(sc["x"], sc["centers"], sc["inv_sr"], sc["strengths"], sc["min_scale"],
                                        knn_idx=sc["knn"], gaussian_idx=sc["gi"], return_opacities=True)[2]
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
            row[name] = {"step_ms": round(statistics.median(ms[name]["step"]), 4),
                         "step_min_ms": round(min(ms[name]["step"]), 4),
                         "step_max_ms": round(max(ms[name]["step"]), 4),
                         "forward_ms": round(statistics.median(ms[name]["forward"]), 4),
                         "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}
        row["torch_over_fused_step"] = round(row["torch"]["step_ms"] / row["fused"]["step_ms"], 2)
        a, b = fns["fused"](), fns["torch"]()
        row["max_abs_grad_diff"] = float((a - b).abs().max())
        row["max_abs_grad"] = float(b.abs().max())
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
