"""Time sugar_deform.deformation_knots against the fp32 torch composition it replaces, on the same card:
forward and forward + backward at the two shipped sizes (T = 32 ticks x P = 1000 graph nodes, with and without the
scale head, and x P = 163 842 vertices), the two sides alternated call by call; transient memory of both sides and the
achieved share of the HBM peak on algorithmic bytes.  Writes profiles/sugar_deform.json.

The torch side is ``forward_dynamic_delta`` as the reference composes it (24 ``grid_sample`` calls on the
``repeat_interleave``d points and ticks, 20 products, a ``cat``, 7 ``Linear`` layers) plus the epilogue, in float32.

Usage:  python profiles/diag_sugar_deform.py [--reps 20] [--out profiles/sugar_deform.json]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))

from sugar_deform import DeformationWeights, HexPlaneBinding, deformation_knots  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
COMBOS = tuple(itertools.combinations(range(4), 2))


def torch_knots(points, ticks, aabb, planes, mlp, normalize):
    T, P = ticks.shape[0], points.shape[0]
    pts = torch.cat([points] * T, 0)
    ts = ticks.unsqueeze(-1).repeat_interleave(P, 0) * 2 - 1
    x = torch.cat([(pts - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0, ts], -1)
    feats = []
    for l in range(len(planes) // 6):
        f = 1.0
        for q, comb in enumerate(COMBOS):
            g = F.grid_sample(planes[6 * l + q], x[:, comb].view(1, 1, -1, 2), align_corners=True, mode="bilinear",
                              padding_mode="border")
            f = f * g.view(32, -1).t()
        feats.append(f)
    h = F.linear(torch.cat(feats, -1), mlp[0], mlp[1])
    outs = []
    for i in range(2, len(mlp), 4):
        r = torch.relu(h)
        outs.append(F.linear(r + F.linear(r, mlp[i], mlp[i + 1]), mlp[i + 2], mlp[i + 3]))
    rot = outs[1].reshape(T, P, 4) + torch.tensor([0.0, 0.0, 0.0, 1.0], device=points.device)
    if normalize:
        rot = rot / rot.norm(dim=-1, keepdim=True)
    return (outs[0].reshape(T, P, 3), rot) + ((outs[2].reshape(T, P, 3),) if len(outs) > 2 else ())


def measure(fns, reps):
    """Alternate the callables; per callable the median ms and the peak bytes above the resting allocation."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms, peak = {k: [] for k in fns}, {k: 0 for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            rest = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - rest)
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "transient_bytes": peak[k]} for k, v in ms.items()}


def run(T, P, d_scale, normalize, reps, gen):
    dev = "cuda"
    points = (torch.rand(P, 3, generator=gen) * 1.8 - 0.9).to(dev)
    n = 32
    ticks = torch.linspace(-1 / (n - 3), 1 + 1 / (n - 3), T).to(dev)
    aabb = torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]], device=dev)
    w = DeformationWeights.init_like_reference(gen, d_scale=d_scale)
    with torch.no_grad():  # trained-like heads: the zero initialisation would leave the backward nothing to do
        for t in w.mlp[2:]:
            t.copy_(torch.randn(t.shape, generator=gen) * 0.1)
    w = w.to(dev).requires_grad_()
    binding = HexPlaneBinding(points, ticks, aabb).to(dev)
    prm = w.parameters()
    ups = [torch.randn(T, P, c, device=dev) for c in ((3, 4, 3) if d_scale else (3, 4))]

    def backward(out):
        torch.autograd.grad(sum((o * u).sum() for o, u in zip(out, ups)), prm)

    fused = lambda: [o for o in deformation_knots(binding, w, normalize, d_scale) if o is not None]  # noqa: E731
    composed = lambda: torch_knots(points, ticks, aabb, w.planes, w.mlp, normalize)  # noqa: E731

    def no_grad(fn):
        def call():
            with torch.no_grad():
                fn()
        return call

    res = measure({"fused_fwd": no_grad(fused), "torch_fwd": no_grad(composed),
                   "fused_fwd_bwd": lambda: backward(fused()), "torch_fwd_bwd": lambda: backward(composed())}, reps)
    S, K, nout = T * P, 128, 10 if d_scale else 7
    n_prm = sum(t.numel() for t in prm)
    # algorithmic bytes: forward reads 24 x 4 texels x 32 channels per sample and writes the outputs; the backward reads
    # that again with the upstream gradients and writes every parameter gradient once
    fwd_bytes = S * (24 * 4 * 32 * 4 + nout * 4) + sum(t.numel() for t in w.mlp) * 4
    bwd_bytes = fwd_bytes + S * nout * 4 + n_prm * 4
    for k, b in (("fused_fwd", fwd_bytes), ("fused_fwd_bwd", fwd_bytes + bwd_bytes)):
        res[k]["algorithmic_bytes"] = b
        res[k]["hbm_share"] = b / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
    res["fwd_torch_over_fused"] = res["torch_fwd"]["ms_median"] / res["fused_fwd"]["ms_median"]
    res["fwd_bwd_torch_over_fused"] = res["torch_fwd_bwd"]["ms_median"] / res["fused_fwd_bwd"]["ms_median"]
    res.update(T=T, P=P, d_scale=d_scale, normalize_rot=normalize, reps=reps, binding_bytes=binding.nbytes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sugar_deform.json"))
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "cases": {}}
    for name, P, d_scale, normalize, reps in (("nodes_scale", 1000, True, True, args.reps),
                                              ("nodes_noscale", 1000, False, True, args.reps),
                                              ("vertices_scale", 163842, True, False, max(3, args.reps // 5))):
        out["cases"][name] = run(32, P, d_scale, normalize, reps, gen)
        c = out["cases"][name]
        print(name, {k: round(c[k]["ms_median"], 3) for k in ("fused_fwd", "torch_fwd", "fused_fwd_bwd", "torch_fwd_bwd")},
              flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
