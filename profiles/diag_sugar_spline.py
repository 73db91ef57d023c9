"""Diagnostic: the fused B-spline of the timed node attributes (sugar_spline.spline_attributes, csrc/gsr_spline.hip)
against the fp32 torch restatement of the reference's Spline.forward on the same GPU, at the two shipped sizes: T = 8
timestamps, 32 knots (SplineGrid.for_frames(32)), degree 3, with the scale attribute, P = 1000 points (the nodes of a
deformation graph) and P = 163 842 (the vertices of icosphere(7): ``use_deform_graph=False``).

The torch composition is tests/sugar_spline_reference.py's restatement (float32, on the GPU, autograd backward): per
attribute four indexed gathers of knot rows, the coefficient polynomials, and for the rotation three Hamilton products,
Logs and Exps and the product chain, all as broadcast tensor expressions.  It FLATTERS the reference: no pypose
LieTensor dispatch, no ``bvv`` outer product and sum, no ``rearrange`` / ``repeat_interleave`` / ``tile`` / ``cat`` of
the segment tensors, one call for the three attributes.

HIP events on the current stream around windows of ``--iters`` calls, warm-up, the two paths alternated window by
window, medians over ``--runs`` windows.  Per path: ms per forward, ms per forward + backward (random upstream
gradients), peak allocated bytes above the inputs.  The fused path launches one kernel per forward and two per
backward; the torch path's launches were not counted.  For the fused path also the bytes the mathematics needs (each input, output and workspace
array once per kernel that touches it) and the fraction of the HBM peak (8 TB/s) that they make of the measured time:
an end-to-end figure of the call (its launches and the allocator included), not of a single kernel.
Prints one JSON object (committed as profiles/sugar_spline.json).
Usage (GPU box): python profiles/diag_sugar_spline.py [--runs 9] [--iters 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from diff_gaussian_rasterization import _C  # noqa: E402
from sugar_spline import SplineGrid, spline_attributes  # noqa: E402
from sugar_spline_reference import spline_reference  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
SIZES = (1000, 163_842)
T, N_KNOTS, DEGREE = 8, 32, 3


def math_bytes(P):
    """(forward, forward + backward) bytes of spline_attributes with scale."""
    seg = (DEGREE + 1) * T * P
    fwd = 4 * T + seg * 40 + T * P * 40  # k_spline_forward: the knot rows of each timestamp, the outputs
    rows = 80 * seg
    # k_spline_rows: the rotation knots, the upstream gradients, the rows; k_spline_knots: each row once, the gradients
    bwd = (4 * T + seg * 16 + T * P * 40 + rows) + (4 * T + rows + N_KNOTS * P * 40)
    return fwd, fwd + bwd


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def make_scene(P, seed=0):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    quat = rnd(N_KNOTS, P, 4) * 0.2
    quat[..., 3] += 1.0
    t = torch.rand(T, generator=gen, device=dev)  # a batch of random timestamps in [0, 1), as the sampler draws them
    return dict(grid=SplineGrid.for_frames(N_KNOTS, DEGREE), t=t,
                knots=[0.1 * rnd(N_KNOTS, P, 3), quat, 0.1 * rnd(N_KNOTS, P, 3)],
                ups=[rnd(T, P, 3), rnd(T, P, 4), rnd(T, P, 3)])


def paths(sc):
    def run(make, backward):
        leaves = [k.detach().requires_grad_() for k in sc["knots"]]
        out = make(*leaves)
        return torch.autograd.grad(out, leaves, sc["ups"]) if backward else out

    return {"fused": lambda backward=True: run(lambda x, r, s: spline_attributes(sc["t"], x, r, sc["grid"], s), backward),
            "torch": lambda backward=True: run(lambda x, r, s: spline_reference(sc["t"], x, r, sc["grid"], s), backward)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters, "T": T, "n_knots": N_KNOTS,
           "degree": DEGREE, "scale": True,
           "torch_composition": "fp32 restatement of Spline.forward for the three attributes as broadcast tensor "
                                "expressions with autograd: no pypose LieTensor dispatch, no bvv, rearrange, "
                                "repeat_interleave, tile or cat, so it flatters the reference",
           "sizes": {}}
    for P in SIZES:
        sc = make_scene(P)
        fns = paths(sc)
        ms = {name: {"step": [], "forward": []} for name in fns}
        for name, fn in fns.items():  # one synchronised call each first: a failure names its path
            fn()
            torch.cuda.synchronize()
            print(f"P = {P} {name}: ran", file=sys.stderr, flush=True)
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():  # alternated: both paths see the same clocks and cache state drift
                step = window(fn, args.iters)
                fwd = window(lambda: fn(backward=False), args.iters)
                if it >= args.warmup:
                    ms[name]["step"].append(step)
                    ms[name]["forward"].append(fwd)
        r = {}
        for name, fn in fns.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            r[name] = {"step_ms": round(statistics.median(ms[name]["step"]), 4),
                       "step_min_ms": round(min(ms[name]["step"]), 4),
                       "step_max_ms": round(max(ms[name]["step"]), 4),
                       "forward_ms": round(statistics.median(ms[name]["forward"]), 4),
                       "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}
        g = fns["fused"]()  # the knots some timestamp covers, from the fused gradient itself
        covered = int(g[0].abs().sum(dim=(1, 2)).ne(0).sum())
        fb, stb = math_bytes(P)
        r["fused"].update(
            covered_knots=covered, forward_math_bytes=fb, step_math_bytes=stb,
            forward_fraction_of_hbm_peak=round(fb / (r["fused"]["forward_ms"] * 1e-3) / HBM_PEAK, 4),
            step_fraction_of_hbm_peak=round(stb / (r["fused"]["step_ms"] * 1e-3) / HBM_PEAK, 4))
        r["torch_over_fused_step"] = round(r["torch"]["step_ms"] / r["fused"]["step_ms"], 2)
        r["torch_over_fused_forward"] = round(r["torch"]["forward_ms"] / r["fused"]["forward_ms"], 2)
        t = fns["torch"]()
        r["max_abs_grad_diff"] = [float((x - y).abs().max()) for x, y in zip(g, t)]
        r["max_abs_grad"] = [float(y.abs().max()) for y in t]
        res["sizes"][str(P)] = r
        del sc, g, t
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
