"""Diagnostic: the densification statistics of a view batch — the fused call (densify.densify_stats, one
k_dstat_views launch per 64 views, csrc/gsr_densify.hip) against the reference-form per-view torch loop
(geometry/gaussian_base.py:845-851 with :815-819: torch.max, norm(grad[vis, :2]) added by mask indexing, denom[vis] += 1)
on the same card with the same tensors, at 64 views x 1M Gaussians and 8 views x 2M Gaussians.

The inputs are seeded random rows on the GPU (radii 0..5, a sixth not visible; gradients N(0, 0.02)); both paths update
the same kind of state ((P,), (P,1), (P,1)) in place, as a training step does.  Per shape and path: HIP events on the
current stream around windows of ``--iters`` calls of the loop and ten times as many of the fused call (the loop's
host syncs fall inside its windows: they are part of what it costs), warm-up windows first, the paths alternated
window by window, the median, min and max over ``--runs`` windows.  Launches: device kernels and memory copies of one call, counted by the torch profiler in a call of its own
after the timing.  For the fused call the algorithmic bytes — V P (4 + 8) read (+ V P with visibility rows), 3 x 4 P read
and written — over its time, and that rate's share of the HBM peak (8 TB/s by specification; 6.3 TB/s is what a copy
reaches on this card).  The two paths' results are compared once per shape (count and max equal; the largest relative
difference of the sums is recorded).
Prints one JSON object (committed as profiles/densify_stats.json).
Usage (GPU box): python profiles/diag_densify_stats.py [--runs 9] [--iters 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
from diff_gaussian_rasterization import _C  # noqa: E402
from diff_gaussian_rasterization.densify import densify_stats  # noqa: E402

SHAPES = ((64, 1_000_000), (8, 2_000_000))
HBM_PEAK = 8.0e12      # bytes / s, specification
HBM_COPY = 6.3e12      # bytes / s, what a float4 copy reaches


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def make_case(V, P, dev):
    gen = torch.Generator(device=dev).manual_seed(V * 31 + 1)
    radii, vps = [], []
    for _ in range(V):
        radii.append(torch.randint(0, 6, (P,), generator=gen, device=dev, dtype=torch.int32))
        vp = torch.zeros(P, 3, device=dev, requires_grad=True)
        vp.grad = torch.randn(P, 3, generator=gen, device=dev) * 0.02
        vps.append(vp)
    return radii, vps, [r > 0 for r in radii]


def new_state(P, dev):
    return torch.zeros(P, device=dev), torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev)


def reference_loop(radii, vps, vis, state):
    """The reference's statements, view by view (the state list is rebound as the reference rebinds max_radii2D)."""
    with torch.no_grad():
        for r, vp, f in zip(radii, vps, vis):
            state[0] = torch.max(state[0], r.float())
            state[1][f] += torch.norm(vp.grad[f, :2], dim=-1, keepdim=True)
            state[2][f] += 1


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    for ev in prof.events():
        if str(ev.device_type).endswith("CUDA"):
            if "memcpy" in ev.name.lower():
                copies += 1
            else:
                kernels += 1
    return kernels, copies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="V,P;V,P (default: 64,1000000;8,2000000)")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    shapes = SHAPES if args.shapes is None else tuple(tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";"))
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": {"loop": args.iters, "fused": 10 * args.iters},
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_copy_bytes_per_s": HBM_COPY, "shapes": []}
    for V, P in shapes:
        radii, vps, vis = make_case(V, P, dev)
        states = {"fused": list(new_state(P, dev)), "fused_rows": list(new_state(P, dev)),
                  "loop": list(new_state(P, dev))}
        fns = {
            "fused": lambda: densify_stats(radii, vps, None, max_radii=states["fused"][0],
                                           grad_norm_sum=states["fused"][1], count=states["fused"][2]),
            "fused_rows": lambda: densify_stats(radii, vps, vis, max_radii=states["fused_rows"][0],
                                                grad_norm_sum=states["fused_rows"][1], count=states["fused_rows"][2]),
            "loop": lambda: reference_loop(radii, vps, vis, states["loop"]),
        }
        # one synchronised call each first (a failure names its path), and the results compared
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            print(f"{V}x{P} {name}: ran", file=sys.stderr, flush=True)
        f, lp = states["fused"], states["loop"]
        agree = {"max_equal": bool(torch.equal(f[0], lp[0])), "count_equal": bool(torch.equal(f[2], lp[2])),
                 "rows_equal_radii_bitwise": all(bool(torch.equal(a, b)) for a, b in zip(f, states["fused_rows"])),
                 "sum_max_rel_diff": float(((f[1] - lp[1]).abs() / lp[1].clamp_min(1e-30)).max())}
        ms = {name: [] for name in fns}
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():  # alternated: the paths see the same clocks
                t = window(fn, args.iters if name == "loop" else 10 * args.iters)  # (sub-millisecond calls)
                if it >= args.warmup:
                    ms[name].append(t)
        entry = {"views": V, "gaussians": P, "agreement": agree, "paths": {}}
        for name in fns:
            med = statistics.median(ms[name])
            entry["paths"][name] = {"call_ms": round(med, 4), "call_min_ms": round(min(ms[name]), 4),
                                    "call_max_ms": round(max(ms[name]), 4)}
            if not args.no_launch_count:
                try:
                    k, c = count_launches(fns[name])
                    entry["paths"][name].update(kernel_launches=k, memory_copies=c)
                except Exception as e:  # (the timings stand without the count)
                    entry["paths"][name].update(kernel_launches=None, launch_count_error=repr(e)[:200])
        for name, rows in (("fused", 0), ("fused_rows", 1)):
            nbytes = V * P * (4 + 8 + rows) + 2 * 3 * 4 * P
            rate = nbytes / (entry["paths"][name]["call_ms"] * 1e-3)
            entry["paths"][name].update(algorithmic_bytes=nbytes, bytes_per_s=round(rate, 1),
                                        share_of_hbm_peak=round(rate / HBM_PEAK, 4),
                                        share_of_hbm_copy_rate=round(rate / HBM_COPY, 4))
        entry["loop_over_fused"] = round(entry["paths"]["loop"]["call_ms"] / entry["paths"]["fused"]["call_ms"], 2)
        res["shapes"].append(entry)
        del radii, vps, vis, states, fns
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
