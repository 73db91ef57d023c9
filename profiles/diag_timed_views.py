"""Diagnostic: a timed view set (batched.rasterize_timed_views, csrc/gsr_timed.hip) at the shipped SuGaR size — T = 8
frames of make_sugar_scene(7) (1 966 080 Gaussians), 800^2, two colours (the frames' face normals as colors2), the
fused clamp, forward + backward — against what the project offered before it and against its ceiling, on the same
card in the same process:

  (a) timed     one rasterize_timed_views call: view t renders frame t (per-view means3D, scales, rotations, colors2)
  (b) per_view  eight one-view rasterize_views calls on the frame slices: the baseline, all the parent commit offers
  (c) shared    one 8-view rasterize_views call on frame 0's geometry: the ceiling (nothing per view)

The frames are frame 0 turned by 0.05 t rad about z, blown up by 1 + 0.02 t, its scales times 1 + 0.05 t (formed on
the GPU before the timing; the geometry stages that would produce them are not part of any path).  Upstream gradients
are fixed random images.  HIP events on the current stream around windows of ``--iters`` steps, warm-up windows, the
three paths alternated window by window, medians over ``--runs`` windows.  Per path: ms per step (forward + backward
of all 8 views), min / max, and the peak allocated bytes above the inputs (transient memory).  For (a) also the
library's per-phase kernel milliseconds from one profiled step (gsr_profile_*): the new kernels are the whole
"preprocess" phase (k_preprocess_timed and the two depth-range kernels) and the whole "gauss_bwd" phase (k_tv_grad);
their share is of the sum over the phases.
Prints one JSON object (committed as profiles/timed_views.json).
Usage (GPU box): python profiles/diag_timed_views.py [--runs 7] [--iters 3] [--subdiv 7] [--size 800] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
import gsr_synthetic as gs  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizationSettings, _C  # noqa: E402
from diff_gaussian_rasterization.batched import rasterize_timed_views, rasterize_views  # noqa: E402
from diff_gaussian_rasterization.cameras import get_cam_info_gaussian, orbit_c2w  # noqa: E402

T = 8
C0 = 0.28209479177387814


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def make_case(subdiv, size):
    dev = "cuda"
    sc = gs.make_sugar_scene(subdiv, sh_degree=0, seed=0)
    t32 = lambda a: torch.tensor(a, device=dev, dtype=torch.float32)  # noqa: E731
    xyz, scales, rot, normals = t32(sc["means3D"]), t32(sc["scales"]), t32(sc["rotations"]), t32(sc["normals"])
    fr = dict(means3D=[], scales=[], rotations=[], colors2=[])
    for t in range(T):
        a = 0.05 * t
        Rz = t32([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        fr["means3D"].append((xyz @ Rz.T) * (1 + 0.02 * t))
        fr["scales"].append(scales * (1 + 0.05 * t))
        q = quat_mul(t32([math.cos(a / 2), 0, 0, math.sin(a / 2)]), rot)
        fr["rotations"].append(q / q.norm(dim=-1, keepdim=True))
        fr["colors2"].append(normals @ Rz.T)
    frames = {k: torch.stack(v).contiguous() for k, v in fr.items()}
    fovy = math.radians(60.0)
    c2w = orbit_c2w(torch.full((T,), 2.5), torch.full((T,), 15.0), torch.arange(T) * (360.0 / T))
    w2c, proj, campos = get_cam_info_gaussian(c2w, torch.full((T,), fovy), torch.full((T,), fovy), znear=0.1, zfar=100)
    bg = torch.ones(3, device=dev)
    settings = [GaussianRasterizationSettings(size, size, math.tan(fovy / 2), math.tan(fovy / 2), bg, 1.0,
                                              w2c[v].to(dev), proj[v].to(dev), 0, campos[v].to(dev), False, False)
                for v in range(T)]
    gen = torch.Generator(device=dev).manual_seed(1)
    ups = [torch.randn(T, c, size, size, generator=gen, device=dev) for c in (3, 1, 1, 3)]
    P = xyz.shape[0]
    return dict(P=P, frames=frames, opacity=t32(sc["opacities"]), colors=(0.5 + C0 * t32(sc["shs"])[:, 0]).contiguous(),
                settings=settings, ups=ups, m2=lambda n: [torch.zeros(P, 3, device=dev, requires_grad=True)
                                                           for _ in range(n)])


def paths(cs):
    fr, ups = cs["frames"], cs["ups"]
    leaf = lambda x: x.detach().requires_grad_()  # noqa: E731

    def loss(outs, sl=slice(None)):
        c, _, d, a, c2 = outs
        return (c * ups[0][sl]).sum() + (d * ups[1][sl]).sum() + (a * ups[2][sl]).sum() + (c2 * ups[3][sl]).sum()

    def timed():
        lv = {k: leaf(v) for k, v in fr.items()}
        op, col = leaf(cs["opacity"]), leaf(cs["colors"])
        outs = rasterize_timed_views(cs["settings"], lv["means3D"], cs["m2"](T), op, col, lv["scales"], lv["rotations"],
                                     colors2=lv["colors2"], clamp=True)
        return torch.autograd.grad(loss(outs), list(lv.values()) + [op, col])

    def per_view():
        op, col = leaf(cs["opacity"]), leaf(cs["colors"])
        total, leaves = 0, [op, col]
        for v in range(T):
            lv = {k: leaf(x[v]) for k, x in fr.items()}
            outs = rasterize_views(cs["settings"][v:v + 1], lv["means3D"], cs["m2"](1), op, colors_precomp=col,
                                   scales=lv["scales"], rotations=lv["rotations"], colors2=lv["colors2"], clamp=True)
            total = total + loss(outs, slice(v, v + 1))
            leaves += list(lv.values())
        return torch.autograd.grad(total, leaves)

    def shared():
        lv = {k: leaf(x[0]) for k, x in fr.items()}
        op, col = leaf(cs["opacity"]), leaf(cs["colors"])
        outs = rasterize_views(cs["settings"], lv["means3D"], cs["m2"](T), op, colors_precomp=col, scales=lv["scales"],
                               rotations=lv["rotations"], colors2=lv["colors2"], clamp=True)
        return torch.autograd.grad(loss(outs), list(lv.values()) + [op, col])

    return {"timed": timed, "per_view": per_view, "shared": shared}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--subdiv", type=int, default=7)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cs = make_case(args.subdiv, args.size)
    fns = paths(cs)
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters, "frames": T, "gaussians": cs["P"],
           "image": [args.size, args.size], "two_colors": True, "clamp": True, "paths": {}}
    ms = {name: [] for name in fns}
    for name, fn in fns.items():  # one synchronised step each first: a failure names its path
        fn()
        torch.cuda.synchronize()
        print(f"{name}: ran", file=sys.stderr, flush=True)
    for it in range(args.warmup + args.runs):
        for name, fn in fns.items():  # alternated: the paths see the same clocks and cache state drift
            step = window(fn, args.iters)
            if it >= args.warmup:
                ms[name].append(step)
    for name, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res["paths"][name] = {"step_ms": round(statistics.median(ms[name]), 3), "step_min_ms": round(min(ms[name]), 3),
                              "step_max_ms": round(max(ms[name]), 3),
                              "views_per_s": round(T / (statistics.median(ms[name]) * 1e-3), 1),
                              "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}
    # the phases of one profiled timed step (event pairs around each phase: not part of the timings above)
    _C.profile_enable(True)
    _C.profile_read(reset=True)
    fns["timed"]()
    torch.cuda.synchronize()
    phases = {k: round(v[0], 3) for k, v in _C.profile_read(reset=True).items()}
    _C.profile_enable(False)
    total = sum(phases.values())
    res["timed_phase_ms"] = phases
    res["timed_new_kernels_share"] = round((phases["preprocess"] + phases["gauss_bwd"]) / total, 4) if total else None
    p = res["paths"]
    res["timed_over_per_view"] = round(p["timed"]["step_ms"] / p["per_view"]["step_ms"], 3)
    res["timed_over_shared"] = round(p["timed"]["step_ms"] / p["shared"]["step_ms"], 3)
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
