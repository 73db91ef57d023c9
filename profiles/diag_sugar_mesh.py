"""Diagnostic: the fused geometry of mesh-bound SuGaR Gaussians (sugar_mesh.bound_gaussians, csrc/gsr_mesh.hip)
against the fp32 torch composition of the same formulas on the same GPU, at C5's size (icosphere(7), G = 6:
V = 163 842, F = 327 680, N = 1 966 080) and at a tenth of it (the first 32 768 faces of the same mesh with the
vertices they use: N = 196 608).

The torch composition is tests/sugar_mesh_reference.py's restatement (float32, on the GPU, autograd backward).  It
FLATTERS the reference: it builds no pytorch3d ``Meshes`` object, and it evaluates the chain once per step, whereas
the reference's renderer reads ``get_xyz`` three times and ``get_scaling``, ``get_rotation``, ``get_gs_normals`` once
each per view (renderer/diff_sugar_rasterizer_normal.py:101-181), every read redoing its part of the chain.

HIP events on the current stream around windows of ``--iters`` calls, warm-up, the two paths alternated window by
window, medians over ``--runs`` windows.  Per path: ms per forward, ms per forward + backward (random upstream
gradients on all four outputs), peak allocated bytes above the inputs.  For the fused path also the bytes the
mathematics needs (counted below from the shapes) and the fraction of the HBM peak (8 TB/s) that they make of the
measured time: an end-to-end figure of the call (three launches and the allocator included), not a kernel's.
Prints one JSON object (committed as profiles/sugar_mesh.json).
Usage (GPU box): python profiles/diag_sugar_mesh.py [--runs 15] [--iters 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "threestudio-3dgs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsr_synthetic as gs  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from sugar_mesh import MeshBinding, bound_gaussians, initial_log_scales  # noqa: E402
from sugar_mesh_reference import bound_gaussians_reference  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
SIZES = (1, 10)  # C5 and a tenth of it: the first F / 10 faces of icosphere(7)
THICKNESS = 3.5e-6


def math_bytes(V, F, G):
    """The bytes the mathematics reads and writes: each input and output once, the workspace once each way."""
    N = F * G
    fwd = 12 * V + 12 * F + 16 * N + 52 * N  # verts, faces, complex + log_scales; the four outputs
    bwd = (12 * V + 12 * F + 16 * N + 52 * N  # the inputs again and the four upstream gradients
           + 16 * N + 2 * 36 * F  # dL/dcomplex + dL/dlog_scales; the corner rows written and read
           + 12 * F + 4 * (V + 1) + 12 * V)  # the incidence; dL/dverts
    return fwd, fwd + bwd


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def paths(sc):
    ups = sc["ups"]

    def run(make, backward):
        leaves = [sc[k].detach().requires_grad_() for k in ("verts", "cplx", "log_scales")]
        out = make(*leaves)
        if not backward:
            return out
        return torch.autograd.grad(out, leaves, ups)

    def fused(backward=True):
        return run(lambda v, c, s: bound_gaussians(v, c, s, sc["binding"], THICKNESS), backward)

    def torch_composition(backward=True):
        return run(lambda v, c, s: bound_gaussians_reference(v, sc["faces64"], sc["bary"], c, s, THICKNESS)[:4],
                   backward)

    return {"fused": fused, "torch": torch_composition}


def make_scene(mesh, part, G=6, seed=0):
    v, f = mesh
    dev = "cuda"
    used, faces = torch.unique(torch.tensor(f[:len(f) // part]), return_inverse=True)  # the vertices these faces use
    verts = torch.tensor(v, dtype=torch.float32)[used].to(dev)
    faces = faces.to(dev)
    binding = MeshBinding.from_reference_count(faces, len(verts), G)
    gen = torch.Generator(device=dev).manual_seed(seed)
    N = binding.n_gaussians
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    return dict(verts=verts, faces64=faces, binding=binding, bary=binding.bary.to(dev), cplx=rnd(N, 2),
                log_scales=initial_log_scales(verts, binding) + 0.3 * rnd(N, 2),
                ups=(rnd(N, 3), rnd(N, 3), rnd(N, 4), rnd(N, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters, "G": 6,
           "torch_composition": "fp32 restatement of the formulas, evaluated once per step, no Meshes object and no "
                                "repeated property reads: it flatters the reference",
           "sizes": {}}
    mesh = gs.icosphere(7)
    for part in SIZES:
        sc = make_scene(mesh, part)
        b = sc["binding"]
        fns = paths(sc)
        ms = {name: {"step": [], "forward": []} for name in fns}
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():  # alternated: both paths see the same clocks and cache state drift
                step = timed(fn, args.iters)
                fwd = timed(lambda: fn(backward=False), args.iters)
                if it >= args.warmup:
                    ms[name]["step"].append(step)
                    ms[name]["forward"].append(fwd)
        row = {"V": b.n_verts, "F": b.n_faces, "N": b.n_gaussians}
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
        fb, sb = math_bytes(b.n_verts, b.n_faces, b.n_per_face)
        row["fused"].update(forward_math_bytes=fb, step_math_bytes=sb,
                            forward_fraction_of_hbm_peak=round(fb / (row["fused"]["forward_ms"] * 1e-3) / HBM_PEAK, 4),
                            step_fraction_of_hbm_peak=round(sb / (row["fused"]["step_ms"] * 1e-3) / HBM_PEAK, 4))
        row["torch_over_fused_step"] = round(row["torch"]["step_ms"] / row["fused"]["step_ms"], 2)
        row["torch_over_fused_forward"] = round(row["torch"]["forward_ms"] / row["fused"]["forward_ms"], 2)
        a, t = fns["fused"](), fns["torch"]()
        row["max_abs_dverts_diff"] = float((a[0] - t[0]).abs().max())
        row["max_abs_dverts"] = float(t[0].abs().max())
        res["sizes"][str(b.n_gaussians)] = row
        del sc, fns, a, t
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
