"""Diagnostic: the fused ARAP energy (sugar_arap.arap_energy, csrc/gsr_arap.hip) against the fp32 torch restatement of
the reference's padded per-frame computation on the same GPU, at the shipped size (T = 8 frames, icosphere(7): V =
163 842, E = 983 040 directed one-ring edges) and at a tenth of it (the first F / 10 faces of the same mesh with the
vertices they use), with quaternion and with matrix rotations.

The torch composition is tests/sugar_arap_reference.py's restatement (float32, on the GPU, autograd backward): per
frame a padded (V, max valence, 3) edge matrix by ``index_put``, a ``bmm``, a norm and a weighted sum, in a Python loop
over the frames.  It FLATTERS the reference: its weights and one-rings come from the CSR binding (the reference's coach
forms a dense (V, V) matrix, 107 GB at this V, which does not run), and the quaternion form spells pypose's
``matrix()`` out instead of going through a LieTensor.

HIP events on the current stream around windows of ``--iters`` calls, warm-up, the two paths alternated window by
window, medians over ``--runs`` windows.  Per form and path: ms per forward, ms per forward + backward (random upstream
weights per frame), peak allocated bytes above the inputs.  For the fused path also the bytes the mathematics needs
(each input, output and workspace array once per kernel that touches it; the gathered neighbour rows once, as if
cached) and the fraction of the HBM peak (8 TB/s) that they make of the measured time: an end-to-end figure of the
call (its launches and the allocator included), not of a single kernel.
Prints one JSON object (committed as profiles/sugar_arap.json).
Usage (GPU box): python profiles/diag_sugar_arap.py [--runs 9] [--iters 5] [--out FILE]"""
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
from sugar_arap import ArapBinding, arap_energy  # noqa: E402
from sugar_arap_reference import arap_energy_reference  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
SIZES = (1, 10)
T = 8


def math_bytes(V, E, form):
    """(forward, forward + backward) bytes of arap_energy."""
    rot = 16 if form == "quat" else 36
    csr = 4 * (V + 1) + 8 * E + 12 * V  # offsets, nbr and w, the rest vertices
    blocks = -(-V // 256)
    fwd = csr + T * V * (12 + rot) + 8 * T * blocks + (8 * T * blocks + 4 * T)  # k_arap_forward; k_arap_reduce
    bwd = csr + T * V * (12 + rot) + 4 * T + T * V * (12 + rot)  # k_arap_backward: the inputs, g, the two gradients
    return fwd, fwd + bwd


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def make_scene(mesh, part, seed=0):
    v, f = mesh
    dev = "cuda"
    used, faces = torch.unique(torch.tensor(f[:len(f) // part]), return_inverse=True)
    verts = torch.tensor(v, dtype=torch.float32)[used].to(dev)
    b = ArapBinding(verts, faces.to(dev))
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    V = b.n_verts
    ii = torch.repeat_interleave(torch.arange(V, device=dev), (b.offsets[1:] - b.offsets[:-1]).long())
    nn = torch.arange(b.n_edges, device=dev) - b.offsets.long()[ii]
    quat = rnd(T, V, 4) * 0.2
    quat[..., 3] += 1.0
    edge = float(b.p.norm(dim=-1).mean())
    return dict(b=b, rings=(ii, b.nbr.long(), nn), xyz=verts[None] + 0.1 * edge * rnd(T, V, 3),
                rot={"quat": quat, "matrix": torch.eye(3, device=dev) + 0.1 * rnd(T, V, 3, 3)}, up=rnd(T))


def paths(sc, form):
    b = sc["b"]

    def run(make, backward):
        leaves = [sc["xyz"].detach().requires_grad_(), sc["rot"][form].detach().requires_grad_()]
        out = make(*leaves)
        return torch.autograd.grad(out, leaves, sc["up"]) if backward else out

    return {"fused": lambda backward=True: run(lambda x, r: arap_energy(x, r, b), backward),
            "torch": lambda backward=True: run(lambda x, r: arap_energy_reference(x, r, b.verts, *sc["rings"], b.w),
                                               backward)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters, "T": T,
           "torch_composition": "fp32 restatement of the reference's padded per-frame computation (index_put, bmm, "
                                "norm, weighted sum; a Python loop over the frames) fed from the CSR binding: no "
                                "dense (V, V) weight matrix and no pypose, so it flatters the reference",
           "sizes": {}}
    mesh = gs.icosphere(7)
    for part in SIZES:
        sc = make_scene(mesh, part)
        b = sc["b"]
        row = {"V": b.n_verts, "F": b.n_faces, "E": b.n_edges, "max_valence": b.max_valence}
        for form in ("quat", "matrix"):
            fns = paths(sc, form)
            ms = {name: {"step": [], "forward": []} for name in fns}
            for name, fn in fns.items():  # one synchronised call each first: a failure names its path
                fn()
                torch.cuda.synchronize()
                print(f"V = {b.n_verts} {form} {name}: ran", file=sys.stderr, flush=True)
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
            fb, stb = math_bytes(b.n_verts, b.n_edges, form)
            r["fused"].update(
                forward_math_bytes=fb, step_math_bytes=stb,
                forward_fraction_of_hbm_peak=round(fb / (r["fused"]["forward_ms"] * 1e-3) / HBM_PEAK, 4),
                step_fraction_of_hbm_peak=round(stb / (r["fused"]["step_ms"] * 1e-3) / HBM_PEAK, 4))
            r["torch_over_fused_step"] = round(r["torch"]["step_ms"] / r["fused"]["step_ms"], 2)
            r["torch_over_fused_forward"] = round(r["torch"]["forward_ms"] / r["fused"]["forward_ms"], 2)
            a, t = fns["fused"](), fns["torch"]()
            r["max_abs_grad_diff"] = [float((x - y).abs().max()) for x, y in zip(a, t)]
            r["max_abs_grad"] = [float(y.abs().max()) for y in t]
            row[form] = r
            del a, t
            torch.cuda.empty_cache()
        res["sizes"][str(b.n_verts)] = row
        del sc
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
