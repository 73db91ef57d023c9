"""Diagnostic: the fused dynamic-SuGaR geometry (sugar_dynamic.skin_vertices and timed_gaussians,
csrc/gsr_dynamic.hip) against the fp32 torch composition of the same formulas on the same GPU, at the shipped size
(T = 8 frames, icosphere(7): V = 163 842, F = 327 680, G = 6, N = 1 966 080; P = 1000 nodes, K = 16) and at a tenth of
it (the first F / 10 faces of the same mesh with the vertices they use, P = 100), with "dqs" and "lbs" skinning and
with the scale inputs.

The torch composition is tests/sugar_dynamic_reference.py's restatement (float32, on the GPU, autograd backward).  It
FLATTERS the reference: no pypose LieTensor and no pytorch3d ``Meshes`` object, and one evaluation for all frames of
the batch, whereas the reference's temporal renderer redoes the whole chain once per view
(``get_timed_gs_all_single_time``).

HIP events on the current stream around windows of ``--iters`` calls, warm-up, the two paths alternated window by
window, medians over ``--runs`` windows.  Per op and path: ms per forward, ms per forward + backward (random upstream
gradients on every output), peak allocated bytes above the inputs.  For the fused path also the bytes the mathematics
needs (each input, output and workspace array once per kernel that touches it, counted below from the shapes) and the
fraction of the HBM peak (8 TB/s) that they make of the measured time: an end-to-end figure of the call (its launches
and the allocator included), not of a single kernel.
Prints one JSON object (committed as profiles/sugar_dynamic.json).
Usage (GPU box): python profiles/diag_sugar_dynamic.py [--runs 9] [--iters 5] [--out FILE]"""
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
from sugar_dynamic import SkinBinding, skin_vertices, timed_gaussians  # noqa: E402
from sugar_dynamic_reference import skin_vertices_reference, timed_gaussians_reference  # noqa: E402
from sugar_mesh import MeshBinding  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
SIZES = (1, 10)
T, K, G, NODES = 8, 16, 6, 1000
THICKNESS = 3.5e-6


def skin_bytes(V, P):
    """(forward, forward + backward) bytes of skin_vertices with node_scales."""
    nodes_in, rec, out = 40 * T * P, 88 * T * P, 40 * T * V
    fwd = nodes_in + rec + (rec + 12 * V + 8 * V * K + out)  # k_skin_nodes; k_skin_forward
    bwd = (nodes_in + rec  # k_skin_nodes
           + rec + 12 * V + 8 * V * K + 28 * T * V + 56 * T * V  # k_skin_vertex: the upstream xyz, rot; rows and terms
           + 12 * T * V + 12 * V  # k_skin_verts_sum
           + 8 * V * K + 4 * P + 56 * T * V + 12 * T * V + rec + 40 * T * P)  # k_skin_node (each row counted once)
    return fwd, fwd + bwd


def timed_bytes(V, F):
    """(forward, forward + backward) bytes of timed_gaussians with the scale inputs."""
    N = F * G
    vin, gin, out = 40 * T * V, 24 * N, 52 * T * N
    fwd = vin + 12 * F + gin + out
    bwd = (vin + 12 * F + gin + out + 120 * T * F  # k_timed_face: the inputs, the upstream gradients, the rows
           + 120 * T * F + 12 * F + 4 * V + 40 * T * V  # k_timed_vertex
           + vin + 12 * F + gin + 28 * T * N + 24 * N)  # k_timed_gauss: upstream rotation and scaling again
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
    faces = faces.to(dev)
    mb = MeshBinding.from_reference_count(faces, len(verts), G)
    gen = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    V, N, P = len(verts), mb.n_gaussians, NODES // part
    node_xyz = verts[torch.randperm(V, generator=gen, device=dev)[:P]].clone()
    sb = SkinBinding.from_euclidean(verts, node_xyz, K)
    rots = rnd(T, P, 4) * 0.2
    rots[..., 3] += 1.0
    vrot = rnd(T, V, 4) * 0.2
    vrot[..., 3] += 1.0
    return dict(
        mb=mb, sb=sb, faces64=faces, bary=mb.bary.to(dev), nbr64=sb.nbr.long(), node_xyz=node_xyz,
        skin_in=[verts, 0.05 * rnd(T, P, 3), rots, 0.1 * rnd(T, P, 3)],
        skin_ups=(rnd(T, V, 3), rnd(T, V, 4), rnd(T, V, 3)),
        timed_in=[verts[None] + 0.01 * rnd(T, V, 3), vrot, torch.nn.functional.normalize(rnd(N, 4), dim=-1),
                  0.1 * rnd(T, V, 3), 0.3 * rnd(N, 2) - 6],
        timed_ups=(rnd(T, N, 3), rnd(T, N, 4), rnd(T, N, 3), rnd(T, N, 3)))


def paths(sc):
    def run(make, inputs, ups, backward):
        leaves = [t.detach().requires_grad_() for t in inputs]
        out = make(*leaves)
        return torch.autograd.grad(out, leaves, ups) if backward else out

    fns = {}
    for method in ("dqs", "lbs"):
        fns[f"skin_{method}"] = {
            "fused": lambda backward=True, m=method: run(
                lambda v, t, q, s: skin_vertices(v, sc["node_xyz"], t, q, sc["sb"], m, s), sc["skin_in"],
                sc["skin_ups"], backward),
            "torch": lambda backward=True, m=method: run(
                lambda v, t, q, s: skin_vertices_reference(v, sc["node_xyz"], t, q, sc["nbr64"], sc["sb"].w, m, s),
                sc["skin_in"], sc["skin_ups"], backward)}
    fns["timed"] = {
        "fused": lambda backward=True: run(
            lambda x, r, q, s, ls: timed_gaussians(x, r, q, sc["mb"], s, ls, THICKNESS), sc["timed_in"],
            sc["timed_ups"], backward),
        "torch": lambda backward=True: run(
            lambda x, r, q, s, ls: timed_gaussians_reference(x, r, q, sc["faces64"], sc["bary"], s, ls, THICKNESS),
            sc["timed_in"], sc["timed_ups"], backward)}
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters, "T": T, "K": K, "G": G,
           "torch_composition": "fp32 restatement of the formulas, one evaluation for all frames, no pypose, no "
                                "Meshes object: it flatters the reference",
           "sizes": {}}
    mesh = gs.icosphere(7)
    for part in SIZES:
        sc = make_scene(mesh, part)
        mb, sb = sc["mb"], sc["sb"]
        row = {"V": mb.n_verts, "F": mb.n_faces, "N": mb.n_gaussians, "P": sb.n_nodes}
        for op, fns in paths(sc).items():
            ms = {name: {"step": [], "forward": []} for name in fns}
            for name, fn in fns.items():  # one synchronised call each first: a failure names its path
                fn()
                torch.cuda.synchronize()
                print(f"N = {mb.n_gaussians} {op} {name}: ran", file=sys.stderr, flush=True)
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
            fb, stb = skin_bytes(mb.n_verts, sb.n_nodes) if op.startswith("skin") else timed_bytes(mb.n_verts,
                                                                                                    mb.n_faces)
            r["fused"].update(
                forward_math_bytes=fb, step_math_bytes=stb,
                forward_fraction_of_hbm_peak=round(fb / (r["fused"]["forward_ms"] * 1e-3) / HBM_PEAK, 4),
                step_fraction_of_hbm_peak=round(stb / (r["fused"]["step_ms"] * 1e-3) / HBM_PEAK, 4))
            r["torch_over_fused_step"] = round(r["torch"]["step_ms"] / r["fused"]["step_ms"], 2)
            r["torch_over_fused_forward"] = round(r["torch"]["forward_ms"] / r["fused"]["forward_ms"], 2)
            a, t = fns["fused"](), fns["torch"]()
            r["max_abs_grad_diff"] = [float((x - y).abs().max()) for x, y in zip(a, t)]
            r["max_abs_grad"] = [float(y.abs().max()) for y in t]
            row[op] = r
            del a, t
            torch.cuda.empty_cache()
        res["sizes"][str(mb.n_gaussians)] = row
        del sc
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
