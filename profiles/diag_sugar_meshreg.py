"""Diagnostic: the fused mesh regularisers (sugar_meshreg.normal_consistency / laplacian_smoothing,
csrc/gsr_meshreg.hip) against the fp32 torch restatement of pytorch3d's mesh_normal_consistency and
mesh_laplacian_smoothing(., "uniform") on the same GPU, at the shipped size (icosphere(7): V = 163 842, F = 327 680,
E = P = 491 520) with T = 8 frames (the dynamic stage) and T = 1 (the static stage).

Paths, per loss ("nc", "lap"):
  fused      the HIP call on the prebuilt MeshTopology.
  torch      tests/sugar_meshreg_reference.py's restatement (float32, on the GPU, autograd backward) FED THE PREBUILT
             edges and pairs.  It FLATTERS the reference: pytorch3d builds a fresh Meshes every step and derives the
             unique edges (a sort over 3 F edges per frame), the face pairs and the sparse Laplacian again.
  torch+edges  (nc and lap together, once per size) the same restatement after deriving the unique edges of the T
             meshes again by torch.unique over the 3 F T sorted edges, as Meshes.edges_packed() does: a lower bound of
             the reference's real per-step cost (the face-pair enumeration is still fed).
The baseline is the restatement, never the code under test.

HIP events on the current stream around windows of ``--iters`` calls, warm-up, the paths alternated window by window,
medians over ``--runs`` windows.  Per path: ms per forward, ms per forward + backward (random upstream weights per
frame), peak allocated bytes above the inputs.  For the fused path also the bytes the mathematics needs (each input,
output and workspace array once per kernel that touches it; gathered rows once, as if cached) and the fraction of the
HBM peak (8 TB/s) that they make of the measured time: an end-to-end figure of the call (its launches and the
allocator included), not of a single kernel.
Prints one JSON object (committed as profiles/sugar_meshreg.json).
Usage (GPU box): python profiles/diag_sugar_meshreg.py [--runs 9] [--iters 5] [--out FILE]"""
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
from sugar_meshreg import MeshTopology, laplacian_smoothing, normal_consistency  # noqa: E402
from sugar_meshreg_reference import laplacian_reference, normal_consistency_reference  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
FRAMES = (8, 1)


def math_bytes(loss, T, V, E, P):
    """(forward, forward + backward) bytes of one fused loss."""
    x = 12 * T * V
    if loss == "nc":
        blocks = -(-P // 256)
        fwd = 16 * P + x + 8 * T * blocks + (8 * T * blocks + 4 * T)  # k_nc_forward; k_meshreg_reduce
        rows = 96 * T * P
        bwd = (16 * P + x + 4 * T + rows) + (4 * (V + 1) + 16 * P + rows + 4 * T + x)  # corner rows; gather
    else:
        blocks = -(-V // 256)
        csr = 4 * (V + 1) + 8 * E
        fwd = csr + x + 8 * T * blocks + (8 * T * blocks + 4 * T)
        bwd = (csr + x + 4 * T + 24 * T * V) + (csr + 24 * T * V + 4 * T + x)  # k_lap_rows; k_lap_gather
    return fwd, fwd + bwd


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def derived_edges(faces, V, T):
    """The unique edges of T packed copies of the mesh, as Meshes.edges_packed() derives them; returns one mesh's."""
    f = (faces[None] + V * torch.arange(T, device=faces.device)[:, None, None]).reshape(-1, 3)
    e = torch.cat([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]])
    lo, hi = e.min(1)[0], e.max(1)[0]
    u = torch.unique(lo * (V * T + 1) + hi)
    edges = torch.stack([u // (V * T + 1), u % (V * T + 1)], 1)
    return edges[:len(edges) // T]


def measure(fns, args):
    ms = {name: {"step": [], "forward": []} for name in fns}
    for name, fn in fns.items():  # one synchronised call each first: a failure names its path
        fn()
        torch.cuda.synchronize()
        print(f"{name}: ran", file=sys.stderr, flush=True)
    for it in range(args.warmup + args.runs):
        for name, fn in fns.items():  # alternated: the paths see the same clocks and cache state drift
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
                   "step_min_ms": round(min(ms[name]["step"]), 4), "step_max_ms": round(max(ms[name]["step"]), 4),
                   "forward_ms": round(statistics.median(ms[name]["forward"]), 4),
                   "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--subdiv", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda"
    res = {"library": _C.load_library().gsr_version().decode(), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "iters_per_window": args.iters,
           "torch_composition": "fp32 restatement of pytorch3d's two losses (gathers, cross, cosine_similarity; "
                                "index_add, norm) FED the prebuilt edges and pairs: it does not pay the per-step "
                                "derivation of Meshes, so it flatters the reference; torch+edges adds only the "
                                "unique-edge derivation (torch.unique over 3 F T edges)",
           "frames": {}}
    v, f = gs.icosphere(args.subdiv)
    verts, faces = torch.tensor(v, dtype=torch.float32, device=dev), torch.tensor(f, device=dev)
    topo = MeshTopology(faces, len(verts))
    V, E, P = topo.n_verts, topo.n_edges, topo.n_pairs
    edges, pairs = topo.edges.long(), topo.pairs.long()
    edge = float((verts[edges[:, 0]] - verts[edges[:, 1]]).norm(dim=-1).mean())
    res["mesh"] = {"V": V, "F": topo.n_faces, "E": E, "P": P, "max_valence": topo.max_valence,
                   "max_slots": topo.max_slots}
    for T in FRAMES:
        gen = torch.Generator(device=dev).manual_seed(T)
        xyz = verts[None] + 0.1 * edge * torch.randn(T, V, 3, generator=gen, device=dev)
        up = torch.randn(T, generator=gen, device=dev)

        def run(make, backward):
            x = xyz.detach().requires_grad_()
            out = make(x)
            return torch.autograd.grad(out, [x], up)[0] if backward else out

        row = {}
        losses = {"nc": (lambda x: normal_consistency(x, topo), lambda x: normal_consistency_reference(x, pairs)),
                  "lap": (lambda x: laplacian_smoothing(x, topo), lambda x: laplacian_reference(x, edges))}
        for loss, (fused, restated) in losses.items():
            fns = {"fused": lambda backward=True, m=fused: run(m, backward),
                   "torch": lambda backward=True, m=restated: run(m, backward)}
            r = measure(fns, args)
            fb, stb = math_bytes(loss, T, V, E, P)
            r["fused"].update(
                forward_math_bytes=fb, step_math_bytes=stb,
                forward_fraction_of_hbm_peak=round(fb / (r["fused"]["forward_ms"] * 1e-3) / HBM_PEAK, 4),
                step_fraction_of_hbm_peak=round(stb / (r["fused"]["step_ms"] * 1e-3) / HBM_PEAK, 4))
            r["torch_over_fused_step"] = round(r["torch"]["step_ms"] / r["fused"]["step_ms"], 2)
            r["torch_over_fused_forward"] = round(r["torch"]["forward_ms"] / r["fused"]["forward_ms"], 2)
            a, t = fns["fused"](), fns["torch"]()
            r["max_abs_grad_diff"], r["max_abs_grad"] = float((a - t).abs().max()), float(t.abs().max())
            r["value_fused"], r["value_torch"] = fused(xyz).tolist(), restated(xyz).tolist()
            row[loss] = r
            del a, t
            torch.cuda.empty_cache()
        both = {"fused": lambda backward=True: run(
                    lambda x: normal_consistency(x, topo) + laplacian_smoothing(x, topo), backward),
                "torch": lambda backward=True: run(
                    lambda x: normal_consistency_reference(x, pairs) + laplacian_reference(x, edges), backward),
                "torch+edges": lambda backward=True: run(
                    lambda x: normal_consistency_reference(x, pairs)
                    + laplacian_reference(x, derived_edges(faces, V, T)), backward)}
        assert torch.equal(derived_edges(faces, V, T), edges)
        r = measure(both, args)
        for name in ("torch", "torch+edges"):
            r[f"{name}_over_fused_step"] = round(r[name]["step_ms"] / r["fused"]["step_ms"], 2)
        row["nc+lap"] = r
        res["frames"][str(T)] = row
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
