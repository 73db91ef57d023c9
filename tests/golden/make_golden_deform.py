"""Generate tests/golden/reference_deform.npz: the reference's own ``DeformationNetwork`` (geometry/deformation.py, the
whole network, lifted from the source text with ``ast`` as tests/golden/make_golden_spline.py lifts the spline) through
``_get_timed_dg_attributes_wo_spline`` and ``_get_timed_vertex_attributes_wo_spline`` of geometry/dynamic_sugar.py
(lifted as plain functions), run on the CPU in float32 (``*_f32``) and float64 (``*_f64``) with autograd gradients to
every trained tensor for stored upstream gradients (tests/test_sugar_deform.py, tests/test_gpu_sugar_deform.py).  Only
inputs, weights, outputs, upstream gradients and parameter gradients are written; no reference source is stored.

No stand-ins: geometry/deformation.py imports only torch.  ``pp.SO3`` of the two epilogues is the identity here (it only
tags the tensor).  The float64 run uses a subclass of ``Deformation`` whose ``query_time`` returns a tensor whose
``.float()`` is a no-op, which drops the cast of ``forward_dynamic_delta``; the built network's ``deformation_net`` is
given that class.

What is run: ``resolution = [4, 5, 6, 3]``, ``multires = [1, 2]`` on the args object, the heads and every bias
randomised (the reference zeroes the heads), P = 7 points of which two lie outside the box (one on each side), one sits
exactly on a texel coordinate (y = 0.5 on the first level; ticks 0 and 1 are texels too) and one at the upper edge, T = 5 ticks; the graph-node epilogue
(normalised rotation) with and without ``d_scale``, and the vertex epilogue with ``d_scale``.  Stored in float32: the
inputs and weights (they are float32 values) and the float32 run; in float64: the float64 run.  To keep the file below
the largest fixture (501 360 bytes), only the first case stores every gradient in both dtypes; the other two store
their outputs and the gradients of the tensors of at most 500 elements (two planes of the first level, every bias and
the final layers), which is where they differ in kind from the first.

Usage:  python tests/golden/make_golden_deform.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import itertools
import os
from types import SimpleNamespace
from typing import Collection, Iterable, Optional, Sequence

import numpy as np
import torch

from make_golden import DTYPES, HERE, TYPING, lift, lift_method

NAMES = ["normalize_aabb", "grid_sample_wrapper", "init_grid_param", "interpolate_ms_features", "HexPlaneField",
         "Linear_Res", "Head_Res_Net", "Deformation", "DeformationNetwork", "initialize_weights"]


SMALL = 500  # the two further cases store the gradients of the tensors of at most this many elements


class _Hidden(torch.Tensor):
    def float(self):
        return self


def _lift(ref, double):
    g = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "init": torch.nn.init, "itertools": itertools,
         "np": np, "Optional": Optional, "Sequence": Sequence, "Iterable": Iterable, "Collection": Collection}
    ns = lift(os.path.join(ref, "geometry/deformation.py"), NAMES, g)

    class Deformation64(ns["Deformation"]):
        def query_time(self, *a):
            return super().query_time(*a).as_subclass(_Hidden)

    def build(args):
        with contextlib.redirect_stdout(io.StringIO()):  # (the reference prints its feature width)
            net = ns["DeformationNetwork"](args)
        if double:
            net.deformation_net.__class__ = Deformation64
        return net

    return build


def _args():
    return SimpleNamespace(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2,
                           opacity_pe=2, timenet_width=64, timenet_output=32, bounds=1.0,
                           kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                                           "resolution": [4, 5, 6, 3]},
                           multires=[1, 2], no_grid=False, no_ds=False, no_dr=False, no_do=True, use_res=True)


def make_deform_reference(ref: str):
    path = os.path.join(ref, "geometry/dynamic_sugar.py")
    pp = SimpleNamespace(SO3=lambda x: x)
    epilogues = {name: lift_method(path, "DynamicSuGaRModel", method, {"torch": torch, "pp": pp})
                 for name, method in (("dg", "_get_timed_dg_attributes_wo_spline"),
                                      ("vert", "_get_timed_vertex_attributes_wo_spline"))}
    torch.manual_seed(20)
    rng = np.random.default_rng(20)
    net = _lift(ref, False)(_args())
    with torch.no_grad():
        for name, prm in net.named_parameters():  # the heads are zero and most biases default: randomise them
            if "grid" not in name and ("deform" in name or name.endswith("bias")):
                prm.copy_(torch.tensor(rng.normal(0, 0.3, size=tuple(prm.shape)), dtype=torch.float32))
            if "grid" in name and "aabb" not in name:  # the time planes are all 1: randomise every plane
                prm.copy_(torch.tensor(rng.uniform(0.1, 1.5, size=tuple(prm.shape)), dtype=torch.float32))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    T, P = 5, 7
    points = rng.uniform(-0.9, 0.9, size=(P, 3)).astype(np.float32)
    points[0] = [1.3, -1.2, 1.1]      # beyond the box on both sides
    points[1] = [-1.25, 1.4, -1.05]
    points[2] = [-1.0 / 3.0, 0.5, -0.2]  # y: n = -0.5, exactly texel 1 of the first level's 5 (x, z: within 1e-7)
    points[3] = [-1.0, -1.0, -1.0]    # n = +1: the upper edge of every axis
    ticks = np.array([-0.1, 0.0, 0.45, 1.0, 1.2], np.float32)
    ups = {"xyz": rng.normal(size=(T, P, 3)), "rotation": rng.normal(size=(T, P, 4)), "scale": rng.normal(size=(T, P, 3))}
    trained = [k for k in sd if k.startswith("deformation_net.") and "opacity" not in k and "aabb" not in k]
    out = {"points": points, "ticks": ticks, "aabb": sd["deformation_net.grid.aabb"].numpy(),
           "names": np.array(trained), "all_names": np.array(list(sd))}
    out.update({"w_" + k: sd[k].numpy() for k in trained})
    out.update({"up_" + k: u for k, u in ups.items()})
    for tag, dt in DTYPES:
        model = _lift(ref, dt == torch.float64)(_args())
        model.load_state_dict(sd)
        model = model.to(dt)
        prm = dict(model.named_parameters())
        for case, epi, d_scale in (("dg", "dg", True), ("dg_noscale", "dg", False), ("vert", "vert", True)):
            me = SimpleNamespace(dynamic_mode="deformation", _deformation=model, cfg=SimpleNamespace(d_scale=d_scale),
                                 _deform_graph_node_xyz=torch.tensor(points).to(dt), _points=torch.tensor(points).to(dt))
            model.deformation_net.args.no_ds = not d_scale
            attrs = epilogues[epi](me, torch.tensor(ticks).to(dt))
            model.deformation_net.args.no_ds = False
            outs = {k: attrs[k].as_subclass(torch.Tensor) for k in ("xyz", "rotation", "scale") if attrs[k] is not None}
            assert set(outs) == {"xyz", "rotation"} | ({"scale"} if d_scale else set())
            assert all(o.dtype == dt and o.shape[:2] == (T, P) for o in outs.values())
            loss = sum((o * torch.tensor(ups[k]).to(dt)).sum() for k, o in outs.items())
            grads = torch.autograd.grad(loss, [prm[k] for k in trained], allow_unused=True)
            out.update({f"{case}_{k}_{tag}": o.detach().numpy() for k, o in outs.items()})
            for k, g in zip(trained, grads):
                assert (g is None) == ("scales_deform" in k and not d_scale), k
                if g is not None and (case == "dg" or g.numel() <= SMALL):
                    out[f"{case}_d_{k}_{tag}"] = g.as_subclass(torch.Tensor).numpy()
    np.savez_compressed(os.path.join(HERE, "reference_deform.npz"), **out)
    return os.path.getsize(os.path.join(HERE, "reference_deform.npz"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    size = make_deform_reference(ap.parse_args().reference)
    print("reference_deform.npz written to", HERE, size, "bytes")
