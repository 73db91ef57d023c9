"""Generate tests/golden/reference_spline.npz: the reference's own ``Spline`` (geometry/spline_utils.py:151-370, with
``SplineConfig`` and ``_EPS``), lifted from the source text with ``ast`` as tests/golden/make_golden.py lifts the other
SuGaR stages, run on the CPU in float32 (``*_f32``) and float64 (``*_f64``) with autograd gradients to the knots for
stored upstream gradients (tests/test_sugar_spline.py, tests/test_gpu_sugar_spline.py).  Only inputs and outputs are
written; no reference source is stored.

pypose is tests/golden/standins.py plus the three functions the spline alone calls, defined here from pypose's
documented conventions: ``bvv`` (the outer product of the last dimensions), ``Exp`` (of an so3) and
``cumprod(..., left=False)`` (y_i = x_1 (x) ... (x) x_i); einops' ``rearrange`` is the library's, or for the one pattern
the spline uses a reshape and a permute; ``assert_never`` and the jaxtyping names are placeholders.

What is run, per degree (1 and 3): P = 5 points, 7 knots 0.3 apart from -0.3, T = 6 timestamps (one below and one above
the valid range, one on an interior knot time, two in one segment), with and without the scale attribute.  The grid is
given as 0-dim float32 tensors, as ``init_cubic_spliner`` gives it, so the segment choice runs in float32 in both runs;
in the float64 run the knots are float64 and the position ``u`` in the segment, which ``Spline.forward`` has computed in
float32, is cast to float64 where it enters ``Spline.interpolation`` (a two-line subclass; torch.lerp does not mix
dtypes).  The float32 bounds of each grid, and of ``init_cubic_spliner``'s grid for 14 and 32 frames, are stored as
(start_time, sampling_interval, end_time, t_lower_bound, t_upper_bound, t_lower_bound + _EPS, t_upper_bound - _EPS).

Usage:  python tests/golden/make_golden_spline.py [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Tuple, Type

import numpy as np
import torch

import standins
from make_golden import DTYPES, HERE, TYPING, _grads, _unit_quats, default_dtype, lift


def _plain(x):
    return x.tensor() if isinstance(x, standins.LieTensor) else x


def bvv(lvec, rvec):
    """(..., n), (..., m) -> (..., n, m): the outer product of the last dimensions, a plain tensor."""
    return _plain(lvec).unsqueeze(-1) @ _plain(rvec).unsqueeze(-2)


def Exp(x):
    return x.Exp()


def cumprod(x, dim, left=True):
    """Along dim: y_i = x_i (x) y_i-1 (left) or y_i-1 (x) x_i (left=False), y_1 = x_1."""
    parts = [p.as_subclass(standins.SO3Tensor) for p in _plain(x).unbind(dim)]
    out = [parts[0]]
    for p in parts[1:]:
        out.append(p * out[-1] if left else out[-1] * p)
    return torch.stack([_plain(o) for o in out], dim).as_subclass(standins.SO3Tensor)


def _rearrange(x, pattern, **sizes):
    try:
        from einops import rearrange
    except ImportError:
        assert pattern == "N (B K) F -> B N K F", pattern
        n, bk, f = x.shape
        return x.reshape(n, sizes["B"], sizes["K"], f).permute(1, 0, 2, 3)
    return rearrange(x, pattern, **sizes)


def _assert_never(x):
    raise AssertionError(f"unexpected value {x!r}")


def _lift_spline(ref):
    pp = SimpleNamespace(**{k: getattr(standins, k) for k in dir(standins) if not k.startswith("_")},
                         bvv=bvv, Exp=Exp, cumprod=cumprod)
    g = {"torch": torch, "pp": pp, "nn": torch.nn, "dataclass": dataclass, "field": field, "Type": Type, "Tuple": Tuple,
         "rearrange": _rearrange, "assert_never": _assert_never, **TYPING, "LieTensor": standins.LieTensor}
    ns = lift(os.path.join(ref, "geometry/spline_utils.py"), ["_EPS", "SplineConfig", "Spline"], g)

    class Spline(ns["Spline"]):
        def interpolation(self, segment, u, name):  # u: float32 from forward; the knots' dtype from here on
            return super().interpolation(segment, u.to(segment.dtype), name)

    return pp, Spline, ns["SplineConfig"], ns["_EPS"]


def _bounds(spline, eps):
    cfg = spline.config
    return torch.stack([torch.as_tensor(x, dtype=torch.float32) for x in (
        spline.start_time, cfg.sampling_interval, spline.end_time, spline.t_lower_bound, spline.t_upper_bound,
        spline.t_lower_bound + eps, spline.t_upper_bound - eps)]).numpy()


def make_spline_reference(ref: str):
    pp, Spline, SplineConfig, eps = _lift_spline(ref)
    rng = np.random.default_rng(97)
    P, n_knots, T = 5, 7, 6
    out = {}
    for n in (14, 32):  # init_cubic_spliner (geometry/dynamic_sugar.py:349-360), without its .cuda()
        t_interv = torch.as_tensor(1 / (n - 3))
        assert t_interv.dtype == torch.float32
        spline = Spline(SplineConfig(degree=3, sampling_interval=t_interv, start_time=-t_interv, n_knots=n))
        out[f"frames{n}_grid"] = _bounds(spline, eps)
    interval = torch.tensor(0.3, dtype=torch.float32)
    timestamps = np.array([-0.5, 0.35, 0.5, 0.6, 0.95, 2.0], np.float32)
    knots_xyz = rng.normal(size=(n_knots, P, 3)).astype(np.float32)
    knots_rot = _unit_quats(rng, (n_knots, P), 1.2)  # float64; adjacent knots are at most 2.4 rad apart
    knots_scale = (0.1 * rng.normal(size=(n_knots, P, 3))).astype(np.float32)
    ups = {"xyz": rng.normal(size=(T, P, 3)), "rotation": rng.normal(size=(T, P, 4)),
           "scale": rng.normal(size=(T, P, 3))}
    out.update(timestamps=timestamps, knots_xyz=knots_xyz, knots_rot=knots_rot, knots_scale=knots_scale)
    out.update({f"up_{k}": u for k, u in ups.items()})
    for degree in (1, 3):
        for tag, dt in DTYPES:
            res = {}
            for d_scale in (True, False):
                leaves = {k: torch.tensor(a).to(dt).requires_grad_() for k, a in
                          (("knots_xyz", knots_xyz), ("knots_rot", knots_rot), ("knots_scale", knots_scale))}
                spline = Spline(SplineConfig(degree=degree, sampling_interval=interval, start_time=-interval,
                                             n_knots=n_knots))
                # _compute_control_knots_dg (geometry/dynamic_sugar.py:382-392): point-major, the rotations as SO3
                spline.set_data("xyz", leaves["knots_xyz"].permute(1, 0, 2))
                spline.set_data("rotation", pp.SO3(leaves["knots_rot"].permute(1, 0, 2)))
                if d_scale:
                    spline.set_data("scale", leaves["knots_scale"].permute(1, 0, 2))
                with default_dtype(dt):
                    outs = spline(torch.tensor(timestamps))
                assert set(outs) == {"xyz", "rotation"} | ({"scale"} if d_scale else set())
                outs = {k: o.as_subclass(torch.Tensor) for k, o in outs.items()}
                assert all(o.dtype == dt and o.shape[:2] == (T, P) for o in outs.values())
                res[d_scale] = {k: o.detach().numpy() for k, o in outs.items()}
                res[d_scale].update(_grads(outs, {k: ups[k] for k in outs}, leaves))
                out[f"deg{degree}_grid"] = _bounds(spline, eps)
            for k in res[False]:  # the scale attribute only adds its output and its gradient
                if k != "dknots_scale":
                    assert np.array_equal(res[False][k], res[True][k]), (degree, tag, k)
            assert not res[False]["dknots_scale"].any()
            out.update({f"deg{degree}_{k}_{tag}": a for k, a in res[True].items()})
    np.savez_compressed(os.path.join(HERE, "reference_spline.npz"), **out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    make_spline_reference(ap.parse_args().reference)
    print("reference_spline.npz written to", HERE)
