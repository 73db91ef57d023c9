"""A torch restatement of the B-spline of the timed node attributes (include/gsr.h gsr_sugar_spline_*), differentiated
by autograd: the checker of tests/test_sugar_spline.py and tests/test_gpu_sugar_spline.py.  It follows the formulas of
the header literally, in the dtype of its knots (float64: the reference; float32: the "fp32 null" the GPU bars are
calibrated on, i.e. what the torch composition the kernels replace would give).  The segment of a timestamp and its
position u are a discrete decision and are always taken in float32, as Spline.forward of geometry/spline_utils.py
takes them, with 0-dim float32 tensors for the grid (a tensor divided by a tensor is a correctly rounded divide on every
device), and then cast.  Quaternions are (x, y, z, w); Log, Exp and the Hamilton product are those of
tests/sugar_dynamic_reference.py."""
import torch

from sugar_dynamic_reference import _evaluate, qconj, qexp, qlog, qmul

SPLINE_INPUTS = ("knots_xyz", "knots_rot", "knots_scale")
SPLINE_OUTPUTS = ("xyz", "rot", "scale")


def segments(grid, timestamps, clamp_index=True):
    """``(first (T,) int64, u (T,) float32)``: the first knot of each timestamp's segment, clamped to
    [0, n_knots - degree - 1] as the kernels clamp it (clamp_index=False: as the reference leaves it), and the position
    in the segment.  grid: anything with degree, n_knots, start_time, sampling_interval, clamp_lo and clamp_hi (float32
    numbers)."""
    t = timestamps.to(torch.float32)
    as_t = lambda x: torch.tensor(float(x), dtype=torch.float32, device=t.device)
    ts = torch.clamp(t, as_t(grid.clamp_lo), as_t(grid.clamp_hi))
    nt = (ts - as_t(grid.start_time)) / as_t(grid.sampling_interval)
    first = torch.floor(nt).int()
    u = nt - first
    if grid.degree == 3:
        first = first - 1
    first = first.long()
    return (first.clamp(0, grid.n_knots - grid.degree - 1) if clamp_index else first), u


def spline_reference(timestamps, knots_xyz, knots_rot, grid, knots_scale=None):
    """(xyz (T, P, 3), rot (T, P, 4) xyzw, scale (T, P, 3) or None); the knots are (n_knots, P, C), frame-major."""
    dt = knots_xyz.dtype
    first, u = segments(grid, timestamps)
    u = u.to(dt)[:, None, None]  # (T, 1, 1)
    D = grid.degree
    seg = lambda knots: [knots[first + j] for j in range(D + 1)]  # D + 1 tensors (T, P, C)
    if D == 3:
        uu, uuu, s = u * u, u * u * u, 1.0 / 6.0
        c = (s - 0.5 * u + 0.5 * uu - s * uuu, 4.0 * s - uu + 0.5 * uuu, s + 0.5 * u + 0.5 * uu - 0.5 * uuu, s * uuu)
        b = (5.0 * s + 0.5 * u - 0.5 * uu + s * uuu, s + 0.5 * u + 0.5 * uu - 2.0 * s * uuu, s * uuu)
        mix = lambda k: c[0] * k[0] + c[1] * k[1] + c[2] * k[2] + c[3] * k[3]
        q = seg(knots_rot)
        rot = q[0]
        for j in range(3):
            rot = qmul(rot, qexp(b[j] * qlog(qmul(qconj(q[j]), q[j + 1]))))
    else:
        mix = lambda k: k[0] + u * (k[1] - k[0])
        q = seg(knots_rot)
        l0, l1 = qlog(q[0]), qlog(q[1])
        rot = qexp(l0 + u * (l1 - l0))
    xyz = mix(seg(knots_xyz))
    scale = None if knots_scale is None else mix(seg(knots_scale))
    return xyz, rot, scale


def evaluate(dtype, inputs, grid, timestamps, ups):
    """Outputs (by SPLINE_OUTPUTS) and gradients ("d" + name of SPLINE_INPUTS) of the restatement in `dtype`.  inputs:
    a dict over SPLINE_INPUTS (knots_scale may be None); ups: the upstream gradients by output name (absent = zero)."""
    return _evaluate(lambda x: spline_reference(timestamps, x["knots_xyz"], x["knots_rot"], grid, x["knots_scale"]),
                     SPLINE_INPUTS, SPLINE_OUTPUTS, dtype, inputs, ups)


# ---- the reference's own Spline: tests/golden/reference_spline.npz, read by sugar_cases.fixture("spline") ----------
SPLINE_KEYS = ("xyz", "rotation", "scale", "dknots_xyz", "dknots_rot", "dknots_scale")


def fixture_grid(z, degree):
    from sugar_spline import SplineGrid

    g = z[f"deg{degree}_grid"]
    return SplineGrid(degree, g[1].item(), g[0].item(), int(z["knots_xyz"].shape[0]))
