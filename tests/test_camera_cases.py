"""CPU census of tests/camera_cases.py (no GPU): every case reaches what its table row says, so that a later
edit of a seed cannot quietly turn a case back into the orbit, and every case is conditioned well enough
for the parity rule of tests/gsr_testutil.py to mean something: `adjudicate` allows the GPU
2 x (the fp32 oracle's misses) + 3 rows beyond the bar, so a scene on which the fp32 oracle itself misses the
fp64 bar widely would pass anything.  The caps here are conditions on the inputs: the fp32 oracle may miss
the fp64 bar on at most 1 % of the pixels (colour, alpha, depth each) and of the rows of each gradient tensor,
and the two fp32 runs may disagree under the row rule (null_beyond) on at most 0.5 % of the rows.

The floors are a handful each, not the measured counts (those are listed in DESIGN.md §Parity).
"""
import numpy as np
import pytest

import camera_cases as cc
import gsr_testutil as tu
from gsr_testutil import gs, run_oracle

MISS_CAP = 0.01
NULL_CAP = 0.005
_CENSUS = {}


def census(name):
    """Counts over the visible Gaussians (fp64 preprocess values) plus the fp32 oracle's own miss shares."""
    if name in _CENSUS:
        return _CENSUS[name]
    scene, cam, bg = cc.get(name)
    W, H = cam["W"], cam["H"]
    grads = gs.upstream_grads(H, W, seed=7)
    ref = run_oracle(scene, cam, bg, grads=grads)
    a = ref["aux64"]
    vis = ref["f64"]["radii"] > 0
    t = cc.view_space(scene["means3D"], cam)
    limx, limy = 1.3 * float(np.float32(cam["tanx"])), 1.3 * float(np.float32(cam["tany"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    z = t[:, 2]
    c = dict(P=int(vis.size), visible=int(vis.sum()),
             guard_x=int((vis & (np.abs(rx) > limx)).sum()), guard_y=int((vis & (np.abs(ry) > limy)).sum()),
             guard_x_neg=int((vis & (rx < -limx)).sum()), guard_x_pos=int((vis & (rx > limx)).sum()),
             off_left=int((vis & (a["px"] < 0)).sum()), off_right=int((vis & (a["px"] >= W)).sum()),
             off_top=int((vis & (a["py"] < 0)).sum()), off_bottom=int((vis & (a["py"] >= H)).sum()),
             near_cull=int((vis & (z > cc.NEAR_CULL) & (z <= 0.21)).sum()),
             below_cull=int(((z > 0.19) & (z <= cc.NEAR_CULL)).sum()),
             big_radius=int((vis & (ref["f64"]["radii"] >= max(W, H))).sum()),
             cut_left=int((vis & (a["px"] - ref["f64"]["radii"] < 0)).sum()),
             cut_top=int((vis & (a["py"] - ref["f64"]["radii"] < 0)).sum()),
             max_tiles=int(a["tiles"].max()), K=int(ref["f32"]["K"]))
    d32 = a["depth"][vis].astype(np.float32)
    c["depth_min"], c["depth_max"] = float(d32.min()), float(d32.max())
    c["depth_key_span"] = int(d32.max().view(np.uint32)) - int(d32.min().view(np.uint32))
    # (pixel, Gaussian) pairs at which the 0.99 clamp binds, and threshold ellipses holding all four corners
    ys, xs = np.mgrid[0:H, 0:W]
    clamp_pairs, full = 0, 0
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    for i in np.nonzero(vis)[0]:
        ca, cb, cq = a["conic"][i]
        o = a["opacity"][i]
        if o > 0.99:
            dx, dy = a["px"][i] - xs, a["py"][i] - ys
            power = -0.5 * (ca * dx * dx + cq * dy * dy) - cb * dx * dy
            clamp_pairs += int(((power <= 0) & (o * np.exp(np.minimum(power, 0)) > 0.99)).sum())
        if o > 1.0 / 255.0:
            dx, dy = a["px"][i] - corners[:, 0], a["py"][i] - corners[:, 1]
            Q = ca * dx * dx + cq * dy * dy + 2 * cb * dx * dy
            full += bool((Q <= 2 * np.log(255.0 * o)).all())
    c["clamp_pairs"], c["full_image"] = clamp_pairs, full
    # tiles holding a pixel with alpha >= 1/255 (what the kernels keep, up to their margins) of the widest ones
    gx = (W + 15) // 16
    kept = []
    for i in np.nonzero(vis & (a["tiles"] >= 1500))[0]:
        ca, cb, cq = a["conic"][i]
        dx, dy = a["px"][i] - xs, a["py"][i] - ys
        hit = ca * dx * dx + cq * dy * dy + 2 * cb * dx * dy <= 2 * np.log(255.0 * a["opacity"][i])
        kept.append(len(np.unique((ys[hit] // 16) * gx + xs[hit] // 16)))
    c["kept_wide"] = sorted(kept)
    # the fp32 oracle against the fp64 bars, as adjudicate counts it (GPU := the fp32 oracle itself)
    miss = {}
    d64 = tu._pixels(ref["f64"]["depth"])
    for key, bar in (("color", tu.RGB_ATOL), ("alpha", tu.RGB_ATOL), ("depth", tu.RGB_ATOL + tu.DEPTH_RTOL * np.abs(d64))):
        p32, p64 = tu._pixels(ref["f32"][key]).astype(np.float64), tu._pixels(ref["f64"][key])
        st = tu.adjudicate(p32, p32, p64, bar, name, key)
        miss[key] = (st["f32_miss"], st["rows"], 0)
    for k in cc.grad_keys(name):
        r64 = ref["b64"][k]
        st = tu.adjudicate(ref["b32"][k], ref["b32"][k], r64, tu.GRAD_TOL * np.maximum(1.0, np.abs(r64)), name,
                           "grad " + k, rowwise=True, r32b=ref["b32r"][k])
        miss["grad " + k] = (st["f32_miss"], st["rows"], st["null_beyond"])
    tu.REPORT.clear()
    c["miss"] = miss
    _CENSUS[name] = c
    return c


@pytest.mark.parametrize("name", list(cc.CASES))
def test_fp32_oracle_stays_under_the_cap(name):
    c = census(name)
    for what, (f32_miss, rows, null) in c["miss"].items():
        assert f32_miss <= MISS_CAP * rows, f"{name}: {what}: the fp32 oracle misses the fp64 bar on {f32_miss} of {rows} rows"
        assert null <= NULL_CAP * rows, f"{name}: {what}: the two fp32 runs disagree on {null} of {rows} rows"


def test_near49_overflows_the_frustum():
    c = census("near49")
    assert c["guard_x"] >= 5 and c["guard_y"] >= 5, c
    assert min(c["off_left"], c["off_right"], c["off_top"], c["off_bottom"]) >= 5, c


def test_tele20_is_the_reference_default():
    c = census("tele20")
    scene, cam, _ = cc.get("tele20")
    assert (cam["W"], cam["H"]) == (176, 120)  # ragged: 120 is no multiple of 16
    assert abs(cam["tanx"] - np.tan(np.radians(10.0))) < 1e-12 and cam["tanx"] == cam["tany"]
    assert 3.0 < c["depth_min"] and c["depth_max"] < 4.6, c  # distance 3.8 -+ the ball's 0.8
    assert c["guard_x"] == 0 and c["guard_y"] == 0, c  # a long lens: the object is well inside the frustum
    assert c["visible"] >= 2000, c


def test_offaxis_binds_one_side_and_cuts_left_and_top():
    c = census("offaxis")
    assert (c["guard_x_neg"] >= 5) != (c["guard_x_pos"] >= 5), c
    assert min(c["guard_x_neg"], c["guard_x_pos"]) == 0, c
    assert c["cut_left"] >= 5 and c["cut_top"] >= 5, c  # getRect truncates (px - r) / 16 < 0 towards zero
    assert c["off_left"] + c["off_right"] >= 5, c


def test_inside_sits_on_the_near_cull():
    c = census("inside")
    assert c["near_cull"] >= 5 and c["below_cull"] >= 5, c
    assert c["big_radius"] >= 5, c
    assert c["depth_key_span"] >= 1 << 24, c  # the depth sort needs its fourth pass
    assert c["clamp_pairs"] >= 300, c


def test_deep_needs_four_sort_passes():
    c = census("deep")
    assert c["depth_key_span"] >= 1 << 24, c
    assert c["depth_min"] < 0.3 and c["depth_max"] > 50.0, c
    scene, cam, bg = cc.deep(moved=False)
    z = cc.view_space(scene["means3D"], cam)[:, 2].astype(np.float32)
    assert scene["means3D"].shape[0] == c["P"] - cc.DEEP_MOVED
    assert int(z.max().view(np.uint32)) - int(z.min().view(np.uint32)) < (1 << 24) - 1  # three passes without them


def test_wide_field_overflows_the_kept_tile_field():
    c = census("wide_field")
    scene, cam, _ = cc.get("wide_field")
    P = scene["means3D"].shape[0]
    tiles = ((cam["W"] + 15) // 16) * ((cam["H"] + 15) // 16)
    assert P > 1 << 20 and tiles >= 2048, (P, tiles)
    vsent = (1 << (32 - int(P - 1).bit_length())) - 1  # the largest kept count the depth-sort value can hold
    assert vsent == 2047
    assert c["full_image"] >= 3 and c["max_tiles"] == tiles, c
    assert c["visible"] <= 400, c  # nothing else of that size
    assert sum(k == tiles for k in c["kept_wide"]) >= 3, c
    # below and above what the field holds, short of the whole image: both sides of the `kept == vsent` branch
    assert sum(1500 <= k < vsent for k in c["kept_wide"]) >= 2, c
    assert sum(vsent <= k < tiles for k in c["kept_wide"]) >= 2, c
    assert c["K"] >= 3 * tiles, c
