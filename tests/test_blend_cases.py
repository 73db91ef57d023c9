"""The constructed blend cases (tests/blend_cases.py) are what they claim, by the CPU oracle alone: list lengths,
the per-quadrant deepest blends, the hit-list fills, the no-termination bound, the margins of the boundary rows,
and that the reference itself (its fp32 run and the second one with contraction and the reverse pixel order)
needs nothing forgiven at a boundary row or a pixel."""
import numpy as np
import pytest

import blend_cases as bc
from gsr_testutil import DEPTH_RTOL, GRAD_TOL, RGB_ATOL, oracle_cam

CASES = bc.all_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(params=CASES, ids=IDS, scope="module")
def case(request):
    cid, build = request.param
    return cid, build, build()


def test_list_length_and_order(case):
    import oracle

    cid, build, (scene, cam, bg, grads, meta) = case
    ref = bc.reference(cid, build)
    P = scene["means3D"].shape[0]
    assert P == meta["L"] and meta["n"] == meta["L"], "every Gaussian is one entry of the tile's list"
    assert (ref["f32"]["radii"] > 0).all() and (ref["f64"]["radii"] > 0).all()
    if cam["W"] == 16:
        assert ref["f32"]["K"] == meta["L"] and ref["f64"]["K"] == meta["L"]
    # list position = index: strictly increasing fp32 depths (distinct depth keys), at least 1 / 8192 apart
    d32 = oracle.gauss_aux(scene, oracle_cam(cam), "f32")["depth"]
    assert (np.diff(d32) >= 1.0 / 8192.0 - 1e-6).all() and d32.min() >= 2.0 - 1e-6 and d32.max() <= 3.0 + 1e-6
    assert len(np.unique(d32.astype(np.float32).view(np.uint32))) == P
    assert np.array_equal(meta["order"], np.arange(P))
    assert int(scene["sh_degree"]) == 0 and (scene["rotations"] == np.array([1, 0, 0, 0], np.float32)).all()


def test_regime(case):
    cid, build, (scene, cam, bg, grads, meta) = case
    quad, fam = meta["quad"], meta["family"]
    assert not meta["fragile"].any(), "no quadrant's deepest blend sits within 5 % of a threshold"
    if cam["W"] != 16:  # ragged: quadrants 1 and 3 of the second tile lie outside the image
        assert meta["tile"] == 1 and list(quad) == [meta["expect_quad"], 0, meta["expect_quad"], 0]
    elif fam == "quadrant_cut":
        c, L = meta["c"], meta["L"]
        assert quad[0] < c + 8 and quad[0] == c and list(quad[1:]) == [L, L, L]
        assert tuple(quad) == meta["expect_quad"]
    else:
        assert (quad == meta["expect_quad"]).all(), quad
    if fam in ("sparse", "hitcap"):
        assert meta["max_alpha"] < 0.99, "no pixel finishes"
        assert (quad[quad > 0] == meta["L"]).all()
    if fam == "cut":
        assert meta["expect_quad"] == meta["c"] and meta["L"] >= meta["c"] + 2
    if fam == "hitcap":
        assert meta["hits"].shape[0] == 1 and int(meta["hits"][0].max()) == meta["expect_fill"]
        assert meta["expect_fill"] == bc.HCAP + (1 if meta["kind"] == "over" else 0)


def test_walk_matches_oracle(case):
    """The numpy walk against the oracle's own blend: the same accumulated alpha per pixel (fp64)."""
    cid, build, (scene, cam, bg, grads, meta) = case
    import oracle

    w = bc.walk(oracle.gauss_aux(scene, oracle_cam(cam), "f64"), cam["W"], cam["H"], meta["tile"])
    a64 = bc.reference(cid, build)["f64"]["alpha"][0]
    x0 = 16 * meta["tile"]
    fa = w["final_alpha"].reshape(16, 16)[:, :cam["W"] - x0]
    assert np.abs(fa - a64[:, x0:]).max() < 1e-12
    assert np.array_equal(w["quad"], meta["quad"])


def test_boundary_margins(case):
    import oracle

    cid, build, (scene, cam, bg, grads, meta) = case
    w = bc.walk(oracle.gauss_aux(scene, oracle_cam(cam), "f64"), cam["W"], cam["H"], meta["tile"])
    pos = np.array(sorted(meta["boundary_pos"]))
    assert pos.size and {0, meta["L"] - 1} <= set(pos.tolist())
    a, t = w["alpha"][pos], w["test"][pos]
    with np.errstate(invalid="ignore"):
        assert not (np.abs(a / bc.ALPHA_MIN - 1.0) < bc.MARGIN).any()
        assert not (np.abs(t / bc.T_EPS - 1.0) < bc.MARGIN).any()
    # a boundary row the list walks blends somewhere, and a lost or doubled row stands 10 bars out
    b64 = bc.reference(cid, build)["b64"]
    reached = pos[pos < meta["quad"].max()]
    assert np.isfinite(t[pos < meta["quad"].max()]).any(1).all()
    g = meta["order"][reached]
    size = np.max([np.abs(b64[k][g]).reshape(g.size, -1).max(1) for k in bc.GRAD_KEYS], 0)
    assert (size >= 10 * GRAD_TOL).all(), size.min()
    beyond = meta["order"][pos[pos > meta["quad"].max()]]
    for k in bc.GRAD_KEYS:
        assert not np.asarray(b64[k])[beyond].any(), "never blended: no gradient"


def test_reference_needs_no_forgiveness(case):
    """Both fp32 runs of the reference within the bars of the fp64 one at every pixel and every boundary row, and
    the second run under the boundary-row rule against the first, nothing excused."""
    cid, build, (scene, cam, bg, grads, meta) = case
    ref = bc.reference(cid, build)
    f32, f64 = ref["f32"], ref["f64"]
    assert np.abs(f32["color"] - f64["color"]).max() <= RGB_ATOL
    assert np.abs(f32["alpha"] - f64["alpha"]).max() <= RGB_ATOL
    assert (np.abs(f32["depth"] - f64["depth"]) <= RGB_ATOL + DEPTH_RTOL * np.abs(f64["depth"])).all()
    rows = sorted(meta["boundary"])
    for run in ("b32", "b32r"):
        for k in bc.GRAD_KEYS:
            r64 = np.asarray(ref["b64"][k], np.float64)[rows]
            err = np.abs(np.asarray(ref[run][k], np.float64)[rows] - r64)
            assert (err <= GRAD_TOL * np.maximum(1.0, np.abs(r64))).all(), (run, k)
    counts, failures = bc.boundary_rule({"g_" + k: ref["b32r"][k] for k in bc.GRAD_KEYS}, ref["b32"], ref["b64"],
                                        bc.GRAD_KEYS, meta, cid)
    assert not failures, failures
    assert sum(v[1] for v in counts.values()) == 0


def test_boundary_positions():
    b = bc.boundary_positions(4400)
    for p in (0, 4399, 63, 64, 255, 256, 3839, 3840, 4095, 4096, 4351, 4352):
        assert p in b
    assert b[255] == {"e64", "e256"} and b[63] == {"e64"} and b[0] == {"end"} and 62 not in b and 4097 not in b
    assert bc.boundary_positions(64) == {0: {"end"}, 63: {"end", "e64"}}
    assert [L for L in bc.SPARSE_L if L in (3840, 4096)] == [3840, 4096] and bc.CH * bc.NCK == 3840
