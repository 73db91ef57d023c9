"""Census of the constructed per-Gaussian cases (tests/gauss_backward_cases.py), on the CPU: each case has the
property its name states, by launch_plan and the fp64 oracle; launch_plan's constants are the ones in the .hip files;
and the reference alone (fp32 oracle against fp64 oracle) stays inside the zero-slack rule the GPU tests apply."""
import numpy as np
import pytest

import gauss_backward_cases as gc
from blend_cases import ALPHA_MIN, MARGIN
from gsr_testutil import REPORT


@pytest.fixture(autouse=True)
def _quiet_report():
    yield
    REPORT.clear()


def test_constants_are_the_sources():
    """A retune of GSR_VG_ITEMS, GSR_CUT_LDS_MAX, GSR_PRE_GAUSS, ... fails here: the cases below are built on them."""
    src = gc.source_constants()
    assert src == {k: getattr(gc, k) for k in src}
    assert gc.CUT_LDS_MAX // 8 == 6144 and gc.PRE_GAUSS * (3 * 21 + 1) <= gc.PRE_LDS_FLOATS < gc.PRE_GAUSS * (3 * 22 + 1)


def test_launch_plan_thresholds():
    for V, n, items in ((64, 15 * 256 * 2, 2), (64, 15 * 256 * 4, 2), (64, 15 * 256 * 4 + 1, 4), (64, 15 * 256 * 8 + 1, 8),
                        (64, 15 * 256 * 16, 8), (64, 15 * 256 * 16 + 1, 16), (1, 1_000_000, 2), (16, 250_000, 8)):
        assert gc.launch_plan(V, n, 4, True, False)["items"] == items, (V, n)
    assert gc.launch_plan(1, 100, 6144, True, False)["cut_in_lds"]
    assert not gc.launch_plan(1, 100, 6145, True, False)["cut_in_lds"]
    assert gc.launch_plan(1, 100, 63, False, True, fused_env=False)["kernel"] == "k_view_grad<true, true>"
    assert gc.launch_plan(1, 100, 63, False, True)["kernel"] == "k_gauss_fused<true>"
    assert not gc.launch_plan(1, 100, 63, True, False)["fused"]  # SHs: never fused
    assert [gc.preprocess_plan(1, 10, M, True)["staged"] for M in (16, 21, 22, 25)] == [True, True, False, False]
    assert gc.preprocess_plan(3, 10, 16, True)["halves"] == [((0, 2), (2, 3))]
    assert gc.preprocess_plan(64, 300, 16, True)["grid"] == 3 and gc.preprocess_plan(65, 300, 16, True)["grid"] == 6
    assert not gc.preprocess_plan(1, 10, 16, False)["staged"]
    # the widest SH row k_gauss_accum can stage in the CU's LDS, and the first that it cannot
    M = gc.max_sh()
    assert gc.accum_lds_bytes(M) <= gc.CU_LDS_BYTES < gc.accum_lds_bytes(M + 1)
    assert gc.accum_lds_bytes(25) == 80 * 1024 + gc.ACCUM_STATIC_LDS


def test_index_layout():
    idx = np.arange(4096)
    for items in (2, 4, 8, 16):
        sl, wave = gc.view_grad_owner(idx, items)
        # thread t of slice s reads s * 256 * items + it * 256 + t, it < items
        t = idx % 256
        assert np.array_equal(wave, t // 64) and np.array_equal(sl, idx // (256 * items))
    assert np.array_equal(gc.view_grad_owner(np.array([4096, 4607, 4608]), 2, g0=4096)[0], [0, 0, 1])
    assert np.array_equal(gc.accum_block(np.array([255, 256, 4351]), g0=0), [0, 1, 16])


def _alone(case, keys, views, total):
    what = case["name"]
    for v, r in enumerate(views):
        st = gc.reference_alone(r["b32"], r["b32r"], r["b64"], ["means2D"], f"{what} view {v}")["means2D"]
        assert st["f32_miss"] == 0 and st["null_beyond"] == 0, (what, v, st)
    for k, st in gc.reference_alone(total["b32"], total["b32r"], total["b64"], keys, what).items():
        assert st["f32_miss"] == 0 and st["null_beyond"] == 0, (what, k, st)


def _ring_census(case):
    """What every ring case holds: each Gaussian is listed in exactly the views it was placed for, and nowhere else."""
    listed = gc.census(case)["tiles"] > 0
    want = gc.placed(case)
    assert np.array_equal(listed, want), (case["name"], np.nonzero((listed != want).any(0))[0][:8])
    return listed


@pytest.mark.parametrize("items", [2, 4, 8, 16])
def test_items_cases(items):
    case = gc.items_case(items)
    P = case["P"]
    plan = gc.launch_plan(64, P, 4, True, False)
    assert plan["items"] == items and plan["cut_in_lds"] and (items == 2 or plan["view_grad_grid"] >= 1024)
    assert P % (256 * items) != 0 and 0 < plan["last_slice"] < 256 * items
    # the chunked rerun: 16 ranges of 4096-aligned size, each small enough for items 2, all but the first at g0 != 0
    cs = -(-(-(-P // 16)) // 4096) * 4096
    assert cs < P and gc.launch_plan(64, cs, 4, True, False)["items"] == 2
    listed = _ring_census(case)
    got = gc.contributed(case)
    assert not (got & ~listed).any()
    seen = np.nonzero(got.any(0))[0]
    # Gaussians with a gradient in every item slot of a thread, in the last partial slice, and at the last index
    sl, _ = gc.view_grad_owner(seen, items)
    slot = (seen % (256 * items)) // 256
    assert set(slot.tolist()) == set(range(items)) and sl.max() == plan["view_grad_grid"] // 64 - 1 and seen[-1] == P - 1
    views, total, _ = gc.reference(case)
    _alone(case, gc.GRAD_KEYS, views, total)


def test_reach_case():
    case = gc.reach_case()
    assert gc.launch_plan(64, case["P"], 9, True, False)["items"] == 2
    assert gc.launch_plan(1, case["P"], 9, True, False)["items"] == 2  # one view per group
    listed = _ring_census(case)
    got = gc.contributed(case)
    assert not (got & ~listed).any()
    idx = np.arange(case["P"])
    sl, wave = gc.view_grad_owner(idx, 2)

    def wave_count(v, s, w):
        return int(got[v, (sl == s) & (wave == w)].sum())

    assert wave_count(0, 0, 0) > 64             # two rounds: the i + 64 < cnt prefetch reload
    assert 1 <= wave_count(0, 0, 2) <= 64 and 1 <= wave_count(5, 0, 3) <= 64
    assert wave_count(0, 0, 1) == 0 and wave_count(5, 0, 0) == 0
    assert int(listed[0, (sl == 0) & (wave == 0)].sum()) == 128
    # k_gauss_accum: a block with every row reached, one with none, partial ones (the last block is short)
    reached = listed.any(0)
    blocks = gc.accum_block(idx)
    nr = np.bincount(blocks, weights=reached).astype(int)
    assert nr[0] == 256 and nr[2] == 0 and 0 < nr[1] < 256 and 0 < nr[-1] < case["P"] - 256 * (len(nr) - 1) < 256
    assert got[:, blocks == 0].any(0).all()
    # the view sets of the two-buffer stream and the reach word's ends
    sets = {tuple(np.nonzero(got[:, i])[0]) for i in np.nonzero(got.any(0))[0]}
    for want in ((63,), (0,), (0, 1), (0, 1, 2), tuple(range(64))):
        assert want in sets, want
    # one view per group: rows only the first / only the last group reaches
    assert got[0, 771:774].all() and not got[1:, 771:774].any()
    assert got[63, 768:771].all() and not got[:63, 768:771].any()
    views, total, _ = gc.reference(case)
    _alone(case, gc.GRAD_KEYS, views, total)
    pre = gc.precomp(case)
    assert gc.launch_plan(64, case["P"], 9, False, False)["fused"]
    _alone(pre, gc.COLOR_KEYS, *gc.reference(pre)[:2])


@pytest.mark.parametrize("tiles", sorted(gc.TILE_SIZES))
def test_tiles_cases(tiles):
    case = gc.tiles_case(tiles)
    plan = gc.launch_plan(1, case["P"], tiles, True, False)
    assert plan["cut_in_lds"] == (tiles <= 6144) and plan["odd_tail"] == (tiles in (1, 63))
    assert gc.tile_bits(tiles) == {1: 1, 63: 6, 4160: 13, 6300: 13}[tiles]
    assert gc.split_fits(1, tiles) == (tiles <= 4096)
    ref = gc.reference_one(case)
    # the last tile (the odd tail of the staged table) holds a Gaussian that receives a gradient
    rect = ref["aux64"]["rect"]
    gx = -(-case["cams"][0]["W"] // 16)
    tx, ty = (tiles - 1) % gx, (tiles - 1) // gx
    in_last = (rect[:, 0] <= tx) & (tx < rect[:, 2]) & (rect[:, 1] <= ty) & (ty < rect[:, 3]) & (ref["aux64"]["tiles"] > 0)
    assert (in_last & (np.asarray(ref["b64"]["means2D"]) != 0).any(1)).any()
    keys = ["means2D"] + list(gc.GRAD_KEYS)
    for k, st in gc.reference_alone(ref["b32"], ref["b32r"], ref["b64"], keys, case["name"]).items():
        assert st["f32_miss"] == 0 and st["null_beyond"] == 0, (k, st)


def test_two_view_two_colour_case_plans():
    assert gc.launch_plan(2, 300, 6300, True, True)["kernel"] == "k_view_grad<true, false>"
    assert gc.launch_plan(2, 300, 6300, False, True, fused_env=False)["kernel"] == "k_view_grad<true, false>"
    assert gc.launch_plan(2, 300, 6300, False, True)["kernel"] == "k_gauss_fused<true>"
    assert gc.launch_plan(1, 300, 6300, True, False)["kernel"] == "k_view_grad<false, false>"
    assert not gc.split_fits(2, 6300)


def test_empty_case():
    case = gc.empty_case()
    w, aux, pos = gc.empty_walk(case)
    e = case["empty"]
    assert aux["tiles"][e] == 1 and w["n"] == case["P"] and (w["quad"] == case["P"]).all()  # listed, no cut-off
    a = w["alpha"][pos]
    assert np.isfinite(a).all() and (a < ALPHA_MIN * (1.0 - MARGIN)).all()   # evaluated at every pixel, never blended
    assert aux["opacity"][e] > ALPHA_MIN * (1.0 + MARGIN)                      # yet its ellipse is not empty
    ref = gc.reference_one(case)
    assert (aux["rgb"][e] == 0).all()                                           # all three channels clamped
    keys = ["means2D"] + list(gc.GRAD_KEYS)
    for k in keys:
        assert not np.asarray(ref["b64"][k])[e].any() and not np.asarray(ref["b32"][k])[e].any(), k
    others = np.delete(np.arange(case["P"]), e)
    assert (np.asarray(ref["b64"]["means2D"])[others] != 0).any(1).all()
    for k, st in gc.reference_alone(ref["b32"], ref["b32r"], ref["b64"], keys, case["name"]).items():
        assert st["f32_miss"] == 0 and st["null_beyond"] == 0, (k, st)


@pytest.mark.parametrize("M,P", gc.SH_CASES)
def test_sh_cases(M, P):
    case = gc.sh_case(M, P)
    plan = gc.preprocess_plan(1, P, M, True)
    assert plan["staged"] == (M <= 21)
    if M in (1, 9):
        assert plan["tail_floats"] % 4 != 0
    assert P % gc.PRE_GAUSS != 0 and P % 256 != 0
    assert case["scene"]["shs"].shape == (P, M, 3) and (case["scene"]["shs"] != 0).all()
    assert gc.accum_lds_bytes(M) <= gc.CU_LDS_BYTES
    ref = gc.reference_one(case)
    if M > 16:
        assert not np.asarray(ref["b64"]["sh"])[:, 16:].any()
    assert np.asarray(ref["b64"]["sh"])[:, :min(M, 16)].any(0).all()
    keys = ["means2D"] + list(gc.GRAD_KEYS)
    for k, st in gc.reference_alone(ref["b32"], ref["b32r"], ref["b64"], keys, case["name"]).items():
        assert st["f32_miss"] == 0 and st["null_beyond"] == 0, (k, st)
