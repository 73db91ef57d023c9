"""The per-Gaussian stage (k_preprocess; k_view_grad, k_gauss_accum, k_gauss_fused) at the counts where its launches
and loops change (tests/gauss_backward_cases.py, whose census tests/test_gauss_backward_cases.py holds on the CPU):

- items per thread 2, 4, 8 and 16 of k_view_grad in one 64-view group with a partial last slice, and again in 16
  Gaussian ranges (g0 != 0, items 2), bitwise equal;
- 1, 63 (odd), 4160 (13 tile bits, no split) and 6300 tiles (cut-off table read from memory), the last also as a
  two-view two-colour set with SHs, with precomputed colours (k_gauss_fused<true>) and with GSR_GAUSS_FUSED=0;
- wave lists of 0, at most 64 and more than 64, accum blocks with no, some and every row reached, view sets {0}, {63},
  {0, 1}, {0, 1, 2} and all 64, as one group and as one view per group (first-group-only and last-group-only rows),
  with SHs and with precomputed colours;
- a Gaussian the tile lists whose alpha stays below 1 / 255 at every pixel;
- SH rows of 1, 4, 9, 16 and 25 coefficients at counts whose last block is no multiple of four floats.

Bars and adjudication are those of tests/gsr_testutil.py (check_forward, check_grads, adjudicate), unchanged, against
the fp64 oracle.  On top of them gauss_backward_cases.strict: no row beyond max(bar, ROW_RATIO x the fp32 oracle's
miss) and no more bar misses than the fp32 oracle (none, by the census); and rows of never-listed Gaussians are
exactly zero."""
import numpy as np
import pytest

import gauss_backward_cases as gc
import oracle
from gsr_testutil import (_settings, adjudicate, check_forward, check_grads, flip_dependents, flip_excuse, oracle_cam,
                          print_report, run_oracle)

pytestmark = pytest.mark.gpu

NAMES = dict(means3D="means3D", scales="scales", rotations="rotations", opacities="opacity", shs="sh",
             colors_precomp="colors", colors2="colors2")


@pytest.fixture(autouse=True)
def _parity_report():
    yield
    print_report()


class _ForceChunks:
    """A grad_reduce stand-in: the last group's per-Gaussian backward in n Gaussian ranges, nothing reduced."""

    def __init__(self, n):
        self.n, self.ranges_seen = n, 0

    def active(self):
        return True

    def chunk_events(self, device):
        import torch

        return [torch.cuda.Event() for _ in range(self.n)]

    def launch(self, grads, P, events=None):
        for e in events:
            e.synchronize()
        self.ranges_seen = len(events)


def _run(case, reduce=None, two=False, monkeypatch=None, budget=None):
    """rasterize_views over the case's views: outputs, K, listed instances, gradients, and the number of view groups
    the backward ran (GAUSS_BWD phases of the library's profile)."""
    import torch

    from diff_gaussian_rasterization import _C, batched
    from diff_gaussian_rasterization.batched import rasterize_views

    if budget is not None:
        monkeypatch.setattr(batched, "WORK_BUDGET", budget)
    dev = "cuda"
    scene, cams = case["scene"], case["cams"]
    V, P = len(cams), case["P"]
    keys = [k for k in ("means3D", "scales", "rotations", "opacities", "shs", "colors_precomp") if scene.get(k) is not None]
    t = {k: torch.tensor(scene[k], device=dev, requires_grad=True) for k in keys}
    if two:
        t["colors2"] = torch.tensor(case["colors2"], device=dev, requires_grad=True)
    m2s = [torch.zeros((P, 3), device=dev, requires_grad=True) for _ in cams]
    settings = [_settings(c, b, int(scene.get("sh_degree", 0))) for c, b in zip(cams, case["bgs"])]
    res = rasterize_views(settings, t["means3D"], m2s, t["opacities"], shs=t.get("shs"),
                          colors_precomp=t.get("colors_precomp"), scales=t["scales"], rotations=t["rotations"],
                          colors2=t.get("colors2"), grad_reduce=reduce)
    c, r, d, a = res[:4]
    out = dict(color=c.detach().cpu().numpy(), depth=d.detach().cpu().numpy(), alpha=a.detach().cpu().numpy(),
               radii=r.cpu().numpy(), K=[k for k, _, _ in list(_C.RECENT_FORWARDS)[-V:]],
               listed=list(_C.RECENT_LISTED)[-V:])
    up = lambda i: torch.stack([torch.tensor(u[i], device=dev) for u in case["ups"]])  # noqa: E731
    loss = (c * up(0)).sum() + (d * up(1)).sum() + (a * up(2)).sum()
    if two:
        out["color2"] = res[4].detach().cpu().numpy()
        loss = loss + (res[4] * torch.stack([torch.tensor(u, device=dev) for u in case["ups2"]])).sum()
    torch.cuda.synchronize()
    _C.profile_enable(True)
    _C.profile_read(reset=True)
    try:
        loss.backward()
        torch.cuda.synchronize()
        out["groups"] = _C.profile_read(reset=True)["gauss_bwd"][1]
    finally:
        _C.profile_enable(False)
    for k, v in t.items():
        out["g_" + NAMES[k]] = v.grad.cpu().numpy()
    out["g_means2D"] = [m.grad.cpu().numpy() for m in m2s]
    return out


def _bitwise(a, b, keys, what):
    for k in ("color", "depth", "alpha", "radii"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"
    for k in keys:
        assert np.array_equal(a["g_" + k], b["g_" + k]), f"{what}: grad {k}"
    for v, (x, y) in enumerate(zip(a["g_means2D"], b["g_means2D"])):
        assert np.array_equal(x, y), f"{what}: means2D of view {v}"


def _m2(gpu, ref, what, excuse):
    b64 = np.asarray(ref["b64"]["means2D"], np.float64)
    return adjudicate(gpu, ref["b32"]["means2D"], b64, gc.bar_of(b64), what, "grad means2D", rowwise=True,
                      r32b=ref["b32r"]["means2D"], excuse=excuse)


def _check_ring(case, gpu, keys, what):
    """Every view against its oracle on the listed rows, the summed gradients against the oracle's sums, no slack;
    every other row exactly zero."""
    views, total, rows = gc.reference(case)
    hidden = np.ones(case["P"], bool)
    hidden[rows] = False
    for v, r in enumerate(views):
        w = f"{what} view {v}"
        check_forward(dict(color=gpu["color"][v], depth=gpu["depth"][v], alpha=gpu["alpha"][v],
                           radii=gpu["radii"][v][rows]), r, w, K_gpu=gpu["K"][v])
        assert not gpu["radii"][v][hidden].any(), w
        gc.strict(dict(means2D=_m2(gpu["g_means2D"][v][rows], r, w, flip_excuse([r]))), w)
        assert not gpu["g_means2D"][v][hidden].any(), f"{w}: means2D row of a never-listed Gaussian"
    sub = {"g_" + k: gpu["g_" + k][rows] for k in keys}
    gc.strict(check_grads(sub, total, keys, what + " summed", excuse=flip_excuse(views)), what + " summed")
    for k in keys:
        assert not gpu["g_" + k][hidden].any(), f"{what}: {k} row of a never-listed Gaussian"


def _check_one(case, gpu, what, keys=gc.GRAD_KEYS):
    ref = gc.reference_one(case)
    check_forward(dict(color=gpu["color"][0], depth=gpu["depth"][0], alpha=gpu["alpha"][0], radii=gpu["radii"][0]),
                  ref, what, K_gpu=gpu["K"][0])
    g = dict(gpu, g_means2D=gpu["g_means2D"][0])
    gc.strict(check_grads(g, ref, ["means2D"] + list(keys), what), what)
    return ref


# ---- 1. items per thread ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items", [2, 4, 8, 16])
def test_items_per_thread(items):
    case = gc.items_case(items)
    what = f"gauss {case['name']}"
    one = _run(case)
    assert one["groups"] == 1, "the 64 views must run as one group for this items value"
    _check_ring(case, one, gc.GRAD_KEYS, what)
    force = _ForceChunks(16)
    chunked = _run(case, reduce=force)
    assert force.ranges_seen == 16 and chunked["groups"] == 1
    _bitwise(one, chunked, gc.GRAD_KEYS, what + " in 16 ranges")


# ---- 2. tile counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", sorted(gc.TILE_SIZES))
def test_tile_counts(tiles):
    case = gc.tiles_case(tiles)
    gpu = _run(case)
    assert gpu["groups"] == 1
    _check_one(case, gpu, f"gauss {case['name']}")


_TWO = {}


def _two_reference(case, first):
    """Per view the first call's run_oracle (`first`: the case or its precomp form) and the sums over the views of
    both calls' backward passes, as test_two_colour_backward forms them."""
    key = first["name"]
    if "second" not in _TWO:
        sc2 = dict(case["scene"], colors_precomp=case["colors2"])
        sc2.pop("shs")
        _TWO["second"] = [
            {name: oracle.backward(sc2, oracle_cam(cam), np.asarray(bg, np.float32), up2, None, None, prec=prec, order=o)
             for prec, o, name in (("f32", 0, "b32"), ("f64", 0, "b64"), ("f32c", 1, "b32r"))}
            for cam, bg, up2 in zip(case["cams"], case["bgs"], case["ups2"])]
        _TWO["second_fwd"] = run_oracle(sc2, case["cams"][0], case["bgs"][0])
    if key not in _TWO:
        refs = [run_oracle(first["scene"], cam, bg, grads=up)
                for cam, bg, up in zip(first["cams"], first["bgs"], first["ups"])]
        col = "sh" if "shs" in first["scene"] else "colors"
        tot = {}
        for name in ("b32", "b64", "b32r"):
            tot[name] = {k: sum(np.asarray(r[name][k], np.float64) + np.asarray(s[name][k], np.float64)
                                for r, s in zip(refs, _TWO["second"]))
                         for k in ("means3D", "scales", "rotations", "opacity")}
            tot[name][col] = sum(np.asarray(r[name][col], np.float64) for r in refs)
            tot[name]["colors2"] = sum(np.asarray(s[name]["colors"], np.float64) for s in _TWO["second"])
        _TWO[key] = (refs, tot, col)
    return _TWO[key]


def _check_two(case, first, gpu, what):
    refs, tot, col = _two_reference(case, first)
    for v, r in enumerate(refs):
        w = f"{what} view {v}"
        check_forward(dict(color=gpu["color"][v], depth=gpu["depth"][v], alpha=gpu["alpha"][v], radii=gpu["radii"][v]),
                      r, w, K_gpu=gpu["K"][v])
        gc.strict(dict(means2D=_m2(gpu["g_means2D"][v], r, w, flip_excuse([r]))), w)  # (the first call's own)
    check_forward(dict(color=gpu["color2"][0], depth=gpu["depth"][0], alpha=gpu["alpha"][0]), _TWO["second_fwd"],
                  what + " second colour")
    keys = ["means3D", "opacity", col, "colors2", "scales", "rotations"]
    gc.strict(check_grads(gpu, tot, keys, what + " summed", excuse=flip_excuse(refs)), what + " summed")
    return keys


def test_unstaged_table_two_views_two_colours(monkeypatch):
    """6300 tiles, two views, two colours: k_view_grad<true, false> with SHs, k_gauss_fused<true> with precomputed
    colours, and k_view_grad<true, false> again under GSR_GAUSS_FUSED=0, bitwise the fused kernel's gradients."""
    case = gc.two_view(gc.tiles_case(6300))
    sh = _run(case, two=True)
    assert sh["groups"] == 1
    _check_two(case, case, sh, "gauss tiles-6300 two colours SH")
    pre = gc.precomp(case)
    fused = _run(pre, two=True)
    keys = _check_two(case, pre, fused, "gauss tiles-6300 two colours fused")
    monkeypatch.setenv("GSR_GAUSS_FUSED", "0")
    split = _run(pre, two=True)
    _bitwise(fused, split, keys, "fused against split")


# ---- 3. reach patterns -----------------------------------------------------------------------------------------------
def test_reach_patterns(monkeypatch):
    case = gc.reach_case()
    one = _run(case)
    assert one["groups"] == 1
    _check_ring(case, one, gc.GRAD_KEYS, "gauss reach")
    groups = _run(case, monkeypatch=monkeypatch, budget=1)  # work = one view's bytes: one view per group
    assert groups["groups"] == len(case["cams"]) >= 3
    _bitwise(one, groups, gc.GRAD_KEYS, "one group against 64")


def test_reach_patterns_precomputed_colours(monkeypatch):
    case = gc.precomp(gc.reach_case())
    fused = _run(case)
    assert fused["groups"] == 1
    _check_ring(case, fused, gc.COLOR_KEYS, "gauss reach fused")
    monkeypatch.setenv("GSR_GAUSS_FUSED", "0")
    split = _run(case)
    _bitwise(fused, split, gc.COLOR_KEYS, "fused against split")
    monkeypatch.delenv("GSR_GAUSS_FUSED")
    groups = _run(case, monkeypatch=monkeypatch, budget=1)
    assert groups["groups"] == len(case["cams"])
    _bitwise(fused, groups, gc.COLOR_KEYS, "fused: one group against 64")


# ---- 4. staged but empty ---------------------------------------------------------------------------------------------
def test_staged_but_empty():
    case = gc.empty_case()
    e = case["empty"]
    gpu = _run(case)
    assert gpu["listed"][0] == case["P"] == gpu["K"][0], "the tile must list every Gaussian, the empty one included"
    ref = _check_one(case, gpu, "gauss empty")
    assert not flip_dependents(ref, ref["gpu_only_px"])[e]
    for k in gc.GRAD_KEYS:
        assert not gpu["g_" + k][e].any(), k
    assert not gpu["g_means2D"][0][e].any()


# ---- 5. SH widths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", gc.SH_CASES)
def test_sh_widths(M, P):
    case = gc.sh_case(M, P)
    gpu = _run(case)
    _check_one(case, gpu, f"gauss {case['name']}")
    if M > 16:
        assert not gpu["g_sh"][:, 16:].any(), "dL/dSH of coefficients the reference never reads"
