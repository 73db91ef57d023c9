"""The blend kernels at the tile-list lengths and cut-offs where their batching and chunking change
(tests/blend_cases.py: staged batches of 64, groups of 8, split chunks of 256 with 15 boundaries, the 256-entry hit
list of the two-colour backward, a quadrant that finishes before its tile), on every path that walks a list:

- default per-view path: the quadrant-wave forward with checkpoints, then the split k_render_bwd;
- GSR_BWD_SPLIT=0: the whole-prefix walk (outputs bitwise the split run's, gradients within 1e-4 max(1, |g|) of it);
- GSR_FWD_KERNEL=tile: k_render_fwd_tile (outputs bitwise the quadrant-wave forward's), whose quadrant masks the
  backward then reads in the tile-wave layout;
- the two-colour backward k_render_bwd_tw<true> (hit lists), against the oracle's two backward passes summed;
- a 16-view set of sparse(257) through rasterize_views (instance ranges that start at inst_start[v] > 0).

Bars and adjudication are those of tests/gsr_testutil.py, unchanged.  On top of them the boundary-row rule
(blend_cases.boundary_rule): the rows at list positions 0, L - 1, 64 k - 1, 64 k, 256 k - 1, 256 k get no slack, and
are left out only as flip dependents of a pixel the GPU flipped on its own — at most 10 % of all boundary rows
over the file, and never every row of a kind within a case.  Each run reads back quad_maxc and holds it to the
fp64 walk's per-quadrant deepest blend, so the intended regime is the one that ran."""
import numpy as np
import pytest

import blend_cases as bc
import oracle
from gsr_testutil import (REPORT, _gpu_views, _image_state, _settings, _sum_grads, _view, adjudicate, check_forward,
                          check_grads, flip_dependents, flip_excuse, gpu_render, oracle_cam, print_report, run_oracle)

pytestmark = pytest.mark.gpu

CASES = bc.all_cases()
BUILD = dict(CASES)
IDS = [c[0] for c in CASES]
KEYS = list(bc.GRAD_KEYS)
TWO_COLOUR = [f"sparse-{L}" for L in bc.TWO_COLOUR_SPARSE_L] + ["hitcap-at", "hitcap-over", "cut-257"]
TALLY = []      # (what, counts per kind [checked, excused]) of every boundary-rule run of this file
_DEFAULT = {}   # the default path's GPU results per case: what the other paths are compared with


@pytest.fixture(autouse=True)
def _parity_report():
    yield
    print_report()


def _regime(cid, what, split, masks):
    """The forward's own record of what it ran: split_mode, and quad_maxc equal to the walk's per-quadrant deepest
    blend (a value may differ only where the walk puts that quadrant's last blend within 5 % of a threshold)."""
    scene, cam, _, _, meta = BUILD[cid]()
    mode, quads = _image_state(scene, cam)
    got, want = quads[meta["tile"]].astype(np.int64), meta["quad"]
    differ = got != want
    REPORT.append((what, "quad_maxc", dict(gpu=got.tolist(), walk=want.tolist(), fragile=meta["fragile"].tolist(),
                                           split_mode=mode)))
    assert not (differ & ~meta["fragile"]).any(), f"{what}: quad_maxc {got} vs the walk's {want}"
    assert (mode[0] != 0) == split and mode[1] == masks, f"{what}: split_mode {mode}"


def _oracle_checks(cid, gpu, what, ref=None, keys=KEYS, excuse=None):
    """check_forward / check_grads with the suite's bars, then the boundary-row rule."""
    meta = BUILD[cid]()[4]
    if ref is None:
        ref = bc.reference(cid, BUILD[cid])
        check_forward(gpu, ref, what, K_gpu=gpu["K"])
        check_grads(gpu, ref, keys, what)
        excuse = flip_dependents(ref, ref["gpu_only_px"])
    else:
        check_grads(gpu, ref, keys, what, excuse=excuse)
    counts, failures = bc.boundary_rule(gpu, ref["b32"], ref["b64"], keys, meta, what, excuse)
    TALLY.append((what, counts))
    assert not failures, "\n".join(failures)
    for kind, (checked, excused) in counts.items():
        assert checked >= 1 or excused == 0, f"{what}: every {kind} boundary row is excused"
    return counts


def _default(cid):
    if cid not in _DEFAULT:
        scene, cam, bg, grads, _ = BUILD[cid]()
        _DEFAULT[cid] = gpu_render(scene, cam, bg, grads=grads)
        _kernels("k_render_fwd<false, true>", "k_render_bwd")
    return _DEFAULT[cid]


def _kernels(fwd, bwd):
    from diff_gaussian_rasterization import _C

    assert _C.profile_kernels() == {"render_fwd": fwd, "render_bwd": bwd}


@pytest.mark.parametrize("cid", IDS)
def test_default_split_path(cid):
    """k_render_fwd<false, true> + k_ckpt_suffix, then k_render_bwd in chunks."""
    what = f"blend {cid} split"
    _regime(cid, what, split=True, masks=2)
    _oracle_checks(cid, _default(cid), what)


@pytest.mark.parametrize("cid", IDS)
def test_whole_prefix_walk(cid, monkeypatch):
    split = _default(cid)
    monkeypatch.setenv("GSR_BWD_SPLIT", "0")
    what = f"blend {cid} whole"
    scene, cam, bg, grads, _ = BUILD[cid]()
    whole = gpu_render(scene, cam, bg, grads=grads)
    _kernels("k_render_fwd<false, false>", "k_render_bwd")
    for k in ("alpha", "radii", "color", "depth"):
        assert np.array_equal(split[k], whole[k]), k
    for k in KEYS:
        ref = whole["g_" + k].astype(np.float64)
        err = float((np.abs(split["g_" + k] - ref) / np.maximum(1.0, np.abs(ref))).max())
        assert err <= 1e-4, f"{k}: {err}"
    _regime(cid, what, split=False, masks=2)
    _oracle_checks(cid, whole, what)


@pytest.mark.parametrize("cid", IDS)
def test_tile_wave_forward(cid, monkeypatch):
    quadrant = _default(cid)
    monkeypatch.setenv("GSR_FWD_KERNEL", "tile")
    what = f"blend {cid} tile-wave"
    scene, cam, bg, grads, _ = BUILD[cid]()
    tile = gpu_render(scene, cam, bg, grads=grads)
    _kernels("k_render_fwd_tile<false>", "k_render_bwd")
    for k in ("alpha", "radii", "color", "depth"):
        assert np.array_equal(quadrant[k], tile[k]), k
    _regime(cid, what, split=False, masks=1)
    _oracle_checks(cid, tile, what)


@pytest.mark.parametrize("cid", TWO_COLOUR)
def test_two_colour_backward(cid):
    """k_render_bwd_tw<true>: driven and referenced as test_second_colors_match_separate_call does, one view."""
    import torch

    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization.batched import rasterize_views

    what = f"blend {cid} two-colour"
    scene, cam, bg, grads, meta = BUILD[cid]()
    P = scene["means3D"].shape[0]
    rng = np.random.default_rng(4)
    n = rng.normal(size=(P, 3)).astype(np.float32)
    normals = n / np.linalg.norm(n, axis=1, keepdims=True)
    up2 = rng.standard_normal((3, cam["H"], cam["W"])).astype(np.float32)
    dev = "cuda"
    t = {k: torch.tensor(scene[k], device=dev, requires_grad=True)
         for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    t["normals"] = torch.tensor(normals, device=dev, requires_grad=True)
    m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
    c, r, d, a, c2 = rasterize_views([_settings(cam, bg, 0)], t["means3D"], [m2], t["opacities"], shs=t["shs"],
                                     scales=t["scales"], rotations=t["rotations"], colors2=t["normals"])
    K = _C.RECENT_FORWARDS[-1][0]
    u = [torch.tensor(x, device=dev) for x in (*grads, up2)]
    ((c[0] * u[0]).sum() + (d[0] * u[1]).sum() + (a[0] * u[2]).sum() + (c2[0] * u[3]).sum()).backward()
    assert _C.profile_kernels() == {"render_fwd": "k_render_fwd<true, false>", "render_bwd": "k_render_bwd_tw<true>"}
    gpu = {"g_" + k: t[src].grad.cpu().numpy() for k, src in (("means3D", "means3D"), ("scales", "scales"),
           ("rotations", "rotations"), ("opacity", "opacities"), ("sh", "shs"), ("normals", "normals"))}
    gpu["g_means2D"] = m2.grad.cpu().numpy()
    out = dict(color=c[0].detach().cpu().numpy(), depth=d[0].detach().cpu().numpy(),
               alpha=a[0].detach().cpu().numpy(), radii=r[0].cpu().numpy())
    ref1 = bc.reference(cid, BUILD[cid])
    check_forward(out, ref1, what, K_gpu=K)
    excuse = flip_dependents(ref1, ref1["gpu_only_px"])
    sc2 = dict(scene, colors_precomp=normals)
    sc2.pop("shs")
    ref2 = run_oracle(sc2, cam, bg)
    check_forward(dict(out, color=c2[0].detach().cpu().numpy()), ref2, what + " second colour")
    ref = {}
    for prec, order, key in (("f32", 0, "b32"), ("f64", 0, "b64"), ("f32c", 1, "b32r")):
        b2 = oracle.backward(sc2, oracle_cam(cam), np.asarray(bg, np.float32), up2, None, None, prec=prec, order=order)
        b1 = ref1[key]
        ref[key] = {k: np.asarray(b1[k], np.float64) + np.asarray(b2[k], np.float64)
                    for k in ("means3D", "scales", "rotations", "opacity")}
        ref[key].update(sh=np.asarray(b1["sh"], np.float64), normals=np.asarray(b2["colors"], np.float64),
                        means2D=np.asarray(b1["means2D"], np.float64))  # (the first call's own means2D gradient)
    keys = ["means3D", "means2D", "opacity", "sh", "normals", "scales", "rotations"]
    # (both colours' forwards blend the same candidates: the one-colour forward's quad_maxc is this one's)
    _regime(cid, what, split=True, masks=2)
    _oracle_checks(cid, gpu, what, ref=ref, keys=keys, excuse=excuse)


def test_sixteen_view_set():
    """sparse(257) 16 times in one rasterize_views set, per-view backgrounds and upstream gradients: view v's list
    starts at inst_start[v] = 257 v, and the boundary rows must keep their list positions."""
    import gsr_synthetic as gs

    cid, V = "sparse-257", 16
    scene, cam, _, _, meta = BUILD[cid]()
    rng = np.random.default_rng(16)
    bgs = rng.random((V, 3)).astype(np.float32).tolist()
    ups = [gs.upstream_grads(16, 16, seed=300 + v) for v in range(V)]
    gpu = _gpu_views(scene, [cam] * V, bgs, ups)
    assert gpu["K"] == [257] * V
    refs = []
    for v in range(V):
        what = f"blend {cid} set view {v}"
        ref = run_oracle(scene, cam, bgs[v], grads=ups[v])
        check_forward(_view(gpu, v), ref, what, K_gpu=gpu["K"][v])
        ex = flip_excuse([ref])
        adjudicate(gpu["g_means2D"][v], ref["b32"]["means2D"], ref["b64"]["means2D"],
                   1e-4 * np.maximum(1.0, np.abs(ref["b64"]["means2D"])), what, "grad means2D", rowwise=True,
                   r32b=ref["b32r"]["means2D"], excuse=ex)
        counts, failures = bc.boundary_rule(dict(g_means2D=gpu["g_means2D"][v]), ref["b32"], ref["b64"], ["means2D"],
                                            meta, what, ex)
        TALLY.append((what, counts))
        assert not failures, "\n".join(failures)
        refs.append(ref)
    keys = ["means3D", "opacity", "sh", "scales", "rotations"]
    tot = dict(b32=_sum_grads(refs, "b32", keys), b64=_sum_grads(refs, "b64", keys), b32r=_sum_grads(refs, "b32r", keys))
    _oracle_checks(cid, gpu, f"blend {cid} set summed", ref=tot, keys=keys, excuse=flip_excuse(refs))


def test_excused_boundary_rows_within_cap():
    """Over every run of this file: excused boundary rows are at most 10 % of all boundary rows."""
    if not TALLY:  # (run on its own)
        test_default_split_path("sparse-257")
    checked = sum(v[0] for _, c in TALLY for v in c.values())
    excused = sum(v[1] for _, c in TALLY for v in c.values())
    REPORT.append(("blend", "boundary rows of the file", dict(runs=len(TALLY), checked=checked, excused=excused,
                                                              share=excused / max(1, checked + excused))))
    assert checked > 0 and excused <= 0.10 * (checked + excused), (checked, excused)
