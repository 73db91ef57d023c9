"""The fused densification statistics (diff_gaussian_rasterization/densify.py) without a GPU: the library exports the
call and checks its arguments on the host; the CPU path — the bit reference of the kernel — against a direct fp32 loop
(bitwise), an fp64 sum (derived bound) and the reference's own mask-indexed form; in-place state, NaN in the running
maximum, calls chained over 130 views; update_states_fused against update_states on a DensifyModel, alone and on two
gloo ranks."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import densify_cases as dc
import densify_reference as dr
from gsr_testutil import gs

V, P = 5, 200
THRESHOLD = 2.0  # of the mean gradient norm (the magnitudes reach 1e2): both the clone and the split select


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _views():
    """V = 5 views of 200 Gaussians: view 1 has no gradient, view 3 visibility rows that differ from radii > 0."""
    return dc.make_views(V, P, seed=1, none_at=(1,), explicit=(3,))


def _stats(views, **state):
    from diff_gaussian_rasterization.densify import densify_stats

    return densify_stats(views["radii"], views["viewspace_points"], views["visibility_filter"], **state)


def test_module_imports_and_library_exports_the_call():
    from diff_gaussian_rasterization import _C, densify

    assert callable(densify.densify_stats) and callable(densify.update_states_fused)
    assert hasattr(_C.load_library(), "gsr_densify_stats")
    assert "gsr_densify_stats" in _C.SIGNATURES and "gsr_densify_batch" in _C.STRUCTS


def test_cpu_path_equals_direct_fp32_loop_bitwise():
    views = _views()
    assert not torch.equal(views["visibility_filter"][3], views["radii"][3] > 0)
    got = _stats(views)
    want = dc.loop_fp32(views)
    for g, w, name in zip(got, want, ("max", "sum", "count")):
        assert g.shape == (P,) and g.dtype == torch.float32
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=name)
    assert float(got[2].max()) == V and float(got[1].max()) > 0


def test_cpu_path_within_the_bound_of_an_fp64_sum():
    views = _views()
    got = _stats(views)[1].double().numpy()
    want = dc.sum_fp64(views)
    assert np.isfinite(want).all() and (want > 0).sum() > P // 2
    assert (np.abs(got - want) <= dc.bound(V) * want).all(), float(np.max(np.abs(got - want) / np.maximum(want, 1e-300)))


def test_cpu_path_against_the_reference_form():
    """torch.norm(grad[vis, :2], dim=-1) added per view by mask indexing, on DensifyModel's state."""
    views = _views()
    model = dr.DensifyModel(gs.make_scene(P, sh_degree=1, seed=8, radius=0.5), "cpu")
    model.max_radii2D = dc.reference_form(views, model.max_radii2D, model.xyz_gradient_accum, model.denom)
    m, s, c = _stats(views)
    assert torch.equal(m, model.max_radii2D) and torch.equal(c, model.denom[:, 0])
    want = dc.sum_fp64(views)
    ref = model.xyz_gradient_accum[:, 0].double().numpy()
    assert (np.abs(ref - want) <= dc.bound(V) * want).all()  # (the reference passes on its own)
    assert (np.abs(s.double().numpy() - ref) <= dc.bound(V) * ref).all()


def test_in_place_state_with_a_nan_in_the_running_maximum():
    """(P,1) and (P,) state that starts from non-zero values is continued in place; a NaN in the running maximum
    stays NaN, as torch.max keeps it."""
    views = _views()
    g = torch.Generator().manual_seed(5)
    m0 = torch.rand(P, generator=g) * 8
    m0[::17] = float("nan")
    s0, c0 = torch.rand(P, 1, generator=g) * 3, torch.randint(0, 4, (P, 1), generator=g).float()
    m, s, c = m0.clone(), s0.clone(), c0.clone()
    out = _stats(views, max_radii=m, grad_norm_sum=s, count=c)
    assert out[0] is m and out[1] is s and out[2] is c and s.shape == (P, 1) and c.shape == (P, 1)
    want = dc.loop_fp32(views, m0.numpy(), s0.numpy(), c0.numpy())
    for got, w in zip((m, s, c), want):
        np.testing.assert_array_equal(_bits(got), _bits(w))
    assert torch.isnan(m[::17]).all() and not torch.isnan(m).all()
    # torch.max, the reference's statement, agrees (NaN where it has NaN: its NaN's payload is its own)
    ref = m0.clone()
    for r in views["radii"]:
        ref = torch.max(ref, r.float())
    np.testing.assert_array_equal(m.numpy(), ref.numpy())
    # a state that is not contiguous fp32 is updated through a copy, with the same bits
    wide = torch.zeros(P, 2)
    wide[:, 0] = s0[:, 0]
    _stats(views, grad_norm_sum=wide[:, :1])
    np.testing.assert_array_equal(_bits(wide[:, 0]), _bits(want[1]))


def test_chained_calls_over_130_views_give_the_bits_of_one_loop():
    views = dc.make_views(130, 64, seed=2, none_at=(0, 63, 64, 100, 129))
    whole = _stats(views)
    m, s, c = torch.zeros(64), torch.zeros(64, 1), torch.zeros(64, 1)
    for lo in range(0, 130, 64):
        part = {k: v[lo:lo + 64] for k, v in views.items()}
        _stats(part, max_radii=m, grad_norm_sum=s, count=c)
    for got, w in zip((m, s, c), whole):
        np.testing.assert_array_equal(_bits(got), _bits(w))
    want = dc.sum_fp64(views)
    assert (np.abs(whole[1].double().numpy() - want) <= dc.bound(130) * want).all()


def test_empty_batches():
    from diff_gaussian_rasterization.densify import densify_stats

    m = torch.full((7,), 3.0)
    out = densify_stats([], [], None, max_radii=m)
    assert out[0] is m and float(m.min()) == 3.0 and torch.equal(out[1], torch.zeros(7))
    out = densify_stats([torch.zeros(0, dtype=torch.int32)], [None])
    assert all(t.shape == (0,) for t in out)
    with pytest.raises(ValueError):
        densify_stats([], [])
    with pytest.raises(ValueError):
        densify_stats([torch.zeros(4, dtype=torch.int32)], [None], max_radii=torch.zeros(5))


def _models():
    scene = gs.make_scene(P, sh_degree=1, seed=8, radius=0.5)
    # (split above the median extent, clone below it)
    cfg = dc.quiet_cfg(densify_grad_threshold=THRESHOLD,
                       split_thresh=float(np.median(np.linalg.norm(scene["scales"], axis=1))))
    return dr.DensifyModel(scene, "cpu", **cfg), dr.DensifyModel(scene, "cpu", **cfg)


def _outputs(lo=0, hi=6):
    return dc.make_views(hi - lo, P, seed=3, none_at=(2,), first=lo)


def test_update_states_fused_equals_update_states():
    from diff_gaussian_rasterization.densify import update_states_fused

    # an iteration that neither prunes nor densifies: the state
    ref, fused = _models()
    outs = _outputs()
    # (the reference needs a gradient in every view: its own restatement of a view without one)
    ref.max_radii2D = dc.reference_form(outs, ref.max_radii2D, ref.xyz_gradient_accum, ref.denom)
    ref.update_states(5, [], [], [])
    m_id = fused.max_radii2D.data_ptr()
    update_states_fused(fused, 5, outs)
    assert not fused.pruned_or_densified and fused.max_radii2D.data_ptr() == m_id  # in place
    assert torch.equal(fused.max_radii2D, ref.max_radii2D) and torch.equal(fused.denom, ref.denom)
    want = dc.sum_fp64(outs)
    for got in (ref.xyz_gradient_accum, fused.xyz_gradient_accum):
        assert (np.abs(got[:, 0].double().numpy() - want) <= dc.bound(6) * want).all()
    # no Gaussian's mean gradient norm lies within the bound of the threshold: the selections must agree exactly
    assert dc.borderline(ref.xyz_gradient_accum, ref.denom, THRESHOLD, 6) == 0
    sel_ref, sel_fused = dc.select_masks(ref, THRESHOLD), dc.select_masks(fused, THRESHOLD)
    assert all(torch.equal(a, b) for a, b in zip(sel_ref, sel_fused))
    assert int(sel_ref[0].sum()) > 0 and int(sel_ref[1].sum()) > 0  # both the clone and the split select something

    # the densify iteration, from those statistics: the same Gaussians afterwards (the same split samples)
    torch.manual_seed(11)
    ref.update_states(1000, [], [], [])
    torch.manual_seed(11)
    update_states_fused(fused, 1000, {"radii": [], "viewspace_points": [], "visibility_filter": []})
    assert ref.pruned_or_densified and fused.pruned_or_densified
    assert fused.get_xyz.shape[0] == ref.get_xyz.shape[0] == P + int(sel_ref[0].sum()) + int(sel_ref[1].sum())
    assert torch.equal(fused.get_xyz, ref.get_xyz)

    # both at once, as a training step calls it
    ref, fused = _models()
    ref.max_radii2D = dc.reference_form(outs, ref.max_radii2D, ref.xyz_gradient_accum, ref.denom)
    torch.manual_seed(12)
    ref.update_states(1000, [], [], [])
    torch.manual_seed(12)
    update_states_fused(fused, 1000, outs)
    assert fused.get_xyz.shape[0] == ref.get_xyz.shape[0] > P and torch.equal(fused.get_xyz, ref.get_xyz)


def test_update_states_fused_covers_the_early_returns():
    """geometry/gaussian_base.py:830-841: at the SuGaR prune and above max_num the statistics are not applied."""
    from diff_gaussian_rasterization.densify import update_states_fused

    scene = gs.make_scene(P, sh_degree=1, seed=8, radius=0.5)
    outs = _outputs()
    for cfg, it in ((dict(sugar_prune_at=7), 7), (dict(max_num=P - 100), 5)):
        ref = dr.DensifyModel(scene, "cpu", **dc.quiet_cfg(**cfg))
        fused = dr.DensifyModel(scene, "cpu", **dc.quiet_cfg(**cfg))
        full = {k: [x for i, x in enumerate(v) if i != 2] for k, v in outs.items()}  # (every view with a gradient)
        torch.manual_seed(4)
        ref.update_states(it, full["visibility_filter"], full["radii"], full["viewspace_points"])
        torch.manual_seed(4)
        update_states_fused(fused, it, full)
        assert ref.pruned_or_densified and fused.pruned_or_densified
        assert fused.get_xyz.shape[0] == ref.get_xyz.shape[0] < P
        assert torch.equal(fused.get_xyz, ref.get_xyz)
        for name in ("max_radii2D", "xyz_gradient_accum", "denom"):
            assert torch.equal(getattr(fused, name), getattr(ref, name)) and float(getattr(fused, name).sum()) == 0


def _worker(rank, world, tmp):
    from diff_gaussian_rasterization.densify import update_states_fused
    from diff_gaussian_rasterization.view_shard import replica_checksum, shard_range

    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "rendezvous"), rank=rank,
                            world_size=world)
    try:
        torch.manual_seed(100 + rank)  # the usual per-rank seeding
        lo, hi = shard_range(6, world, rank)
        outs = _outputs(lo, hi)
        quiet, dens = _models()
        update_states_fused(quiet, 5, outs)
        update_states_fused(dens, 1000, outs)
        same = replica_checksum(dens.parameters() + [dens.xyz_gradient_accum, dens.max_radii2D]) and \
            replica_checksum([quiet.max_radii2D, quiet.xyz_gradient_accum, quiet.denom])
        np.savez(os.path.join(tmp, f"rank{rank}.npz"), same=same, P=dens.get_xyz.shape[0],
                 xyz=dens.get_xyz.detach().numpy(), m=quiet.max_radii2D.numpy(), s=quiet.xyz_gradient_accum.numpy(),
                 c=quiet.denom.numpy())
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_stay_identical_and_match_world_one(tmp_path):
    from diff_gaussian_rasterization.densify import update_states_fused

    world = 2
    mp.spawn(_worker, args=(world, str(tmp_path)), nprocs=world, join=True)
    z = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    quiet, dens = _models()
    update_states_fused(quiet, 5, _outputs())
    assert dc.borderline(quiet.xyz_gradient_accum, quiet.denom, THRESHOLD, 6) == 0
    update_states_fused(dens, 1000, _outputs())
    assert bool(z[0]["same"]) and bool(z[1]["same"])
    np.testing.assert_array_equal(z[0]["xyz"], z[1]["xyz"])
    assert int(z[0]["P"]) == int(z[1]["P"]) == dens.get_xyz.shape[0] > P
    for r in range(world):
        np.testing.assert_array_equal(z[r]["m"], quiet.max_radii2D.numpy())
        np.testing.assert_array_equal(z[r]["c"], quiet.denom.numpy())
        want = quiet.xyz_gradient_accum.double().numpy()
        assert (np.abs(z[r]["s"] - want) <= dc.bound(6) * want).all()


def test_argument_errors_without_gpu():
    """Host-only library calls: every one fails its check before any device work (the pointers are never read)."""
    from diff_gaussian_rasterization import _C

    lib = _C.load_library()
    a = 16

    def call(V=3, P=10, radii=(a, a, a), visible=(None, None, None), **out):
        b = _C.DensifyBatch(V=V, P=P, accumulate=0, **dict(dict(max_radii=a, grad_norm_sum=a, count=a), **out))
        for k, (r, f) in enumerate(zip(radii, visible)):
            b.radii[k], b.grads[k], b.visible[k] = r, a, f
        rc = lib.gsr_densify_stats(ctypes.byref(b), None)
        return rc, lib.gsr_last_error()

    assert call(V=65) == (1, b"a densification call takes 0..64 views")
    assert call(V=-1)[0] == 1 and call(P=-1)[0] == 1
    rc, msg = call(radii=(a, None, a))
    assert rc == 1 and b"radii row" in msg
    rc, msg = call(visible=(a, None, a))
    assert rc == 1 and b"for every view or for none" in msg
    for name in ("max_radii", "grad_norm_sum", "count"):
        rc, msg = call(**{name: None})
        assert rc == 1 and name.encode() in msg
    assert lib.gsr_densify_stats(None, None) == 1
    # nothing to do: no launch, no error, whatever the pointers
    assert call(P=0) == (0, b"") and call(V=0) == (0, b"")
