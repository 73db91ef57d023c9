"""sugar_field.neighbor_density / get_field_values (include/gsr.h gsr_sugar_field_*, csrc/gsr_field.hip) on the GPU
against an fp64 evaluation of the same formula.

The checker (`_field` of tests/sugar_cases.py) is a short torch evaluation with autograd, on the CPU, over the
fp32-rounded inputs:
    d = x_m - c_j,  w = A_j^T d,  q = clamp(w.w, 0, 1e8),  op = density_factor s_j exp(-q / 2),
    density = sum_k op,  beta_avg = (sum_k min_scale_j) / K,
pairs whose index (or whose sample's row) is out of range masked to 0.  `_terms` restates every output element and
every gradient element as the sum of its per-pair terms, from the hand-derived gradient (asserted equal to autograd
on the CPU), and returns S, the sum of the absolute values of those terms.

Bars.  The scene (flat SuGaR-like Gaussians, 1/s up to ~1e3) amplifies fp32 rounding so that a flat
1e-4 max(1, |g|) bar is missed by plain fp32 torch on dL/dx and dL/dcenters; so each element is held to
    |gpu - ref64| <= c 2^-24 S,      c = 4 c0,
with c0 the largest such ratio of the fp32 torch composition of the same formula (`_field` in float32 on the CPU,
same inputs) against fp64, per output tensor, measured on the full scene (M = 8192) at the case's K when the test
runs (cached); the factor 4 covers another legitimate summation order and the device exp.  Where S = 0 the result must
be exactly 0.  No element is exempted.

Underflow.  A third of the scene's pairs have exp(-q / 2) below 2^-126, where fp32 holds it with an absolute error
(2^-150 = 2^-24 2^-126, or flushes it), not a relative one: against such a term alone the null's ratio is 2^24 and
says nothing about precision (c0 = 1.7e7 .. 4.5e7 on op and the three op-weighted per-Gaussian gradients).  So the
bar is asserted twice: as stated, and with S_floored, the same sum with every pair's exp(-q / 2) raised to at least
2^-126 (every term is linear in that factor or free of it), against its own c0.  The second is the one with teeth.

Measured c0 (CPU, this scene, all three upstream gradients), as stated / with S_floored:
    K = 1:   op 840  density 840  beta_avg 0  dx 2.5e5  dcenters 5.2e3  dinv_sr 2.4e3  dstrengths 140  dmin_scale 1.8
             (no underflowing pair matters: both forms agree)
    K = 4:   op 3.2e7 / 1.6e3  density 439  beta_avg 1.8  dx 2.1e5  dcenters 1.7e7 / 5.2e3  dinv_sr 1.7e7 / 2.4e3
             dstrengths 1.7e7 / 223  dmin_scale 2.0
    K = 16:  op 4.1e7 / 2.2e3  density 439  beta_avg 3.2  dx 2.1e5  dcenters 1.7e7 / 992  dinv_sr 1.7e7 / 495
             dstrengths 1.7e7 / 242  dmin_scale 2.7
    K = 32:  op 4.5e7 / 2.2e3  density 439  beta_avg 2.7  dx 2.1e5  dcenters 994  dinv_sr 497  dstrengths 124
             dmin_scale 2.3
    (the hundreds and thousands are the exponent's: a relative error r in q becomes q r / 2 in exp(-q / 2), with q
    up to 174 before underflow, and w = A^T d cancels from products of ~25 to ~1; dx's 2e5 comes from single elements
    where one pair's A dw nearly cancels, which S, a sum over pairs, does not see.)
"""
import math

import pytest

torch = pytest.importorskip("torch")

from sugar_cases import (EPS, M_FULL, N_REF, NAMES, _Case, _compose64, _field, _full_case, _inputs,  # noqa: E402
                         _mask, _scene, _terms)


def _gpu(inp, ups, df=1.0, want_op=True, **index):
    """neighbor_density on the GPU with gradients: dict by NAMES (op None without want_op)."""
    from sugar_field import neighbor_density

    leaves = [inp[k].cuda().requires_grad_() for k in ("x", "centers", "inv_sr", "strengths", "min_scale")]
    index = {k: v.cuda() for k, v in index.items()}
    den, beta, op = neighbor_density(*leaves, density_factor=df, return_opacities=want_op, **index)
    assert (op is None) == (not want_op)
    outs, gos = [], []
    for o, g in zip((op, den, beta), ups):
        if o is not None and g is not None:
            outs.append(o)
            gos.append(g.cuda())
    grads = torch.autograd.grad(outs, leaves, gos, allow_unused=True) if outs else [None] * 5
    res = dict(op=op, density=den, beta_avg=beta)
    res.update(zip(NAMES[3:], grads))
    return {k: (None if v is None else v.detach()) for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_full_scene(K):
    inp, gi, idx, ups = _inputs(M_FULL, K)
    case = _full_case(K)
    got = _gpu(inp, ups, closest_gaussians_idx=idx)
    case.check(got, case.c0, f"K={K}")
    for k in NAMES[4:]:  # the Gaussians no row references: exactly zero
        assert not got[k][N_REF:].any(), k


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_sample_counts(M):
    inp, gi, idx, ups = _inputs(M, 16)
    case = _Case(inp, idx, _mask(idx, inp["centers"].shape[0]), 1.0, ups)
    case.check(_gpu(inp, ups, closest_gaussians_idx=idx), _full_case(16).c0, f"M={M}")


@pytest.mark.gpu
def test_index_forms_give_the_same_bits():
    inp, gi, idx, ups = _inputs(M_FULL, 16)
    a = _gpu(inp, ups, closest_gaussians_idx=idx)
    b = _gpu(inp, ups, knn_idx=_scene()["knn"][:, :16].contiguous(), gaussian_idx=gi)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_upstream_gradient_alone(which):
    inp, gi, idx, ups = _inputs(1024, 16)
    ups = tuple(g if i == which else None for i, g in enumerate(ups))
    case = _Case(inp, idx, _mask(idx, inp["centers"].shape[0]), 1.0, ups)
    got = _gpu(inp, ups, closest_gaussians_idx=idx)
    case.check(got, _full_case(16).c0, f"upstream {which}")


@pytest.mark.gpu
def test_opacities_on_and_off_give_the_same_density_bits():
    inp, gi, idx, ups = _inputs(1024, 16)
    a = _gpu(inp, ups, closest_gaussians_idx=idx)
    b = _gpu(inp, (None,) + ups[1:], want_op=False, closest_gaussians_idx=idx)
    assert b["op"] is None
    assert torch.equal(a["density"], b["density"]) and torch.equal(a["beta_avg"], b["beta_avg"])


@pytest.mark.gpu
def test_density_factor():
    inp, gi, idx, ups = _inputs(257, 16)
    case = _Case(inp, idx, _mask(idx, inp["centers"].shape[0]), 2.5, ups)
    case.check(_gpu(inp, ups, df=2.5, closest_gaussians_idx=idx), _full_case(16).c0, "df=2.5")


@pytest.mark.gpu
def test_knn_padding_columns():
    """A 5-point cloud searched with K = 16: columns 5..15 of the table are knn_points' -1 padding."""
    from simple_knn import knn_points

    inp, gi, idx, ups = _inputs(300, 16)
    inp = {k: (v if k == "x" else v[:5].contiguous()) for k, v in inp.items()}
    table = knn_points(inp["centers"].cuda(), K=16).idx.cpu()
    assert (table[:, 5:] == -1).all() and (table[:, :5] >= 0).all()
    rows = gi % 5
    inp["x"] = (inp["centers"][rows] + 0.05 * (inp["x"] - _scene()["centers"][gi])).contiguous()
    idx = table[rows]
    case = _Case(inp, idx, _mask(idx, 5), 1.0, ups)
    got = _gpu(inp, ups, knn_idx=table, gaussian_idx=rows)
    case.check(got, _full_case(16).c0, "padding")
    assert not got["op"][:, 5:].any()


@pytest.mark.gpu
def test_indices_and_rows_out_of_range():
    inp, gi, idx, ups = _inputs(513, 16)
    n = inp["centers"].shape[0]
    table = _scene()["knn"][:, :16].clone()
    g = torch.Generator().manual_seed(3)
    bad = torch.rand(table.shape, generator=g) < 0.2
    junk = torch.tensor([n, n + 1, 2 ** 31, 2 ** 40, -1, -2 ** 40])[torch.randint(0, 6, table.shape, generator=g)]
    table[bad] = junk[bad]
    rows = gi.clone()
    rows[::7] = torch.tensor([-1, n, 2 ** 33, -2 ** 35])[torch.arange(len(rows[::7])) % 4]
    row_ok = (rows >= 0) & (rows < n)
    idx = table[rows.clamp(0, n - 1)]
    case = _Case(inp, idx, _mask(idx, n, row_ok), 1.0, ups)
    got = _gpu(inp, ups, knn_idx=table, gaussian_idx=rows)
    case.check(got, _full_case(16).c0, "out of range")
    for k in ("op", "density", "beta_avg", "dx"):
        assert not got[k][~row_ok].any(), k
    # the same through the gathered form (its table rows carry the bad indices; bad rows masked by hand)
    idx2 = torch.where(row_ok[:, None], idx, torch.full_like(idx, -1))
    got2 = _gpu(inp, ups, closest_gaussians_idx=idx2)
    for k in NAMES:
        assert torch.equal(got[k], got2[k]), k


@pytest.mark.gpu
def test_clamp_cuts_value_and_gradient():
    """A Gaussian of scale 1e-6 seen from 0.5 away: w.w = 2.5e11 > 1e8, so op = exp(-5e7) = 0 exactly and nothing
    flows; the second slot (an ordinary Gaussian) still does."""
    f = torch.float32
    centers = torch.tensor([[0., 0., 0.], [0.4, 0.1, 0.]], dtype=f)
    inv_sr = torch.stack([torch.eye(3) * 1e6, torch.eye(3) * 2.0]).to(f)
    inp = dict(x=torch.tensor([[0.5, 0., 0.]], dtype=f), centers=centers, inv_sr=inv_sr,
               strengths=torch.tensor([0.9, 0.8], dtype=f), min_scale=torch.tensor([1e-6, 0.5], dtype=f))
    idx = torch.tensor([[0, 1]])
    ups = (torch.tensor([[1.5, -0.5]], dtype=f), torch.tensor([2.0], dtype=f), None)
    got = _gpu(inp, ups, closest_gaussians_idx=idx)
    assert got["op"][0, 0] == 0 and got["op"][0, 1] > 0
    for k in ("dcenters", "dinv_sr", "dstrengths"):
        assert not got[k][0].any() and got[k][1].any(), k
    assert all(torch.isfinite(v).all() for v in got.values() if v is not None)
    _Case(inp, idx, _mask(idx, 2), 1.0, ups).check(got, _full_case(16).c0, "clamp")
    # overflow of w.w itself (scale 1e-30 -> inf): still 0, still finite gradients
    inp["inv_sr"] = torch.stack([torch.eye(3) * 1e30, torch.eye(3) * 2.0]).to(f)
    got = _gpu(inp, ups, closest_gaussians_idx=idx)
    assert got["op"][0, 0] == 0 and all(torch.isfinite(v).all() for v in got.values() if v is not None)
    assert not got["dinv_sr"][0].any() and not got["dcenters"][0].any()


@pytest.mark.gpu
def test_bitwise_repeatable():
    inp, gi, idx, ups = _inputs(M_FULL, 16)
    a = _gpu(inp, ups, closest_gaussians_idx=idx)
    b = _gpu(inp, ups, closest_gaussians_idx=idx)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_no_samples():
    inp, gi, idx, ups = _inputs(0, 16)
    got = _gpu(inp, ups, closest_gaussians_idx=idx)
    assert got["op"].shape == (0, 16) and got["density"].shape == (0,) and got["dx"].shape == (0, 3)
    for k in NAMES[4:]:
        assert got[k].shape == inp[{"dcenters": "centers", "dinv_sr": "inv_sr", "dstrengths": "strengths",
                                    "dmin_scale": "min_scale"}[k]].shape and not got[k].any(), k


@pytest.mark.gpu
def test_non_default_stream():
    inp, gi, idx, ups = _inputs(1024, 16)
    want = _gpu(inp, ups, closest_gaussians_idx=idx)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _gpu(inp, ups, closest_gaussians_idx=idx)
    side.synchronize()
    for k in NAMES:
        assert torch.equal(want[k], got[k]), k


# ---------------------------------------------------------------------------------- get_field_values


def _fields_inputs():
    """513 samples of the scene at K = 16; row 0 sits on Gaussian 7's centre with every neighbour's strength
    raised so that density >= 1 there, and row 1 is moved far away so that all its opacities are exactly 0."""
    inp, gi, idx, ups = _inputs(513, 16)
    inp = dict(inp)
    x = inp["x"].clone()
    x[0] = inp["centers"][7]
    x[1] = torch.tensor([50., 50., 50.])
    inp["x"] = x
    return inp, gi, idx


@pytest.mark.gpu
@pytest.mark.parametrize("return_sdf", [True, False])
@pytest.mark.parametrize("mode", ["average", "weighted_average", "learnable"])
def test_get_field_values(mode, return_sdf):
    """density, closest_gaussian_opacities and the average beta are the fused op's outputs: the c-bars above.  The
    rest is fp32 torch on those outputs, so it is compared with the same composition in fp64 applied to (a) the
    checker's fp64 outputs, with the fused outputs' bars propagated, which reduces to: (b) the fp64 composition of
    the GPU's own fp32 outputs, at the bar of the fp32 format.  With t = sqrt(-2 ln d), an error of u = 4 x 2^-24
    relative in d (the division, the log, the product, the root) moves t by min(u / t, sqrt(2 u)) + u t; beta's
    weighted average is a convex combination (relative error <= (K + 3) 2^-24); sdf = beta (t - t0)."""
    from sugar_field import get_field_values

    inp, gi, idx = _fields_inputs()
    n = inp["centers"].shape[0]
    strengths = inp["strengths"].clone()
    strengths[_scene()["knn"][7, :16]] = 1.0
    inp["strengths"] = strengths
    sc = _scene()
    log_beta = torch.tensor([-3.0])
    case = _Case(inp, idx, _mask(idx, n), 1.0, (None, None, None))
    dev = {k: v.cuda() for k, v in inp.items()}
    fields = get_field_values(
        dev["x"], points=dev["centers"], inv_scaled_rotation=dev["inv_sr"], strengths=dev["strengths"][:, None],
        scaling=sc["scaling"].cuda(), knn_idx=sc["knn"][:, :16].contiguous().cuda(), gaussian_idx=gi.cuda(),
        beta_mode=mode, log_beta=log_beta.cuda(), return_sdf=return_sdf, density_threshold=0.7,
        return_closest_gaussian_opacities=True, return_beta=True)
    assert set(fields) == {"density", "closest_gaussian_opacities", "beta"} | ({"sdf"} if return_sdf else set())
    c0 = _full_case(16).c0
    got = dict(density=fields["density"], op=fields["closest_gaussian_opacities"])
    if mode == "average":
        got["beta_avg"] = fields["beta"]
    case.check({k: v.detach() for k, v in got.items()}, c0, mode)
    d32, op32 = fields["density"].detach().cpu(), fields["closest_gaussian_opacities"].detach().cpu()
    assert (d32 >= 1).any() and not op32[1].any()  # the normalised rows and the beta fill path are exercised
    ms_nb = inp["min_scale"].double()[idx]
    beta_avg64 = ms_nb.sum(-1) / 16
    dens, beta, t, sdf = _compose64(d32.double(), op32.double(), beta_avg64, ms_nb, mode, log_beta, 0.7, 1e-16)
    u = 4 * EPS
    rel_beta = 19 * EPS if mode == "weighted_average" else (4 * c0["beta_avg"][1] * EPS if mode == "average" else 4 * EPS)
    b32 = fields["beta"].detach().cpu().double()
    assert ((b32 - beta).abs() <= rel_beta * beta.abs()).all()
    if mode == "weighted_average":
        assert b32[1] == ms_nb.max().float().double()
    if return_sdf:
        dt = torch.minimum(u / t.clamp(min=1e-300), torch.full_like(t, math.sqrt(2 * u))) + u * t
        t0 = math.sqrt(-2. * math.log(0.7))
        bar = beta.abs() * (dt + u * t0) + rel_beta * beta.abs() * (t - t0).abs() + u * sdf.abs()
        err = (fields["sdf"].detach().cpu().double() - sdf).abs()
        print(f"{mode} sdf: worst err / bar {float((err / bar).max()):.3g}")
        assert (err <= bar).all()


@pytest.mark.gpu
def test_get_field_values_gradients_flow():
    from sugar_field import get_field_values

    inp, gi, idx = _fields_inputs()
    sc = _scene()
    leaves = {k: inp[k].cuda().requires_grad_() for k in ("x", "centers", "inv_sr", "strengths")}
    scaling = sc["scaling"].cuda().requires_grad_()
    fields = get_field_values(leaves["x"], points=leaves["centers"], inv_scaled_rotation=leaves["inv_sr"],
                              strengths=leaves["strengths"], scaling=scaling, closest_gaussians_idx=idx.cuda(),
                              beta_mode="average", return_sdf=True)
    fields["sdf"][2:].abs().mean().backward()
    for t in (*leaves.values(), scaling):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.any()
