"""sugar_field.neighbor_normal_loss / coarse_density_regulation (include/gsr.h gsr_sugar_normal_*, csrc/gsr_normal.hip)
on the GPU against an fp64 evaluation of the same formula.

The checker (`_normal` of tests/sugar_cases.py) is the reference's composition (utils/sugar_utils.py:726-757) in torch
with autograd, on the CPU, over the fp32-rounded inputs:
    s = sign(n_j . n_i),  a = |(x - c_j) . (s n_j)|,  w = op a / max(ms_j, 1e-6)^2,  W = sum_k w,
    wh = w / max(W, 1e-6),  r = n_i - sum_k wh s n_j,  loss = r . r,
with s, a and W detached (gradients reach the normals only), pairs whose index is out of range masked to 0 and the
loss of a sample whose own Gaussian is out of range 0.  The scene is that of tests/test_gpu_sugar_field.py (N = 2000
flat Gaussians + 100 unreferenced, M = 8192 samples, a quarter of them in Gaussian 7, the 32-NN table), normals = the
scene's smallest axes, op = the fp64 field rounded to fp32, upstream gradient = that scene's g_density.

Bar.  Per element of loss_normal and of dL/dnormals:  |gpu - ref64| <= 4 c0 2^-24 S.  S is the sum of the absolute
values of the element's per-pair terms: for dL/dnormals the terms |2 g wh_k s_k r| (to j) and |2 g r| (to i); for
the loss, linearised in r, S = 2 sum_c |r_c| (|n_i,c| + sum_k |wh_k s_k n_j,c|).  c0 is the largest such ratio of the
fp32 torch composition (`_normal` in float32, same inputs) against fp64 over the full scene at the case's K, measured
when the test runs and cached; the factor 4 covers another legitimate summation order.  Where S = 0 the result must be
exactly 0.

Excluded, by a condition on the fp64 reference and not by a measurement: a sample with a valid pair of
|n_i . n_j| < 1e-5 (the sign is a discrete decision there), or with W within 1e-3 relative of the 1e-6 clamp.  Their
loss is not compared and their upstream gradient is set to 0 on both sides.  The excluded share is asserted <= 1 %
(this scene: 0 samples by either rule; min |dot| ~ 6e-5, and 4-10 samples have W < 1e-6 at all).

The checker's arrangement.  Summed literally, r = n_i - sum_k wh s n_j cancels n_i against the sample's own slot
(j = i, s = 1, and in this scene, as in a trained one, wh_self = 1 - 1e-7 .. 1 - 1e-22): even in fp64 that leaves r
with an absolute error of 1e-16 |n_i| where the true r is 1e-21, i.e. no correct digit, and r = 0 (so S = 0) for
368 of the 8192 samples at K = 4 whose true r is not 0.  A reference without digits cannot hold anything to a bar, so
the fp64 checker sums the equal arrangement r = (1 - W / Wc) n_i + sum_k wh (n_i - s n_j) (1 - W / Wc exactly 0
when W >= 1e-6), whose own-slot term is exactly 0; autograd gives the same gradients (the coefficients of n_i sum to
1).  The fp32 null keeps the reference's literal order: it is the torch composition the bar is calibrated on.  S
keeps the formula's own terms as stated above.

Measured c0 (CPU, this scene), loss / dnormals:
    K = 1:   66 / 132           K = 4:   2.3e3 / 4.6e7
    K = 16:  2.3e3 / 1.7e7      K = 17:  2.3e3 / 2.3e6      K = 32:  2.3e3 / 4.8e6
(the loss's 2.3e3 is the fp32 cancellation of (x - c_j) . n_j; dnormals' millions are the literal order's
cancellation in r, every gradient term being proportional to r, and from 2^24 = 1.7e7 on also fp32 underflow: a
term below 2^-149 is held with an absolute error.  An fp32 emulation of the kernel's arithmetic on the CPU gives
0.9-2.5 for the loss and 2-71 for dnormals apart from those underflowing elements; each test prints the GPU's.)

The second bar for dL/dnormals (the one with teeth).  With c0 in the millions the stated bar is 1-11 x S: it admits a
gradient of zeros.  So dL/dnormals is also held, element by element, to a bound derived from the fp32 format alone,
for any evaluation in the arrangement above whose sums follow the orders of include/gsr.h.  u = 2^-24 bounds one
rounding; first order:
    w = op a / ms^2: 4 roundings (a from fp64, op a, ms^2, the division);  W: at most 32 more (any order of <= 32
    terms);  wh = w / Wc: 41;  coefficient 2 g wh s: 42;
    r_c = (1 - W / Wc) n_i,c + sum_k wh_k (n_i - s_k n_j)_c: each product 42 + 1 (the difference), the sum at most 33
    deep: d(r_c) <= 76 u T_c,  T_c = [W < 1e-6] (1 + W / Wc) |n_i,c| + sum_k wh_k |n_i - s_k n_j|_c
    (the clamp rule keeps 1 - W / Wc away from its own cancellation; T, not |r|: r may cancel between neighbours);
    a gradient term coefficient x r_c: (42 + 76 + 1) u |coefficient| T_c; a Gaussian's P terms are added in
    ceil(P / 16) + 6 steps at most (16 or 64 partials, then the butterfly):
    |gpu - ref64| <= (126 + P / 16) u S2,   S2 = sum over the Gaussian's terms of |coefficient| T_c  (>= S),
plus the format's absolute resolution where a product underflows: 2^-149 per rounding, carried through the divisions
by ms^2 and Wc (f_k = 2^-149 (1 + 1 / (ms_j^2 Wc)) on wh_k, hence on the coefficient and on r).  No constant in it is
measured.  `check` also asserts the teeth of this bar on every case whose reference gradient is not all zero: the
reference scaled by 0.5 and by 2, negated, and replaced by zeros must each fail it.

The K = 1 cases are nearly trivial, and are kept for the shapes: a Gaussian's nearest neighbour is itself, so r = 0
exactly unless W < 1e-6 (10 of the 8192 samples).  `test_residual_of_order_one` is the case where every sample's r
is O(1): random unit normals, neighbours drawn at random, weights of comparable size.
"""
import functools

import pytest

torch = pytest.importorskip("torch")

from sugar_cases import (EPS, M_FULL, N_EXTRA, N_REF, WMIN, _field, _mask, _normal, _ratios,  # noqa: E402
                         _scene)

DENORM = 2.0 ** -149  # the spacing of fp32 below 2^-126


@functools.lru_cache(maxsize=None)
def _extras():
    """normals (the scene's smallest axes, fp32-rounded, not exactly unit) and the fp64 field's opacities at K = 32."""
    sc = _scene()
    n = sc["centers"].shape[0]
    am = sc["scaling"].argmin(-1)
    normals = (sc["inv_sr"].double()[torch.arange(n), :, am] * sc["scaling"].double().min(-1)[0][:, None]).float()
    idx = sc["knn"][sc["gi"]]
    x, c, A, s, ms = (sc[k].double() for k in ("x", "centers", "inv_sr", "strengths", "min_scale"))
    op = _field(x, idx, _mask(idx, n), c, A, s, ms, 1.0)[0].float()
    return dict(normals=normals, op=op)


def _inputs(M=M_FULL, K=16):
    sc, ex = _scene(), _extras()
    inp = dict(x=sc["x"][:M], centers=sc["centers"], normals=ex["normals"], min_scale=sc["min_scale"],
               op=ex["op"][:M, :K].contiguous())
    own = sc["gi"][:M]
    return inp, own, sc["knn"][own][:, :K].contiguous(), sc["g_density"][:M]


class _Case:
    """A checker evaluation computed once: the exclusions, the reference values, S, and the null's c0."""

    def __init__(self, inp, idx, own, g):
        n = inp["centers"].shape[0]
        self.own_ok = (own >= 0) & (own < n)
        self.ok = _mask(idx, n, self.own_ok)
        probe = _normal(torch.float64, inp, idx, own, self.ok, self.own_ok, g)
        sign_risk = ((probe["dot"].abs() < 1e-5) & self.ok).any(-1)
        clamp_risk = ((probe["W"] - WMIN).abs() <= 1e-3 * WMIN) & self.own_ok
        self.excluded = sign_risk | clamp_risk
        self.g = torch.where(self.excluded, torch.zeros_like(g), g)  # excluded samples: no gradient on either side
        ref = _normal(torch.float64, inp, idx, own, self.ok, self.own_ok, self.g)
        self.ref = dict(loss=ref["loss"], dnormals=ref["dnormals"])
        # S from the per-pair terms; the hand-derived gradient must sum to autograd's
        okf, g64 = self.ok.double(), self.g.double()
        r, wh, s, nj, ni = ref["r"] * self.own_ok[:, None], ref["wh"], ref["s"], ref["nj"], ref["ni"]
        t_pair = -2 * g64[:, None, None] * (wh * s * okf)[..., None] * r[:, None]  # (M, K, 3) to j
        t_own = 2 * g64[:, None] * r  # (M, 3) to i

        def scatter(pair, own_t):
            out = torch.zeros(n, 3, dtype=torch.float64).index_add_(0, ref["j"].reshape(-1), pair.reshape(-1, 3))
            return out.index_add_(0, own.clamp(0, max(n - 1, 0)), own_t)

        S_r = ni.abs() + ((wh * s.abs() * okf)[..., None] * nj.abs()).sum(1)
        self.S = dict(loss=2 * (r.abs() * S_r).sum(-1), dnormals=scatter(t_pair.abs(), t_own.abs()))
        assert _ratios(scatter(t_pair, t_own), self.ref["dnormals"], self.S["dnormals"]) < 1e-3
        # the format-derived bar for dL/dnormals (module docstring)
        K, W = idx.shape[1], ref["W"]
        Wc = W.clamp(min=WMIN)
        whk = wh * okf
        diff = (ni[:, None] - s[..., None] * nj).abs()
        own_f = self.own_ok.double()
        T = (torch.where(W < WMIN, 1 + W / Wc, torch.zeros_like(W)))[:, None] * ni.abs() + (whk[..., None] * diff).sum(1)
        T = T * own_f[:, None]
        ga = 2 * g64.abs()
        S2 = scatter((ga[:, None] * whk)[..., None] * T[:, None], (ga * own_f)[:, None] * T)
        P = scatter(okf[..., None].expand(-1, -1, 3), own_f[:, None].expand(-1, 3))
        msc = inp["min_scale"].double()[ref["j"]].clamp(min=1e-6)
        f = DENORM * (1 + 1 / (msc ** 2 * Wc[:, None])) * okf
        R_abs = ((f[..., None] * diff).sum(1) + K * DENORM) * own_f[:, None]
        A = scatter((ga[:, None] * f + DENORM * okf)[..., None] * r.abs()[:, None]
                    + (ga[:, None] * whk)[..., None] * R_abs[:, None] + DENORM * okf[..., None],
                    (ga * own_f)[:, None] * R_abs + DENORM * own_f[:, None])
        self.bar2 = (126 + P / 16) * EPS * S2 + A
        null = _normal(torch.float32, inp, idx, own, self.ok, self.own_ok, self.g, literal=True)
        self.keep = dict(loss=~self.excluded, dnormals=torch.ones(n, dtype=torch.bool))
        self.c0 = {k: self.ratio(k, null[k]) for k in ("loss", "dnormals")}

    def ratio(self, k, got):
        keep = self.keep[k]
        return _ratios(got.cpu()[keep], self.ref[k][keep], self.S[k][keep])

    def check(self, got, c0, tag=""):
        assert float(self.excluded.double().mean()) <= 0.01 if len(self.excluded) else True
        worst = {}
        for k in ("loss", "dnormals"):
            assert got[k].dtype == torch.float32 and got[k].shape == self.ref[k].shape, (tag, k, got[k].shape)
            worst[k] = self.ratio(k, got[k])
            print(f"{tag} {k}: ratio {worst[k]:.4g}  c0 {c0[k]:.4g}  excluded {int(self.excluded.sum())}")
        for k, v in worst.items():
            assert v <= 4 * c0[k], (tag, k, v, c0[k])
        ref, err = self.ref["dnormals"], (got["dnormals"].cpu().double() - self.ref["dnormals"]).abs()
        print(f"{tag} dnormals, format bar: worst err / bar {float((err / self.bar2.clamp(min=1e-300)).max()):.4g}")
        assert self.within(got["dnormals"].cpu().double()), (tag, float((err / self.bar2.clamp(min=1e-300)).max()))
        if ref.any():  # the teeth: wrong gradients fail
            for wrong in (0.5 * ref, 2 * ref, -ref, torch.zeros_like(ref)):
                assert not self.within(wrong), tag

    def within(self, dnormals):
        return bool(((dnormals - self.ref["dnormals"]).abs() <= self.bar2).all())


@functools.lru_cache(maxsize=None)
def _full_case(K):
    inp, own, idx, g = _inputs(M_FULL, K)
    return _Case(inp, idx, own, g)


def _gpu(inp, g, *, own, knn_idx=None, closest_gaussians_idx=None, backwards=1):
    """neighbor_normal_loss on the GPU with its gradient (`backwards` times on one graph)."""
    from sugar_field import neighbor_normal_loss

    dev = {k: v.cuda() for k, v in inp.items()}
    nrm = dev["normals"].requires_grad_()
    index = dict(knn_idx=knn_idx, closest_gaussians_idx=closest_gaussians_idx)
    loss = neighbor_normal_loss(dev["x"], dev["centers"], nrm, dev["min_scale"], dev["op"], gaussian_idx=own.cuda(),
                                **{k: v.cuda() for k, v in index.items() if v is not None})
    grads = [torch.autograd.grad(loss, nrm, g.cuda(), retain_graph=b + 1 < backwards)[0] for b in range(backwards)]
    for other in grads[1:]:
        assert torch.equal(grads[0], other)
    return dict(loss=loss.detach(), dnormals=grads[0])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_full_scene_both_table_forms(K):
    """Also the hot Gaussian (number 7: more than 2000 terms at every K, its own 2048 samples alone) through the
    64-lane per-Gaussian sum: M (K + 1) >= 48 N only from K = 16 on, so K = 1 and 4 take the 16-lane one."""
    inp, own, idx, _ = _inputs(M_FULL, K)
    case = _full_case(K)
    a = _gpu(inp, case.g, own=own, closest_gaussians_idx=idx)
    case.check(a, case.c0, f"K={K}")
    assert not a["dnormals"][N_REF:].any()  # the Gaussians no row references: exactly zero
    b = _gpu(inp, case.g, own=own, knn_idx=_scene()["knn"][:, :K].contiguous())
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(1, 1), (17, 17), (0, 16)])
def test_smallest_shapes(M, K):
    """One sample; one past a 16-sample block with one slot past the 16 partials; none."""
    inp, own, idx, g = _inputs(M, K)
    case = _Case(inp, idx, own, g)
    got = _gpu(inp, case.g, own=own, closest_gaussians_idx=idx)
    assert got["loss"].shape == (M,) and got["dnormals"].shape == inp["normals"].shape
    if M == 0:
        assert not got["dnormals"].any()
        return
    case.check(got, _full_case(K).c0, f"M={M} K={K}")


@pytest.mark.gpu
def test_hot_gaussian_16_lane_sum():
    """M = 4096 at K = 16: M (K + 1) < 48 N, so the per-Gaussian sums use 16 lanes, and Gaussian 7 (2048 of the
    samples) has more than 4000 terms."""
    inp, own, idx, g = _inputs(4096, 16)
    n = inp["centers"].shape[0]
    assert 4096 * 17 < 48 * n and int((idx == 7).sum() + (own == 7).sum()) > 4000
    case = _Case(inp, idx, own, g)
    case.check(_gpu(inp, case.g, own=own, closest_gaussians_idx=idx), _full_case(16).c0, "hot, L=16")


@functools.lru_cache(maxsize=None)
def _order_one_case():
    """N = 64 Gaussians with random unit normals, M = 300 samples with K = 8 neighbours drawn at random (the own
    Gaussian among them or not), opacities and scales of order one: every weight matters and |r| is O(1)."""
    gen = torch.Generator().manual_seed(21)
    n, M, K = 64, 300, 8
    nrm = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    inp = dict(x=torch.randn(M, 3, generator=gen), centers=torch.randn(n, 3, generator=gen),
               normals=(nrm / nrm.norm(dim=-1, keepdim=True)).float(),
               min_scale=torch.rand(n, generator=gen) * 0.5 + 0.5, op=torch.rand(M, K, generator=gen) * 0.9 + 0.1)
    own = torch.randint(0, n, (M,), generator=gen)
    idx = torch.randint(0, n, (M, K), generator=gen)
    g = torch.randn(M, generator=gen)
    return inp, own, idx, _Case(inp, idx, own, g)


@pytest.mark.gpu
def test_residual_of_order_one():
    """Both bars where nothing cancels or underflows: the stated one against this case's own fp32 null (c0 of a few
    units), the format one, and the values themselves are O(1) (so a factor or a sign in either gradient term, or a
    dropped own term, shows)."""
    inp, own, idx, case = _order_one_case()
    assert float(case.ref["loss"].min()) > 1e-3 and float(case.ref["dnormals"].abs().max()) > 1
    assert max(case.c0.values()) < 1e3
    got = _gpu(inp, case.g, own=own, closest_gaussians_idx=idx)
    case.check(got, case.c0, "order one")
    rel = (got["dnormals"].cpu().double() - case.ref["dnormals"]).abs().max() / case.ref["dnormals"].abs().max()
    assert float(rel) < 1e-5  # far inside either bar's reach; plain to read
    # without the own terms, or with the neighbour terms doubled, the reference itself leaves the bar
    own_only = _Case(inp, torch.full_like(idx, -1), own, case.g).ref["dnormals"]
    assert not case.within(case.ref["dnormals"] - own_only) and not case.within(2 * case.ref["dnormals"] - own_only)


@pytest.mark.gpu
def test_indices_out_of_range():
    """-1 padding, indices >= N, and a gaussian_idx outside [0, N): the checker with these pairs masked."""
    inp, own, idx, g = _inputs(513, 16)
    n = inp["centers"].shape[0]
    table = _scene()["knn"][:, :16].clone()
    gen = torch.Generator().manual_seed(3)
    bad = torch.rand(table.shape, generator=gen) < 0.2
    junk = torch.tensor([n, n + 1, 2 ** 31, 2 ** 40, -1, -2 ** 40])[torch.randint(0, 6, table.shape, generator=gen)]
    table[bad] = junk[bad]
    table[:, 12:] = -1  # the padding of a short cloud
    own = own.clone()
    own[::7] = torch.tensor([-1, n, 2 ** 33, -2 ** 35])[torch.arange(len(own[::7])) % 4]
    own_ok = (own >= 0) & (own < n)
    idx = table[own.clamp(0, n - 1)]
    case = _Case(inp, idx, own, g)
    got = _gpu(inp, case.g, own=own, knn_idx=table)
    case.check(got, _full_case(16).c0, "out of range")
    assert not got["loss"][~own_ok].any() and not got["dnormals"][N_REF:].any()
    # the same through the per-sample form (its rows carry the bad indices)
    got2 = _gpu(inp, case.g, own=own, closest_gaussians_idx=idx)
    for k in got:
        assert torch.equal(got[k], got2[k]), k


@pytest.mark.gpu
def test_orthogonal_neighbour_contributes_nothing():
    """n_i = e_x with neighbours n_1 = e_y (sign 0: no weight, no gradient, bit-exactly) and n_2."""
    f = torch.float32
    base = dict(x=torch.tensor([[0.1, 0.2, 0.3]], dtype=f),
                centers=torch.tensor([[0., 0., 0.], [0.5, 0.1, 0.], [0.2, 0.4, 0.1]], dtype=f),
                normals=torch.tensor([[1., 0., 0.], [0., 1., 0.], [0.6, 0., 0.8]], dtype=f),
                min_scale=torch.tensor([0.1, 0.2, 0.3], dtype=f))
    own, g = torch.tensor([0]), torch.tensor([1.5], dtype=f)
    with_it = _gpu(dict(base, op=torch.tensor([[0.5, 0.9, 0.7]], dtype=f)), g, own=own,
                   closest_gaussians_idx=torch.tensor([[0, 1, 2]]))
    without = _gpu(dict(base, op=torch.tensor([[0.5, 0.7]], dtype=f)), g, own=own,
                   closest_gaussians_idx=torch.tensor([[0, 2]]))
    assert torch.equal(with_it["loss"], without["loss"]) and torch.equal(with_it["dnormals"], without["dnormals"])
    assert not with_it["dnormals"][1].any() and with_it["dnormals"][2].any() and with_it["loss"][0] > 0


@pytest.mark.gpu
def test_bitwise_repeatable():
    inp, own, idx, g = _inputs(M_FULL, 16)
    a = _gpu(inp, g, own=own, closest_gaussians_idx=idx, backwards=2)  # backward twice on one graph
    b = _gpu(inp, g, own=own, closest_gaussians_idx=idx)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# --------------------------------------------------------------------------- coarse_density_regulation


@pytest.mark.gpu
def test_coarse_density_regulation(monkeypatch):
    """End to end at N = 2100, n_samples = 8192, K = 16, against the fp64 restatement of utils/sugar_utils.py:683-759
    fed the same samples (drawn by the same seeded generator) and the same fp32 N-sized tensors (rotations, normals).
    Bars, per sample, then their mean plus 16 x 2^-24 of the mean for the fp32 mean itself:
      density_regulation |density - t|, t = exp(-u / 2), u = sdf^2 / beta^2: the density's and beta's bars of
        tests/test_gpu_sugar_field.py (4 c0 2^-24 S with that file's c0 at K = 16), and for the fp32 torch part
        d(sdf) <= 4 x 2^-24 sum_c |(x - p)_c n_c|, du <= 2 |sdf| d(sdf) / beta^2 + u (2 d(beta) / beta + 3 x 2^-24),
        dt <= t (du / 2 + 2 x 2^-24), plus 2^-24 (|density| + t) for the difference;
      normal_regulation: the loss bar above, and the opacities the kernel is fed: they are the fused field's, within
        rho = 4 c0_op 2^-24 relative of the fp64 ones (that file's floored c0; the floor's absolute part, 2^-126
        per pair, is below 1e-30 of any weight here), so dwh_k <= 2 rho wh_k and, in the form
        r = (1 - W / Wc) n_i + sum_k wh_k (n_i - s_k n_j),  dr_c <= P_c = 2 rho sum_k wh_k |n_i - s_k n_j|_c +
        rho [W < 1e-6] (W / Wc) |n_i,c|,  d(loss) <= 2 |r| . P + P . P."""
    import sugar_field
    from sugar_cases import _full_case as _field_full_case

    sc = _scene()
    g = torch.Generator().manual_seed(11)
    n, K, M = N_REF + N_EXTRA, 16, 8192
    quats = torch.randn(n, 4, generator=g)
    params = dict(points=sc["centers"], quaternions=quats, scaling=sc["scaling"],
                  strengths=sc["strengths"][:, None].contiguous())
    knn = sc["knn"][:, :K].contiguous().cuda()
    leaves = {k: v.cuda().requires_grad_() for k, v in params.items()}

    def gen():
        return torch.Generator(device="cuda").manual_seed(5)

    out = sugar_field.coarse_density_regulation(*leaves.values(), knn, n_samples=M, use_sdf_better_normal_loss=True,
                                                generator=gen())
    assert set(out) == {"density_regulation", "normal_regulation"}
    (out["density_regulation"] + out["normal_regulation"]).backward()
    for k, t in leaves.items():
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.any(), k

    # the same samples and the same fp32 N-sized tensors, then fp64
    with torch.no_grad():
        x, own = sugar_field.sample_points_in_gaussians(leaves["points"], leaves["quaternions"], leaves["scaling"], M,
                                                        1.5, probabilities_proportional_to_volume=False,
                                                        generator=gen())
        rot = sugar_field._quaternion_to_matrix(leaves["quaternions"])
        inv_sr = (rot * (1. / leaves["scaling"].clamp(min=1e-8))[:, None]).cpu()
        normals = sugar_field.smallest_axis(leaves["quaternions"], leaves["scaling"]).cpu()
    x, own = x.cpu(), own.cpu()
    idx = knn.cpu()[own]
    ok = _mask(idx, n)
    c64, A64, s64, ms64 = sc["centers"].double(), inv_sr.double(), sc["strengths"].double(), sc["min_scale"].double()
    op64, density, beta = _field(x.double(), idx, ok, c64, A64, s64, ms64, 1.0)
    ni = normals.double()[own]
    d = x.double() - c64[own]
    sdf = (d * ni).sum(-1)
    u = sdf ** 2 / beta ** 2
    t = torch.exp(-0.5 * u)
    want_density = (density - t).abs().mean()
    fc0 = _field_full_case(K).c0
    d_density = 4 * fc0["density"][1] * EPS * density
    d_beta = 4 * max(fc0["beta_avg"][1], 1.0) * EPS * beta
    d_sdf = 4 * EPS * (d * ni).abs().sum(-1)
    du = 2 * sdf.abs() * d_sdf / beta ** 2 + u * (2 * d_beta / beta + 3 * EPS)
    bar = (d_density + t * (du / 2 + 2 * EPS) + EPS * (density + t)).mean() + 16 * EPS * want_density
    err = abs(float(out["density_regulation"].detach()) - float(want_density))
    print(f"density_regulation {float(out['density_regulation'].detach()):.8g} want {float(want_density):.8g} "
          f"err {err:.3g} bar {float(bar):.3g}")
    assert err <= float(bar)

    inp = dict(x=x, centers=sc["centers"], normals=normals, min_scale=sc["min_scale"], op=op64.float())
    case = _Case(inp, idx, own, torch.ones(M))
    assert float(case.excluded.double().mean()) <= 0.01
    keep = ~case.excluded
    ref = _normal(torch.float64, dict(inp, op=op64), idx, own, ok, case.own_ok, case.g)
    rho = 4 * fc0["op"][1] * EPS
    diff = (ref["ni"][:, None] - ref["s"][..., None] * ref["nj"]).abs()
    W = ref["W"]
    P = 2 * rho * (ref["wh"][..., None] * diff).sum(1) + (rho * torch.where(W < WMIN, W / WMIN, 0 * W))[:, None] * \
        ref["ni"].abs()
    r = ref["r"].abs()
    per = 4 * _full_case(K).c0["loss"] * EPS * case.S["loss"] + 2 * (r * P).sum(-1) + (P * P).sum(-1)
    want_normal = ref["loss"].mean()
    # an excluded sample (a sign or the clamp may legitimately fall either way) moves the mean by at most its share
    slack = (ref["loss"][~keep].sum() + 4.01 * (~keep).sum()) / M  # |r| <= |n_i| + sum wh |n_j| <= 2
    bar = per[keep].sum() / M + slack + 16 * EPS * want_normal
    err = abs(float(out["normal_regulation"].detach()) - float(want_normal))
    print(f"normal_regulation {float(out['normal_regulation'].detach()):.8g} want {float(want_normal):.8g} "
          f"err {err:.3g} bar {float(bar):.3g} excluded {int((~keep).sum())}")
    assert err <= float(bar)

    # flag off: normal_regulation is 0 and the normal kernel is not launched
    def boom(*a, **k):
        raise AssertionError("neighbor_normal_loss called with the flag off")

    monkeypatch.setattr(sugar_field, "neighbor_normal_loss", boom)
    off = sugar_field.coarse_density_regulation(*leaves.values(), knn, n_samples=M, use_sdf_better_normal_loss=False,
                                                generator=gen())
    assert off["normal_regulation"] == 0
    assert torch.equal(off["density_regulation"], out["density_regulation"])
