"""What more than one SuGaR test module uses: the meshes, quaternions, error measure, bar (``check_against_null``) and
case skeleton (``NullCase``, ``backprop``) of the geometry stages, and the scene, restatements and checker of the
neighbour density field and normal loss (tests/test_gpu_sugar_field.py and tests/test_gpu_sugar_normal.py describe
their bars).  No tests here: the test modules import from this one and not from each other."""
import functools
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402

D = torch.float64


def _rel(a, b):
    scale = float(b.double().abs().max()) if b.numel() else 0.0
    return float((a.double() - b.double()).abs().max()) / scale if scale > 0 else 0.0


def check_against_null(got, ref64, null32, keys, tag, *, null_ref=None, note=""):
    """The bar of the geometry stages, stated once (tests/test_null_bar.py holds it to its word).  Per tensor:
    float32, the reference's shape, and max |got - ref64| / max |ref64| <= 2 x the same figure of the fp32 null (which
    is measured against null_ref where that is not ref64); where the reference is all zero, exactly zero.  Prints both
    figures."""
    null_ref = ref64 if null_ref is None else null_ref
    for k in keys:
        assert got[k].dtype == torch.float32 and got[k].shape == ref64[k].shape, (tag, k, got[k].shape)
        err, bar = _rel(got[k], ref64[k]), 2 * _rel(null32[k], null_ref[k])
        print(f"{tag} {k}: gpu {err:.3g}  fp32 null {bar / 2:.3g}{note}")
        if not ref64[k].any():
            assert not got[k].any(), (tag, k)  # nothing contributes: exactly zero
        else:
            assert torch.isfinite(got[k]).all() and err <= bar, (tag, k, err, bar)


# ---- the fixtures computed by the reference's own code (tests/golden/reference_*.npz, made by make_golden*.py) -------
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OUT_BAR, GRAD_BAR = 1e-12, 1e-10


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, f"reference_{name}.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def close(got, want, bar, tag):
    assert got.dtype == want.dtype == D and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    err = _rel(got, want)
    print(f"{tag}: {err:.3g} (bar {bar:g})")
    if not want.any():
        assert not got.any(), tag
    else:
        assert err <= bar, (tag, err, bar)


def null_is_usable(z, prefix, keys):
    """Every float32 tensor is finite, and differs from the float64 one (so 2 x the null is a bar, not zero), unless
    the float64 tensor is all zero (then the GPU must give exact zeros)."""
    for k in keys:
        a, b = z[f"{prefix}{k}_f32"], z[f"{prefix}{k}_f64"]
        assert a.dtype == torch.float32 and b.dtype == D and a.shape == b.shape, (prefix, k)
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (prefix, k)
        assert _rel(a, b) > 0 or not b.any(), (prefix, k)


def backprop(out, out_names, leaves, grad_names, ups, which):
    """`got` of a stage called on the GPU: its outputs by name and, under grad_names, the gradients of
    sum((o * up).sum()) over the outputs named in `which`.  Outputs and leaves that are None are left out."""
    loss = sum((o * ups[k].cuda()).sum() for k, o in zip(out_names, out) if k in which)
    have = [(k, t) for k, t in zip(grad_names, leaves) if t is not None]
    grads = torch.autograd.grad(loss, [t for _, t in have])
    got = {k: o.detach().cpu() for k, o in zip(out_names, out) if o is not None}
    got.update({k: g.cpu() for (k, _), g in zip(have, grads)})
    return got


class NullCase:
    """What the cases of the geometry stages share.  A case draws its inputs, `ups` (the upstream gradients by output
    name) and `keys` (what is compared), and has evaluate(dtype, ups), its reference, and gpu(which), its stage."""

    outputs = property(lambda self: tuple(self.ups))

    def references(self, ups):
        return tuple(self.evaluate(dt, ups) for dt in (torch.float64, torch.float32))

    def reference(self, which):
        """The fp64 reference and the fp32 null for the upstream gradients named in `which`, computed once."""
        refs = self.__dict__.setdefault("_refs", {})
        if which not in refs:
            refs[which] = self.references({k: self.ups[k] for k in which})
        return refs[which]

    def check(self, got, which=None, tag=""):
        check_against_null(got, *self.reference(self.outputs if which is None else tuple(which)), self.keys, tag)


def _fan(n=200):
    """n faces around vertex 0 (a closed, slightly crumpled fan) and one extra vertex no face uses."""
    ang = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7 * ang)], 1)
    verts = np.concatenate([[[0.0, 0.0, 0.3]], ring, [[2.0, 2.0, 2.0]]])
    faces = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    return verts, faces


def random_quats(gen, shape, dtype=torch.float32, max_angle=2.6, identity_every=7):
    """(x, y, z, w) quaternions: rotation angles within +-max_angle, both signs of w, norms in [0.5, 1.5], every
    identity_every-th row exactly the identity."""
    axis = torch.nn.functional.normalize(torch.randn(*shape, 3, generator=gen, dtype=D), dim=-1)
    ang = (torch.rand(*shape, 1, generator=gen, dtype=D) * 2 - 1) * max_angle
    q = torch.cat([axis * torch.sin(ang / 2), torch.cos(ang / 2)], -1)
    sign = torch.where(torch.rand(*shape, 1, generator=gen) < 0.5, -1.0, 1.0).to(D)
    q = q * sign * (0.5 + torch.rand(*shape, 1, generator=gen, dtype=D))
    if identity_every:
        q.view(-1, 4)[::identity_every] = torch.tensor([0., 0., 0., 1.], dtype=D)
    return q.to(dtype).contiguous()


TRIANGLE = ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.5, 0.4, 0.1]], [[0, 1, 2]])  # obtuse at vertex 0
TETRAHEDRON = ([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.8, 0.4, 0.0], [0.1, 0.4, 1.0]],  # closed; obtuse at vertex 0
               [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])


def jittered_icosphere(subdiv, amount=0.45, seed=0):
    """The icosphere with its vertices moved by `amount` of the mean edge length: some corners become obtuse."""
    v, f = gs.icosphere(subdiv)
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    return v + amount * edge * np.random.default_rng(seed).uniform(-1, 1, v.shape), f


def open_fan(n=7):
    """n faces around vertex 0 that do not close: the rim's two ends have valence 2.  Every other rim vertex is pulled
    in, so the corners there are obtuse."""
    ang = np.arange(n + 1) * 0.5
    rad = 1.0 - 0.6 * (np.arange(n + 1) % 2)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.2 * np.sin(3 * ang)], 1)
    return np.concatenate([[[0.0, 0.0, 0.3]], ring]), np.stack([np.zeros(n, np.int64), 1 + np.arange(n),
                                                                2 + np.arange(n)], 1)


def isolated_and_degenerate():
    """A jittered icosphere(0), vertex 12 in no face, and a collinear (zero-area) face on three vertices of its own."""
    v, f = jittered_icosphere(0, seed=3)
    extra = [[2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [1.01, 1.0, 1.0], [1.02, 1.0, 1.0]]
    return np.concatenate([v, extra]), np.concatenate([f, [[13, 14, 15]]])


MESHES = {"triangle": lambda: TRIANGLE, "tetrahedron": lambda: TETRAHEDRON,
          "icosphere1": lambda: jittered_icosphere(1), "open_fan": open_fan, "fan200": lambda: _fan(200),
          "isolated_degenerate": isolated_and_degenerate}


def mesh(name):
    v, f = MESHES[name]()
    return torch.as_tensor(np.asarray(v), dtype=torch.float32), torch.as_tensor(np.asarray(f), dtype=torch.int64)


# ---- the neighbour density field -------------------------------------------------------------------------------------
EPS = 2.0 ** -24
N_REF, N_EXTRA, M_FULL = 2000, 100, 8192
NAMES = ("op", "density", "beta_avg", "dx", "dcenters", "dinv_sr", "dstrengths", "dmin_scale")


def _quat_to_matrix(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def _scene():
    """N = 2000 flat Gaussians + 100 that no table row references; M = 8192 samples, a quarter of them drawn in
    Gaussian 7; the exact 32-NN table (its first K columns are the K-NN); upstream gradients.  fp32 tensors."""
    g = torch.Generator().manual_seed(0)
    f64 = dict(dtype=torch.float64, generator=g)
    n = N_REF + N_EXTRA
    c = torch.rand(n, 3, **f64) * 2 - 1
    sc = torch.exp(torch.randn(n, 3, **f64) * 0.5) * 0.08
    sc[:, 2] *= 0.05
    rot = _quat_to_matrix(torch.randn(n, 4, **f64))
    s = torch.sigmoid(torch.randn(n, **f64) * 2)
    knn = torch.cdist(c, c[:N_REF]).topk(32, largest=False).indices  # every row lists referenced Gaussians only
    gi = torch.randint(0, N_REF, (M_FULL,), generator=g)
    gi[:M_FULL // 4] = 7
    x = c[gi] + (rot[gi] @ (1.5 * sc[gi] * torch.randn(M_FULL, 3, **f64))[..., None])[..., 0]
    A = rot * (1 / sc.clamp(min=1e-8))[:, None]
    out = dict(x=x.float(), centers=c.float(), inv_sr=A.float(), strengths=s.float(), min_scale=sc.min(-1)[0].float(),
               scaling=sc.float(), knn=knn, gi=gi, g_op=torch.randn(M_FULL, 32, **f64).float(),
               g_density=torch.randn(M_FULL, **f64).float(), g_beta=torch.randn(M_FULL, **f64).float())
    cnt = torch.bincount(knn[gi][:, :16].reshape(-1), minlength=n)
    assert cnt.max() > 2000 and (cnt[N_REF:] == 0).all()
    return out


def _mask(idx, n, row_ok=None):
    ok = (idx >= 0) & (idx < n)
    return ok if row_ok is None else ok & row_ok[:, None]


def _field(x, idx, ok, c, A, s, ms, df):
    """op, density, beta_avg in the dtype of the inputs (the reference's composition; masked pairs contribute 0)."""
    j = idx.clamp(0, max(c.shape[0] - 1, 0))
    shift = x[:, None] - c[j]
    warped = (A[j].transpose(-1, -2) @ shift[..., None])[..., 0]
    q = (warped * warped).sum(-1).clamp(min=0., max=1e8)
    op = df * s[j] * torch.exp(-0.5 * q) * ok
    return op, op.sum(-1), (ms[j] * ok).sum(-1) / idx.shape[1]


def _run(dtype, inp, idx, ok, df, ups):
    """Outputs and gradients (NAMES order) of `_field` in `dtype` for the upstream gradients ups = (g_op, g_density,
    g_beta), any None."""
    leaves = [inp[k].to(dtype).clone().requires_grad_() for k in ("x", "centers", "inv_sr", "strengths", "min_scale")]
    op, den, beta = _field(leaves[0], idx, ok, *leaves[1:], df)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip((op, den, beta), ups) if g is not None)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True) if torch.is_tensor(loss) else [None] * 5
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    return [t.detach() for t in (op, den, beta, *grads)]


TINY = 2.0 ** -126  # the smallest normal fp32


def _terms(inp, idx, ok, df, ups):
    """fp64: (sum, S, S_floored) per NAMES entry from the per-pair terms of the hand-derived gradient.  S_floored
    is S with every pair's exp(-q / 2) raised to at least 2^-126 (every term is linear in it, or free of it)."""
    x, c, A, s, ms = (inp[k].double() for k in ("x", "centers", "inv_sr", "strengths", "min_scale"))
    n, (M, K) = c.shape[0], idx.shape
    g_op, g_den, g_beta = (None if g is None else g.double() for g in ups)
    j = idx.clamp(0, max(n - 1, 0))
    okf = ok.double()
    d = x[:, None] - c[j]
    w = torch.einsum("mkai,mka->mki", A[j], d)
    qr = (w * w).sum(-1)
    dop = torch.zeros(M, K, dtype=torch.float64)
    if g_op is not None:
        dop = dop + g_op
    if g_den is not None:
        dop = dop + g_den[:, None]
    t_ms = (torch.zeros(M, K, dtype=torch.float64) if g_beta is None else (g_beta[:, None] / K).expand(M, K)) * okf

    def scatter(t):
        flat = t.reshape(M * K, -1)
        return torch.zeros(n, flat.shape[1], dtype=torch.float64).index_add_(0, j.reshape(-1), flat)

    def pair_terms(e):
        op = df * s[j] * e
        dw = -w * (dop * op * (qr <= 1e8))[..., None]
        dd = torch.einsum("mkai,mki->mka", A[j], dw)
        return dict(op=op, dd=dd, t_A=d[..., :, None] * dw[..., None, :], t_s=dop * df * e)

    def sums(t, absolute):
        f = (lambda v: v.abs()) if absolute else (lambda v: v)
        return dict(op=f(t["op"]), density=f(t["op"]).sum(-1), beta_avg=f(ms[j] * okf).sum(-1) / K,
                    dx=f(t["dd"]).sum(1), dcenters=scatter(f(-t["dd"])).reshape(n, 3),
                    dinv_sr=scatter(f(t["t_A"])).reshape(n, 3, 3), dstrengths=scatter(f(t["t_s"])).reshape(n),
                    dmin_scale=scatter(f(t_ms)).reshape(n))

    e = torch.exp(-0.5 * qr.clamp(0, 1e8)) * okf
    exact = pair_terms(e)
    tot, S, Sf = sums(exact, False), sums(exact, True), sums(pair_terms(e.clamp(min=TINY) * okf), True)
    return {k: (tot[k], S[k], Sf[k]) for k in NAMES}


def _ratios(got, ref, S):
    """max over elements of |got - ref| / (2^-24 S); an element with S = 0 must be exact (ratio 0, else inf)."""
    err = (got.double() - ref).abs()
    r = torch.where(S > 0, err / (EPS * S.clamp(min=1e-300)), torch.where(err == 0, 0.0, math.inf))
    return float(r.max()) if r.numel() else 0.0


class _Case:
    """A checker evaluation computed once: reference values, S, and the null's c0 per tensor."""

    def __init__(self, inp, idx, ok, df, ups):
        self.ref = dict(zip(NAMES, _run(torch.float64, inp, idx, ok, df, ups)))
        self.terms = _terms(inp, idx, ok, df, ups)
        for k in NAMES:  # the hand-derived terms sum to what autograd gives
            tot, S, _ = self.terms[k]
            assert _ratios(tot, self.ref[k], S) < 1e-3, k
        null = dict(zip(NAMES, _run(torch.float32, inp, idx, ok, df, ups)))
        self.c0 = {k: tuple(_ratios(null[k], self.ref[k], self.terms[k][i]) for i in (1, 2)) for k in NAMES}

    def check(self, got, c0, tag=""):
        worst = {}
        for k, t in got.items():
            if t is None:
                continue
            assert t.dtype == torch.float32 and t.shape == self.ref[k].shape, (tag, k, t.shape)
            worst[k] = tuple(_ratios(t.cpu(), self.ref[k], self.terms[k][i]) for i in (1, 2))
            print(f"{tag} {k}: ratio {worst[k][0]:.4g} (floored S: {worst[k][1]:.4g})  "
                  f"c0 {c0[k][0]:.4g} (floored S: {c0[k][1]:.4g})")
        for k, r in worst.items():
            assert r[0] <= 4 * c0[k][0] and r[1] <= 4 * c0[k][1], (tag, k, r, c0[k])


def _inputs(M=M_FULL, K=16):
    sc = _scene()
    inp = {k: sc[k] for k in ("centers", "inv_sr", "strengths", "min_scale")}
    inp["x"] = sc["x"][:M]
    gi = sc["gi"][:M]
    idx = sc["knn"][gi][:, :K].contiguous()
    ups = (sc["g_op"][:M, :K].contiguous(), sc["g_density"][:M], sc["g_beta"][:M])
    return inp, gi, idx, ups


@functools.lru_cache(maxsize=None)
def _full_case(K):
    inp, gi, idx, ups = _inputs(M_FULL, K)
    return _Case(inp, idx, _mask(idx, inp["centers"].shape[0]), 1.0, ups)


def _compose64(density, op, beta_avg, ms_nb, mode, log_beta, threshold, clampv):
    """The reference's remainder (utils/sugar_utils.py:313-341, 417-471) in fp64 from fp64 density / op / beta_avg."""
    dens = density.clone()
    m = dens >= 1.
    dens[m] = dens[m] / (dens[m] + 1e-12)
    if mode == "learnable":
        beta = torch.exp(log_beta.double()).expand(len(density))
    elif mode == "average":
        beta = beta_avg
    else:
        osum = op.sum(-1, keepdim=True)
        beta = (ms_nb * (op / osum.clamp(min=clampv))).sum(-1)
        beta[osum[..., 0] == 0.] = ms_nb.max()
    t = torch.sqrt(-2. * torch.log(dens.clamp(min=clampv)))
    return dens, beta, t, beta * (t - math.sqrt(-2. * math.log(min(threshold, 1.))))


FIELD_RUNS = {"a": ("average", 1.0, True, True), "w": ("weighted_average", 1.3, True, True),
              "l": ("learnable", 1.0, False, False)}  # beta_mode, density_factor, return_sdf, opacities returned
FIELD_LEAVES = ("x", "points", "inv_sr", "strengths", "scaling", "log_beta")


def field_keys(run, grads=True):
    mode, df, sdf_on, want_op = FIELD_RUNS[run]
    keys = ("density", "beta") + (("sdf",) if sdf_on else ()) + (("closest_gaussian_opacities",) if want_op else ())
    return keys + (tuple("d" + k for k in FIELD_LEAVES) if grads and run != "a" else ())


# ---- the neighbour-normal loss ---------------------------------------------------------------------------------------
WMIN = 1e-6


def _normal(dtype, inp, idx, own, ok, own_ok, g, literal=False):
    """loss (M,), dL/dnormals (N, 3), and the intermediates, of the reference's composition in `dtype`.  `literal`:
    r summed as the reference writes it, n_i - sum_k wh s n_j (the fp32 null); otherwise in the equal arrangement
    (1 - W / Wc) n_i + sum_k wh (n_i - s n_j), which does not cancel n_i against the sample's own slot (the fp64
    checker: see the docstring of tests/test_gpu_sugar_normal.py)."""
    x, c, ms, op = (inp[k].to(dtype) for k in ("x", "centers", "min_scale", "op"))
    nrm = inp["normals"].to(dtype).clone().requires_grad_()
    n = c.shape[0]
    j = idx.clamp(0, max(n - 1, 0))
    ni = nrm[own.clamp(0, max(n - 1, 0))]
    nj = nrm[j]
    dot = (nj * ni[:, None]).sum(dim=-1, keepdim=True)
    njs = nj * torch.sign(dot).detach()
    a = ((x[:, None] - c[j]) * njs).sum(dim=-1).abs().detach()
    w = op * a / ms[j].clamp(min=1e-6) ** 2 * ok
    W = w.sum(dim=-1).detach()
    wh = w / W.unsqueeze(-1).clamp(min=WMIN)
    if literal:
        r = ni - (wh[..., None] * njs).sum(dim=-2)
    else:
        rest = torch.where(W >= WMIN, torch.zeros_like(W), 1 - W / W.clamp(min=WMIN))
        r = rest[:, None] * ni + (wh[..., None] * (ni[:, None] - njs)).sum(dim=-2)
    loss = r.pow(2).sum(dim=-1) * own_ok
    grad, = torch.autograd.grad((loss * g.to(dtype)).sum(), nrm) if len(loss) else (torch.zeros_like(nrm),)
    return dict(loss=loss.detach(), dnormals=grad, r=r.detach(), wh=wh.detach(), s=torch.sign(dot).detach()[..., 0],
                dot=dot.detach()[..., 0], W=W, nj=nj.detach(), ni=ni.detach(), j=j)
