"""What more than one SuGaR test module uses: the meshes, quaternions and error measure of the geometry stages and the
scene, restatement and checker of the neighbour density field (tests/test_gpu_sugar_field.py describes its bar).  No
tests here: the test modules import from this one and not from each other."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402

D = torch.float64


def _rel(a, b):
    scale = float(b.double().abs().max()) if b.numel() else 0.0
    return float((a.double() - b.double()).abs().max()) / scale if scale > 0 else 0.0


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
