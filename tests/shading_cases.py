"""What the shading-epilogue tests share (tests/test_shading.py, tests/test_shading_cases.py,
tests/test_gpu_shading_edges.py): inputs that look like a render (an empty background, a silhouette, isolated spurs,
opaque surfaces across the 32 x 8 tile seams, a light on the surface), the torch references of every entry point, and
the per-pixel bar `check_pixels`.  No tests here.

Every input is drawn in float32 and upcast for the fp64 reference, so the input-side decisions (alpha > 0.99, alpha
exactly 0) are the same in every precision.  The computed decisions (the albedo and image clamps, dot(s, l) >= 0) are
adjudicated between the two references by `tie_masks`, never from the kernel's values.

The bar, per element of every output and gradient (the row rule of tests/gsr_testutil.py made local to the stencil):

    |got - ref64| <= max(bar, ROW_RATIO * m(p)),   m(p) = max |null32 - ref64| over the 5 x 5 pixels around p, all
                                                   channels (the reach of the depth gradient's two-step stencil)
    bar = RGB_ATOL for outputs, GRAD_TOL * max(1, |ref64|) for gradients

non-finite values fail, and where ref64 and the null are exactly zero over the whole 5 x 5 neighbourhood, got is
exactly zero."""
import functools
import math

import pytest

torch = pytest.importorskip("torch")

import torch_reference as tr  # noqa: E402
from gsr_testutil import GRAD_TOL, RGB_ATOL, ROW_RATIO  # noqa: E402

F = torch.nn.functional
TILE_X, TILE_Y = 32, 8          # csrc/gsr_shading.hip: one workgroup per 32 x 8 pixel tile
REACH = 2                       # the depth gradient reaches two pixels (normal stencil of the stencil's neighbours)
SHAPES = ((1, 1), (1, 33), (9, 1), (8, 32), (9, 33), (17, 65))
SILHOUETTE_SHAPE, CHUNK_SHAPE, CHUNK_VIEWS = (19, 70), (9, 33), 65  # 65 views cross the 64-view launch chunk
KA, KD = (0.1, 0.2, 0.15), (0.9, 0.7, 0.8)
MODES = ("diffuse", "albedo", "textureless")
OUTPUTS = ("render", "normal", "depth", "unit", "nmap", "out")  # every other name is a gradient
TIE_RATIO = 4.0
EXCUSED_CAP = 0.02


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _grid(H, W):
    return torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")


def _frame(v, H, W, g):
    """What every case shares for view v: a bumpy depth surface near 2, threestudio's pinhole rays (x right, y up,
    -z forward, not normalised) under a random rotation, one ray origin, the background image (a tenth of its
    entries exactly 0 or 1: the closed ends of the image clamp), a target albedo that crosses both clamp edges (and
    is exactly 0 on a few columns), the predicted normals and the upstream gradients.  float32."""
    ys, xs = _grid(H, W)
    surf = 2.0 + 0.3 * torch.sin(xs / 7.0 + 0.7 * v) * torch.cos(ys / 5.0) + 0.002 * torch.rand((H, W), generator=g)
    f = 0.5 * max(H, W, 16) / math.tan(math.radians(30))
    d = torch.stack([(xs + 0.5 - W / 2) / f, -(ys + 0.5 - H / 2) / f, -torch.ones_like(xs)], -1)
    rot = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    rays_d = d @ rot.T
    # the ray origin in multiples of 2^-10: at a corner of an empty image both central differences are +-rays_o (X is
    # zero-padded), and their cross product is exactly zero only if the products are exact — a torch build that fuses
    # the float32 multiply-subtract would otherwise leave the null a rounding residue for a normal there
    rays_o = torch.round(torch.randn(3, generator=g, dtype=torch.float64) * 1024.0) / 1024.0
    bg =torch.rand((H, W, 3), generator=g, dtype=torch.float64)
    edge = torch.rand((H, W, 3), generator=g)
    bg = torch.where(edge < 0.05, torch.zeros_like(bg), torch.where(edge > 0.95, torch.ones_like(bg), bg))
    albedo = torch.rand((3, H, W), generator=g, dtype=torch.float64) * 1.3 - 0.15
    albedo[:, :, 3::11] = 0.0
    # a light beside the surface, a little towards the camera: dot(s, l) takes both signs over the bumps
    centre = rays_o + 2.0 * rays_d[H // 2, W // 2]
    light = centre + rot @ torch.tensor([0.35, 0.2, 0.25], dtype=torch.float64) \
        + 0.05 * torch.randn(3, generator=g, dtype=torch.float64)
    pred = torch.rand((3, H, W), generator=g, dtype=torch.float64)
    ups = [torch.randn((3, H, W), generator=g), torch.randn((3, H, W), generator=g),
           torch.randn((1, H, W), generator=g)]
    return dict(surf=surf.float(), albedo=albedo.float(), rays_o=rays_o.float().expand(H, W, 3).clone(),
                rays_d=rays_d.float(), bg=bg.float(), light=light.float(), pred=pred.float(), ups=ups)


def _finish(fr, alpha):
    """The rasterizer's outputs for a coverage plane: alpha exactly 0 below 1 / 255 (as the blend drops such
    contributions), depth and colour weighted by alpha."""
    alpha = torch.where(alpha < 1.0 / 255.0, torch.zeros_like(alpha), alpha).float()
    return dict(color=fr["albedo"] * alpha[None], depth=(fr["surf"] * alpha)[None], alpha=alpha[None],
                rays_o=fr["rays_o"], rays_d=fr["rays_d"], bg=fr["bg"], light=fr["light"], pred=fr["pred"],
                ups=fr["ups"])


def silhouette(V, H, W, seed=0):
    """A soft-edged disc (an ellipse in pixels) of about 40 % of the image on an empty background: alpha above 0.99
    inside, a smooth ramp to exactly 0 outside."""
    g = torch.Generator().manual_seed(1000 + seed)
    ys, xs = _grid(H, W)
    rho = torch.sqrt(((xs + 0.5 - W / 2) / (W / 2)) ** 2 + ((ys + 0.5 - H / 2) / (H / 2)) ** 2)
    r_in, r_out = 0.42, 0.73            # pi 0.73^2 / 4 = 0.42 of the image is covered at all
    t = ((r_out - rho) / (r_out - r_in)).clamp(0, 1)
    ramp = t * t * (3 - 2 * t)
    out = []
    for v in range(V):
        fr = _frame(v, H, W, g)
        inside = 0.992 + 0.008 * torch.rand((H, W), generator=g, dtype=torch.float64)
        out.append(_finish(fr, inside * ramp))
    return out


def _clip(lo, hi, n):
    return range(max(0, min(lo, n - 1)), max(0, min(hi, n - 1)) + 1)


def spur_pixels(H, W):
    """(y, x, kind) of the spurs, positions clipped to the image: isolated pixels, one-pixel lines and a 2 x 2 block at
    x in {0, 31, 32, W - 1} and y in {0, 7, 8, H - 1} (tile seams and image borders)."""
    px = {}

    def put(ys_, xs_, kind):
        for y in ys_:
            for x in xs_:
                px.setdefault((y, x), kind)

    put(_clip(7, 8, H), _clip(31, 32, W), "block")                      # across both seams
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 32), (H - 1, 31), (3, 0), (12, W - 1),
                 (3, 31), (8, 2), (13, 50), (13, 20)):          # the last four away from the borders
        put(_clip(y, y, H), _clip(x, x, W), "pixel")
    put(_clip(8, 8, H), _clip(36, W - 1, W), "hline")                   # first row of the second tile row, to the border
    put(_clip(7, 7, H), _clip(4, 27, W), "hline")                       # last row of the first tile row
    put(_clip(11, H - 1, H), _clip(31, 31, W), "vline")                 # last column of the first tile column
    put(_clip(0, 4, H), _clip(34, 34, W), "vline")
    put(_clip(2, 5, H), _clip(W - 1, W - 1, W), "vline")                # along the right border
    return sorted((y, x, k) for (y, x), k in px.items())


SPUR_ALPHA = (1.0, 0.995, 0.7, 0.9925, 0.99, 0.3, 0.9900001)  # both sides of 0.99 (0.99 itself is not above)


def spurs(V, H, W, seed=0):
    """An all-zero image with isolated covered pixels, lines and a block (`spur_pixels`).  Along a line the normal is
    exactly zero (one of the two central differences vanishes, the other does not) while alpha > 0.99 lets the
    upstream gradient through: F.normalize's backward runs with |n| = 0 and hands the neighbours 1e12 x the upstream."""
    g = torch.Generator().manual_seed(2000 + seed)
    out = []
    for v in range(V):
        fr = _frame(v, H, W, g)
        alpha = torch.zeros((H, W), dtype=torch.float64)
        for i, (y, x, _) in enumerate(spur_pixels(H, W)):
            alpha[y, x] = SPUR_ALPHA[(i + v) % len(SPUR_ALPHA)]
        out.append(_finish(fr, alpha))
    return out


def seams(V, H, W, seed=0):
    """A fully opaque smooth surface: every pixel has a normal and all gradients, so the stencil gather is live across
    every tile seam."""
    g = torch.Generator().manual_seed(3000 + seed)
    return [_finish(_frame(v, H, W, g), torch.ones((H, W), dtype=torch.float64)) for v in range(V)]


def surface_pixel(H, W):
    return H // 2, W // 2


def light_on_surface(V, H, W, seed=0):
    """`seams` with view 0's light at X of `surface_pixel`: L = light - X is exactly zero there in every precision (the
    ray origin and that pixel's ray direction are multiples of 2^-10 and its depth is 2, so X is exact in float32)."""
    out = seams(V, H, W, seed)
    y, x = surface_pixel(H, W)
    sc = out[0]
    snap = lambda t: torch.round(t * 1024.0) / 1024.0  # noqa: E731
    sc["rays_o"] = snap(sc["rays_o"])
    sc["rays_d"][y, x] = snap(sc["rays_d"][y, x])
    sc["color"][:, y, x] = sc["color"][:, y, x].clamp(0.2, 0.8)  # alpha is 1: the albedo, kept off 0 so that the
    sc["depth"][0, y, x] = 2.0                                   # gradient reaches the light direction
    sc["light"] = (sc["rays_o"][y, x] + 2.0 * sc["rays_d"][y, x]).clone()
    return out


CASES = {"silhouette": silhouette, "spurs": spurs, "seams": seams, "light_on_surface": light_on_surface}
SEEDS = {}  # (name, H, W) -> seed, where the default draw puts a decision tie on a named pixel or over the cap


@functools.lru_cache(maxsize=None)
def get(name, H, W, V=1):
    """The case's views (float32 tensors; treat them as read-only, they are shared)."""
    return CASES[name](V, H, W, SEEDS.get((name, H, W), 0))


NORMAL_MAP_CASES = [("silhouette",) + SILHOUETTE_SHAPE] + [("spurs", H, W) for H, W in SHAPES]


@functools.lru_cache(maxsize=None)
def normal_map_scene(name, H, W, V=2):
    """For `sugar_normal_map`: the case's alpha planes with face normals that are exactly zero at the spur pixels (for
    the silhouette: on every third column), where alpha lies on both sides of 0.99."""
    out = []
    for v, s in enumerate(get(name, H, W, V)):
        g = torch.Generator().manual_seed(50 + v)
        normal = torch.randn((3, H, W), generator=g)
        if name == "spurs":
            for y, x, _ in spur_pixels(H, W):
                normal[:, y, x] = 0.0
        else:
            normal[:, :, ::3] = 0.0
        out.append(dict(normal=normal, alpha=s["alpha"], ups=s["ups"]))
    return out


def old_scene(V, H, W, seed):
    """tests/test_shading.py's `_scene` (drawn in float64, every pixel covered) as float32 inputs."""
    from test_shading import _scene

    return as_float32(_scene(V, H, W, seed))


def as_float32(scenes):
    """Views drawn in float64 as the float32 inputs the GPU gets (the references then upcast these)."""
    return [{k: ([u.float() for u in s[k]] if k == "ups" else s[k].float()) for k in s} for s in scenes]


def view_tables(V):
    """Per-view (mode, ka, kd) as the material draws them once per view (soft shading: kd in (0, 1), ka = 1 - kd)."""
    modes = [MODES[(7 * v) % 3] for v in range(V)]
    kd = [(0.25 + 0.7 * ((v * 0.37) % 1.0),) * 3 for v in range(V)]
    ka = [(1.0 - d[0],) * 3 for d in kd]
    return modes, ka, kd


# ---- references ------------------------------------------------------------------------------------------------------
def _normalize_r(x, dim):
    """F.normalize with one reciprocal and three multiplies (the arrangement of the HIP backward)."""
    return x * (1.0 / x.norm(2, dim, keepdim=True).clamp_min(1e-12))


def _epilogue_recip(color, depth, alpha, rays_o, rays_d, bg_hwc, light, ambient, diffuse, shading="diffuse",
                    pred_normal=None):
    """tests/torch_reference.py's `shading_epilogue` with reciprocal-multiply in place of its three divisions (the
    two normalisations and the albedo): a second float32 evaluation for the checker's self-test."""
    H, W = depth.shape[-2:]
    xyz = rays_o + depth.permute(1, 2, 0) * rays_d
    normal_map = _normalize_r(tr.depth_to_normal(xyz.permute(2, 0, 1).unsqueeze(0))[0], 0)
    if pred_normal is not None:
        sn = F.normalize(pred_normal.permute(1, 2, 0).detach() * 2 - 1, dim=2)
    else:
        sn = normal_map.permute(1, 2, 0)
    ldir = _normalize_r(light[None, None, :].expand(H, W, -1) - xyz, -1)
    tl = torch.sum(sn * ldir, -1, keepdim=True).clamp(min=0.0) * diffuse + ambient
    albedo = (color * (1.0 / (alpha + 1e-6))).permute(1, 2, 0)
    if shading == "albedo":
        fg = albedo + tl * 0
    elif shading == "textureless":
        fg = albedo * 0 + tl
    else:
        fg = albedo.clamp(0.0, 1.0) * tl
    img = fg.permute(2, 0, 1) * alpha + (1 - alpha) * bg_hwc.reshape(H, W, 3).permute(2, 0, 1)
    nmap = normal_map * 0.5 * alpha + 0.5
    mask = alpha.float() > 0.99
    nmap = torch.where(mask.repeat(3, 1, 1), nmap, nmap.detach())
    return img.clamp(0, 1), nmap, torch.where(mask, depth, depth.detach())


def _normal_from_dist_recip(depth, alpha, rays_o, rays_d):
    xyz = rays_o + depth.permute(1, 2, 0) * rays_d
    n = _normalize_r(tr.depth_to_normal(xyz.permute(2, 0, 1).unsqueeze(0))[0], 0)
    nmap = n * 0.5 * alpha + 0.5
    nmask = (alpha.float() > 0.99).repeat(3, 1, 1)
    return torch.where(nmask, n, n.detach()), torch.where(nmask, nmap, nmap.detach())


def normal_map_ref(normal, alpha):
    """renderer/diff_sugar_rasterizer_normal.py:192-197 for one view (the mask is the reference's fp32 comparison)."""
    n = F.normalize(normal, dim=0)
    n = torch.cat([-n[:2], n[2:]], 0)
    nmap = n * 0.5 * alpha + 0.5
    return torch.where((alpha.float() > 0.99).repeat(3, 1, 1), nmap, nmap.detach())


ENTRY_OUTPUTS = {"shade": ("render", "normal", "depth"), "depth_normal": ("unit", "nmap"), "normal_map": ("out",)}
ENTRY_LEAVES = {"shade": ("color", "depth", "alpha", "bg"), "depth_normal": ("depth", "alpha"),
                "normal_map": ("normal", "alpha")}


def reference(sc, dtype, entry="shade", shading="diffuse", use_pred=False, ka=KA, kd=KD, which=None, recip=False,
              bg_const=False):
    """One view through the torch restatement in `dtype`: the outputs by name and, as "d" + leaf, the gradients of
    sum_i (out_i * ups_i).sum() over the outputs listed in `which` (all by default); a leaf nothing feeds gets zeros.
    `bg_const`: the background is the (3,) colour sc["bg"][0, 0], and "dbg" is (3,)."""
    t = lambda k: sc[k].to(dtype)  # noqa: E731
    names, lnames = ENTRY_OUTPUTS[entry], ENTRY_LEAVES[entry]
    leaves = {k: (t(k)[0, 0] if (k == "bg" and bg_const) else t(k)).clone().requires_grad_(True) for k in lnames}
    if entry == "shade":
        H, W = sc["depth"].shape[-2:]
        bg = leaves["bg"].expand(H, W, 3) if bg_const else leaves["bg"]
        fn = _epilogue_recip if recip else tr.shading_epilogue
        outs = fn(leaves["color"], leaves["depth"], leaves["alpha"], t("rays_o"), t("rays_d"), bg, t("light"),
                  torch.tensor(ka, dtype=dtype), torch.tensor(kd, dtype=dtype), shading, t("pred") if use_pred else None)
        ups = sc["ups"]
    elif entry == "depth_normal":
        fn = _normal_from_dist_recip if recip else tr.sugar_normal_from_dist
        outs = fn(leaves["depth"], leaves["alpha"], t("rays_o"), t("rays_d"))
        ups = sc["ups"][:2]
    else:
        outs = (normal_map_ref(leaves["normal"], leaves["alpha"]),)
        ups = sc["ups"][:1]
    which = tuple(range(len(outs))) if which is None else tuple(which)
    loss = sum((outs[i] * ups[i].to(dtype)).sum() for i in which)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    res = {n: o.detach() for n, o in zip(names, outs)}
    for k, gr in zip(lnames, grads):
        res["d" + k] = torch.zeros_like(leaves[k]) if gr is None else gr
    return res


def references(sc, **kw):
    """(fp64 reference, fp32 null) of one view."""
    return reference(sc, torch.float64, **kw), reference(sc, torch.float32, **kw)


def stencil(sc, dtype):
    """a, b (the central differences of X with zero padding), n = -(a x b) as tests/torch_reference.py forms it, and
    L = light - X; (3, H, W) each."""
    xyz = (sc["rays_o"].to(dtype) + sc["depth"].to(dtype).permute(1, 2, 0) * sc["rays_d"].to(dtype)).permute(2, 0, 1)
    pad = F.pad(xyz, (1, 1, 1, 1))
    a = pad[:, 1:-1, 2:] - pad[:, 1:-1, :-2]
    b = pad[:, 2:, 1:-1] - pad[:, :-2, 1:-1]
    return a, b, tr.depth_to_normal(xyz.unsqueeze(0))[0], sc["light"].to(dtype)[:, None, None] - xyz


def quantities(sc, dtype, shading="diffuse", use_pred=False, ka=KA, kd=KD, bg_const=False):
    """The computed quantities a decision hangs on, by the operations of `shading_epilogue` (so with its bits): "alb"
    against the albedo clamp (diffuse), "img" against the image clamp, "dt" = dot(s, l) against 0 (not for albedo,
    where the light term is multiplied by 0).  (C, H, W) each; the census pins img.clamp(0, 1) to the render."""
    with torch.no_grad():
        t = lambda k: sc[k].to(dtype)  # noqa: E731
        H, W = sc["depth"].shape[-2:]
        color, depth, alpha = t("color"), t("depth"), t("alpha")
        xyz = t("rays_o") + depth.permute(1, 2, 0) * t("rays_d")
        normal_map = F.normalize(tr.depth_to_normal(xyz.permute(2, 0, 1).unsqueeze(0))[0], dim=0)
        sn = F.normalize(t("pred").permute(1, 2, 0) * 2 - 1, dim=2) if use_pred else normal_map.permute(1, 2, 0)
        ldir = F.normalize(t("light")[None, None, :].expand(H, W, -1) - xyz, dim=-1)
        dt = torch.sum(sn * ldir, -1, keepdim=True)
        tl = dt.clamp(min=0.0) * torch.tensor(kd, dtype=dtype) + torch.tensor(ka, dtype=dtype)
        albedo = (color / (alpha + 1e-6)).permute(1, 2, 0)
        fg = {"albedo": albedo + tl * 0, "textureless": albedo * 0 + tl, "diffuse": albedo.clamp(0.0, 1.0) * tl}[shading]
        bg = t("bg")[0, 0].expand(H, W, 3) if bg_const else t("bg")
        img = fg.permute(2, 0, 1) * alpha + (1 - alpha) * bg.permute(2, 0, 1)
    q = {"img": img}
    if shading == "diffuse":
        q["alb"] = albedo.permute(2, 0, 1)
    if shading != "albedo":
        q["dt"] = dt.permute(2, 0, 1)
    return q


THRESHOLDS = {"alb": (0.0, 1.0), "img": (0.0, 1.0), "dt": (0.0, None)}  # closed intervals: torch's clamp masks


def _side(q, lo, hi):
    s = (q >= lo).to(torch.int8)
    return s if hi is None else s + (q > hi).to(torch.int8)


def tie_masks(scenes, shadings, use_pred=False, kas=None, kds=None, bg_const=False):
    """Per view, the (H, W) pixels whose computed decisions the two references do not settle: for each quantity the
    tie width is TIE_RATIO x the largest |q32 - q64| over the views of the case; a pixel is a tie if its fp64 value is
    within that width of a threshold or the fp32 null decides otherwise — unless both references sit exactly on the
    threshold (then the closed-interval side is the answer, for the kernel too)."""
    V = len(scenes)
    shadings = [shadings] * V if isinstance(shadings, str) else list(shadings)
    kas = [KA] * V if kas is None else ([kas] * V if not isinstance(kas[0], (tuple, list)) else kas)
    kds = [KD] * V if kds is None else ([kds] * V if not isinstance(kds[0], (tuple, list)) else kds)
    qs = [(quantities(sc, torch.float64, m, use_pred, a, d, bg_const),
           quantities(sc, torch.float32, m, use_pred, a, d, bg_const)) for sc, m, a, d in zip(scenes, shadings, kas, kds)]
    width = {}
    for q64, q32 in qs:
        for k in q64:
            width[k] = max(width.get(k, 0.0), TIE_RATIO * float((q32[k].double() - q64[k]).abs().max()))
    masks = []
    for q64, q32 in qs:
        tie = torch.zeros(q64["img"].shape[-2:], dtype=torch.bool)
        for k in q64:
            lo, hi = THRESHOLDS[k]
            a, b = q64[k], q32[k].double()
            flip = _side(a, lo, hi) != _side(b, lo, hi)
            for thr in (lo, hi):
                if thr is None:
                    continue
                near = ((a - thr).abs() <= width[k]) | flip
                tie |= (near & ~((a == thr) & (b == thr))).any(0)
        masks.append(tie)
    return masks, width


# ---- the bar ---------------------------------------------------------------------------------------------------------
def _pool(x, reach=REACH):
    """(H, W) -> the largest value over the (2 reach + 1)^2 pixels around each pixel."""
    k = 2 * reach + 1
    return F.max_pool2d(x[None, None], k, 1, reach)[0, 0]


def dilate(mask, reach=REACH):
    return _pool(mask.double(), reach) > 0


def _planes(x, name):
    x = x.detach().double().cpu()
    if name == "dbg" and x.dim() == 3:
        x = x.permute(2, 0, 1)
    return x


def pixel_stats(name, got, ref64, null32, tie=None):
    """One tensor of one view against the bar: dict(worst, at, excused, fails, reason)."""
    g, r, n = (_planes(x, name) for x in (got, ref64, null32))
    assert g.shape == r.shape == n.shape, (name, g.shape, r.shape, n.shape)
    bar = torch.full_like(r, RGB_ATOL) if name in OUTPUTS else GRAD_TOL * r.abs().clamp(min=1.0)
    err, nerr = (g - r).abs(), (n - r).abs()
    if r.dim() == 1:  # a sum over the pixels (the constant background's gradient): one neighbourhood, any tie excuses
        m = torch.full_like(r, float(nerr.max()))
        exc = torch.full_like(r, bool(tie is not None and tie.any()), dtype=torch.bool)
        zero = torch.zeros_like(exc)
    else:
        m = _pool(nerr.amax(0)).expand_as(r)
        exc = torch.zeros(r.shape[-2:], dtype=torch.bool) if tie is None else (dilate(tie) if name == "ddepth" else tie)
        zero = ((_pool(r.abs().amax(0)) == 0) & (_pool(n.abs().amax(0)) == 0)).expand_as(r)
        exc = exc.expand_as(r)
    finite = bool(torch.isfinite(g).all())
    ratio = torch.where(exc, torch.zeros_like(err), err / torch.maximum(bar, ROW_RATIO * m))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, math.inf))
    nonzero = zero & ~exc & (g != 0)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    at = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)) if ratio.numel() else ()
    reason = None
    if not finite:
        reason = "non-finite values"
    elif worst > 1.0:
        reason = f"{int((ratio > 1).sum())} elements beyond the bar, worst {worst:.3g} x at {at}"
    elif bool(nonzero.any()):
        reason = f"{int(nonzero.sum())} elements not exactly zero where nothing contributes"
    return dict(worst=worst, at=at, excused=int(exc[0].sum()) if r.dim() > 1 else int(exc.any()), reason=reason)


def check_pixels(got, ref64, null32, tie=None, tag="", report=None):
    """Every tensor of `got` (name -> tensor of one view) against the bar of this module's docstring; `tie` is the
    view's (H, W) mask of decision ties, which excuses p itself, and for "ddepth" the 5 x 5 pixels around p.  Prints
    per tensor the worst ratio, the excused count and the pixel of the worst miss, then fails on any miss."""
    failed = []
    for name in got:
        st = pixel_stats(name, got[name], ref64[name], null32[name], tie)
        print(f"SHADE {tag} {name}: worst ratio {st['worst']:.3g} at {st['at']}, excused {st['excused']}")
        if report is not None:
            report[name] = st
        if st["reason"]:
            failed.append(f"{tag} {name}: {st['reason']}")
    assert not failed, "; ".join(failed)


def seam_band(H, W):
    """(H, W): the pixels within REACH of a tile seam (and so the pixels whose stencils cross it)."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")

    def near(c, tile, n):
        hit = torch.zeros_like(c, dtype=torch.bool)
        for s in range(tile, n, tile):
            hit |= (c >= s - REACH) & (c < s + REACH)
        return hit

    return near(xs, TILE_X, W) | near(ys, TILE_Y, H)
