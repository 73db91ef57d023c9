"""Fixtures of the timed view-set tests (test infrastructure, no tests here).

- ``make_frames``: a small scene deformed per frame (moved, rotated, rescaled; a block of Gaussians behind the camera
  in the odd frames only), as numpy scenes the oracle and the rasterizer both take.
- ``run_timed`` / ``run_loop``: ``rasterize_timed_views`` on the frames, and the path the project had before it —
  one one-view ``rasterize_views`` call per frame — with the same upstream gradients.
- ``torch_rasterize_timed_views``: ``rasterize_timed_views`` restated as a loop over
  ``renderer_fixtures.torch_rasterize`` (CPU tests), and ``TimedGeometry`` / ``TimedRenderer``: stand-ins for
  geometry/dynamic_sugar.py's timed getters and for renderer/diff_sugar_rasterizer_temporal.py:82-224.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import gsr_synthetic as gs
import renderer_fixtures as rf
from diff_gaussian_rasterization import GaussianRasterizationSettings

C0 = 0.28209479177387814
BEHIND = slice(1000, 1300)  # the block of Gaussians put behind the camera in the odd frames


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) quaternions (numpy or torch, broadcasting)."""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    lib = torch if isinstance(b, torch.Tensor) else np
    return lib.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                      aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def make_frames(P, cams, seed, identical=False):
    """len(cams) frames of gs.make_scene(P, sh_degree=0) with precomputed colours.  Frame v is the base scene turned
    by 0.4 v rad about z, blown up by 1 + 0.05 v and shifted, its scales times 1 + 0.2 v, its quaternions turned with
    it; in the odd frames the Gaussians of BEHIND sit behind that view's camera (culled there, visible elsewhere).
    Rendering frame 0's geometry for view v > 0 is a different image altogether."""
    base = gs.make_scene(P, sh_degree=0, seed=seed)
    rng = np.random.default_rng(seed + 1)
    colors = rng.random((P, 3)).astype(np.float32)
    normals = rng.normal(size=(P, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    frames = []
    for v, cam in enumerate(cams):
        t = 0 if identical else v
        ang = 0.4 * t
        c, s = math.cos(ang), math.sin(ang)
        Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
        xyz = (base["means3D"] @ Rz.T) * np.float32(1 + 0.05 * t) + np.array([0.06, -0.04, 0.03], np.float32) * t
        q = quat_mul(np.array([math.cos(ang / 2), 0, 0, math.sin(ang / 2)], np.float32), base["rotations"])
        if t % 2 == 1 and P > BEHIND.stop:
            n = BEHIND.stop - BEHIND.start
            xyz[BEHIND] = cam["campos"] * np.float32(1.4) + rng.normal(0, 0.05, size=(n, 3)).astype(np.float32)
        frames.append(dict(means3D=xyz.astype(np.float32), scales=(base["scales"] * np.float32(1 + 0.2 * t)),
                           rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                           opacities=base["opacities"], colors_precomp=colors, normals=(normals @ Rz.T),
                           sh_degree=0))
    return frames


def _settings(cam, bg):
    from gsr_testutil import _settings as s

    return s(cam, bg, 0)


def _loss(outs, ups, ups2, bg_t):
    color, _, depth, alpha = outs[:4]
    dev = color.device
    gc, gd, ga = (torch.stack([torch.tensor(u[i], device=dev) for u in ups]) for i in range(3))
    loss = (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()
    if len(outs) == 5:
        loss = loss + (outs[4] * torch.stack([torch.tensor(u, device=dev) for u in ups2])).sum()
    return loss


def _images(outs):
    res = dict(color=outs[0].detach().cpu().numpy(), radii=outs[1].cpu().numpy(), depth=outs[2].detach().cpu().numpy(),
               alpha=outs[3].detach().cpu().numpy())
    if len(outs) == 5:
        res["color2"] = outs[4].detach().cpu().numpy()
    return res


def run_timed(frames, cams, bgs, ups=None, two=False, ups2=None, shared_scales=False, background=None, clamp=False,
              twice=False):
    """rasterize_timed_views on the frames (colors2 = the frames' normals with `two`; scales of frame 0 shared with
    shared_scales).  Returns numpy images, K per view and, with ups, the gradients: per view g_means3D / g_scales /
    g_rotations / g_colors2 / g_means2D (V, P, .), shared g_opacity / g_colors (/ g_scales), g_background."""
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization.batched import rasterize_timed_views

    dev = "cuda"
    V, P = len(frames), frames[0]["means3D"].shape[0]
    leaf = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev, requires_grad=True)  # noqa: E731
    t = dict(means3D=leaf(np.stack([f["means3D"] for f in frames])),
             scales=leaf(frames[0]["scales"] if shared_scales else np.stack([f["scales"] for f in frames])),
             rotations=leaf(np.stack([f["rotations"] for f in frames])), opacity=leaf(frames[0]["opacities"]),
             colors=leaf(frames[0]["colors_precomp"]))
    if two:
        t["colors2"] = leaf(np.stack([f["normals"] for f in frames]))
    m2s = [torch.zeros((P, 3), device=dev, requires_grad=True) for _ in cams]
    bg_t = None if background is None else leaf(background)
    outs = rasterize_timed_views([_settings(c, b) for c, b in zip(cams, bgs)], t["means3D"], m2s, t["opacity"],
                                 t["colors"], t["scales"], t["rotations"], colors2=t.get("colors2"), background=bg_t,
                                 clamp=clamp)
    res = _images(outs)
    res["K"] = [k for k, _, _ in list(_C.RECENT_FORWARDS)[-V:]]
    if ups is None:
        return res
    loss = _loss(outs, ups, ups2, bg_t)
    loss.backward(retain_graph=twice)

    def collect(prefix):
        for k, x in t.items():
            res[prefix + k] = x.grad.cpu().numpy().copy()
        res[prefix + "means2D"] = np.stack([m.grad.cpu().numpy() for m in m2s])
        if bg_t is not None:
            res[prefix + "background"] = bg_t.grad.cpu().numpy().copy()

    collect("g_")
    if twice:
        for x in list(t.values()) + m2s:
            x.grad = None
        loss.backward()
        collect("h_")
    return res


def run_loop(frames, cams, bgs, ups, two=False, ups2=None, shared_scales=False, background=None, clamp=False):
    """What the project offered before timed sets: one one-view rasterize_views call per frame with that frame's
    arrays.  Same result layout as run_timed (per-view gradients stacked, shared ones summed by autograd)."""
    from diff_gaussian_rasterization.batched import rasterize_views

    dev = "cuda"
    V, P = len(frames), frames[0]["means3D"].shape[0]
    leaf = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev, requires_grad=True)  # noqa: E731
    shared = dict(opacity=leaf(frames[0]["opacities"]), colors=leaf(frames[0]["colors_precomp"]))
    if shared_scales:
        shared["scales"] = leaf(frames[0]["scales"])
    per = [dict(means3D=leaf(f["means3D"]), rotations=leaf(f["rotations"]), colors2=leaf(f["normals"]) if two else None,
                scales=None if shared_scales else leaf(f["scales"])) for f in frames]
    m2s = [torch.zeros((P, 3), device=dev, requires_grad=True) for _ in cams]
    bg_t = None if background is None else leaf(background)
    outs = []
    for v, (cam, bg) in enumerate(zip(cams, bgs)):
        outs.append(rasterize_views([_settings(cam, bg)], per[v]["means3D"], [m2s[v]], shared["opacity"],
                                    colors_precomp=shared["colors"],
                                    scales=shared["scales"] if shared_scales else per[v]["scales"],
                                    rotations=per[v]["rotations"], colors2=per[v]["colors2"],
                                    background=None if bg_t is None else bg_t[v:v + 1], clamp=clamp))
    outs = [torch.cat([o[i] for o in outs]) for i in range(len(outs[0]))]
    res = _images(outs)
    _loss(outs, ups, ups2, bg_t).backward()
    for k, x in shared.items():
        res["g_" + k] = x.grad.cpu().numpy().copy()
    for k in ("means3D", "rotations", "colors2", "scales"):
        if per[0][k] is not None:
            res["g_" + k] = np.stack([p[k].grad.cpu().numpy() for p in per])
    res["g_means2D"] = np.stack([m.grad.cpu().numpy() for m in m2s])
    if bg_t is not None:
        res["g_background"] = bg_t.grad.cpu().numpy().copy()
    return res


# ---- the batch renderer's "sugar_temporal" mode ----------------------------------------------------------------------

def torch_rasterize_timed_views(settings_list, means3D, means2D_list, opacities, colors_precomp, scales, rotations,
                                colors2=None, background=None, clamp=False, grad_reduce=None):
    """batched.rasterize_timed_views restated as a loop over renderer_fixtures.torch_rasterize (any device)."""
    assert grad_reduce is None
    pick = lambda t, v: t[v] if t.dim() == 3 else t  # noqa: E731
    outs = [rf.torch_rasterize(s, means3D[v], m2, opacities, colors_precomp=colors_precomp, scales=pick(scales, v),
                               rotations=pick(rotations, v))
            for v, (s, m2) in enumerate(zip(settings_list, means2D_list))]
    color, radii, depth, alpha = (torch.stack([o[i] for o in outs]) for i in range(4))
    if background is not None:
        color = (color + (1 - alpha) * background.permute(0, 3, 1, 2)).clamp(0, 1)
    elif clamp:
        color = color.clamp(0, 1)
    if colors2 is None:
        return color, radii, depth, alpha
    second = [rf.torch_rasterize(s, means3D[v], torch.zeros_like(m2), opacities, colors_precomp=pick(colors2, v),
                                 scales=pick(scales, v), rotations=pick(rotations, v))[0]
              for v, (s, m2) in enumerate(zip(settings_list, means2D_list))]
    return color, radii, depth, alpha, torch.stack(second)


class TimedGeometry(rf.FakeGeometry):
    """The timed getters of geometry/dynamic_sugar.py (:339-346, :618-669) over a small closed-form deformation of
    the leaves: at time t the Gaussians are turned by 0.5 t rad about z, blown up by 1 + 0.1 t and moved by t x the
    leaf `drift`; the quaternions and normals turn with them; with d_scale the scales grow by 1 + 0.3 t."""

    def __init__(self, scene, device, dtype=torch.float32, d_scale=True):
        super().__init__(scene, device, dtype)
        self.params["drift"] = torch.tensor([0.08, -0.05, 0.04], device=device, dtype=dtype, requires_grad=True)
        self.cfg = SimpleNamespace(pred_normal=False, d_scale=d_scale)
        self.calls = dict(attributes=0, normals=0)

    def _rz(self, t):
        c, s, z, o = torch.cos(0.5 * t), torch.sin(0.5 * t), torch.zeros_like(t), torch.ones_like(t)
        return torch.stack([torch.stack([c, -s, z], -1), torch.stack([s, c, z], -1), torch.stack([z, z, o], -1)], -2)

    def get_points_rgb(self):  # geometry/sugar.py:650-660: SH2RGB of the DC coefficients
        return 0.5 + C0 * self.params["shs"][:, 0]

    def get_timed_gs_attributes(self, timestamp=None, frame_idx=None):
        self.calls["attributes"] += 1
        t = timestamp.to(self.get_xyz.dtype)
        R = self._rz(t)  # (T, 3, 3)
        xyz = torch.einsum("tij,pj->tpi", R, self.get_xyz) * (1 + 0.1 * t)[:, None, None]
        xyz = xyz + t[:, None, None] * self.params["drift"]
        z = torch.zeros_like(t)
        qz = torch.stack([torch.cos(0.25 * t), z, z, torch.sin(0.25 * t)], -1)  # half of the 0.5 t turn
        rot = torch.nn.functional.normalize(quat_mul(qz[:, None, :], self.get_rotation[None]), dim=-1)
        attrs = {"xyz": xyz, "rotation": rot}
        if self.cfg.d_scale:
            attrs["scale"] = self.get_scaling[None] * (1 + 0.3 * t)[:, None, None]
        return attrs

    def get_timed_gs_normals(self, timestamp=None, frame_idx=None):
        self.calls["normals"] += 1
        return torch.einsum("tij,pj->tpi", self._rz(timestamp.to(self.get_xyz.dtype)), self.get_gs_normals)

    def get_timed_gs_all_single_time(self, timestamp=None, frame_idx=None):
        if timestamp is not None and timestamp.ndim == 0:
            timestamp = timestamp[None]
        if frame_idx is not None and frame_idx.ndim == 0:
            frame_idx = frame_idx[None]
        attrs = self.get_timed_gs_attributes(timestamp, frame_idx)
        scales = attrs["scale"][0] if self.cfg.d_scale else self.get_scaling
        return attrs["xyz"][0], scales, attrs["rotation"][0], self.get_opacity, self.get_points_rgb()


class TimedRenderer(rf.FakeRenderer):
    """renderer/diff_sugar_rasterizer_temporal.py:82-224 per view; batch_render_mode "sugar_temporal" or "per_view"."""

    def __init__(self, batch_render_mode, scene, device, dtype=torch.float32, training=False, d_scale=True):
        super().__init__("sugar_temporal", scene, device, dtype, training=training)
        self.batch_render_mode = batch_render_mode
        self.geometry = TimedGeometry(scene, device, dtype, d_scale=d_scale)

    def forward(self, cam, bg_color, scaling_modifier=1.0, override_color=None, compute_normal_from_dist=True, **kwargs):
        pc = self.geometry
        bg_color = 1.0 - bg_color  # (:97-104: always inverted, the draw is commented out)
        sp = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
        sp.retain_grad()
        settings = GaussianRasterizationSettings(
            image_height=int(cam.image_height), image_width=int(cam.image_width),
            tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg_color,
            scale_modifier=scaling_modifier, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree, campos=cam.camera_center,
            prefiltered=False, debug=False)
        means3D, scales, rotations, opacity, colors = pc.get_timed_gs_all_single_time(cam.timestamp, cam.frame_idx)
        kw = dict(means3D=means3D, means2D=sp, shs=None, colors_precomp=colors, opacities=opacity, scales=scales,
                  rotations=rotations, cov3D_precomp=None)
        img, radii, depth, alpha = rf.RASTERIZE(settings, **kw)
        b = kwargs["batch_idx"]
        nmap_dist = None
        if compute_normal_from_dist:
            _, nmap_dist = rf.tr.sugar_normal_from_dist(depth, alpha, kwargs["rays_o"][b], kwargs["rays_d"][b])
        normals = pc.get_timed_gs_normals(cam.timestamp[None], cam.frame_idx[None])[0]
        normal, _, _, _ = rf.RASTERIZE(settings, **dict(kw, means2D=torch.zeros_like(sp), colors_precomp=normals))
        normal = torch.nn.functional.normalize(normal, dim=0)
        normal = torch.cat([-normal[:2], normal[2:]], 0)
        nmap = normal * 0.5 * alpha + 0.5
        mask = alpha > 0.99
        nmap = torch.where(mask.expand_as(nmap), nmap, nmap.detach())
        depth = torch.where(mask, depth, depth.detach())
        return {"render": img.clamp(0, 1), "normal": nmap, "normal_from_dist": nmap_dist, "depth": depth, "mask": alpha,
                "viewspace_points": sp, "visibility_filter": radii > 0, "radii": radii}


def make_timed_batch(B, H, W, device, dtype=torch.float32, seed=0):
    """renderer_fixtures.make_batch plus the temporal data module's timestamps and frame indices."""
    batch = rf.make_batch(B, H, W, device, dtype, seed=seed)
    batch["timestamp"] = torch.linspace(0.0, 1.0, B).to(device, dtype)
    batch["frame_indices"] = torch.arange(B, device=device)
    return batch
