"""Cameras and scenes away from the default orbit (distance 2.5, fov 60 deg), shared by the CPU census
(tests/test_camera_cases.py), the oracle-vs-torch check (tests/test_oracle.py) and the GPU parity tests
(tests/test_gpu_cameras.py).  No GPU code.

Each case is a (scene, camera, background) triple built from gsr_synthetic.make_scene with fixed seeds:

  near49      distance 1.5, fov 49.1 deg, 160 x 160: the object overflows the frustum, the 1.3 tan(fov/2) guard
              binds in x and in y on visible Gaussians, centres lie off every image side
  tele20      distance 3.8, fovx = fovy = 20 deg, 176 x 120 (ragged): 3x the orbit's focal length
  offaxis     eye at 1.2, looking 0.7 beside the centre, fovx 70 / fovy 40 deg, 200 x 120: the guard binds on
              one side only, rectangles are cut at the left and top edges (getRect divides a negative number)
  inside      eye inside the ball, 0.3 from the centre, 60 deg, 128 x 128, scale_mult 2, opacity up to 1.0:
              Gaussians just above and just below the 0.2 near cull, radii beyond the image, far / near depth
              > 4 (4-pass depth sort), the 0.99 alpha clamp binding
  deep        the orbit, with 200 Gaussians moved along the view axis to depths 0.25 .. 60 (4-pass depth sort)
  wide_field  2^20 + 1 Gaussians (21 index bits: the kept-tile field of the depth-sort value holds at most
              2047), 768 x 768 = 2304 tiles, all but ~300 behind the camera, three opaque close Gaussians
              that keep every tile and a handful around 1500 - 2600 kept tiles

tests/test_camera_cases.py asserts that each case is what this table says.
"""
from __future__ import annotations

import math

import numpy as np

import gsr_synthetic as gs

NEAR_CULL = 0.2


def make_lookat_camera(eye, target, W, H, fovx_deg, fovy_deg, up=(0.0, 0.0, 1.0)):
    """Look-at camera (same axes and matrices as gsr_testutil.make_camera: OpenGL c2w through
    cameras.get_cam_info_gaussian)."""
    import torch

    from diff_gaussian_rasterization.cameras import get_cam_info_gaussian

    F = torch.nn.functional
    pos = torch.tensor(eye, dtype=torch.float32)
    lookat = F.normalize(torch.tensor(target, dtype=torch.float32) - pos, dim=-1)
    right = F.normalize(torch.cross(lookat, torch.tensor(up, dtype=torch.float32), dim=-1), dim=-1)
    upv = F.normalize(torch.cross(right, lookat, dim=-1), dim=-1)
    c2w = torch.zeros(4, 4, dtype=torch.float32)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3], c2w[3, 3] = right, upv, -lookat, pos, 1.0
    fovx, fovy = math.radians(fovx_deg), math.radians(fovy_deg)
    wv, fp, cc = get_cam_info_gaussian(c2w, fovx, fovy, 0.1, 100.0)
    return dict(view=wv.numpy().astype(np.float32), proj=fp.numpy().astype(np.float32),
                campos=cc.numpy().astype(np.float32), tanx=math.tan(fovx / 2), tany=math.tan(fovy / 2), W=W, H=H)


def orbit_eye(distance, elevation_deg=15.0, azimuth_deg=0.0):
    e, a = math.radians(elevation_deg), math.radians(azimuth_deg)
    return (distance * math.cos(e) * math.cos(a), distance * math.cos(e) * math.sin(a), distance * math.sin(e))


def view_space(means, cam):
    """(P, 3) float64 view-space positions t = (x, y, z, 1) @ view (row-vector convention of the C ABI)."""
    v = np.asarray(cam["view"], np.float64).reshape(4, 4)
    return np.asarray(means, np.float64) @ v[:3, :3] + v[3, :3]


def world_from_view(t, cam):
    """Inverse of view_space (the view matrix is rigid)."""
    v = np.asarray(cam["view"], np.float64).reshape(4, 4)
    return (np.asarray(t, np.float64) - v[3, :3]) @ v[:3, :3].T


def camera(name, W=None, H=None):
    """The camera of case near49 / tele20 / offaxis / inside, optionally at another image size."""
    if name == "near49":
        return make_lookat_camera(orbit_eye(1.5, 15.0, 20.0), (0.0, 0.0, 0.0), W or 160, H or 160, 49.1, 49.1)
    if name == "tele20":
        return make_lookat_camera(orbit_eye(3.8, 15.0, 140.0), (0.0, 0.0, 0.0), W or 176, H or 120, 20.0, 20.0)
    if name == "offaxis":
        eye = np.array(orbit_eye(1.2, 15.0, 250.0))
        side = np.cross(-eye / np.linalg.norm(eye), (0.0, 0.0, 1.0))
        target = 0.7 * side / np.linalg.norm(side)
        return make_lookat_camera(tuple(eye), tuple(target), W or 200, H or 120, 70.0, 40.0)
    if name == "inside":
        return make_lookat_camera(orbit_eye(0.3, 15.0, 60.0), (0.0, 0.0, 0.0), W or 128, H or 128, 60.0, 60.0)
    raise KeyError(name)


def near49():
    scene = gs.make_scene(5000, sh_degree=1, seed=101, scale_mult=1.5)
    cam = camera("near49")
    return scene, cam, np.array([1.0, 1.0, 1.0], np.float32)


def tele20():
    scene = gs.make_scene(2500, sh_degree=3, seed=102)
    cam = camera("tele20")
    return scene, cam, np.array([0.0, 0.0, 0.0], np.float32)


def offaxis():
    scene = gs.make_scene(1500, sh_degree=2, seed=103)
    cam = camera("offaxis")
    return scene, cam, np.array([0.2, 0.5, 0.9], np.float32)


def inside():
    scene = gs.make_scene(1200, sh_degree=0, seed=104, scale_mult=2.0, opacity_range=(0.05, 1.0))
    cam = camera("inside")
    # a few Gaussians are placed on the view axis side just above and just below the near cull
    t = view_space(scene["means3D"], cam)
    rng = np.random.default_rng(204)
    ids = rng.choice(t.shape[0], 24, replace=False)
    t[ids[:12], 2] = np.linspace(0.2005, 0.2095, 12)
    t[ids[12:], 2] = np.linspace(0.19, 0.1995, 12)
    t[ids, :2] = rng.uniform(-0.12, 0.12, size=(24, 2))
    scene["means3D"] = world_from_view(t, cam).astype(np.float32)
    # the top of the opacity range (a saturated sigmoid), so that the 0.99 alpha clamp binds over whole regions
    scene["opacities"][rng.choice(t.shape[0], 60, replace=False)] = 1.0
    return scene, cam, np.array([0.3, 0.3, 0.3], np.float32)


DEEP_MOVED = 200


def deep(moved=True):
    """moved=False: the same scene without its DEEP_MOVED moved Gaussians (it sorts in 3 passes)."""
    scene = gs.make_scene(3000, sh_degree=1, seed=105)
    from gsr_testutil import make_camera

    cam = make_camera(144, 112, azimuth=75.0)
    t = view_space(scene["means3D"], cam)
    z = np.geomspace(0.25, 60.0, DEEP_MOVED)
    t[:DEEP_MOVED, 2] = z
    t[:DEEP_MOVED, :2] *= (z / 2.5)[:, None] * 0.6  # keep them inside the frustum
    scene["means3D"] = world_from_view(t, cam).astype(np.float32)
    if not moved:
        scene = {k: (v[DEEP_MOVED:] if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    return scene, cam, np.array([1.0, 1.0, 1.0], np.float32)


WIDE_P = (1 << 20) + 1
WIDE_VISIBLE = 300
WIDE_FULL = 3  # opaque, close, large: their alpha >= 1/255 ellipse covers the image
WIDE_MID = 8  # around 1500 - 2600 kept tiles


def wide_field():
    from gsr_testutil import make_camera

    cam = make_camera(768, 768, azimuth=200.0)
    vis = gs.make_scene(WIDE_VISIBLE, sh_degree=0, seed=106)
    rng = np.random.default_rng(206)
    P, n = WIDE_P, WIDE_VISIBLE
    t = view_space(vis["means3D"], cam)
    k = WIDE_FULL + WIDE_MID
    t[:k, :2] = rng.uniform(-0.15, 0.15, size=(k, 2))
    t[:WIDE_FULL, 2] = (0.9, 1.1, 1.3)
    vis["scales"][:WIDE_FULL] = rng.uniform(0.9, 1.2, size=(WIDE_FULL, 3))
    vis["opacities"][:WIDE_FULL, 0] = (0.97, 0.9, 0.8)
    t[WIDE_FULL:k, 2] = np.linspace(1.4, 1.7, WIDE_MID)
    vis["scales"][WIDE_FULL:k] = np.linspace(0.26, 0.42, WIDE_MID)[:, None] * rng.uniform(0.9, 1.1, size=(WIDE_MID, 3))
    vis["opacities"][WIDE_FULL:k, 0] = rng.uniform(0.5, 0.9, size=WIDE_MID)
    vis["means3D"] = world_from_view(t, cam).astype(np.float32)
    # everything else sits behind the camera (culled at once); the visible ones are spread over the index
    # range so that their indices need all 21 bits
    where = np.sort(rng.choice(P, n, replace=False))
    where[-1] = P - 1
    back = np.zeros((P, 3))
    back[:, 2] = rng.uniform(-3.0, -1.0, size=P)
    back[:, :2] = rng.uniform(-1.0, 1.0, size=(P, 2))
    scene = dict(means3D=world_from_view(back, cam).astype(np.float32),
                 scales=np.full((P, 3), 0.02, np.float32),
                 rotations=np.tile(np.array([[1, 0, 0, 0]], np.float32), (P, 1)),
                 opacities=np.full((P, 1), 0.5, np.float32),
                 colors_precomp=rng.random((P, 3)).astype(np.float32), sh_degree=0)
    for key in ("means3D", "scales", "rotations", "opacities"):
        scene[key][where] = vis[key]
    return scene, cam, np.array([0.1, 0.2, 0.3], np.float32)


CASES = dict(near49=near49, tele20=tele20, offaxis=offaxis, inside=inside, deep=deep, wide_field=wide_field)
GRAD_KEYS = dict(near49="sh", tele20="sh", offaxis="sh", inside="sh", deep="sh", wide_field="colors")


def grad_keys(name):
    return ["means3D", "means2D", "opacity", GRAD_KEYS[name], "scales", "rotations"]


_CACHE = {}


def get(name):
    """The case, built once per process (treat the arrays as read-only)."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]
