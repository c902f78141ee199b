"""Seeded synthetic plane-sweep inputs (SURVEY.md section 8d recipe).

There are no datasets in this environment, so every parity test, the golden fixtures and
``bench.py`` use the same generator: uniform-random frames in [-1, 1] (the range the
reference's dataset transform produces, datasets/multi_view_stereo_dataset.py:100-106), a
pin-hole K with focal 0.8*cols and the principal point at the image centre, and source
cameras rotated about y and translated sideways.  A ``smooth`` option renders a band-limited
texture instead of white noise so that cost volumes have real minima.

The output is a *batch dict* in the layout the reference's DataLoader yields and
``multi_view_unpack_batch`` consumes (multi_view_stereonet_utils.py:541-594):
  left_image (B,3,H,W), right_image [S x (B,3,H,W)], K (B,1,4,4), T_right_in_left [S x (B,1,4,4)].
Everything is generated with a CPU ``torch.Generator`` so the numbers are identical on the
build container and on the GPU box.
"""
import math
from typing import Dict, List

import torch


def _smooth_image(gen: torch.Generator, batch: int, rows: int, cols: int) -> torch.Tensor:
    """Sum of a few random low-frequency sinusoids per channel, scaled into [-1, 1]."""
    yy = torch.arange(rows, dtype=torch.float32).view(1, 1, rows, 1) / rows
    xx = torch.arange(cols, dtype=torch.float32).view(1, 1, 1, cols) / cols
    img = torch.zeros(batch, 3, rows, cols)
    for _ in range(6):
        fx = torch.rand(batch, 3, 1, 1, generator=gen) * 12.0
        fy = torch.rand(batch, 3, 1, 1, generator=gen) * 12.0
        ph = torch.rand(batch, 3, 1, 1, generator=gen) * (2.0 * math.pi)
        amp = torch.rand(batch, 3, 1, 1, generator=gen)
        img = img + amp * torch.sin(2.0 * math.pi * (fx * xx + fy * yy) + ph)
    img = img / img.abs().amax(dim=(2, 3), keepdim=True).clamp_min(1e-6)
    return img.contiguous()


def make_batch(rows: int, cols: int, num_sources: int, batch: int = 1, seed: int = 0,
               smooth: bool = False, pose_jitter: float = 0.0) -> Dict[str, object]:
    """Return a DataLoader-style batch dict of synthetic frames and cameras.

    ``pose_jitter`` > 0 perturbs the angle and translation of every batch element
    independently (relative magnitude), so that batched kernels are exercised with a
    different homography family per element.
    """
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)

    def frame():
        if smooth:
            return _smooth_image(gen, batch, rows, cols)
        return (torch.rand(batch, 3, rows, cols, generator=gen) * 2.0 - 1.0).contiguous()

    left = frame()
    rights: List[torch.Tensor] = [frame() for _ in range(num_sources)]

    K = torch.eye(4, dtype=torch.float32)
    K[0, 0] = 0.8 * cols
    K[1, 1] = 0.8 * cols
    K[0, 2] = (cols - 1) / 2.0
    K[1, 2] = (rows - 1) / 2.0
    K = K.view(1, 1, 4, 4).repeat(batch, 1, 1, 1).contiguous()

    poses = []
    for i in range(num_sources):
        ang = 0.03 * (i + 1)
        sign = 1.0 if i % 2 == 0 else -1.0
        T = torch.eye(4, dtype=torch.float32)
        c, s = math.cos(ang), math.sin(ang)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
        T[0, 3], T[1, 3], T[2, 3] = sign * 0.5 * (i + 1), 0.05, 0.02
        Tb = T.view(1, 1, 4, 4).repeat(batch, 1, 1, 1).contiguous()
        if pose_jitter > 0.0:
            for b in range(batch):
                j = (torch.rand(4, generator=gen) * 2.0 - 1.0) * pose_jitter
                a = ang * (1.0 + float(j[0]))
                cb, sb = math.cos(a), math.sin(a)
                Tb[b, 0, 0, 0], Tb[b, 0, 0, 2], Tb[b, 0, 2, 0], Tb[b, 0, 2, 2] = cb, sb, -sb, cb
                Tb[b, 0, 0, 3] *= 1.0 + float(j[1])
                Tb[b, 0, 1, 3] *= 1.0 + float(j[2])
                Tb[b, 0, 2, 3] *= 1.0 + float(j[3])
        poses.append(Tb)

    return {"left_image": left, "right_image": rights, "K": K, "T_right_in_left": poses,
            "left_filename": ["synthetic"] * batch,
            "right_filename": [["synthetic"] * batch for _ in range(num_sources)]}


def with_camera(batch: Dict[str, object], fy_scale=1.0, dcx=0.0, dcy=0.0, fx=None, fy=None, cx=None, cy=None):
    """The same batch seen through another pin-hole camera: K (B,1,4,4) is changed IN PLACE (and the batch returned), in
    fp32, before any unpacker sees it.  `fx` / `fy` / `cx` / `cy` set an entry outright; then fy = fy_scale * fx replaces
    fy (fy_scale != 1) and the principal point moves by (dcx, dcy).  Every argument is a number for the whole batch or a
    sequence with one value per batch element (a different camera per element)."""
    K = batch["K"]
    B = K.shape[0]

    def per_element(v):
        return torch.as_tensor(v, dtype=torch.float32).expand(B) if v is not None else None

    for (i, j), v in (((0, 0), fx), ((1, 1), fy), ((0, 2), cx), ((1, 2), cy)):
        if v is not None:
            K[:, 0, i, j] = per_element(v)
    scale = per_element(fy_scale)
    K[:, 0, 1, 1] = torch.where(scale != 1.0, K[:, 0, 0, 0] * scale, K[:, 0, 1, 1])
    K[:, 0, 0, 2] += per_element(dcx)
    K[:, 0, 1, 2] += per_element(dcy)
    return batch


# ---- an analytic scene with exact depth, for the depth-map fusion (fusion.py) ----------------------------------------
# A slanted plane n.X = h behind a sphere, seen by cameras on an arc about the y axis that all look at a pivot point.
# Depth is ray-cast exactly (fp64), so a fusion can be checked against the true surface.
SCENE_PLANE_NORMAL = (0.15, -0.25, -1.0)     # (normalised in fusion_scene_raycast)
SCENE_PLANE_POINT = (0.0, 0.0, 7.0)
SCENE_SPHERE_CENTER = (0.2, -0.1, 4.4)
SCENE_SPHERE_RADIUS = 0.9
SCENE_PIVOT = (0.0, 0.0, 5.0)


def fusion_scene_poses(views: int, arc: float = 0.3, dtype=torch.float64) -> torch.Tensor:
    """T_cam_in_world (V,4,4): camera i on a circle of radius 5 about SCENE_PIVOT in the x-z plane, at angle
    (i - (V-1)/2) * arc / (V-1) (the whole arc spans `arc` radians), looking at the pivot, y axis shared."""
    T = torch.zeros(views, 4, 4, dtype=dtype)
    px, py, pz = SCENE_PIVOT
    for i in range(views):
        th = (i - (views - 1) / 2.0) * (arc / max(views - 1, 1))
        s, c = math.sin(th), math.cos(th)
        T[i, :3, 0] = torch.tensor([c, 0.0, s], dtype=dtype)        # camera x in the world
        T[i, :3, 1] = torch.tensor([0.0, 1.0, 0.0], dtype=dtype)    # camera y
        T[i, :3, 2] = torch.tensor([-s, 0.0, c], dtype=dtype)       # camera z: towards the pivot
        T[i, :3, 3] = torch.tensor([px + 5.0 * s, py, pz - 5.0 * c], dtype=dtype)
        T[i, 3, 3] = 1.0
    return T


def fusion_scene_intrinsics(views: int, rows: int, cols: int, dtype=torch.float64) -> torch.Tensor:
    K = torch.eye(4, dtype=dtype)
    K[0, 0] = K[1, 1] = 0.8 * cols
    K[0, 2], K[1, 2] = (cols - 1) / 2.0, (rows - 1) / 2.0
    return K.expand(views, 4, 4).clone()


def fusion_scene_raycast(K: torch.Tensor, T: torch.Tensor, x: torch.Tensor, y: torch.Tensor):
    """Exact z-depth and surface label (0 plane, 1 sphere, -1 nothing) of the rays through pixel (x, y) of cameras
    (K, T_cam_in_world), all fp64; x, y broadcast against K[..., 0, 0]."""
    K, T = K.to(torch.float64), T.to(torch.float64)
    x, y = x.to(torch.float64), y.to(torch.float64)
    fx, fy, sk = K[..., 0, 0, None], K[..., 1, 1, None], K[..., 0, 1, None]
    cx, cy = K[..., 0, 2, None], K[..., 1, 2, None]
    yc = (y - cy) / fy
    xc = (x - cx - sk * yc) / fx
    d = torch.stack([xc, yc, torch.ones_like(xc)], -1)                        # camera ray, z = 1
    R, c = T[..., None, :3, :3], T[..., None, :3, 3]
    dw = (R @ d[..., None])[..., 0]                                           # world ray
    cw = c.expand_as(dw)
    n = torch.tensor(SCENE_PLANE_NORMAL, dtype=torch.float64, device=dw.device)
    n = n / n.norm()
    h = (n * torch.tensor(SCENE_PLANE_POINT, dtype=torch.float64, device=dw.device)).sum()
    t_plane = (h - (cw * n).sum(-1)) / (dw * n).sum(-1)
    s0 = torch.tensor(SCENE_SPHERE_CENTER, dtype=torch.float64, device=dw.device)
    oc = cw - s0
    a = (dw * dw).sum(-1)
    b = (oc * dw).sum(-1)
    disc = b * b - a * ((oc * oc).sum(-1) - SCENE_SPHERE_RADIUS ** 2)
    t_sph = (-b - disc.clamp_min(0).sqrt()) / a
    sph = (disc > 0) & (t_sph > 0)
    plane = t_plane > 0
    depth = torch.where(sph, t_sph, torch.where(plane, t_plane, torch.zeros_like(t_plane)))
    label = torch.where(sph, torch.ones_like(t_sph, dtype=torch.int8),
                        torch.where(plane, torch.zeros_like(t_sph, dtype=torch.int8),
                                    torch.full_like(t_sph, -1, dtype=torch.int8)))
    return depth, label


def fusion_scene_surface_distance(points: torch.Tensor) -> torch.Tensor:
    """Distance of world points (N,3) to the nearer of the two analytic surfaces (fp64)."""
    p = points.to(torch.float64)
    n = torch.tensor(SCENE_PLANE_NORMAL, dtype=torch.float64, device=p.device)
    n = n / n.norm()
    h = (n * torch.tensor(SCENE_PLANE_POINT, dtype=torch.float64, device=p.device)).sum()
    s0 = torch.tensor(SCENE_SPHERE_CENTER, dtype=torch.float64, device=p.device)
    return torch.minimum(((p * n).sum(-1) - h).abs(), ((p - s0).norm(dim=-1) - SCENE_SPHERE_RADIUS).abs())


def fusion_scene(views: int, rows: int, cols: int, arc: float = 0.3, device="cpu", K=None) -> Dict[str, torch.Tensor]:
    """Posed frames of the analytic scene: depth (V,1,H,W) fp32, label (V,1,H,W) int8, images (V,3,H,W) fp32 in [-1,1]
    (a texture fixed to the surfaces), K and T_cam_in_world (V,4,4) fp32 (the depth is ray-cast with these fp32
    cameras).  `K` (V,4,4): the views' own intrinsics instead of fusion_scene_intrinsics (fx != fy, off-centre, a
    camera per view)."""
    K = (fusion_scene_intrinsics(views, rows, cols) if K is None else K.cpu()).to(torch.float32)
    T = fusion_scene_poses(views, arc).to(torch.float32)
    ys, xs = torch.meshgrid(torch.arange(rows, dtype=torch.float64, device=device),
                            torch.arange(cols, dtype=torch.float64, device=device), indexing="ij")
    depth, label = fusion_scene_raycast(K.to(device)[:, None], T.to(device)[:, None], xs.reshape(1, 1, -1),
                                        ys.reshape(1, 1, -1))
    depth, label = depth.reshape(views, 1, rows, cols), label.reshape(views, 1, rows, cols)
    # world point of every pixel -> texture
    Kd, Td = K.to(device, torch.float64), T.to(device, torch.float64)
    xc = (xs - Kd[:, None, None, 0, 2]) / Kd[:, None, None, 0, 0]
    yc = (ys - Kd[:, None, None, 1, 2]) / Kd[:, None, None, 1, 1]
    cam = torch.stack([xc, yc, torch.ones_like(xc)], -1) * depth[:, 0, :, :, None]
    Xw = (Td[:, None, None, :3, :3] @ cam[..., None])[..., 0] + Td[:, None, None, :3, 3]
    freq = torch.tensor([[3.1, 1.7, 2.3], [1.3, 4.1, 0.7], [2.2, 0.9, 3.7]], dtype=torch.float64, device=device)
    img = torch.sin(Xw @ freq.T * 2.0 + torch.tensor([0.3, 1.1, 2.0], dtype=torch.float64, device=device))
    img = torch.where(depth[:, 0, :, :, None] > 0, img, torch.zeros_like(img)).permute(0, 3, 1, 2)
    return {"depth": depth.to(torch.float32).contiguous(), "label": label.contiguous(),
            "images": img.to(torch.float32).contiguous(), "K": K.to(device), "T_cam_in_world": T.to(device)}
