"""The ray-cast of the TSDF volume on the device (csrc/mvsn_tsdf_raycast.hip) against the numpy restatement
(tests/tsdf_raycast_reference.py): the hit mask exactly and the four maps within the derived bounds outside the borderline
pixels, all-zero maps where nothing can be hit, the exact properties (repeatable, a view alone = the view among others, the
state-level function = the method), and the scene end to end.  Inputs sit in poisoned buffers and every output and the
workspace between guard bands."""
import functools

import numpy as np
import pytest
import torch

from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, synthetic, tsdf
from multi_view_stereonet_amd.tsdf import TSDFVolume
from tsdf_raycast_reference import CASE_IDS, CASES, EPS, NO_HIT_IDS, reference, render_case, scene, scene_camera
from tsdf_reference import scene_mesh_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAPS = ("depth", "normals", "colors", "weight")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _device_raycast(name, fill=POISON_NAN):
    """mvsn_tsdf_raycast on a case whose inputs sit in poisoned buffers of their own (16-byte aligned only), the four
    maps and the workspace carved between guard bands: a dict of numpy arrays (V,C,H,W), colors None without colour.
    Made once per (case, poison), never modified."""
    c = render_case(name)
    s_np, w_np, c_np = c["state"]
    nz, ny, nx = s_np.shape
    V, (H, W) = c["K"].shape[0], c["size"]
    kw = c["kw"]
    guard = Guard(_alloc, fill)
    put = lambda a: guard.poisoned(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))   # noqa: E731
    s, w = put(s_np), put(w_np)
    col = put(c_np) if c_np is not None else None
    K, T = put(c["K"]), put(c["T"])
    lib = _native.load()
    ws_bytes = lib.mvsn_tsdf_raycast_workspace_bytes(nx, ny, nz)
    assert ws_bytes >= 4 * nx * ny * nz
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    depth, normals = guard.empty((V, 1, H, W), torch.float32, DEV), guard.empty((V, 3, H, W), torch.float32, DEV)
    colors = guard.empty((V, 3, H, W), torch.float32, DEV) if col is not None else None
    weight = guard.empty((V, 1, H, W), torch.float32, DEV)
    o = np.asarray(c["origin"], np.float32)
    f = lambda x: float(np.float32(x))   # noqa: E731
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_tsdf_raycast(
            _native.ptr(s), _native.ptr(w), _native.ptr(col), nx, ny, nz, f(c["voxel_size"]), float(o[0]), float(o[1]),
            float(o[2]), _native.ptr(K), _native.ptr(T), V, H, W, f(kw.get("min_weight", 1.0)), f(kw.get("min_depth", 0.0)),
            f(kw.get("max_depth", np.inf)), f(kw["step"]), _native.ptr(ws), ws_bytes, _native.ptr(depth),
            _native.ptr(normals), _native.ptr(colors), _native.ptr(weight), _native.stream()), "mvsn_tsdf_raycast")
    torch.cuda.synchronize()
    guard.check()
    return {"depth": depth.cpu().numpy(), "normals": normals.cpu().numpy(),
            "colors": colors.cpu().numpy() if colors is not None else None, "weight": weight.cpu().numpy()}


def _compare_view(got, ref, what):
    """One view: got maps (C,H,W) fp32, ref a dict of raycast_reference.  Returns the largest ratios to the bounds."""
    depth, weight = got["depth"][0].astype(np.float64), got["weight"][0].astype(np.float64)
    normals = got["normals"].astype(np.float64)
    colors = got["colors"].astype(np.float64) if got["colors"] is not None else None
    assert (ref["colors"] is None) == (colors is None)
    for a in (depth, weight, normals) + ((colors,) if colors is not None else ()):
        assert np.isfinite(a).all(), "a NaN came through"
    # the output conventions, on every pixel: no hit <=> depth 0, and then zeros everywhere; a normal is a unit vector or 0
    hit = depth != 0
    assert (depth >= 0).all()
    nlen = np.sqrt((normals ** 2).sum(0))
    assert ((nlen == 0) | (np.abs(nlen - 1) <= 4 * EPS)).all()
    miss = ~hit
    assert not weight[miss].any() and not normals[:, miss].any() and (colors is None or not colors[:, miss].any())
    assert (weight[hit] >= 0).all()
    if colors is not None:                                        # an undefined hit cell zeroes the three together
        assert not colors[:, weight == 0].any() and not normals[:, weight == 0].any()
    clear = ~ref["borderline"]
    np.testing.assert_array_equal(hit[clear], ref["hit"][clear], err_msg="the hit mask differs off the borderline pixels")
    sel = clear & ref["hit"]
    ratios = {"depth": 0.0, "weight": 0.0, "colors": 0.0, "angle": 0.0}
    if sel.any():
        err = np.abs(depth - ref["depth"])[sel]
        ratios["depth"] = float((err / ref["depth_bound"][sel]).max())
        here = sel & ref["defined"]
        np.testing.assert_array_equal((weight != 0)[sel], here[sel])          # (a defined cell has weights >= min_weight > 0)
        if here.any():
            ratios["weight"] = float((np.abs(weight - ref["weight"])[here] / ref["weight_bound"][here]).max())
            if colors is not None:
                ratios["colors"] = float((np.abs(colors - ref["colors"])[:, here] / ref["color_bound"][None, here]).max())
            bounded = here & np.isfinite(ref["angle_bound"])
            np.testing.assert_array_equal((nlen != 0)[bounded], (ref["normals"] != 0).any(0)[bounded])
            unit = bounded & (nlen != 0)
            if unit.any():
                cosine = np.clip((normals * ref["normals"]).sum(0)[unit] / nlen[unit], -1, 1)
                sine = np.linalg.norm(np.cross(normals[:, unit].T, ref["normals"][:, unit].T), axis=1)
                ratios["angle"] = float((np.arctan2(sine, cosine) / ref["angle_bound"][unit]).max())
    print(f"{what}: {int(ref['hit'].sum())} hits of {hit.size}, {int(ref['borderline'].sum())} borderline, "
          f"{int((sel & ~np.isfinite(ref['angle_bound'])).sum())} hits at a cell face; error / bound max: "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert ratios["depth"] <= 1 and ratios["weight"] <= 1 and ratios["colors"] <= 1 and ratios["angle"] <= 1, ratios
    return ratios


@pytest.mark.parametrize("name", CASE_IDS)
def test_raycast_matches_the_restatement(name):
    got = _device_raycast(name)
    for v, ref in enumerate(reference(name)):
        _compare_view({k: (None if got[k] is None else got[k][v]) for k in MAPS}, ref, f"{name}[{v}]")


@pytest.mark.parametrize("name", NO_HIT_IDS)
def test_no_hit_cases_give_zero_bits(name):
    got = _device_raycast(name)
    for key in MAPS:
        assert got[key] is not None and not got[key].view(np.uint32).any(), key


@pytest.mark.parametrize("name", ["shape_1x1", "shape_1x1029", "shape_37x61", "views3_37x61", "sphere_rolled_17x9",
                                  "nan_under_weight_0_rolled_23x31", "no_colour_rolled_23x31", "case0_novel_step",
                                  "case4_input_clip"])
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _device_raycast; an element nobody writes, or a read of
    # foreign memory that reaches a result, differs between the two fills)
    a, b = _device_raycast(name, POISON_NAN), _device_raycast(name, POISON_FINITE)
    for key in MAPS:
        assert (a[key] is None) == (b[key] is None)
        if a[key] is not None:
            assert a[key].tobytes() == b[key].tobytes(), key


def _sphere_volume(name):
    c = render_case(name)
    s, w, col = c["state"]
    nz, ny, nx = s.shape
    vol = TSDFVolume((nx, ny, nz), c["voxel_size"], c["origin"], 0.4, device=DEV, color=col is not None)
    vol.sdf_sum.copy_(torch.from_numpy(s))
    vol.weight.copy_(torch.from_numpy(w))
    if col is not None:
        vol.color_sum.copy_(torch.from_numpy(col))
    return vol, c


def test_reproducible_view_by_view_and_on_the_state():
    vol, c = _sphere_volume("views3_37x61")
    K, T = torch.from_numpy(c["K"]).to(DEV), torch.from_numpy(c["T"]).to(DEV)
    kw = dict(c["kw"])
    whole = vol.raycast(K, T, c["size"], **kw)
    assert isinstance(whole, tsdf.TSDFRender) and whole.depth.shape == (3, 1, 37, 61) and whole.colors.shape == (3, 3, 37, 61)
    assert float((whole.depth > 0).float().mean()) > 0.5
    again = vol.raycast(K, T, c["size"], **kw)
    state = tsdf.raycast(vol.sdf_sum, vol.weight, vol.color_sum, vol.voxel_size, vol.origin, K.double(), T.double(),
                         c["size"], **kw)
    for a, b, s in zip(whole, again, state):
        assert bits_equal(a, b) and bits_equal(a, s)
    for v in range(3):
        one = vol.raycast(K[v:v + 1], T[v:v + 1], c["size"], **kw)
        for a, b in zip(whole, one):
            assert bits_equal(a[v:v + 1], b)
    # the method's default step (min(voxel_size, trunc / 4) = voxel_size here) is the state-level default, and the C
    # entry's maps are these bits too
    default = vol.raycast(K, T, c["size"])
    entry = _device_raycast("views3_37x61")
    for a, b, key in zip(whole, default, MAPS):
        assert bits_equal(a, b) and a.cpu().numpy().tobytes() == entry[key].tobytes()
    plain = TSDFVolume(vol.dims, vol.voxel_size, vol.origin, 0.4, device=DEV)
    plain.sdf_sum.copy_(vol.sdf_sum)
    plain.weight.copy_(vol.weight)
    r = plain.raycast(K, T, c["size"])
    assert r.colors is None and bits_equal(r.depth, whole.depth) and bits_equal(r.normals, whole.normals)


def test_scene_end_to_end():
    index = 0
    shape, dims, vs, origin, trunc = CASES[index]
    depth_np, images_np, K_np, T_np = scene(index)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)     # noqa: E731
    vol = TSDFVolume(dims, vs, origin, trunc, device=DEV, color=True)
    vol.integrate(to(depth_np)[:, None].contiguous(), to(K_np), to(T_np), images=to(images_np))

    def render(pose):
        K, T, size = scene_camera(index, pose, 1.0)
        r = vol.raycast(to(K)[None], to(T)[None], size)
        d = r.depth[0, 0].cpu().numpy().astype(np.float64)
        ys, xs = np.nonzero(d)
        cam = np.linalg.solve(K[:3, :3].astype(np.float64), np.stack([xs, ys, np.ones_like(xs)]).astype(np.float64)) * d[ys, xs]
        world = (T[:3, :3].astype(np.float64) @ cam).T + T[:3, 3].astype(np.float64)
        return r, d, world
    # every hit of the novel view lies near a true surface: the hit point lies between two samples of which the farther
    # has a negative interpolant, so a corner of its cell is inside, and section 15's bound for a mesh vertex holds for it
    bound = scene_mesh_bound(CASES[index], depth_np, K_np)
    r, d, world = render("novel")
    dist = synthetic.fusion_scene_surface_distance(torch.from_numpy(world)).numpy()
    ref = reference("case0_novel_step")[0]
    print(f"scene, novel pose: {world.shape[0]} hits (restatement on its own volume {int(ref['hit'].sum())}), distance to "
          f"the nearer analytic surface max {dist.max():.3e}, median {np.median(dist):.3e}, bound {bound:.3e}")
    assert world.shape[0] >= 200 and abs(world.shape[0] - int(ref["hit"].sum())) <= 0.05 * world.shape[0]
    assert dist.max() <= bound
    assert float((r.weight[0, 0][r.depth[0, 0] > 0] >= 1).float().mean()) > 0.9 and r.colors is not None
    # an integrating pose: the rendered map against the view's own input depth (recorded in DESIGN.md, no condition
    # beyond the bound above)
    r, d, world = render("input")
    dist = synthetic.fusion_scene_surface_distance(torch.from_numpy(world)).numpy()
    both = (d > 0) & (depth_np[shape[0] // 2] > 0)
    diff = np.abs(d - depth_np[shape[0] // 2])[both]
    print(f"scene, integrating pose: {world.shape[0]} hits, distance max {dist.max():.3e}; |rendered - input depth| over "
          f"{int(both.sum())} pixels hit in both: median {np.median(diff):.3e}, max {diff.max():.3e}")
    assert world.shape[0] >= 200 and dist.max() <= bound
    # normals face the camera on most of what it sees
    n = r.normals[0].cpu().numpy().astype(np.float64)[:, d > 0].T
    towards = T_np[shape[0] // 2][:3, 3].astype(np.float64) - world
    assert float(((n * towards).sum(1) > 0).mean()) > 0.9
