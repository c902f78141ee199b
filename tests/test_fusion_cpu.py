"""Depth-map fusion without a GPU: the float64 restatement (tests/fusion_reference.py) on the analytic scene of
synthetic.fusion_scene, the PLY writer, host-side validation and the library's exports."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fusion_reference import fuse_reference, nearest_neighbours
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import fuse_depthmaps, reconstruct, write_ply

VIEWS, ROWS, COLS = 6, 96, 128


@pytest.fixture(scope="module")
def scene():
    return synthetic.fusion_scene(VIEWS, ROWS, COLS)


@pytest.fixture(scope="module")
def fused(scene):
    nb = nearest_neighbours(VIEWS, VIEWS - 1)
    return nb, fuse_reference(scene["depth"], scene["K"], scene["T_cam_in_world"], nb, images=scene["images"])


def _clean_visible_slots(scene, nb):
    """Per reference pixel, the number of neighbour slots that see its surface point unoccluded, with all four taps
    (and the taps beside them) on the same surface and inside the image: slots that must confirm the pixel."""
    K, T = scene["K"].double(), scene["T_cam_in_world"].double()
    depth, label = scene["depth"][:, 0].double(), scene["label"][:, 0].long()
    ys, xs = torch.meshgrid(torch.arange(ROWS, dtype=torch.float64), torch.arange(COLS, dtype=torch.float64),
                            indexing="ij")
    lab = label.numpy()
    # label windows: a tap is clean where its 3x3 neighbourhood carries one surface
    from numpy.lib.stride_tricks import sliding_window_view
    pad = np.pad(lab, ((0, 0), (1, 1), (1, 1)), constant_values=-2)
    win = sliding_window_view(pad, (3, 3), axis=(1, 2))
    uniform = (win.min(axis=(-1, -2)) == win.max(axis=(-1, -2)))
    out = np.zeros((VIEWS, ROWS * COLS), np.int64)
    for r in range(VIEWS):
        Kinv = torch.linalg.inv(K[r, :3, :3])
        X = depth[r].reshape(-1) * (Kinv @ torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(ROWS * COLS,
                                                                                                   dtype=torch.float64)]))
        Xw = T[r, :3, :3] @ X + T[r, :3, 3:]
        for s in nb[r]:
            Ts = torch.linalg.inv(T[s])
            Xs = Ts[:3, :3] @ Xw + Ts[:3, 3:]
            uvw = K[s, :3, :3] @ Xs
            u, v = (uvw[0] / uvw[2]).numpy(), (uvw[1] / uvw[2]).numpy()
            fu, fv = np.floor(u), np.floor(v)
            inside = (Xs[2].numpy() > 0) & (fu >= 0) & (fu + 1 <= COLS - 1) & (fv >= 0) & (fv + 1 <= ROWS - 1)
            x0 = np.clip(fu, 0, COLS - 2).astype(np.int64)
            y0 = np.clip(fv, 0, ROWS - 2).astype(np.int64)
            own = lab[r].reshape(-1)
            clean = inside.copy()
            for dy in (0, 1):
                for dx in (0, 1):
                    clean &= uniform[s, y0 + dy, x0 + dx] & (lab[s, y0 + dy, x0 + dx] == own)
            # unoccluded: the ray of (u, v) in s meets the surface at the point's own depth
            seen, _ = synthetic.fusion_scene_raycast(K[s], T[s], torch.from_numpy(np.where(inside, u, 0.0)),
                                                     torch.from_numpy(np.where(inside, v, 0.0)))
            clean &= np.abs(seen.numpy() - Xs[2].numpy()) < 1e-6 * Xs[2].numpy()
            out[r] += clean
    return out.reshape(VIEWS, 1, ROWS, COLS)


def test_restatement_keeps_every_cleanly_visible_pixel(scene, fused):
    nb, ref = fused
    visible = _clean_visible_slots(scene, nb)
    must = visible >= 2
    assert must.mean() > 0.8, must.mean()
    assert ref["keep"][must].all(), int((must & ~ref["keep"]).sum())
    # every clean slot confirms: the count is at least the number of clean slots
    assert (ref["count"] >= visible).all()


def test_restatement_points_lie_on_the_surface(scene, fused):
    _, ref = fused
    pts = torch.from_numpy(ref["points"])
    depth = ref["fused"][ref["keep"]]
    rel = synthetic.fusion_scene_surface_distance(pts).numpy() / depth
    # Bilinear sampling of depth is exact on neither the slanted plane nor the sphere, and a neighbour's taps next to the
    # sphere's silhouette mix the two surfaces with a weight small enough to stay within max_rel_depth.  Measured on
    # this scene: median 1.3e-6, 99 % 3.8e-4, max 3.2e-3 (plane pixels beside the silhouette in a neighbour).
    assert np.quantile(rel, 0.99) < 1e-3
    assert rel.max() < 4e-3
    assert len(pts) == ref["keep"].sum() and len(pts) > 0.8 * VIEWS * ROWS * COLS


def test_restatement_rejects_a_scaled_view(scene, fused):
    nb, ref = fused
    depth = scene["depth"].clone()
    depth[2] *= 1.05
    bad = fuse_reference(depth, scene["K"], scene["T_cam_in_world"], nb)
    # the scaled view emits nothing, except where a neighbour's taps straddle the sphere's silhouette and the bilinear
    # mix of the two surfaces happens to match the scaled depth (4 pixels on this scene, all next to the silhouette)
    from numpy.lib.stride_tricks import sliding_window_view
    win = sliding_window_view(np.pad(scene["label"][:, 0].numpy(), ((0, 0), (3, 3), (3, 3)), mode="edge"), (7, 7),
                              axis=(1, 2))
    near_edge = (win.min(axis=(-1, -2)) != win.max(axis=(-1, -2)))[:, None]
    emitted = bad["pixel"][bad["view"] == 2]
    assert len(emitted) <= 8 and near_edge[2].reshape(-1)[emitted].all(), emitted
    # the other views lose exactly the confirmations the scaled view gave: re-run them with view 2 masked out of
    # their neighbour lists and compare with the clean run
    was = np.zeros_like(ref["count"])
    for r in range(VIEWS):
        if r == 2:
            continue
        only2 = np.where(nb[r:r + 1] == 2, 2, -1)
        one = fuse_reference(scene["depth"], scene["K"], scene["T_cam_in_world"], only2, ref_views=[r],
                             min_consistent=1)
        was[r] = one["count"][0]
    # (the same kind of chance match -- a bilinear mix across a depth discontinuity that lands within the thresholds --
    # can let the scaled view still confirm a pixel: 42 of the other views' 61440 pixels on this scene)
    drop = ref["count"] - bad["count"]
    off = (drop != was)
    off[2] = False
    assert off.sum() <= 1e-3 * off.size, off.sum()
    assert (np.abs(drop - was)[off] == 1).all()
    assert (np.delete(was, 2, axis=0) > 0).mean() > 0.5


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    for colors in (None, cols):
        path = os.path.join(tmp_path, "cloud.ply")
        write_ply(path, torch.from_numpy(pts), None if colors is None else torch.from_numpy(colors))
        blob = open(path, "rb").read()
        end = blob.index(b"end_header\n") + len(b"end_header\n")
        header = blob[:end].decode("ascii").splitlines()
        assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
        props = [ln.split()[1:] for ln in header if ln.startswith("property")]
        want = [["float", "x"], ["float", "y"], ["float", "z"]]
        if colors is not None:
            want += [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
        assert props == want and header[-1] == "end_header"
        dt = [("p", "<f4", 3)] + ([("c", "u1", 3)] if colors is not None else [])
        rec = np.frombuffer(blob[end:], dtype=dt)
        assert len(rec) == 37
        np.testing.assert_array_equal(rec["p"], pts)
        if colors is not None:
            np.testing.assert_array_equal(rec["c"], cols)


def _args(V=4, H=8, W=12):
    depth = torch.ones(V, 1, H, W)
    K = torch.eye(4).expand(V, 4, 4).clone()
    T = torch.eye(4).expand(V, 4, 4).clone()
    return depth, K, T


@pytest.mark.parametrize("neighbours, kwargs, match", [
    ([[0, 1], [0, 2], [0, 1], [0, 1]], {}, "own neighbour"),          # view 0 lists itself
    ([[1, 4], [0, 2], [0, 1], [0, 1]], {}, r"\[-1, 4\)"),              # index >= V
    ([[1, -2], [0, 2], [0, 1], [0, 1]], {}, r"\[-1, 4\)"),
    (np.zeros((4, 0), np.int64), {}, "1..32 slots"),                   # M = 0
    (np.full((4, 33), -1, np.int64), {}, "1..32 slots"),               # M > 32
    ([[1, 2], [0, 2]], {}, "rows for 4 reference views"),              # R != len(ref_views)
    ([[1, 2], [0, 2]], {"ref_views": [0, 1]}, None),                   # ... unless ref_views says so: then the CPU
    ([[1, 2], [2, 3]], {"ref_views": [0, 2]}, "own neighbour"),
])
def test_host_validation(neighbours, kwargs, match):
    depth, K, T = _args()
    if match is None:   # valid arguments on CPU tensors: no CPU implementation
        with pytest.raises(RuntimeError, match="HIP devices only"):
            fuse_depthmaps(depth, K, T, neighbours, **kwargs)
        return
    with pytest.raises(ValueError, match=match):
        fuse_depthmaps(depth, K, T, neighbours, **kwargs)


def test_host_validation_shapes():
    depth, K, T = _args()
    nb = [[1], [0], [1], [2]]
    with pytest.raises(ValueError, match=r"K must be a \(4,4,4\)"):
        fuse_depthmaps(depth, K[:3], T, nb)
    with pytest.raises(ValueError, match="T_cam_in_world"):
        fuse_depthmaps(depth, K, T[:, :3], nb)
    with pytest.raises(ValueError, match="images must be"):
        fuse_depthmaps(depth, K, T, nb, images=torch.zeros(4, 3, 8, 11))
    with pytest.raises(ValueError, match="valid must be"):
        fuse_depthmaps(depth, K, T, nb, valid=torch.ones(4, 1, 7, 12, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"\(V,1,H,W\)"):
        fuse_depthmaps(depth[:, 0], K, T, nb)
    with pytest.raises(ValueError, match="at least one pixel"):
        fuse_depthmaps(torch.ones(4, 1, 0, 5), K, T, nb)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        fuse_depthmaps(depth, K, T, nb)


def test_fusion_symbols_are_exported():
    lib = ctypes.CDLL(_native.library_path())
    for name in ("mvsn_fusion_workspace_bytes", "mvsn_fusion_consistency", "mvsn_fusion_emit"):
        assert hasattr(lib, name) and name in _native.SIGNATURES
    typed = _native.load()
    assert typed.mvsn_fusion_workspace_bytes(64, 4, 256, 512) > 0
    assert typed.mvsn_fusion_workspace_bytes(64, 0, 256, 512) == 0       # M out of 1..32: no plan
    assert typed.mvsn_fusion_workspace_bytes(64, 33, 256, 512) == 0


def test_reconstruct_rejects_a_zero_baseline_before_any_launch():
    sc = synthetic.fusion_scene(3, 16, 32)
    T = sc["T_cam_in_world"].clone()
    T[1] = T[0]                                   # view 1 sits on view 0: zero baseline for view 0's first source
    with pytest.raises(AssertionError, match="baseline"):
        reconstruct(None, sc["images"], sc["K"], T, np.array([[1, 2], [0, 2], [1, 0]]))
    with pytest.raises(ValueError, match="S real source views"):
        reconstruct(None, sc["images"], sc["K"], sc["T_cam_in_world"], np.array([[1, -1], [0, 2], [1, 0]]))
