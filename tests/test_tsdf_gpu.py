"""The TSDF volume on the device (csrc/mvsn_tsdf.hip) against the numpy restatement (tests/tsdf_reference.py): the
integration within the derived per-voxel bound outside the borderline voxels (whose share is capped), the exact
properties of the sums (view by view = all at once, repeatable, untouched voxels keep their bits), Surface Nets with M, F,
the cell indices and the faces exactly and the vertices, normals and colours within their bounds, and the scene end to
end.  Inputs sit in poisoned buffers and the state and the outputs between guard bands."""
import functools

import numpy as np
import pytest
import torch

from guarded_alloc import POISON_FINITE, POISON_NAN, Guard, bits_equal
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.tsdf import TSDFVolume
from tsdf_reference import (BORDERLINE_CAP, CASES, SPHERE, case_id, case_variants, check_sphere_mesh, scene_mesh_bound,
                            sphere_state, surface_nets_reference, tsdf_integrate_reference)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


@functools.lru_cache(maxsize=None)
def _scene(shape):
    """depth (V,H,W), images (V,3,H,W), K, T_cam_in_world as numpy arrays: made once per shape, never modified."""
    sc = synthetic.fusion_scene(*shape)
    return sc["depth"][:, 0].numpy(), sc["images"].numpy(), sc["K"].numpy(), sc["T_cam_in_world"].numpy()


@functools.lru_cache(maxsize=None)
def _reference(index, variant, color):
    shape, dims, vs, origin, trunc = CASES[index]
    depth, images, K, T = _scene(shape)
    valid, weights, min_depth = case_variants(CASES[index])[variant]
    return tsdf_integrate_reference(depth, K, T, dims, vs, origin, trunc, images=images if color else None, valid=valid,
                                    weights=weights, min_depth=min_depth)


def _device_integrate(index, variant="plain", color=True, state=None, fill=POISON_NAN):
    """mvsn_tsdf_integrate on inputs that sit in poisoned buffers of their own (16-byte aligned only) and a state carved
    between guard bands: (sdf_sum, weight, color_sum) as numpy arrays."""
    shape, dims, vs, origin, trunc = CASES[index]
    V, H, W = shape
    nx, ny, nz = dims
    depth, images, K, T = _scene(shape)
    valid, weights, min_depth = case_variants(CASES[index])[variant]
    guard = Guard(_alloc, fill)
    put = lambda a, dtype: guard.poisoned(torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV))   # noqa: E731
    d, k, t = put(depth, torch.float32), put(K, torch.float32), put(T, torch.float32)
    m = put(valid, torch.uint8) if valid is not None else None
    wt = put(weights, torch.float32) if weights is not None else None
    im = put(images, torch.float32) if color else None
    if state is None:
        state = (np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32),
                 np.zeros((3, nz, ny, nx), np.float32))
    s, w = put(state[0], torch.float32), put(state[1], torch.float32)
    c = put(state[2], torch.float32) if color else None
    o = np.asarray(origin, np.float32)
    lib = _native.load()
    with torch.cuda.device(DEV):
        _native.check(lib.mvsn_tsdf_integrate(
            _native.ptr(d), _native.ptr(m), _native.ptr(wt), _native.ptr(im), _native.ptr(k), _native.ptr(t), V, H, W, nx,
            ny, nz, float(np.float32(vs)), float(o[0]), float(o[1]), float(o[2]), float(np.float32(trunc)),
            float(np.float32(min_depth)), _native.ptr(s), _native.ptr(w), _native.ptr(c), _native.stream()),
            "mvsn_tsdf_integrate")
    torch.cuda.synchronize()
    guard.check()
    return s.cpu().numpy(), w.cpu().numpy(), c.cpu().numpy() if color else None


def _compare(got, ref, unit_weights, what):
    s, w, c = (None if a is None else a.astype(np.float64) for a in got)
    assert np.isfinite(s).all() and np.isfinite(w).all() and (c is None or np.isfinite(c).all()), "a NaN came through"
    border = ref["borderline"]
    share = border.mean()
    clear = ~border
    dw = np.abs(w - ref["weight"])
    ds = np.abs(s - ref["sdf_sum"])
    ratio = (ds[clear] / np.maximum(ref["bound"][clear], 1e-300)).max() if clear.any() else 0.0
    dc = np.abs(c - ref["color_sum"]) if c is not None else np.zeros((3,) + s.shape)
    print(f"{what}: borderline {100 * share:.2f} %, weight differs on {int((dw[clear] > 0).sum())} clear and "
          f"{int((dw[border] > 0).sum())} of {int(border.sum())} borderline voxels, sdf_sum error / bound max {ratio:.3f}, "
          f"colour error max {dc[:, clear].max() if clear.any() else 0.0:.2e}")
    assert share <= BORDERLINE_CAP, share
    if unit_weights:
        assert (dw[clear] == 0).all(), "the set of updating views differs outside the borderline voxels"
    else:
        assert (dw[clear] <= ref["weight_bound"][clear]).all()
    assert (ds[clear] <= ref["bound"][clear]).all(), ratio
    if c is not None:
        assert (dc[:, clear] <= ref["color_bound"][:, clear]).all()
    assert (dw[border] <= ref["flippable"][border] * (1 + 2.0 ** -20)).all()      # (weights are at most 1)


@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_integration_matches_the_restatement(index, color):
    _compare(_device_integrate(index, color=color), _reference(index, "plain", color), True,
             f"{case_id(CASES[index])} colour={color}")


@pytest.mark.parametrize("variant", ["holes", "weights", "min_depth"])
@pytest.mark.parametrize("index", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_integration_with_optional_inputs(index, variant):
    _compare(_device_integrate(index, variant), _reference(index, variant, True), variant != "weights",
             f"{case_id(CASES[index])} {variant}")


def test_poison_does_not_reach_the_state():
    a = _device_integrate(0, "holes", fill=POISON_NAN)
    b = _device_integrate(0, "holes", fill=POISON_FINITE)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _volume(index, color=True):
    _, dims, vs, origin, trunc = CASES[index]
    return TSDFVolume(dims, vs, origin, trunc, device=DEV, color=color)


def _views(index):
    depth, images, K, T = _scene(CASES[index][0])
    to = lambda a: torch.from_numpy(a).to(DEV)     # noqa: E731
    return to(depth)[:, None].contiguous(), to(images), to(K), to(T)


@pytest.mark.parametrize("index", [0, 4], ids=[case_id(CASES[0]), case_id(CASES[4])])
def test_view_by_view_gives_the_bits_of_one_call(index):
    depth, images, K, T = _views(index)
    conf = torch.from_numpy(np.nan_to_num(case_variants(CASES[index])["weights"][1], nan=0.5)).to(DEV)[:, None].contiguous()
    whole, steps = _volume(index), _volume(index)
    whole.integrate(depth, K, T, images=images, weights=conf)
    for v in range(depth.shape[0]):
        steps.integrate(depth[v:v + 1], K[v:v + 1], T[v:v + 1], images=images[v:v + 1], weights=conf[v:v + 1])
    assert float(whole.weight.max()) > 1.5
    for a, b in ((whole.sdf_sum, steps.sdf_sum), (whole.weight, steps.weight), (whole.color_sum, steps.color_sum)):
        assert bits_equal(a, b)
    # and a second identical call on a reset volume gives identical bits
    again = _volume(index)
    again.integrate(depth, K, T, images=images, weights=conf)
    again.reset()
    assert not again.sdf_sum.any() and not again.weight.any() and not again.color_sum.any()
    again.integrate(depth, K, T, images=images, weights=conf)
    for a, b in ((whole.sdf_sum, again.sdf_sum), (whole.weight, again.weight), (whole.color_sum, again.color_sum)):
        assert bits_equal(a, b)
    vals = whole.values()
    assert bool((torch.isnan(vals) == (whole.weight == 0)).all())


def test_a_voxel_no_view_reaches_keeps_its_state():
    index = 0
    _, dims, _, _, _ = CASES[index]
    nx, ny, nz = dims
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2 ** 32, (5, nz, ny, nx), dtype=np.uint64).astype(np.uint32)    # any bits: NaNs, infinities, -0
    state = (bits[0].view(np.float32), bits[1].view(np.float32), bits[2:].view(np.float32))
    got = _device_integrate(index, "min_depth", state=state)
    ref = _reference(index, "min_depth", True)
    untouched = (ref["updates"] == 0) & ~ref["borderline"]
    assert untouched.sum() > 1000
    assert (got[0].view(np.uint32)[untouched] == bits[0][untouched]).all()
    assert (got[1].view(np.uint32)[untouched] == bits[1][untouched]).all()
    assert (got[2].view(np.uint32)[:, untouched] == bits[2:][:, untouched]).all()
    touched = (ref["updates"] > 0) & ~ref["borderline"]
    assert (got[1].view(np.uint32)[touched] != bits[1][touched]).mean() > 0.3     # (w + 1 == w above 2^24)


# ---- extraction ------------------------------------------------------------------------------------------------------
def _device_extract(state, min_weight, voxel_size, origin, fill=POISON_NAN):
    """mvsn_tsdf_classify + mvsn_tsdf_extract on a state in poisoned buffers, the workspace and every output between
    guard bands: a dict of numpy arrays like surface_nets_reference's."""
    s_np, w_np, c_np = state
    nz, ny, nx = s_np.shape
    guard = Guard(_alloc, fill)
    put = lambda a: guard.poisoned(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))   # noqa: E731
    s, w = put(s_np), put(w_np)
    c = put(c_np) if c_np is not None else None
    lib = _native.load()
    ws_bytes = lib.mvsn_tsdf_workspace_bytes(nx, ny, nz)
    assert ws_bytes > 0
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((2,), torch.int64, DEV)
    o = np.asarray(origin, np.float32)
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_tsdf_classify(_native.ptr(s), _native.ptr(w), nx, ny, nz, float(np.float32(min_weight)),
                                             _native.ptr(head), _native.ptr(ws), ws_bytes, st), "mvsn_tsdf_classify")
        m, both = head.tolist()
        assert 0 <= m <= nx * ny * nz and m <= both <= m + 3 * nx * ny * nz, (m, both)
        quads = both - m
        vertices, normals = guard.empty((m, 3), torch.float32, DEV), guard.empty((m, 3), torch.float32, DEV)
        colors = guard.empty((m, 3), torch.uint8, DEV) if c is not None else None
        faces, cell = guard.empty((2 * quads, 3), torch.int64, DEV), guard.empty((m,), torch.int64, DEV)
        _native.check(lib.mvsn_tsdf_extract(_native.ptr(s), _native.ptr(w), _native.ptr(c), nx, ny, nz,
                                            float(np.float32(voxel_size)), float(o[0]), float(o[1]), float(o[2]),
                                            float(np.float32(min_weight)), _native.ptr(ws), ws_bytes, m, quads,
                                            _native.ptr(vertices), _native.ptr(normals), _native.ptr(colors),
                                            _native.ptr(faces), _native.ptr(cell), st), "mvsn_tsdf_extract")
    torch.cuda.synchronize()
    guard.check()
    return {"vertices": vertices.cpu().numpy(), "normals": normals.cpu().numpy(),
            "colors": colors.cpu().numpy() if colors is not None else None, "faces": faces.cpu().numpy(),
            "cell": cell.cpu().numpy()}


def _compare_mesh(got, ref, what):
    assert got["cell"].shape == ref["cell"].shape and got["faces"].shape == ref["faces"].shape, \
        (got["cell"].shape, ref["cell"].shape, got["faces"].shape, ref["faces"].shape)
    np.testing.assert_array_equal(got["cell"], ref["cell"])
    np.testing.assert_array_equal(got["faces"], ref["faces"])
    if ref["cell"].shape[0] == 0:
        return
    assert np.isfinite(got["vertices"]).all() and np.isfinite(got["normals"]).all()
    dv = np.abs(got["vertices"].astype(np.float64) - ref["vertices"])
    n = got["normals"].astype(np.float64)
    defined = (ref["normals"] != 0).any(1)
    np.testing.assert_array_equal((n != 0).any(1), defined)
    cosine = np.clip((n * ref["normals"]).sum(1) / np.maximum(np.linalg.norm(n, axis=1), 1e-300), -1, 1)
    sine = np.linalg.norm(np.cross(n, ref["normals"]), axis=1)
    angle = np.arctan2(sine, cosine)[defined]
    print(f"{what}: M {ref['cell'].shape[0]}, F {ref['faces'].shape[0]}, vertex error / bound max "
          f"{(dv / ref['position_bound']).max():.3f}, angle / bound max "
          f"{(angle / ref['angle_bound'][defined]).max() if defined.any() else 0.0:.3f}")
    assert (dv <= ref["position_bound"]).all()
    assert (angle <= ref["angle_bound"][defined]).all()
    assert (np.abs(np.linalg.norm(n[defined], axis=1) - 1) <= 4 * 2.0 ** -24).all()
    if ref["colors"] is not None:
        assert np.abs(got["colors"].astype(np.int64) - ref["colors"].astype(np.int64)).max() <= 1
    else:
        assert got["colors"] is None


def _sphere_states():
    s, w, c = sphere_state(**SPHERE)
    holed = w.copy()
    holed[6:11, 7:12, 2:8] = 0.0
    s_nan, c_nan = s.copy(), c.copy()
    s_nan[holed == 0] = np.nan
    c_nan[:, holed == 0] = np.nan
    light = w.copy()
    light[6:11, 7:12, 2:8] = 0.5
    return {"sphere": ((s, w, c), 1.0), "hole": ((s, holed, c), 1.0), "nan_under_weight_0": ((s_nan, holed, c_nan), 1.0),
            "min_weight": ((s * light, light, c * light), 0.75), "no_colour": ((s, w, None), 1.0)}


@pytest.mark.parametrize("name", ["sphere", "hole", "nan_under_weight_0", "min_weight", "no_colour"])
def test_extraction_matches_the_restatement(name):
    state, min_weight = _sphere_states()[name]
    ref = surface_nets_reference(*state, min_weight, SPHERE["voxel_size"], SPHERE["origin"])
    assert ref["cell"].shape[0] > 400
    got = _device_extract(state, min_weight, SPHERE["voxel_size"], SPHERE["origin"])
    _compare_mesh(got, ref, name)
    if name == "sphere":                 # the manifold, Euler and orientation checks on the device mesh
        check_sphere_mesh(got["vertices"].astype(np.float64), got["normals"].astype(np.float64), got["faces"],
                          got["vertices"].shape[0])
        again = _device_extract(state, min_weight, SPHERE["voxel_size"], SPHERE["origin"], fill=POISON_FINITE)
        for key in ("vertices", "normals", "colors", "faces", "cell"):
            assert got[key].tobytes() == again[key].tobytes(), key


def test_extraction_of_one_cell_and_of_a_long_row():
    w = np.ones((2, 2, 2), np.float32)
    s = np.full((2, 2, 2), 3.0, np.float32)
    s[0, 0, 0] = -1.0
    ref = surface_nets_reference(s, w, None, 1.0, 2.0, (10.0, 20.0, 30.0))
    got = _device_extract((s, w, None), 1.0, 2.0, (10.0, 20.0, 30.0))
    assert got["cell"].tolist() == [0] and got["faces"].shape == (0, 3)
    _compare_mesh(got, ref, "2x2x2")
    # 1029 x 2 x 2: a workgroup boundary inside the row; a wave of sign changes along x, some voxels unobserved
    x = np.arange(1029, dtype=np.float64)
    s = (np.sin(0.05 * (x - 1023.6))[None, None, :] + np.array([0.1, -0.07])[None, :, None] +
         np.array([-0.04, 0.09])[:, None, None]).astype(np.float32)
    w = np.ones(s.shape, np.float32)
    w[:, :, 500:520] = 0.0
    w[1, 0, 1027:1029] = 0.0
    c = np.stack([s, -s, 0.5 * s]).astype(np.float32)
    ref = surface_nets_reference(s, w, c, 1.0, 0.005, (-2.503, -0.0031, 3.52))
    assert ref["cell"].shape[0] > 50 and {1022, 1023, 1024} <= set((ref["cell"] % 1029).tolist())
    _compare_mesh(_device_extract((s, w, c), 1.0, 0.005, (-2.503, -0.0031, 3.52)), ref, "1029x2x2")
    # no active cell: empties, and nothing launched for them
    got = _device_extract((np.ones((2, 2, 2), np.float32), w[:, :, :2].copy(), None), 1.0, 1.0, (0.0, 0.0, 0.0))
    assert got["cell"].shape == (0,) and got["faces"].shape == (0, 3)


def test_extraction_with_more_workgroup_counts_than_scan_threads():
    # 132 x 64 x 65 voxels: 537 workgroups, so 1074 counts [vertices | quads] for the scan's 1024 threads: every thread
    # owns a run of 2 and the last 487 none, and the first quad count (whose prefix is M) is the second count of thread
    # 268's run.  One slanted plane crosses the volume: few cells are active, most counts are zero.
    nx, ny, nz = 132, 64, 65
    assert 2 * -(-nx * ny * nz // 1024) == 1074
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    s = ((0.31 * i + 0.52 * j + 0.80 * k - 55.3) * 0.05).astype(np.float32)
    w = np.ones(s.shape, np.float32)
    w[20:30, 10:20, 40:60] = 0.0                                        # a hole in the sheet
    ref = surface_nets_reference(s, w, None, 1.0, 0.05, (-3.3, -1.6, 2.0))
    assert 5000 < ref["cell"].shape[0] < 30000 and ref["faces"].shape[0] > 10000
    _compare_mesh(_device_extract((s, w, None), 1.0, 0.05, (-3.3, -1.6, 2.0)), ref, "132x64x65")


def _cells_clear_of(borderline):
    """Per linear voxel index: True where none of the 8 corners of the cell with that lowest corner is borderline."""
    nz, ny, nx = borderline.shape
    pad = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    pad[:nz, :ny, :nx] = borderline
    hit = np.zeros((nz, ny, nx), bool)
    for c in range(8):
        hit |= pad[(c >> 2):nz + (c >> 2), ((c >> 1) & 1):ny + ((c >> 1) & 1), (c & 1):nx + (c & 1)]
    return ~hit.reshape(-1)


def _crossing_gap(d, cells):
    """Per cell (linear index of its lowest corner): the least |d_lo - d_hi| over its edges whose ends differ in sign."""
    nz, ny, nx = d.shape
    k, rest = np.divmod(cells, ny * nx)
    j, i = np.divmod(rest, nx)
    gap = np.full(cells.shape, np.inf)
    for axis in range(3):
        for b in range(4):
            ua, va = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
            lo = ((b & 1) << ua) | ((b >> 1) << va)
            hi = lo | (1 << axis)
            dl = d[k + (lo >> 2), j + ((lo >> 1) & 1), i + (lo & 1)]
            dh = d[k + (hi >> 2), j + ((hi >> 1) & 1), i + (hi & 1)]
            gap = np.where((dl < 0) != (dh < 0), np.minimum(gap, np.abs(dl - dh)), gap)
    return gap


def test_scene_end_to_end():
    index = 0
    depth, images, K, T = _views(index)
    vol = _volume(index)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    M, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    ref_state = _reference(index, "plain", True)
    ref = surface_nets_reference(ref_state["sdf_sum"].astype(np.float32), ref_state["weight"].astype(np.float32),
                                 ref_state["color_sum"].astype(np.float32), 1.0, CASES[index][2], CASES[index][3])
    dist = synthetic.fusion_scene_surface_distance(mesh.vertices.cpu())
    # the bound the restatement's mesh meets (tests/test_tsdf_reference_cpu.py), with 1 % of room for the fp32 volume:
    # its values differ from the restatement's by 1e-6 of a voxel, which moves a crossing by as much
    bound = 1.01 * scene_mesh_bound(CASES[index], _scene(CASES[index][0])[0], _scene(CASES[index][0])[2])
    print(f"scene: M {M} (restatement {ref['cell'].shape[0]}), F {F} (restatement {ref['faces'].shape[0]}), distance max "
          f"{float(dist.max()):.3e}, median {float(dist.median()):.3e}, bound {bound:.3e}")
    assert M > 300 and F > 300 and abs(M - ref["cell"].shape[0]) <= 0.05 * M
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < M
    assert bool((mesh.cell[1:] > mesh.cell[:-1]).all())
    assert mesh.colors is not None and mesh.colors.shape == (M, 3) and mesh.colors.dtype == torch.uint8
    assert float(dist.max()) <= bound and float(dist.median()) <= CASES[index][2]
    # the placement itself: the restatement's Surface Nets on the device's own state gives the same cells and faces,
    # and every vertex, normal and colour within the bounds of the sphere tests
    own = surface_nets_reference(vol.sdf_sum.cpu().numpy(), vol.weight.cpu().numpy(), vol.color_sum.cpu().numpy(), 1.0,
                                 CASES[index][2], CASES[index][3])
    _compare_mesh({"vertices": mesh.vertices.cpu().numpy(), "normals": mesh.normals.cpu().numpy(),
                   "colors": mesh.colors.cpu().numpy(), "faces": mesh.faces.cpu().numpy(),
                   "cell": mesh.cell.cpu().numpy()}, own, "scene, against the restatement on the device's state")
    # and against the restatement's own volume, on the cells both have whose corners are no borderline voxels.  There the
    # two volumes' values differ by at most e = max (bound / weight) + the quotient's rounding, a crossing
    # t = d_lo / (d_lo - d_hi) moves by at most 2 e / |d_lo - d_hi| (to first order; doubled for room), and so does the mean
    clear_cells = _cells_clear_of(ref_state["borderline"])
    common, at_dev, at_ref = np.intersect1d(mesh.cell.cpu().numpy(), ref["cell"], return_indices=True)
    keep = clear_cells[common]
    assert keep.sum() >= 0.9 * ref["cell"].shape[0], (keep.sum(), ref["cell"].shape[0])
    seen = ref_state["weight"] >= 1
    d = np.where(seen, ref_state["sdf_sum"] / np.where(seen, ref_state["weight"], 1.0), 0.0)
    e = (np.where(seen, ref_state["bound"] / np.where(seen, ref_state["weight"], 1.0), 0.0) + 2.0 ** -23 * np.abs(d)).max()
    gap = _crossing_gap(d.astype(np.float32).astype(np.float64), common[keep])
    allowed = CASES[index][2] * 4 * e / gap[:, None] + ref["position_bound"][at_ref[keep]]
    moved = np.abs(mesh.vertices.cpu().numpy().astype(np.float64)[at_dev[keep]] - ref["vertices"][at_ref[keep]])
    print(f"scene: {int(keep.sum())} common cells clear of borderline voxels, value error {e:.2e}, least crossing gap "
          f"{gap.min():.2e}, vertices apart by at most {moved.max():.2e}, moved / allowed max {(moved / allowed).max():.3f}")
    assert (moved <= allowed).all()
    # orientation: towards the middle camera as often as the restatement's mesh, whose vertices are the same cells'
    # but for borderline voxels (the walls the volume closes a silhouette with are seen edge-on: either sign there),
    # and for most of the surface
    centre = T[1, :3, 3].cpu().numpy().astype(np.float64)
    facing = float((((centre - mesh.vertices.cpu().numpy()) * mesh.normals.cpu().numpy()).sum(1) > 0).mean())
    ref_facing = float((((centre - ref["vertices"]) * ref["normals"]).sum(1) > 0).mean())
    print(f"scene: normals towards the middle camera {facing:.3f} (restatement {ref_facing:.3f})")
    assert abs(facing - ref_facing) <= 0.05 and facing > 0.5
