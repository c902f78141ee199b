"""integrate_cloud on the device (csrc/mvsn_tsdf_cloud.hip) against the numpy restatement
(tests/tsdf_cloud_reference.py): every named case byte for byte, with no tolerance, through the C entries with every
buffer between guard bands under both poisons; repeatability and the order of the rows; the Python calls; the sphere
from the cloud to a mesh and on through the mesh tools; and a cloud added to a depth-integrated volume.

Figures of one MI355X run are in DESIGN.md section 31."""
import functools

import numpy as np
import pytest
import torch

import tsdf_cloud_reference as tc
from cloud_reference import radius_scalars
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd.fusion import read_ply, write_ply
from multi_view_stereonet_amd.mesh import mesh_nearest, mesh_simplify, mesh_smooth
from multi_view_stereonet_amd.tsdf import TSDFVolume, integrate_cloud
from tsdf_reference import CASES, SPHERE, mesh_topology

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entry(c, fill=POISON_NAN, state=None):
    """mvsn_cloud_index_build, then mvsn_tsdf_cloud_integrate: every input in a poisoned buffer of its own (16-byte
    aligned only); the index workspace, the flag workspace, the status word and the three state tensors carved between
    guard bands and poisoned too.  `state`: "poison" leaves the fill as the prior state, None is the case's own (zeros
    without one).  Returns (sdf_sum, weight, color_sum or None) as numpy arrays."""
    h, inv, r2 = radius_scalars(c["radius"])
    nx, ny, nz = c["dims"]
    n = len(c["points"])
    guard = Guard(_alloc, fill)
    p, nr = guard.poisoned(_to(c["points"])), guard.poisoned(_to(c["normals"]))
    w = guard.poisoned(_to(c["weights"])) if c["weights"] is not None else None
    col = guard.poisoned(_to(c["colors"])) if c["colors"] is not None else None
    lib = _native.load()
    ws_bytes, flag_bytes = lib.mvsn_cloud_workspace_bytes(n), lib.mvsn_tsdf_cloud_workspace_bytes(nx, ny, nz)
    assert flag_bytes >= -(-nx // 8) * -(-ny // 8) * -(-nz // 8)
    ws, status = guard.empty((ws_bytes,), torch.uint8, DEV), guard.empty((1,), torch.int64, DEV)
    flags = guard.empty((flag_bytes,), torch.uint8, DEV)
    s, wt = guard.empty((nz, ny, nx), torch.float32, DEV), guard.empty((nz, ny, nx), torch.float32, DEV)
    cs = guard.empty((3, nz, ny, nx), torch.float32, DEV) if col is not None else None
    if state != "poison":
        prior = c["state"] if state is None else state
        for t, a in zip((s, wt, cs), prior if prior is not None else (None, None, None)):
            if t is not None:
                t.zero_() if a is None else t.copy_(_to(a))
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(p), n, float(h), float(inv), _native.ptr(status), _native.ptr(ws),
                                                 ws_bytes, st), "mvsn_cloud_index_build")
        _native.check(lib.mvsn_tsdf_cloud_integrate(
            _native.ptr(p), _native.ptr(nr), _native.ptr(w), _native.ptr(col), n, _native.ptr(ws), ws_bytes, float(h),
            float(inv), float(r2), nx, ny, nz, float(np.float32(c["voxel_size"])), *(float(np.float32(o)) for o in c["origin"]),
            float(np.float32(c["trunc"])), _native.ptr(s), _native.ptr(wt), _native.ptr(cs), _native.ptr(flags), flag_bytes, st),
            "mvsn_tsdf_cloud_integrate")
    torch.cuda.synchronize()
    guard.check()
    assert int(status.item()) == 0
    return s.cpu().numpy(), wt.cpu().numpy(), None if cs is None else cs.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(name, fill=POISON_NAN):
    """Made once per (case, poison), never modified."""
    return _entry(tc.case(name), fill)


CASES_ON_DEVICE = tuple(n for n in tc.CASE_IDS if n != "empty")       # (the entry rejects n = 0: Python answers it)


@pytest.mark.parametrize("fill", [POISON_NAN, POISON_FINITE], ids=["nan", "finite"])
@pytest.mark.parametrize("name", CASES_ON_DEVICE)
def test_cases_equal_the_restatement_byte_for_byte(name, fill):
    ref, got = tc.case_reference(name), _device(name, fill)
    for k, a in zip(("sdf_sum", "weight", "color_sum"), got):
        if a is None:
            assert ref[k] is None
            continue
        same = a.view(np.uint32) == ref[k].view(np.uint32)
        assert same.all(), (name, k, int((~same).sum()), "voxels differ; first at", np.argwhere(~same)[0].tolist())
    assert ref["updated"].any()


@pytest.mark.parametrize("name", ["sphere", "outside", "brick_border", "one_8x8x8", "limit"])
def test_with_the_finite_poison_as_the_prior_state_every_voxel_out_of_reach_keeps_its_bytes(name):
    c, ref = tc.case(name), tc.case_reference(name)
    s, w, _ = _entry(dict(c, colors=None), POISON_FINITE, state="poison")
    out = ~ref["updated"]
    assert out.any()
    word = np.uint32(0x7B7B7B7B)
    assert (s.view(np.uint32)[out] == word).all() and (w.view(np.uint32)[out] == word).all()
    # ... and what is within reach is the restatement started from that state
    nz, ny, nx = s.shape
    prior = np.full((nz, ny, nx), word, np.uint32).view(np.float32)
    want = tc.tsdf_cloud_reference(c["points"], c["normals"], c["radius"], c["dims"], c["voxel_size"], c["origin"], c["trunc"],
                                   weights=c["weights"], state=(prior, prior.copy(), None))
    assert tc.state_bytes((s, w, None)) == tc.state_bytes(want)


def test_a_second_run_and_permuted_rows_give_the_same_bytes():
    for name in ("colours", "bad_rows", "sphere"):
        c, base = tc.case(name), _device(name)
        assert tc.state_bytes(_entry(c)) == tc.state_bytes(base), name
        perm = np.random.default_rng(321).permutation(len(c["points"]))
        moved = dict(c, points=c["points"][perm], normals=c["normals"][perm],
                     weights=None if c["weights"] is None else c["weights"][perm],
                     colors=None if c["colors"] is None else c["colors"][perm])
        assert tc.state_bytes(_entry(moved)) == tc.state_bytes(base), name


def _volume(c):
    vol = TSDFVolume(c["dims"], c["voxel_size"], c["origin"], c["trunc"], device=DEV, color=c["colors"] is not None)
    if c["state"] is not None:
        vol.sdf_sum.copy_(_to(c["state"][0]))
        vol.weight.copy_(_to(c["state"][1]))
        if c["state"][2] is not None:
            vol.color_sum.copy_(_to(c["state"][2]))
    return vol


def _state(vol):
    return (vol.sdf_sum.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.color_sum is None else vol.color_sum.cpu().numpy())


def _strided(a):
    """The tensor of `a` as a non-contiguous view."""
    t = _to(a)
    wide = torch.empty((t.shape[0], 2) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV)
    wide[:, 0] = t
    out = wide[:, 0]
    assert t.shape[0] < 2 or not out.is_contiguous()
    return out


@pytest.mark.parametrize("name", ["colours", "bad_rows", "prior", "offset", "empty", "one_1x1x1"])
def test_both_python_calls_equal_the_restatement_and_take_non_contiguous_tensors(name):
    c, ref = tc.case(name), tc.case_reference(name)
    kw = dict(weights=None if c["weights"] is None else _strided(c["weights"]),
              colors=None if c["colors"] is None else _strided(c["colors"]))
    vol = _volume(c)
    vol.integrate_cloud(_strided(c["points"]), _strided(c["normals"]), c["radius"], **kw)
    assert tc.state_bytes(_state(vol)) == tc.state_bytes(ref)
    vol = _volume(c)
    integrate_cloud(vol.sdf_sum, vol.weight, vol.color_sum, c["voxel_size"], c["origin"], c["trunc"], _to(c["points"]),
                    _to(c["normals"]), c["radius"], weights=_to(c["weights"]), colors=_to(c["colors"]))
    assert tc.state_bytes(_state(vol)) == tc.state_bytes(ref)


def test_colours_and_the_volume_go_together_and_the_grid_has_its_range():
    c = tc.case("colours")
    p, n = _to(c["points"]), _to(c["normals"])
    plain = TSDFVolume(c["dims"], c["voxel_size"], c["origin"], c["trunc"], device=DEV)
    with pytest.raises(ValueError, match="colors need a volume made with color=True"):
        plain.integrate_cloud(p, n, c["radius"], colors=_to(c["colors"]))
    with pytest.raises(ValueError, match="colors need a volume made with color=True"):
        _volume(c).integrate_cloud(p, n, c["radius"])
    assert not plain.weight.any()
    far = c["points"].copy()
    far[7, 1] = 2.0 ** 20 * c["radius"]
    with pytest.raises(ValueError, match="max_dist too small for the target's extent"):
        plain.integrate_cloud(_to(far), n, c["radius"])


def test_sphere_cloud_to_a_mesh_and_through_the_mesh_tools(tmp_path):
    c = tc.case("sphere")
    p, n = _to(c["points"]), _to(c["normals"])
    vol = TSDFVolume.around(p, SPHERE["voxel_size"], tc.SPHERE_TRUNC)
    assert vol.sdf_sum.is_cuda and min(vol.dims) >= 18 and max(vol.dims) <= 22
    vol.integrate_cloud(p, n, tc.SPHERE_RADIUS)
    mesh = vol.extract_mesh(min_weight=1.0)
    v, f = mesh.vertices.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy()
    closed, euler, boundary = mesh_topology(f, len(v))
    assert closed and boundary == 0 and euler == 2, (closed, euler, boundary)
    centre = np.asarray(SPHERE["centre"], np.float64)
    dist = np.linalg.norm(v - centre, axis=1) - SPHERE["radius"]
    bound = tc.sphere_mesh_bound()
    near = mesh_nearest(p, mesh.vertices, mesh.faces, 2 * bound)
    d2 = near.dist2.cpu().numpy()
    print(f"sphere: volume {vol.dims}, {len(v)} vertices, {len(f)} faces, vertex distance {dist.min():.4f} to {dist.max():.4f}, "
          f"cloud to mesh max {np.sqrt(d2.max()):.4f}, bound {bound:.4f}")
    assert np.abs(dist).max() <= bound
    assert (d2 <= bound * bound).all()
    tri = v[f]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((fn * (tri.mean(1) - centre)).sum(1) > 0).all(), "a face is wound inwards"
    smooth = mesh_smooth(mesh.vertices, mesh.faces, 5)
    small = mesh_simplify(smooth.vertices, mesh.faces, 2 * SPHERE["voxel_size"])
    assert 0 < len(small.vertices) < len(v) and len(small.faces) > 100
    path = str(tmp_path / "sphere.ply")
    write_ply(path, small.vertices, faces=small.faces)
    back = read_ply(path)
    assert back.points.numpy().tobytes() == small.vertices.cpu().numpy().tobytes()
    assert back.faces.numpy().tobytes() == small.faces.cpu().numpy().tobytes()
    assert back.normals is None and back.colors is None and back.confidence is None


def test_a_cloud_on_top_of_depth_maps_equals_the_restatement_started_from_the_same_state():
    shape, dims, vs, origin, trunc = CASES[tc.PRIOR_CASE]
    sc = synthetic.fusion_scene(*shape)
    vol = TSDFVolume(dims, vs, origin, trunc, device=DEV, color=True)
    vol.integrate(sc["depth"].to(DEV), sc["K"].to(DEV), sc["T_cam_in_world"].to(DEV), images=sc["images"].to(DEV))
    before = _state(vol)
    assert (before[1] > 0).any()
    c = tc.case("prior")
    vol.integrate_cloud(_to(c["points"]), _to(c["normals"]), c["radius"], colors=_to(c["colors"]))
    want = tc.tsdf_cloud_reference(c["points"], c["normals"], c["radius"], dims, vs, origin, trunc, colors=c["colors"], state=before)
    assert want["updated"].any() and (before[1][want["updated"]] > 0).any()
    assert tc.state_bytes(_state(vol)) == tc.state_bytes(want)
