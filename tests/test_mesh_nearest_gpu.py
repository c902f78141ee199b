"""mesh_nearest on the device (csrc/mvsn_mesh_nearest.hip) against the numpy restatement (tests/mesh_nearest_reference.py:
the brute force over every (query, face) pair).  Every case goes through the C ABI with the inputs in poisoned buffers
of their own and the workspace and every output between guard bands, under both poisons.  The restatement performs the
kernel's fp64 and fp32 operations one for one: dist2, face, point, weights and within are compared byte for byte and no
tolerance applies to any output of a kernel (the one bound in this file is on a mean that torch forms, and is derived
where it stands)."""
import functools

import numpy as np
import pytest
import torch

import mesh_nearest_reference as mr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native, metrics
from multi_view_stereonet_amd.fusion import cloud_nearest
from multi_view_stereonet_amd.mesh import NEAREST_BOX_CELLS, MeshNearest, mesh_nearest

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _nearest(points, vertices, faces, max_dist, fill=POISON_NAN):
    """mvsn_mesh_nearest_count, _build and mvsn_mesh_nearest: numpy arrays of the five outputs and the counts."""
    n, m, f = len(points), len(vertices), len(faces)
    _, inv, r2 = mr.radius_scalars(max_dist)
    guard = Guard(_alloc, fill)
    q, v, fc = guard.poisoned(_to(points)), guard.poisoned(_to(vertices)), guard.poisoned(_to(faces))
    lib = _native.load()
    head = guard.empty((3,), torch.int64, DEV)
    out = {"dist2": guard.empty((n,), torch.float32, DEV), "face": guard.empty((n,), torch.int64, DEV),
           "point": guard.empty((n, 3), torch.float32, DEV), "weights": guard.empty((n, 3), torch.float32, DEV),
           "within": guard.empty((n,), torch.int32, DEV)}
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_nearest_count(_native.ptr(v), m, _native.ptr(fc), f, float(inv), _native.ptr(head), st),
                      "mvsn_mesh_nearest_count")
        pairs, large, status = head.tolist()
        assert status == 0 and 0 <= pairs < 2 ** 31 and 0 <= large <= f
        ws_bytes = lib.mvsn_mesh_nearest_workspace_bytes(pairs, large)
        ws = guard.empty((ws_bytes,), torch.uint8, DEV)
        _native.check(lib.mvsn_mesh_nearest_build(_native.ptr(v), m, _native.ptr(fc), f, float(inv), pairs, large,
                                                  _native.ptr(ws), ws_bytes, st), "mvsn_mesh_nearest_build")
        _native.check(lib.mvsn_mesh_nearest(_native.ptr(q), n, _native.ptr(v), m, _native.ptr(fc), f, float(inv), float(r2),
                                            pairs, large, _native.ptr(ws), ws_bytes, *(_native.ptr(out[k]) for k in
                                                                                       mr.NEAREST_OUTPUTS), st),
                      "mvsn_mesh_nearest")
    torch.cuda.synchronize()
    guard.check()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got["counts"] = (pairs, large, status)
    return got


@functools.lru_cache(maxsize=None)
def _device(name, fill=POISON_NAN):
    """Made once per (case, poison), never modified."""
    c = mr.nearest_case(name)
    return _nearest(c["points"], c["vertices"], c["faces"], c["max_dist"], fill)


def _same_bits(a, b, keys=mr.NEAREST_OUTPUTS):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_the_box_limit_is_the_restatements():
    assert _native.load().mvsn_mesh_nearest_box_cells() == NEAREST_BOX_CELLS == mr.BOX_CELLS


# ---- every case of mr.NEAREST_CASES: the seven regions; a query at reach and one beyond; the shared side; point faces;
# ---- a collinear face; faces that take no part; one face in 2 x 2 x 2 cells; a box of 512 cells and of 513; a face 40
# ---- cells long; the shifted mesh; far and non-finite queries; max_dist 1e-20; the height field at three radii and
# ---- permuted; N around the workgroup; F around every workgroup, table and scan-run size --------------------------------
@pytest.mark.parametrize("name", mr.NEAREST_CASES)
def test_cases_match_the_restatement_byte_for_byte(name):
    got, ref = _device(name), mr.nearest_case_reference(name)
    assert got["counts"] == ref["counts"]
    _same_bits(got, ref)


@pytest.mark.parametrize("name", mr.NEAREST_CASES)
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _nearest; an element nobody writes, or a read of foreign memory
    # or of the uninitialised workspace that reaches a result, differs between the two fills)
    a, b = _device(name, POISON_NAN), _device(name, POISON_FINITE)
    assert a["counts"] == b["counts"]
    _same_bits(a, b)


@pytest.mark.parametrize("name", ["field_1", "field_3_permuted", "long_face", "box_513", "faces_1025"])
def test_calling_twice_gives_the_same_bytes(name):
    c = mr.nearest_case(name)
    _same_bits(_nearest(c["points"], c["vertices"], c["faces"], c["max_dist"]), _device(name))


def test_the_seven_regions_are_exact():
    got = _device("seven_regions")
    assert got["dist2"].tolist() == [d2 for _, d2, _ in mr.SEVEN_REGIONS]
    assert got["point"].tolist() == [list(p) for _, _, p in mr.SEVEN_REGIONS]
    assert got["face"].tolist() == [0] * 7 and got["within"].tolist() == [1] * 7
    assert (got["weights"] >= 0).all() and got["weights"].sum(axis=1).tolist() == [1.0] * 7


def test_a_query_at_reach_is_within_and_one_beyond_is_not():
    got = _device("at_reach")
    assert got["dist2"].tolist() == [0.25, np.inf, 0.25] and got["face"].tolist() == [0, -1, 0]
    assert got["within"].tolist() == [1, 0, 1] and not got["point"][1].any() and not got["weights"][1].any()


def test_the_lower_row_wins_a_tie_and_swapping_the_faces_flips_face_alone():
    a, b = _device("shared_side"), _device("shared_side_swapped")
    assert a["face"].tolist() == [0, 0, 0, 1] and b["face"].tolist() == [0, 0, 1, 0]
    assert a["within"].tolist() == [2, 2, 2, 2]
    _same_bits(a, b, ("dist2", "point", "within"))
    # (the equidistant queries keep row 0, which is the other face now: its weights follow its own corner order)
    assert a["weights"][2:].tobytes() == b["weights"][2:].tobytes()


def test_point_faces_give_cloud_nearests_dist2_bit_for_bit():
    c, got = mr.nearest_case("point_faces"), _device("point_faces")
    cloud = cloud_nearest(_to(c["points"]), _to(c["vertices"]), c["max_dist"])
    assert got["dist2"].tobytes() == cloud.dist2.cpu().numpy().tobytes()
    assert got["face"].tolist() == cloud.index.tolist() and got["within"].tolist() == cloud.within.tolist()
    assert (got["face"] >= 0).sum() > 100


def test_a_face_in_eight_cells_is_counted_once():
    got = _device("span_2x2x2")
    assert got["counts"] == (8, 0, 0) and got["within"].tolist() == [1, 1, 1, 1]


def test_the_box_limit_decides_between_the_grid_and_the_list():
    small, large = _device("box_512"), _device("box_513")
    assert small["counts"] == (NEAREST_BOX_CELLS, 0, 0) and large["counts"] == (0, 1, 0)
    assert small["within"].max() == 1 and large["within"].max() == 1 and (large["face"] == 0).sum() > 100


def test_queries_far_outside_and_non_finite_queries_miss():
    got = _device("far_and_non_finite")
    assert got["counts"][1] == 1
    assert (got["face"][:9] == -1).all() and np.isinf(got["dist2"][:9]).all() and not got["within"][:9].any()
    assert (got["face"][9:] >= 0).sum() > 20


def test_the_shifted_mesh_gives_the_same_faces():
    base, moved = _device("queries_300"), _device("shifted")           # (the same mesh and queries, 1000 away on every axis)
    c = mr.nearest_case("shifted")
    assert (np.abs(c["vertices"]) > 900).all() and (moved["face"] >= 0).sum() > 150
    # (the shift rounds the jitter of the vertices to the coarser fp32 grid out there: a query at the edge of reach can flip)
    assert (moved["face"] == base["face"]).mean() > 0.9


def test_the_order_of_the_faces_shows_in_face_alone():
    perm = mr.permutation(288)
    for h in ("0.5", "1", "3"):
        base, moved = _device("field_" + h), _device("field_%s_permuted" % h)
        _same_bits(base, moved, ("dist2", "within"))
        hit = base["face"] >= 0
        assert hit.tobytes() == (moved["face"] >= 0).tobytes()
        # the same face unless two faces tie on d2 (a query nearest to a shared side or corner)
        same = perm[moved["face"][hit]] == base["face"][hit]
        assert same.mean() > 0.8
        assert base["point"][hit][same].tobytes() == moved["point"][hit][same].tobytes()


# ---- the Python interface ------------------------------------------------------------------------------------------------
def test_the_python_call_is_the_library_call():
    for name in ("field_1", "far_and_non_finite", "box_513", "tiny_radius", "invalid_mixed"):
        c = mr.nearest_case(name)
        got = mesh_nearest(_to(c["points"]), _to(c["vertices"]), _to(c["faces"]), c["max_dist"])
        assert isinstance(got, MeshNearest)
        _same_bits({k: getattr(got, k).cpu().numpy() for k in mr.NEAREST_OUTPUTS}, mr.nearest_case_reference(name))
    # no face takes part: the all-miss answer after the count
    v = _to(np.full((3, 3), np.nan, np.float32))
    none = mesh_nearest(_to(np.zeros((4, 3), np.float32)), v, _to(np.array([[0, 1, 2], [0, 1, 7]])), 1.0)
    assert none.face.tolist() == [-1] * 4 and none.within.tolist() == [0] * 4 and torch.isinf(none.dist2).all()
    with pytest.raises(ValueError, match="max_dist too small for the mesh's extent"):
        mesh_nearest(_to(np.zeros((4, 3), np.float32)), _to(np.array([[0, 0, 0], [3e6, 0, 0], [0, 1, 0]], np.float32)),
                     _to(np.array([[0, 1, 2]])), 1.0)


def test_mesh_metrics_on_a_flat_mesh_against_a_grid_above_it():
    """Every grid point lies 0.01 above the inside of a face, so every d2 is the same fp32 number and the completeness is
    the mean of n copies of c = float64(sqrt(float32 d2)).  A sum of n copies of a 53-bit number is exact whatever its
    order only for n <= 2 (c + c = 2 c; 3 c needs two more bits), so the equality is asserted on the 2 x 1 grid; on the
    17 x 17 grid the n - 1 additions and the division are each within 2^-53, relatively: |mean - c| <= n 2^-53 c."""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int64)
    y, x = np.mgrid[0:17, 0:17]
    truth = np.stack([x * 0.25, y * 0.25, np.full(x.shape, 0.01)], -1).reshape(-1, 3).astype(np.float32)
    ref = mr.nearest_reference(truth, v, f, 0.05)
    assert (ref["face"] >= 0).all() and len(np.unique(ref["dist2"])) == 1
    c = float(np.sqrt(np.float64(ref["dist2"][0])))
    pair = np.array([[1.25, 0.5, 0.01], [3.5, 2.75, 0.01]], np.float32)                  # one point over each face
    two = metrics.mesh_metrics(_to(v), _to(f), _to(pair), 0.05, samples=2000, seed=3)
    print("completeness on the 2 x 1 grid", repr(two["completeness"]), "c", repr(c))
    assert two["completeness"] == c and two["recall"] == 1.0 and two["n_truth"] == 2
    got = metrics.mesh_metrics(_to(v), _to(f), _to(truth), 0.05, samples=2000, seed=3)
    print("completeness on the 17 x 17 grid", repr(got["completeness"]))
    assert abs(got["completeness"] - c) <= 289 * 2.0 ** -53 * c and got["recall"] == 1.0
    assert got["n_truth"] == 289 and got["n_samples"] == got["n_pred"] == 2000
    # the samples lie in the plane z = 0, the grid 0.01 above with 0.25 between its points
    assert got["precision"] < 1.0 and 0.01 <= got["accuracy"] <= 0.05 and 0 < got["fscore"] < 1
    assert set(got) == {"accuracy", "completeness", "precision", "recall", "fscore", "n_pred", "n_truth", "n_samples"}
    wide = metrics.mesh_metrics(_to(v), _to(f), _to(truth), 0.05, 0.5, samples=2000, seed=3)
    assert wide["recall"] == 1.0 and wide["completeness"] == got["completeness"] and wide["precision"] == got["precision"]
    assert wide["accuracy"] > got["accuracy"]
