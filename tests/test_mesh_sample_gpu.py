"""mesh_sample on the device (csrc/mvsn_mesh_sample.hip) against the numpy restatement (tests/mesh_nearest_reference.py).
Every case goes through the C ABI with the inputs in poisoned buffers of their own and the workspace and every output
between guard bands, under both poisons.  The weights are integers, the draws integer work and every fp64 step of the
restatement one numpy operation: points, face, weights, normals and colours are compared byte for byte and no tolerance
applies anywhere."""
import functools

import numpy as np
import pytest
import torch

import mesh_nearest_reference as mr
from guarded_alloc import POISON_FINITE, POISON_NAN, Guard
from multi_view_stereonet_amd import _native
from multi_view_stereonet_amd.mesh import MESH_SAMPLE_STATUS_NO_AREA, MeshSamples, mesh_sample

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _alloc(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def _to(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _sample(vertices, faces, n, seed=0, normals=None, colors=None, fill=POISON_NAN):
    """mvsn_mesh_sample_prefix and mvsn_mesh_sample_draw: numpy arrays of the outputs, the total and the status.  The
    draw is launched whatever the status says: with no area it writes -1 and zeros everywhere."""
    m, f = len(vertices), len(faces)
    guard = Guard(_alloc, fill)
    v, fc = guard.poisoned(_to(vertices)), guard.poisoned(_to(faces))
    nor = guard.poisoned(_to(normals)) if normals is not None else None
    col = guard.poisoned(_to(colors)) if colors is not None else None
    lib = _native.load()
    ws_bytes = lib.mvsn_mesh_sample_workspace_bytes(f)
    ws = guard.empty((ws_bytes,), torch.uint8, DEV)
    head = guard.empty((2,), torch.int64, DEV)
    out = {"points": guard.empty((n, 3), torch.float32, DEV), "face": guard.empty((n,), torch.int64, DEV),
           "weights": guard.empty((n, 3), torch.float32, DEV),
           "normals": guard.empty((n, 3), torch.float32, DEV) if normals is not None else None,
           "colors": guard.empty((n, 3), torch.uint8, DEV) if colors is not None else None}
    with torch.cuda.device(DEV):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_sample_prefix(_native.ptr(v), m, _native.ptr(fc), f, _native.ptr(head), _native.ptr(ws),
                                                  ws_bytes, st), "mvsn_mesh_sample_prefix")
        _native.check(lib.mvsn_mesh_sample_draw(_native.ptr(v), m, _native.ptr(fc), f, _native.ptr(ws), ws_bytes, n, seed,
                                                _native.ptr(nor), _native.ptr(col), _native.ptr(out["points"]),
                                                _native.ptr(out["face"]), _native.ptr(out["weights"]),
                                                _native.ptr(out["normals"]), _native.ptr(out["colors"]), st),
                      "mvsn_mesh_sample_draw")
    torch.cuda.synchronize()
    guard.check()
    got = {k: t.cpu().numpy() if t is not None else None for k, t in out.items()}
    got["total"], got["status"] = head.tolist()
    return got


@functools.lru_cache(maxsize=None)
def _device(name, fill=POISON_NAN):
    """Made once per (case, poison), never modified."""
    c = mr.sample_case(name)
    return _sample(c["vertices"], c["faces"], c["n"], c["seed"], c["normals"], c["colors"], fill)


def _same_bits(a, b, keys=mr.SAMPLE_OUTPUTS):
    for key in keys:
        if b[key] is None:
            assert a[key] is None, key
            continue
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("name", mr.SAMPLE_CASES)
def test_cases_match_the_restatement_byte_for_byte(name):
    got, ref = _device(name), mr.sample_case_reference(name)
    assert got["total"] == ref["total"]                       # P[F-1]: the scan over every workgroup and every run
    assert got["status"] == (MESH_SAMPLE_STATUS_NO_AREA if ref["total"] == 0 else 0)
    _same_bits(got, ref)


@pytest.mark.parametrize("name", mr.SAMPLE_CASES)
def test_buffers_under_both_poisons(name):
    # (the guard bands of every buffer are checked inside _sample; an element nobody writes, or a read of foreign memory
    # or of the uninitialised workspace that reaches a result, differs between the two fills)
    a, b = _device(name, POISON_NAN), _device(name, POISON_FINITE)
    assert (a["total"], a["status"]) == (b["total"], b["status"])
    _same_bits(a, b)


@pytest.mark.parametrize("name", ["field_1000", "equal_2049", "invalid_mixed"])
def test_calling_twice_gives_the_same_bytes(name):
    c = mr.sample_case(name)
    _same_bits(_sample(c["vertices"], c["faces"], c["n"], c["seed"], c["normals"], c["colors"]), _device(name))


def test_the_six_triangles_are_drawn_by_area():
    got = _device("six_triangles")
    assert np.bincount(got["face"], minlength=6).tolist() == [223, 460, 910, 1845, 0, 658]
    assert (got["weights"] >= 0).all()


@pytest.mark.parametrize("f", [1025, 2049])
def test_equal_faces_are_drawn_equally_and_every_boundary_decides(f):
    got = _device("equal_%d" % f)
    # every face has weight 2^31: the face is floor(pick / 2^31), whatever workgroup and run its prefix came from
    c = np.uint64(3) * np.arange(1000, dtype=np.uint64)
    pick = mr.umul64hi(mr.splitmix(2, c + np.uint64(1)), np.uint64(f << 31))
    assert got["total"] == f << 31 and got["face"].tolist() == (pick >> np.uint64(31)).tolist()
    assert got["face"].min() < 256 and got["face"].max() >= f - 256      # the first and the last workgroup are reached


def test_faces_without_weight_are_never_drawn():
    tiny = _device("tiny_face")
    assert tiny["total"] == (1 << 31) + 1 and set(tiny["face"].tolist()) <= {1, 3} and (tiny["face"] == 1).sum() >= 999
    bad = _device("invalid_mixed")
    c = mr.sample_case("invalid_mixed")
    ok, _ = mr.valid_faces(c["vertices"], c["faces"])
    assert (~ok).sum() >= 7 and ok[bad["face"]].all() and np.isfinite(bad["points"]).all()


def test_no_area_gives_the_status_and_writes_every_output():
    got = _device("no_area")
    assert got["total"] == 0 and got["status"] == MESH_SAMPLE_STATUS_NO_AREA
    assert (got["face"] == -1).all() and not got["points"].any() and not got["weights"].any()
    assert not got["normals"].any() and not got["colors"].any()


def test_the_prefix_property():
    c = mr.sample_case("field_1000")
    long = _device("field_1000")
    for n in (1, 64, 65):
        _same_bits({k: (v[:n] if v is not None else None) for k, v in long.items() if k in mr.SAMPLE_OUTPUTS},
                   _device("field_%d" % n))
    other = _sample(c["vertices"], c["faces"], 65, c["seed"] + 1)
    assert other["face"].tolist() != long["face"][:65].tolist()


def test_normals_and_colours():
    got, c = _device("field_1000"), mr.sample_case("field_1000")
    zero = got["face"] == mr.ZERO_NORMAL_FACE                  # the face whose three normals are zero
    assert zero.any() and not got["normals"][zero].any()
    nan = got["face"] == mr.NAN_NORMAL_FACE                    # a NaN among its normals: no direction either
    assert nan.any() and not got["normals"][nan].any() and np.isfinite(got["normals"]).all()
    length = np.linalg.norm(got["normals"], axis=1)           # unit, or (0,0,0) where the sum has no direction
    assert ((length == 0) | (np.abs(length - 1) <= 1e-6)).all() and (length > 0).mean() > 0.9
    lo, hi = c["colors"][c["faces"][got["face"]]].min(axis=1), c["colors"][c["faces"][got["face"]]].max(axis=1)
    assert (got["colors"] >= lo).all() and (got["colors"] <= hi).all()
    # each gather alone gives the same bytes, and neither touches the samples
    only = _sample(c["vertices"], c["faces"], 1000, c["seed"], normals=c["normals"])
    assert only["colors"] is None and only["normals"].tobytes() == got["normals"].tobytes()
    only = _sample(c["vertices"], c["faces"], 1000, c["seed"], colors=c["colors"])
    assert only["normals"] is None and only["colors"].tobytes() == got["colors"].tobytes()
    _same_bits(only, got, ("points", "face", "weights"))


def test_the_python_call_is_the_library_call():
    c = mr.sample_case("field_1000")
    v, f = _to(c["vertices"]), _to(c["faces"])
    got = mesh_sample(v, f, 1000, seed=c["seed"], normals=_to(c["normals"]), colors=_to(c["colors"]))
    assert isinstance(got, MeshSamples)
    _same_bits({k: getattr(got, k).cpu().numpy() for k in mr.SAMPLE_OUTPUTS}, mr.sample_case_reference("field_1000"))
    bare = mesh_sample(v, f, 65)
    assert bare.normals is None and bare.colors is None
    assert bare.points.cpu().numpy().tobytes() == mr.sample_reference(c["vertices"], c["faces"], 65)["points"].tobytes()
    assert torch.equal(mesh_sample(v, f, 1000)[0][:65], bare.points)
    none = mr.sample_case("no_area")
    with pytest.raises(ValueError, match="the mesh has no area"):
        mesh_sample(_to(none["vertices"]), _to(none["faces"]), 5)
    assert mesh_sample(_to(none["vertices"]), _to(none["faces"]), 0).points.shape == (0, 3)
