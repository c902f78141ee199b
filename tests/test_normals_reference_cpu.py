"""The numpy restatement of depth_normals and voxel_normals (tests/normals_reference.py) against the analytic scene, no
GPU: the plane's normals within the derived per-pixel bound of the analytic one, the sphere's within the discretisation,
every normal facing its camera; the voxel mean direction independent of the order of the points and within its
quantisation of the float64 one."""
import numpy as np
import pytest

from multi_view_stereonet_amd import synthetic
from normals_reference import angle, normals_reference, voxel_normals_reference
from voxel_reference import voxel_reference

SCENES = [(4, 48, 64), (3, 37, 61)]
STEP = 0.05
VOXEL = 0.25            # a few pixel footprints (0.11 at the plane): several points per voxel
_cache = {}


def _scene(shape, posed):
    """The scene, its restated normals and the masks the tests share: computed once per case, never modified."""
    key = (shape, posed)
    if key not in _cache:
        V, H, W = shape
        sc = synthetic.fusion_scene(V, H, W)
        depth, K, T = sc["depth"].numpy(), sc["K"].numpy(), sc["T_cam_in_world"].numpy().astype(np.float64)
        ref = normals_reference(depth, K, T_cam_in_world=T if posed else None, max_rel_step=STEP)
        label = sc["label"][:, 0].numpy()
        same = ref["defined"] & ref["usable"].all(0)
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            same &= np.roll(label, (-dy, -dx), (1, 2)) == label        # (the four neighbours are inside: usable)
        R = T[:, :3, :3] if posed else np.broadcast_to(np.eye(3), (V, 3, 3))
        _cache[key] = {"depth": depth, "K": K, "T": T, "ref": ref, "label": label, "same": same, "R": R,
                       "n": ref["normals"].transpose(0, 2, 3, 1)}
    return _cache[key]


def _check_conditions(s):
    # conditions on the inputs, first: with them the assertions below mean what they say
    defined, bound = s["ref"]["defined"], s["ref"]["bound"]
    assert bound[defined].max() < 2e-3, bound[defined].max()
    assert defined.sum() >= 0.99 * (s["depth"][:, 0] > 0).sum(), (defined.sum(), (s["depth"] > 0).sum())


@pytest.mark.parametrize("posed", [False, True], ids=["camera", "world"])
@pytest.mark.parametrize("shape", SCENES, ids=lambda s: "x".join(map(str, s)))
def test_plane_normals_within_the_bound_of_the_analytic_normal(shape, posed):
    s = _scene(shape, posed)
    _check_conditions(s)
    n_world = np.asarray(synthetic.SCENE_PLANE_NORMAL, np.float64)
    n_world /= np.linalg.norm(n_world)                                  # (towards the cameras: z < 0)
    plane = s["same"] & (s["label"] == 0)
    assert plane.sum() > 0.3 * plane.size
    for v in range(shape[0]):
        want = n_world if posed else s["T"][v, :3, :3].T @ n_world
        err = angle(s["n"][v][plane[v]], want)
        print(f"view {v}: plane pixels {plane[v].sum()}, max angle {err.max():.3e}, "
              f"min bound {s['ref']['bound'][v][plane[v]].min():.3e}")
        assert (err <= s["ref"]["bound"][v][plane[v]]).all(), (err / s["ref"]["bound"][v][plane[v]]).max()


@pytest.mark.parametrize("posed", [False, True], ids=["camera", "world"])
@pytest.mark.parametrize("shape", SCENES, ids=lambda s: "x".join(map(str, s)))
def test_sphere_normals_within_the_discretisation(shape, posed):
    s = _scene(shape, posed)
    _check_conditions(s)
    sphere = s["same"] & (s["label"] == 1)
    assert sphere.sum() >= 20, sphere.sum()
    centre = np.asarray(synthetic.SCENE_SPHERE_CENTER, np.float64)
    for v in range(shape[0]):
        Xw = s["ref"]["X"][v] @ s["T"][v, :3, :3].T + s["T"][v, :3, 3]
        want = (Xw - centre) / synthetic.SCENE_SPHERE_RADIUS
        if not posed:
            want = want @ s["T"][v, :3, :3]                             # R^T n, row-wise
        err = angle(s["n"][v][sphere[v]], want[sphere[v]])
        print(f"view {v}: sphere pixels {sphere[v].sum()}, max angle {err.max():.3e}")
        assert err.max() < 0.1, err.max()                               # a check of the discretisation, not of precision


@pytest.mark.parametrize("posed", [False, True], ids=["camera", "world"])
@pytest.mark.parametrize("shape", SCENES, ids=lambda s: "x".join(map(str, s)))
def test_every_defined_normal_faces_its_camera(shape, posed):
    s = _scene(shape, posed)
    _check_conditions(s)
    defined = s["ref"]["defined"]
    for v in range(shape[0]):
        towards = s["ref"]["X"][v] @ s["R"][v].T                        # camera centre -> point, in the normals' frame
        dots = (s["n"][v] * towards).sum(-1)
        assert (dots[defined[v]] < 0).all(), (dots[defined[v]] >= 0).sum()
        assert (s["n"][v][~defined[v]] == 0).all()
        np.testing.assert_allclose(np.linalg.norm(s["n"][v][defined[v]], axis=-1), 1.0, atol=1e-12)


def _cloud(shape):
    """Every depth > 0 pixel of the scene as a world point with its restated world normal (fp32), merged on a grid."""
    s = _scene(shape, True)
    keep = s["depth"][:, 0] > 0
    pts = np.concatenate([(s["ref"]["X"][v] @ s["T"][v, :3, :3].T + s["T"][v, :3, 3])[keep[v]]
                          for v in range(shape[0])]).astype(np.float32)
    nrm = np.concatenate([s["n"][v][keep[v]] for v in range(shape[0])]).astype(np.float32)
    return pts, nrm


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: "x".join(map(str, s)))
def test_voxel_restatement_is_independent_of_the_order_of_the_points(shape):
    pts, nrm = _cloud(shape)
    vox = voxel_reference(pts, VOXEL)
    m = len(vox["first"])
    assert 1 < m < len(pts) / 2
    out, _ = voxel_normals_reference(nrm, vox["inverse"], m)
    perm = np.random.default_rng(21).permutation(len(pts))
    vox_p = voxel_reference(pts[perm], VOXEL)
    out_p, _ = voxel_normals_reference(nrm[perm], vox_p["inverse"], len(vox_p["first"]))
    # rows are ordered by the lowest input index, which the permutation changes: compare through the voxel keys
    by_key = {tuple(c): o.tobytes() for c, o in zip(vox["cells"].tolist(), out)}
    by_key_p = {tuple(c): o.tobytes() for c, o in zip(vox_p["cells"].tolist(), out_p)}
    assert len(by_key) == m and by_key == by_key_p


@pytest.mark.parametrize("shape", SCENES, ids=lambda s: "x".join(map(str, s)))
def test_voxel_restatement_against_the_float64_mean_direction(shape):
    pts, nrm = _cloud(shape)
    vox = voxel_reference(pts, VOXEL)
    m = len(vox["first"])
    out, sums = voxel_normals_reference(nrm, vox["inverse"], m)
    total = np.zeros((m, 3), np.float64)
    np.add.at(total, vox["inverse"], nrm.astype(np.float64))
    length = np.linalg.norm(total, axis=1)
    firm = length >= 0.1 * vox["count"]
    assert firm.sum() > 0.9 * m
    err = np.abs(out[firm].astype(np.float64) - total[firm] / length[firm, None])
    print(f"{m} voxels, {firm.sum()} with a firm direction, max component error {err.max():.3e}")
    assert err.max() <= 2.0 ** -20, err.max()
    # a voxel of undefined pixels only has a zero sum and a zero normal
    zero = (sums == 0).all(axis=1)
    assert (out[zero] == 0).all() and (np.abs(np.linalg.norm(out[~zero].astype(np.float64), axis=1) - 1) < 1e-6).all()


def test_voxel_restatement_skips_what_does_not_count():
    nrm = np.array([[0, 0, 1], [np.nan, 0, 1], [0, np.inf, 0], [0, 0, 0], [2 ** -22, 0, 0], [3, -3, 0], [0, 1, 0],
                    [0.5 * 2 ** -20, 1.5 * 2 ** -20, 2.5 * 2 ** -20]], np.float32)
    inverse = np.array([0, 0, 0, 0, 0, 1, 5, 2])                       # row 5 does not exist (m = 4); row 3 stays empty
    out, sums = voxel_normals_reference(nrm, inverse, 4)
    assert sums.tolist() == [[0, 0, 2 ** 20], [2 ** 20, -2 ** 20, 0], [0, 2, 2], [0, 0, 0]]   # clamped; halves to even
    np.testing.assert_array_equal(out[0], [0, 0, 1])
    np.testing.assert_allclose(out[1], [2 ** -0.5, -2 ** -0.5, 0], rtol=1e-7)
    np.testing.assert_array_equal(out[3], [0, 0, 0])
