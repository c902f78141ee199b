"""The restatement of the ray-cast (tests/tsdf_raycast_reference.py) against the analytic sphere, within bounds derived
here, and the conditions its cases must meet to be a test of the kernel: few borderline pixels, enough hits."""
import math

import numpy as np
import pytest

from tsdf_raycast_reference import (BORDERLINE_CAP, CASE_IDS, EPS, NO_HIT_IDS, SPHERE, SPHERE_HITS, camera, raycast_reference,
                                    reference, render_case, sphere_camera, sphere_variants)

FINE_STEP = 0.025          # a quarter of a voxel: the sphere is six voxels in radius, see sphere_ray_bounds


def sphere_ray_bounds(h, r, step, length, cosine, shift):
    """How far the restatement's hit may lie from the analytic ray-sphere depth, and its normal from the radial
    direction, for a ray whose camera-frame direction (x, y, 1) has `length` and which meets the sphere at the incidence
    cosine `cosine`.  Along the ray, by depth t, the true distance phi(t) = |p(t) - c| - r is convex with
    |phi'| = length * (incidence cosine) and phi'' <= length^2 / rho, rho the distance from the centre.
      * The trilinear interpolant I of f on a cell of side h is within e = 3 h^2 / (8 rho) of f: h^2 / 8 times the second
        derivative along each of the three axes, each at most 1 / rho.
      * The march finds the first samples with I0 >= 0 > I1.  I1 < 0 needs phi(t1) < e and I0 >= 0 needs
        phi(t0) >= -e, so with s the least slope |phi'| about the true depth t' the bracket lies inside
        [t' - e/s - step, t' + e/s + step].  Taking e/s <= h/2 (returned as a condition), every point met is within
        dist = (step + h/2) * length of the true hit, the corners of its cell within a further h sqrt(3):
        rho >= r - dist - h sqrt(3) =: rho_min; the radial direction turns by at most dist / rho_min over dist, so the
        incidence cosine stays above cosine - dist / rho_min and s = length * (cosine - dist / rho_min).
      * The chord of I between the two samples is within e of the chord of phi, which is within
        e2 = step^2 length^2 / (8 rho_min) of phi (the linear-crossing term): |phi(t*)| <= e + e2 at the chord's zero
        t*.  The restatement's ray is that of A and g0 rounded to fp32, each of the twelve numbers within u = 2^-24 of
        itself: its point at depth t lies within shift = h |(u (t S_a + |g0_a|))_a| of the exact camera's,
        S_a = |A_a0 x| + |A_a1 y| + |A_a2| (passed in, per ray, at the analytic depth plus the step), and f moves by no
        more than the point does: |phi(t*)| <= e + e2 + shift, so |t* - t'| <= (e + e2 + shift) / s.
      * Normal: a component of grad I is a convex combination of difference quotients along four edges of the cell,
        each the derivative of f at a point of its edge, within h sqrt(3) of the hit; grad f turns by at most 1 / rho per
        unit length, so each component is within h sqrt(3) / rho_min and the vector within 3 h / rho_min of grad f, which
        has length 1: an angle of at most asin(3 h / rho_min), and the radial direction at the restatement's hit differs
        from that at the true hit by length * |t* - t'| / rho_min.
    Returns (depth bound, angle bound, condition e/s <= h/2) per ray; the bounds are inf where s <= 0."""
    dist = (step + 0.5 * h) * length
    rho = r - dist - h * math.sqrt(3.0)
    assert np.all(rho > 0)
    e, e2 = 3.0 * h * h / (8.0 * rho), step * step * length * length / (8.0 * rho)
    s = length * (cosine - dist / rho)
    with np.errstate(all="ignore"):
        depth = np.where(s > 0, (e + e2 + shift) / s, np.inf)
        angle = np.where(s > 0, np.arcsin(np.minimum(1.0, 3.0 * h / rho)) + length * depth / rho, np.inf)
        ok = (s > 0) & (e / s <= 0.5 * h)
    return depth, angle, ok


def analytic_sphere(K, T, size):
    """(hit, depth, radial (3,H,W), incidence cosine, |(xc, yc, 1)|) of the rays of the fp32 camera, in fp64."""
    H, W = size
    K, T = K.astype(np.float64), T.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.linalg.solve(K[:3, :3], np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1))
    v = (T[:3, :3] @ cam).reshape(3, H, W)                        # the world ray per unit depth
    oc = (T[:3, 3] - np.asarray(SPHERE["centre"]))[:, None, None]
    a, b = (v * v).sum(0), (oc * v).sum(0)
    disc = b * b - a * ((oc * oc).sum(0) - SPHERE["radius"] ** 2)
    with np.errstate(all="ignore"):
        t = (-b - np.sqrt(disc)) / a
    hit = (disc > 0) & (t > 0)
    t = np.where(hit, t, 0.0)
    radial = (oc + t * v) / SPHERE["radius"]
    cosine = -(radial * v).sum(0) / np.sqrt(a)
    return hit, t, radial, cosine, np.sqrt((cam * cam).sum(0)).reshape(H, W)


@pytest.mark.parametrize("cam", SPHERE_HITS)
def test_restatement_meets_the_analytic_sphere(cam):
    size = (23, 31)
    K, T = sphere_camera(cam, size)
    state, _ = sphere_variants()["sphere"]
    h, r = SPHERE["voxel_size"], SPHERE["radius"]
    ref = raycast_reference(*state, h, SPHERE["origin"], K, T, size, step=FINE_STEP)
    hit, depth, radial, cosine, length = analytic_sphere(K, T, size)
    steep = hit & (cosine >= 0.5)
    A, g0 = camera(K, T, h, SPHERE["origin"])
    ys, xs = np.meshgrid(np.arange(size[0], dtype=np.float64), np.arange(size[1], dtype=np.float64), indexing="ij")
    S = np.stack([np.abs(A[a, 0] * xs) + np.abs(A[a, 1] * ys) + np.abs(A[a, 2]) for a in range(3)])
    shift = h * np.sqrt(((EPS * ((depth + FINE_STEP) * S + np.abs(g0)[:, None, None])) ** 2).sum(0))
    depth_bound, angle_bound, ok = sphere_ray_bounds(h, r, FINE_STEP, length, cosine, shift)
    assert steep.sum() >= 300 and ok[steep].all() and np.isfinite(depth_bound[steep]).all()
    assert ref["hit"][steep].all() and ref["defined"][steep].all()
    err = np.abs(ref["depth"] - depth)[steep]
    n = ref["normals"]
    angle = np.arccos(np.clip((n * radial).sum(0), -1, 1))[steep]
    print(f"{cam}: {int(steep.sum())} rays, depth error max {err.max():.2e} (bound {depth_bound[steep].min():.2e} to "
          f"{depth_bound[steep].max():.2e}, ratio max {(err / depth_bound[steep]).max():.2f}; the rounding term is at most "
          f"{shift[steep].max():.1e}), normal angle max {angle.max():.2e} (bound {angle_bound[steep].min():.2e}, ratio max "
          f"{(angle / angle_bound[steep]).max():.2f})")
    assert (err <= depth_bound[steep]).all()
    assert (angle <= angle_bound[steep]).all()
    assert (np.abs(np.sqrt((n * n).sum(0)) - 1)[steep] < 1e-12).all()
    assert ((n * radial).sum(0)[steep] > 0).all()                 # outwards, as the mesh's normals


def test_the_axis_camera_has_a_ray_along_a_grid_axis():
    for size in ((23, 31), (17, 9)):
        K, T = sphere_camera("axis", size)
        A, _ = camera(K, T, SPHERE["voxel_size"], SPHERE["origin"])
        x, y = np.float32(K[0, 2]), np.float32(K[1, 2])
        assert x == int(x) and y == int(y) and 0 < x < size[1] and 0 < y < size[0]
        a = A.astype(np.float32)
        # the kernel's own fp32 expression: the product of a power of two is exact, so the sum is exactly 0
        d = [np.float32(np.float64(a[m, 0]) * x + np.float64(np.float32(np.float64(a[m, 1]) * y + np.float64(a[m, 2]))))
             for m in range(3)]
        assert d[0] == 0 and d[1] == 0 and d[2] > 0
        ref = reference(f"sphere_axis_{size[0]}x{size[1]}")[0]
        assert ref["dirs"][0, int(y), int(x)] == 0 and ref["dirs"][1, int(y), int(x)] == 0
        assert ref["hit"][int(y), int(x)] and not ref["borderline"][int(y), int(x)]


@pytest.mark.parametrize("name", [n for n in CASE_IDS if n not in NO_HIT_IDS])
def test_conditions_on_the_inputs(name):
    case = render_case(name)
    for v, ref in enumerate(reference(name)):
        share, hits = float(ref["borderline"].mean()), int(ref["hit"].sum())
        print(f"{name}[{v}]: borderline {100 * share:.2f} %, hits {hits} of {ref['hit'].size} "
              f"({100 * ref['hit'].mean():.1f} %), undefined samples {ref['undefined']} of {ref['samples']}")
        assert share <= BORDERLINE_CAP
        if case["small"]:
            assert hits >= 1
        else:
            assert hits >= 100 and hits >= 0.1 * ref["hit"].size
        assert np.isfinite(ref["depth_bound"][ref["hit"] & ~ref["borderline"]]).all()


@pytest.mark.parametrize("name", NO_HIT_IDS)
def test_no_hit_cases_give_zero_maps(name):
    for ref in reference(name):
        assert not ref["hit"].any() and not ref["borderline"].any()
        for key in ("depth", "normals", "colors", "weight"):
            assert not ref[key].any(), key


def test_variants_differ_from_the_plain_sphere_where_the_block_is():
    plain, hole = reference("sphere_rolled_23x31")[0], reference("hole_rolled_23x31")[0]
    lost = plain["hit"] & ~hole["hit"]
    assert lost.sum() >= 50                                        # the block is seen
    nan = reference("nan_under_weight_0_rolled_23x31")[0]
    light = reference("min_weight_rolled_23x31")[0]
    for other in (nan, light):
        np.testing.assert_array_equal(other["hit"], hole["hit"])
    np.testing.assert_array_equal(nan["depth"], hole["depth"])     # the values under weight 0 reach nothing
    assert np.isfinite(nan["colors"]).all() and np.isfinite(nan["normals"]).all()
    assert reference("no_colour_rolled_23x31")[0]["colors"] is None


def test_the_shells_case_needs_the_back_face_rule():
    # from inside the inner sphere every ray leaves it from behind and would meet the outer shell from the front: with
    # the rule no pixel hits, without it every clear pixel does, so a march that lacks the rule fails this case
    name = "shells_inside_23x31"
    assert name in NO_HIT_IDS
    with_rule, without = reference(name)[0], reference(name, back_face=False)[0]
    clear = ~with_rule["borderline"] & ~without["borderline"]
    assert not with_rule["hit"].any() and clear.sum() >= 0.97 * clear.size
    # (the camera is 0.1 from the centre, so the outer shell is at least 0.6 away, 0.42 in depth on the corner rays,
    # whose (x, y, 1) has length 1.42: well behind the inner sphere's far side)
    assert without["hit"][clear].all() and (without["depth"][clear] > 0.35).all()
    # and on the plain sphere seen from inside the rule decides nothing: the reason the shells are a case of their own
    assert not reference("sphere_inside_23x31", back_face=False)[0]["hit"].any()
