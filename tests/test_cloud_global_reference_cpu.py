"""The numpy restatement of global registration (tests/cloud_global_reference.py) against independent forms, and the
condition the end-to-end GPU test rests on, checked on the restatement alone.

Bounds.  u = 2^-24 (fp32), U = 2^-53 (fp64).
  * a block of a defined FPFH row: the 11 fp64 values (F_b 100) / S sum to 100 (1 + 14 U) at most (11 products, 11 quotients
    and the sum S of 11 terms itself, each within U); each is rounded to fp32 once, which moves it by at most u times itself:
    |sum - 100| <= 100 u (1 + 2^-20) when the fp32 values are added in fp64.
  * the descriptor distance: a term (q - t)^2 carries 3 roundings, the sum of 33 non-negative terms 32 more:
    |d2 - exact| <= 35 u d2 (1 + 2^-20).  Two candidates whose exact distances differ by more than 72 u times the larger
    cannot swap.
  * a cloud under a rigid motion (fp64, rounded to fp32 once): a coordinate moves by at most delta = 2^-24 max|p'| from its
    exact place, a difference of two by 2 delta per axis and as much again for its own rounding: |e' - R e| <= 4 sqrt(3) delta.
    A unit normal moves by sqrt(3) u.  The features are products of at most three unit vectors and l = e / d, so each moves
    by at most eps = 8 (4 sqrt(3) delta / d + 4 u) (to first order, with the roundings of the dozen fp32 operations in the 4 u),
    d2 by 2 d 4 sqrt(3) delta + 3 u d2, and the two dot products that choose the source by d eps.  A pair within those of the
    radius, of a bin edge, of a sector boundary or of the tie is `fragile`; a row without a fragile pair has equal counts.
  * the pose of three exact correspondences: a frame vector carries a relative error of a few U over the sine of the
    triangle's angle at p0; with sin^2 > 1/16 (the cases are chosen so) R and t are within 2^10 U (1 + |c_s|) of the truth.
"""
import numpy as np
import pytest

import cloud_global_reference as cg
from cloud_normals_reference import _surface

U32, U64 = 2.0 ** -24, 2.0 ** -53


def test_the_sector_table_and_the_bins():
    k = np.arange(1, 11)
    ang = -np.pi + 2 * np.pi * k / 11
    assert np.array_equal(cg.SECTOR, np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))
    rng = np.random.default_rng(271)
    phi = rng.uniform(-np.pi, np.pi, 20000)
    away = np.abs((phi + np.pi) / (2 * np.pi / 11) - np.round((phi + np.pi) / (2 * np.pi / 11))) > 1e-4
    r = rng.uniform(0.1, 3.0, 20000)
    got = cg.sector_bin((r * np.cos(phi)).astype(np.float32), (r * np.sin(phi)).astype(np.float32))
    want = np.clip(np.floor(11 * (phi + np.pi) / (2 * np.pi)), 0, 10).astype(int)
    assert (got[away] == want[away]).all() and away.mean() > 0.99
    assert cg.sector_bin(np.float32(-1), np.float32(0)) == 10 and cg.sector_bin(np.float32(-1), np.float32(-1e-30)) == 0
    assert cg.sector_bin(np.float32(1), np.float32(0)) == 5
    f = np.array([-1.5, -1, -1 + 2 / 11 - 1e-3, -1 + 2 / 11 + 1e-3, 0, 0.999, 1, 1.5, np.nan, np.inf, -np.inf], np.float32)
    assert cg.linear_bin(f).tolist() == [0, 0, 0, 1, 5, 10, 10, 10, 0, 10, 0]


@pytest.mark.parametrize("name", cg.FPFH_IDS)
def test_block_sums(name):
    ref = cg.fpfh_case_reference(name)
    assert (ref["spfh"].reshape(-1, 3, 11).sum(axis=2) == ref["pairs"][:, None]).all() and (ref["spfh"] >= 0).all()
    sums = ref["features"].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    d = ref["defined"]
    assert (np.abs(sums[d] - 100.0) <= 100 * U32 * (1 + 2.0 ** -20)).all() and not ref["features"][~d].any()
    assert (ref["features"] >= 0).all() and np.isfinite(ref["features"]).all()
    if name in ("s300", "s2049", "crowded", "hand"):
        assert d.sum() > len(d) // 2
    if name == "hand":
        c = cg.fpfh_case(name)
        assert not ref["pairs"][~cg.normal_ok(c["normals"])].any() and (~d).sum() > 60


def _rigid(p, n, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    moved = (p.astype(np.float64) @ q.T + rng.uniform(-2, 2, 3)).astype(np.float32)
    return moved, (n.astype(np.float64) @ q.T).astype(np.float32)


@pytest.mark.parametrize("name", ["s300", "s2049"])
def test_descriptors_follow_a_rigid_motion_and_a_permutation(name):
    c = cg.fpfh_case(name)
    p, n, h = c["points"], c["normals"], c["h"]
    detail = []
    spfh, pairs = cg.spfh_reference(p, n, h, detail)
    moved, turned = _rigid(p, n, 273)
    perm = np.random.default_rng(274).permutation(len(p))
    spfh2, pairs2 = cg.spfh_reference(moved[perm], turned[perm], h)
    d = {k: np.concatenate([x[k] for x in detail]) for k in detail[0]}
    r2 = float(np.float32(h) * np.float32(h))
    delta = U32 * float(np.abs(moved).max())
    dist = np.sqrt(d["d2"].astype(np.float64))
    eps = 8 * (4 * np.sqrt(3) * delta / dist + 4 * U32)
    frag = np.abs(np.abs(d["ai"]) - np.abs(d["aj"])) <= dist * eps
    for f in (d["f1"], d["f2"]):
        x = (f.astype(np.float64) + 1) * 5.5
        frag |= (np.abs(x - np.round(x)) <= 5.5 * eps) & (np.round(x) >= 1) & (np.round(x) <= 10)
    cross = cg.SECTOR[None, :, 0].astype(np.float64) * d["s3"][:, None] - cg.SECTOR[None, :, 1].astype(np.float64) * d["c3"][:, None]
    frag |= (np.abs(cross) <= 2 * eps[:, None]).any(axis=1) | (np.abs(d["s3"]) <= eps)
    fragile_row = np.zeros(len(p), bool)
    fragile_row[d["i"][frag]] = True
    # a neighbour near the radius, counted or not
    dd = ((p[:, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(axis=2)
    edge = np.abs(dd - r2) <= 2 * np.sqrt(r2) * 4 * np.sqrt(3) * delta + 4 * U32 * r2
    fragile_row |= edge.any(axis=1)
    same = (spfh2 == spfh[perm]).all(axis=1) & (pairs2 == pairs[perm])
    print(f"{name}: {int(frag.sum())} fragile pairs of {len(frag)}, {int(fragile_row.sum())} fragile rows of {len(p)}, "
          f"{int((~same).sum())} rows differ")
    assert same[~fragile_row[perm]].all()
    # the cap, on pairs (a row has a hundred pairs or more and is fragile with one of them).  At the typical d = h / 2 eps is
    # about 6e-5; f1 and f2 have ten inner edges each on a range of 2 and a window of 2 eps around each, the angle ten
    # boundaries with windows of about 4 eps on a range of 2 pi: 1.5e-3 of the pairs were the features spread evenly, and
    # they pile up (f1 near 0, the angle near 0) on a smooth surface by a small factor.  One per cent is the cap.
    assert frag.mean() <= 0.01
    # the permutation alone changes nothing at all (no tie between the two angles of a pair in these clouds)
    spfh3, pairs3 = cg.spfh_reference(p[perm], n[perm], h)
    assert np.array_equal(spfh3, spfh[perm]) and np.array_equal(pairs3, pairs[perm])
    assert not (np.abs(d["ai"]) == np.abs(d["aj"])).any()


@pytest.mark.parametrize("name", ["sizes_257_513", "ties", "absent", "none", "scene"])
def test_feature_nearest_against_float64(name):
    c = cg.match_case(name)
    q, t = c["query"], c["target"]
    ref = cg.feature_nearest_reference(q, t, mutual=True)
    pq, pt = cg.takes_part(q), cg.takes_part(t)
    assert (ref["index"][~pq] == -1).all() and np.isposinf(ref["dist2"][~pq]).all()
    if not pt.any():
        assert (ref["index"] == -1).all() and not ref["mutual"].any()
        return
    with np.errstate(all="ignore"):
        q64, t64 = np.where(pq[:, None], q, 0).astype(np.float64), np.where(pt[:, None], t, 0).astype(np.float64)
        d = (q64 ** 2).sum(1)[:, None] - 2 * q64 @ t64.T + (t64 ** 2).sum(1)[None, :]
        if len(q) * len(t) < 1 << 18:
            d = ((q64[:, None, :] - t64[None, :, :]) ** 2).sum(axis=2)
    d[:, ~pt] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(q))
    best = d[rows, order[:, 0]]
    second = d[rows, order[:, 1]] if len(t) > 1 else np.full(len(q), np.inf)
    clear = pq & (second - best > 72 * U32 * second + 1e-9 * (name == "scene") * second)
    assert (ref["index"][clear] == order[clear, 0]).all() and clear.sum() >= (0.5 * pq.sum() if name != "ties" else 1)
    found = ref["index"] >= 0
    assert (np.abs(ref["dist2"][found] - best[found]) <= 36 * U32 * best[found] + 1e-9 * (name == "scene") * best[found] + 1e-30).all()
    back = cg.feature_nearest_reference(t, q)["index"]
    assert (ref["mutual"] == (found & (back[np.maximum(ref["index"], 0)] == rows))).all()
    assert (ref["second_dist2"] >= ref["dist2"]).all()


def test_ties_go_to_the_lowest_row():
    c = cg.match_case("ties")
    ref = cg.feature_nearest_reference(c["query"], c["target"])
    assert (ref["index"][:20] == 3).all() and (ref["index"][20:40] == 258).all() and not ref["second_dist2"][:40].any()


def test_the_pose_of_three_exact_correspondences():
    rng = np.random.default_rng(275)
    s = rng.uniform(-2, 2, (400, 3, 3))
    a, b = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
    sin2 = (np.cross(a, b) ** 2).sum(1) / ((a ** 2).sum(1) * (b ** 2).sum(1))
    s = s[sin2 > 1 / 16]
    M = np.linalg.inv(cg.scene_motion())
    t = s @ M[:3, :3].T + M[:3, 3]
    ok, R, tt = cg.ransac_pose(s, t, 0.9)
    assert ok.all() and len(s) > 200
    cs = np.abs(s.mean(axis=1)).max(axis=1)
    bound = 2.0 ** 10 * U64 * (1 + cs)
    assert (np.abs(R - M[:3, :3]).max(axis=(1, 2)) <= bound).all() and (np.abs(tt - M[:3, 3]).max(axis=1) <= bound * 8).all()
    assert (np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) <= 64 * U64).all()
    # the rejections: a stretched edge, a degenerate triangle
    t2 = t.copy()
    t2[:, 2] = t[:, 0] + 1.2 * (t[:, 2] - t[:, 0])
    assert not cg.ransac_pose(s, t2, 0.9)[0].any() and cg.ransac_pose(s, t2, 0.5)[0].all()
    s3 = s.copy()
    s3[:, 2] = s[:, 0] + 2 * (s[:, 1] - s[:, 0])
    assert not cg.ransac_pose(s3, s3, 0.9)[0].any()
    assert cg.ransac_pose(s, t, 1.0)[0].mean() < 0.5 and cg.ransac_pose(s, s, 1.0)[0].all()   # 1.0 wants equal edges, bit for bit


@pytest.mark.parametrize("seed", [0, 1, 2, 2 ** 64 - 1, 0x9E3779B97F4A7C15])
def test_the_draws_cover_the_range_and_are_uniform(seed):
    c, hyp = 97, 20000
    d = cg.ransac_draws(seed, np.arange(hyp), c)
    assert d.shape == (hyp, 3) and d.min() == 0 and d.max() == c - 1
    counts = np.bincount(d.reshape(-1), minlength=c)
    assert (counts > 0).all()
    chi2 = float(((counts - 3 * hyp / c) ** 2 / (3 * hyp / c)).sum())
    df = c - 1
    critical = df * (1 - 2 / (9 * df) + 3.09 * np.sqrt(2 / (9 * df))) ** 3    # Wilson-Hilferty, p = 0.001
    print(f"seed {seed}: chi-square {chi2:.1f} on {df} degrees of freedom (critical {critical:.1f})")
    assert chi2 < critical
    # the same integers by Python's own arithmetic
    for h in (0, 1, 12345, hyp - 1):
        for j in range(3):
            z = (seed + (3 * h + j + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
            z ^= z >> 31
            assert d[h, j] == ((z >> 32) * c) >> 32
    assert cg.ransac_draws(seed, [5], 1).tolist() == [[0, 0, 0]] and cg.ransac_draws(seed, np.arange(50), 2 ** 31 - 1).max() < 2 ** 31 - 1


@pytest.mark.parametrize("name", [n for n in cg.RANSAC_IDS if not n.startswith("scene")])
def test_the_ransac_cases_say_what_they_are_for(name):
    c, ref = cg.ransac_case(name), cg.ransac_case_reference(name)
    status = {"rejected": 2, "two": 1, "unusable": 1}.get(name)
    if status is not None:
        assert ref["best"].tolist() == [-1, 0, status] and not ref["inlier"].any() and np.array_equal(ref["T64"], np.eye(4))
        return
    if name.startswith("c257") and c["hypotheses"] > 1 or name in ("messy", "exact_edge_1"):
        assert ref["best"][2] == 0 and ref["best"][1] >= 3 and ref["inlier"].sum() == ref["best"][1]
        assert ref["best"][1] == ref["counts"].max() and ref["best"][0] == np.argmax(ref["counts"])
        again = cg.ransac_reference(c["source"], c["target"], c["corr"], c["max_dist"], hypotheses=c["hypotheses"], seed=c["seed"] + 1,
                                    edge_similarity=c["edge_similarity"])
        assert again["best"][0] != ref["best"][0] or c["hypotheses"] == 1
    if name == "messy":
        assert not ref["usable"][30:34].any() and not ref["inlier"][30:34].any() and not ref["usable"][40:43].any()
    if name == "exact_edge_1":
        assert np.abs(ref["T64"] - c["T_true"]).max() < 1e-12 and 0 < ref["ok"].sum() < c["hypotheses"]


@pytest.mark.parametrize("seed", cg.SCENE_SEEDS)
def test_the_condition_the_end_to_end_test_rests_on(seed):
    """The coarse pose puts the source within max_dist (RMS) of its true place, the basin of cloud_register, and its inlier
    count is at least twice that of any hypothesis outside the basin."""
    sc, f = cg.scene(), cg.scene_features()
    assert len(sc["target"]) == 4096 and len(sc["source"]) == 3072
    assert f["source_features"]["defined"].all() and f["target_features"]["defined"].all()
    r = cg.scene_ransac(seed, 2.0 ** -30)
    assert r["best"][2] == 0
    rms = cg.rms_to_truth(r["T64"])
    live = np.nonzero(r["ok"])[0]
    T = np.tile(np.eye(4), (len(live), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = r["R"][live], r["t"][live]
    each = np.array([cg.rms_to_truth(x) for x in T])
    outside = each > cg.SCENE_MAX_DIST
    worst = int(r["counts"][live][outside].max()) if outside.any() else 0
    print(f"seed {seed}: {len(f['correspondences'])} correspondences, {len(live)} hypotheses accepted of {cg.SCENE_HYPOTHESES}, winner "
          f"{r['best'][0]} with {r['best'][1]} inliers at RMS {rms:.4f}; best outside the basin {worst}; {int(r['near'].sum())} "
          f"hypotheses with a residual within 2^-30 of the threshold")
    assert rms < cg.SCENE_MAX_DIST
    assert r["best"][1] >= 2 * worst
    assert r["near"].mean() <= 0.01
