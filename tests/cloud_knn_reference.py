"""numpy restatement of the k-nearest-neighbour query between clouds and of the statistical outlier filter (DESIGN.md
section 22; multi_view_stereonet_amd/fusion.py: cloud_knn, statistical_outlier_mask), on top of cloud_reference.py.

The brute force over every (query, target) pair with the kernel's own fp32 operations (cloud_reference.squared_distances),
the candidates masked (d2 <= r2, a usable target, not the query's own row with exclude_self), a stable sort on d2 (stable:
ties keep the order of the rows, so the order is (d2, row)), the first k, padding with (+inf, -1).  dist2, index and within
are the device's exactly and no margin class is needed.  `mean` is the fp64 sum of the k fp64 square roots in slot order,
over k; the statistics are the plain float64 two-pass mean and sample deviation.

The named cases of tests/test_cloud_knn_gpu.py are data here, and tests/test_cloud_knn_reference_cpu.py asserts on the
CPU that none of them is vacuous."""
import functools

import numpy as np

from cloud_reference import grid_edge_clouds, radius_scalars, reach2_clouds, squared_distances, target_cells

MAX_K = 64
U = 2.0 ** -53                     # the unit roundoff of fp64
ALL_K = (1, 2, 7, 8, 9, 16, 17, 32, 33, 63, 64)


def candidates(query, target, max_dist, exclude_self=False):
    """(d2 (N,T) fp32, ok (N,T) bool): the squared distances and which pairs are candidates."""
    q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    _, _, r2 = radius_scalars(max_dist)
    usable, _, _ = target_cells(p, max_dist)
    d2 = squared_distances(q, p)
    with np.errstate(invalid="ignore"):
        ok = (d2 <= r2) & usable[None, :]                    # a NaN compares false
    if exclude_self:
        assert len(q) == len(p)
        ok[np.arange(len(q)), np.arange(len(q))] = False
    return d2, ok


def mean_of_slots(dist2, within, k):
    """(sum_j sqrt((double)dist2[:, j])) / k for j = 0 .. k-1 in that order, one fp64 operation per step; NaN where
    within < k."""
    s = np.zeros(len(dist2), np.float64)
    with np.errstate(all="ignore"):
        for j in range(k):
            s = s + np.sqrt(dist2[:, j].astype(np.float64))
        m = s / np.float64(k)
    return np.where(within >= k, m, np.nan)


def cloud_knn_reference(query, target, k, max_dist, exclude_self=False):
    """dict of dist2 (N,k) f32 (+inf past the last candidate), index (N,k) i64 (-1), within (N,) i32, mean (N,) f64."""
    assert 1 <= k <= MAX_K
    d2, ok = candidates(query, target, max_dist, exclude_self)
    n, m = d2.shape
    masked = np.where(ok, d2, np.float32(np.inf))
    order = np.argsort(masked, axis=1, kind="stable")[:, :k]     # ties: the lowest row first
    rows = np.arange(n)[:, None]
    found = ok[rows, order]
    dist2 = np.full((n, k), np.inf, np.float32)
    index = np.full((n, k), -1, np.int64)
    dist2[:, :order.shape[1]] = np.where(found, masked[rows, order], np.float32(np.inf))
    index[:, :order.shape[1]] = np.where(found, order, -1)
    within = ok.sum(axis=1).astype(np.int32)
    return {"dist2": dist2, "index": index, "within": within, "mean": mean_of_slots(dist2, within, k)}


def mean_stats_reference(mean):
    """(count, mu, sigma) in float64 over the entries that are not NaN: two passes, the sample deviation; sigma = 0 for
    count < 2 and mu = NaN for count = 0."""
    m = np.asarray(mean, np.float64)
    v = m[~np.isnan(m)]
    count = len(v)
    mu = v.sum() / np.float64(count) if count else np.float64(np.nan)
    sigma = np.sqrt(((v - mu) ** 2).sum() / np.float64(count - 1)) if count >= 2 else np.float64(0.0)
    return np.float64(count), np.float64(mu), np.float64(sigma)


def mean_stats_bounds(mean):
    """(bound on |mu - mu'|, bound on |sigma - sigma'|) between two evaluations of mean_stats_reference's formulas that
    add their n terms in fp64 in ANY order (the device's is one, numpy's pairwise sum another).

    u = 2^-53.  A sum of n terms in any order is within gamma_(n-1) sum|x| of the exact sum, gamma_j = j u / (1 - j u)
    (Higham, Accuracy and Stability, section 4.2); the divide adds u: every evaluation of mu is within
    b = (n + 2) u mean|m| of the exact mean (the slack of one u covers the denominator up to n = 2^31), two of them
    within 2 b.  For the exact mean, sum (m - mu) = 0, so sum (m - mu - d)^2 = S0 + count d^2 exactly: an error d <= b of
    the mean adds count b^2 to S0 = sum (m - mu)^2.  Each term fl(fl(m - mu)^2) carries (1 + u)^3 and the sum of these
    non-negative terms gamma_(n-1): S is within ((n + 3) u S0 + count b^2) of S0 to first order; the divide and the square
    root add u each and the root halves the relative error of S: one sigma is within
    sigma ((n + 3) u / 2 + 2 u + count b^2 / (2 S0)), two of them within sigma ((n + 8) u + count b^2 / S0), one u of
    slack covering the second-order terms."""
    m = np.asarray(mean, np.float64)
    v = m[~np.isnan(m)]
    n, count = len(m), len(v)
    _, mu, sigma = mean_stats_reference(m)
    b = (n + 2) * U * np.abs(v).mean()
    s0 = ((v - mu) ** 2).sum()
    assert count >= 2 and s0 > 0
    return 2 * b, sigma * ((n + 8) * U + count * b * b / s0)


def statistical_outlier_reference(points, k, std_ratio, max_dist):
    """dict of keep (N,) bool, mean_dist (N,) f64, mean, std (f64 scalars), threshold."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    md = cloud_knn_reference(p, p, k, max_dist, exclude_self=True)["mean"]
    _, mu, sigma = mean_stats_reference(md)
    threshold = mu + np.float64(std_ratio) * sigma           # one fp64 multiply, one fp64 add
    with np.errstate(invalid="ignore"):
        keep = md <= threshold                               # a NaN compares false
    return {"keep": keep, "mean_dist": md, "mean": mu, "std": sigma, "threshold": threshold}


def outlier_margin(ref, k, std_ratio):
    """(N,) the distance from the threshold within which the device's comparison may differ from the restatement's:
    the device's mean_dist is within (k + 2) 2^-52 of the restatement's (tests/test_cloud_knn_gpu.py derives it), its mu
    and sigma within mean_stats_bounds, and the threshold's multiply and add round once each on either side."""
    b_mu, b_sigma = mean_stats_bounds(ref["mean_dist"])
    return (k + 2) * 2.0 ** -52 * np.abs(ref["mean_dist"]) + b_mu + std_ratio * b_sigma + 4 * U * abs(ref["threshold"])


# ---- the cases ----------------------------------------------------------------------------------------------------------
H = 0.25
CLUMPS = ALL_K                    # isolated clumps of exactly this many targets, each with a query in its middle


def _lattice():
    """The integer lattice {0..5}^3 times 2^-4: every coordinate, difference, square and sum is exact in fp32, so equal
    integer distances are equal d2: ties everywhere, and more than 64 lattice points within 0.25 = 4 steps of any of
    them."""
    g = np.arange(6, dtype=np.float64)
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * 2.0 ** -4).astype(np.float32)


def _sheet(rng, n):
    """n points near the saddle z = 0.3 x y over [-3,3]^2, moved to (10, 0, 0): a point or two per radius."""
    xy = rng.uniform(-3.0, 3.0, (n, 2))
    z = 0.3 * xy[:, 0] * xy[:, 1] / 3.0 + rng.normal(0.0, 0.02, n)
    return (np.column_stack([xy[:, 0] + 10.0, xy[:, 1], z])).astype(np.float32)


def _clump_centre(j):
    return np.array([-4.0 - 2.0 * j, 6.0, 1.0])


def _mixed_target(seed):
    """Lattice, sparse sheet, clumps of exactly CLUMPS[j] points, exact duplicates, non-finite rows; in a shuffled row
    order, so that ties are not decided by the order of construction."""
    rng = np.random.default_rng(seed)
    lat, sheet = _lattice(), _sheet(rng, 400)
    clumps = [(_clump_centre(j) + rng.uniform(-0.1, 0.1, (c, 3))).astype(np.float32) for j, c in enumerate(CLUMPS)]
    dup = np.concatenate([np.repeat(lat[[43, 86, 129]], 3, axis=0), np.repeat(sheet[:5], 2, axis=0)])
    bad = np.array([[np.nan, 0.1, 0.1], [0.1, -np.inf, 0.1], [np.nan, np.nan, np.nan], [0.2, 0.2, np.inf]], np.float32)
    t = np.concatenate([lat, sheet, dup, bad] + clumps)
    return t[rng.permutation(len(t))]


def _mixed_queries(target, nq, seed):
    """Row 0: the lattice's centre cell's middle (ties, more than 64 candidates).  Then in turn: lattice points
    themselves, lattice cell middles, points around the sheet, the clumps' centres, rows that are not finite, rows far
    outside the grid, empty space."""
    rng = np.random.default_rng(seed)
    lat = _lattice()
    special = [np.array([2.5, 2.5, 2.5]) * 2.0 ** -4]
    special += [_clump_centre(j) for j in range(len(CLUMPS))]
    special += [(np.nan, 0, 0), (np.inf, 0, 0), (0.1, -np.inf, np.nan), (1.0e6, 0, 0),
                (2.0 ** 20 * H + 0.1, 0, -(2.0 ** 20) * H - 1.0), (-3.0e38, 3.0e38, 0), (50.0, 50.0, 50.0)]
    q = np.zeros((max(nq, len(special)), 3), np.float32)
    for i in range(len(q)):
        kind = i % 4
        if kind == 0:
            q[i] = lat[rng.integers(len(lat))]
        elif kind == 1:
            q[i] = lat[rng.integers(len(lat))] + np.float32(2.0 ** -5) * rng.integers(0, 2, 3).astype(np.float32)
        else:
            q[i] = _sheet(rng, 1)[0] + rng.normal(0, 0.05, 3).astype(np.float32)
    q[:len(special)] = np.asarray(special, np.float32)
    return q[:nq]


def _mixed(nq, seed, ks=ALL_K):
    t = _mixed_target(seed)
    return dict(query=_mixed_queries(t, nq, seed + 1), target=t, h=H, ks=ks, exclude_self=(False,))


def _self():
    """The mixed target against itself, with and without exclude_self: every row has itself at distance 0, and the
    duplicated rows have exact duplicates of the query."""
    t = _mixed_target(171)
    return dict(query=t, target=None, h=H, ks=(1, 8, 33, 64), exclude_self=(False, True))


def _tiny():
    """The mixed case times 2^-72 (a power of two: the lattice stays exact): h = 2^-74, r2 < 2^-100, the two-cell
    reach; squares of differences are denormals."""
    c = _mixed(257, 172, ks=(8, 17))
    s = np.float32(2.0 ** -72)
    far = np.abs(np.nan_to_num(c["query"], nan=0.0, posinf=0.0, neginf=0.0)).max(axis=1) >= 40
    q = np.where(far[:, None], c["query"], c["query"] * s)
    return dict(query=q.astype(np.float32), target=(c["target"] * s).astype(np.float32), h=H * 2.0 ** -72, ks=c["ks"],
                exclude_self=(False,))


def _dense(order):
    """600 targets inside one radius of query 0, as 200 distinct points three times each (a tie at every k-th place that
    is not a multiple of 3), sorted by increasing (+1) or decreasing (-1) distance from it: the best and the worst
    arrival order for an insertion.  Query 1 sees the edge of the cluster only, query 2 nothing."""
    rng = np.random.default_rng(173)
    centre = np.array([0.6, 0.6, 0.6])
    d = rng.normal(size=(200, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.11, (200, 1))
    t = np.repeat((centre + d).astype(np.float32), 3, axis=0)
    q = np.array([centre, centre + [0.33, 0.0, 0.0], centre + [3.0, 0.0, 0.0]], np.float32)
    d2 = squared_distances(q[:1], t)[0]
    t = t[np.argsort(d2, kind="stable")[::order]]
    return dict(query=q, target=t, h=H, ks=(8, 64), exclude_self=(False,))


_CASES = {"n1": lambda: _mixed(1, 161), "n255": lambda: _mixed(255, 163), "n256": lambda: _mixed(256, 165),
          "n257": lambda: _mixed(257, 167), "self": _self, "tiny": _tiny, "dense_up": lambda: _dense(1),
          "dense_down": lambda: _dense(-1)}
CASE_IDS = tuple(_CASES)
# one query cannot have both more and fewer candidates than k <= 64 and a list longer than 64: n1 is the query in the
# lattice (more than k, ties, longer than 64) and is exempt from "fewer"
SINGLE_IDS = ("n1",)




def _walk(clouds):
    q, t, h = clouds()
    return dict(query=q, target=t, h=h, ks=(1, 9), exclude_self=(False,))


# cloud_nearest's two hard inputs at a few dozen points (cloud_reference.py), through the visitor form of the walk.  Too
# small for what every case of CASE_IDS holds (a list longer than 64, a tie at every k): they stand beside them.
_WALK_CASES = {"reach2": lambda: _walk(reach2_clouds), "grid_edge": lambda: _walk(grid_edge_clouds)}
WALK_IDS = tuple(_WALK_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """Made once, never modified."""
    return (_CASES.get(name) or _WALK_CASES[name])()


RUNS = tuple((name, k, ex) for name in CASE_IDS + WALK_IDS for k in case(name)["ks"] for ex in case(name)["exclude_self"])


def case_target(name):
    c = case(name)
    return c["query"] if c["target"] is None else c["target"]


@functools.lru_cache(maxsize=None)
def case_reference(name, k, exclude_self=False):
    c = case(name)
    return cloud_knn_reference(c["query"], case_target(name), k, c["h"], exclude_self)


# ---- the statistical outlier filter's cases -----------------------------------------------------------------------------
def _plane():
    """A jittered 40 x 40 grid of spacing 0.05 on the plane z = 0.1 x, twelve planted points 0.2 to 0.3 above it (they have
    their k neighbours within max_dist, far away), two points with nobody within max_dist and one row that is not finite."""
    rng = np.random.default_rng(181)
    g = np.arange(40, dtype=np.float64) * 0.05
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    x, y = x + rng.uniform(-0.01, 0.01, x.shape), y + rng.uniform(-0.01, 0.01, y.shape)
    plane = np.column_stack([x, y, 0.1 * x + rng.normal(0, 0.002, x.shape)])
    px, py = rng.uniform(0.3, 1.6, 12), rng.uniform(0.3, 1.6, 12)
    planted = np.column_stack([px, py, 0.1 * px + rng.uniform(0.2, 0.3, 12)])
    lone = np.array([[9.0, 9.0, 9.0], [-7.0, 3.0, 1.0]])
    p = np.concatenate([plane, planted, lone, [[np.nan, 0.5, 0.5]]]).astype(np.float32)
    perm = rng.permutation(len(p))
    kind = np.concatenate([np.zeros(len(plane), int), np.ones(12, int), np.full(2, 2), [3]])
    return dict(points=p[perm], kind=kind[perm], k=8, std_ratio=2.0, h=0.5)


def _two_density():
    """Two jittered 30 x 30 sheets with spacings 0.02 and 0.06, far apart: the far wall of a scene next to its near
    one.  radius_outlier_mask at RADIUS_COUNT keeps the dense sheet's interior and drops the sparse sheet."""
    rng = np.random.default_rng(182)
    sheets = []
    for spacing, z in ((0.02, 0.0), (0.06, 2.0)):
        g = np.arange(30, dtype=np.float64) * spacing
        x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
        j = spacing * 0.05
        sheets.append(np.column_stack([x + rng.uniform(-j, j, x.shape), y + rng.uniform(-j, j, y.shape),
                                       z + rng.uniform(-j, j, x.shape)]))
    p = np.concatenate(sheets).astype(np.float32)
    perm = rng.permutation(len(p))
    kind = np.repeat([0, 1], 900)
    gi, gj = (a.reshape(-1) for a in np.meshgrid(np.arange(30), np.arange(30), indexing="ij"))
    interior = np.tile((gi >= 1) & (gi <= 28) & (gj >= 1) & (gj <= 28), 2)
    return dict(points=p[perm], kind=kind[perm], interior=interior[perm], k=8, std_ratio=3.0, h=0.25)


RADIUS_COUNT = (0.03, 4)           # radius_outlier_mask's arguments on the two-density case
_SOR = {"plane": _plane, "two_density": _two_density}
SOR_IDS = tuple(_SOR)


@functools.lru_cache(maxsize=None)
def sor_case(name):
    return _SOR[name]()


@functools.lru_cache(maxsize=None)
def sor_reference(name):
    c = sor_case(name)
    return statistical_outlier_reference(c["points"], c["k"], c["std_ratio"], c["h"])


# ---- inputs of mvsn_cloud_mean_stats -------------------------------------------------------------------------------------
STATS_SIZES = (1, 2, 1023, 1024, 1025, 1024 * 1024 + 1)


@functools.lru_cache(maxsize=None)
def stats_input(n):
    """n positive fp64 values of the size of mean distances, every seventh (from the fourth) NaN."""
    rng = np.random.default_rng(190 + n % 97)
    m = rng.gamma(4.0, 0.01, n)
    m[3::7] = np.nan
    return m
