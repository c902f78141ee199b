"""numpy restatement of the density-based clustering of a cloud and of the cluster selection (DESIGN.md section 24;
multi_view_stereonet_amd/fusion.py: cloud_clusters, cloud_cluster_mask), on top of cloud_reference.py.

The brute force over every pair of rows with the kernel's own fp32 operations (cloud_reference.squared_distances): the
neighbour relation (d2 <= r2, both rows usable), `within` its row sums, the core flags from `within`, the components of the
graph on the core rows by min-label propagation with a pointer jump to a fixed point (as mesh_reference.py), dense ids by
lowest core row, and the border rows by the minimum of (d2 bits, row) over their core neighbours.  Everything is integer
work on exact fp32 distances: the device is compared with this byte for byte and no margin class is needed.

The named cases of tests/test_cloud_cluster_gpu.py are data here, and tests/test_cloud_cluster_reference_cpu.py asserts on
the CPU that none of them is vacuous."""
import functools

import numpy as np

from cloud_reference import (CHUNK_ELEMENTS, grid_edge_clouds, radius_scalars, reach2_clouds, squared_distances,
                             target_cells)
from multi_view_stereonet_amd.fusion import CloudClusters

MAX_POINTS = 16384                 # per case: the brute force stays within a few seconds


def neighbour_pairs(points, eps):
    """(i, j, d2): every ordered pair of rows that are neighbours (i == j included), in row-major order, with its fp32 d2.
    Raises ValueError where a finite point has no cell (cloud_reference.target_cells)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(p)
    _, _, r2 = radius_scalars(eps)
    usable, _, _ = target_cells(p, eps)
    ii, jj, dd = [], [], []
    chunk = max(1, CHUNK_ELEMENTS // max(n, 1))
    for a in range(0, n, chunk):
        d2 = squared_distances(p[a:a + chunk], p)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= r2) & usable[None, :]                # a NaN compares false: a row that is not finite has no pair
        i, j = np.nonzero(ok)
        ii.append(i + a), jj.append(j), dd.append(d2[i, j])
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64), np.concatenate(dd)


def _keys(d2, row):
    """(d2 bits << 32) | row: d2 >= 0, so the order of the bits is the order of the values."""
    return (d2.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | row.astype(np.uint64)


def cloud_clusters_reference(points, eps, min_points, pairs=None):
    """dict of label (N) i64, core (N) bool, within (N) i32, count, core_count, first (C) i64, and `tied` (N) bool: the
    border rows whose least distance to a core neighbour is shared by more than one core neighbour.  `pairs`:
    neighbour_pairs(points, eps) where it is at hand."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(p)
    assert n <= MAX_POINTS and int(min_points) == min_points and min_points >= 1
    i, j, d2 = neighbour_pairs(p, eps) if pairs is None else pairs
    within = np.bincount(i, minlength=n).astype(np.int32)
    finite = np.isfinite(p).all(axis=1)
    core = finite & (within >= min_points)
    # ---- the components of the core graph ----
    e = core[i] & core[j]
    u, v = i[e], j[e]
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, u, label[v])                      # (the pairs are symmetric: both directions are in the list)
        while True:                                          # label[v] is a row of v's component, never above v: jump
            jump = new[new]
            if (jump == new).all():
                break
            new = jump
        if (new == label).all():
            break
        label = new
    first = np.nonzero(core & (label == np.arange(n)))[0].astype(np.int64)       # ascending
    c = len(first)
    out = np.full(n, -1, np.int64)
    out[core] = np.searchsorted(first, label[core])
    # ---- the border rows: the core neighbour with the least (d2 bits, row) ----
    b = ~core[i] & core[j]
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(n, none, np.uint64)
    np.minimum.at(best, i[b], _keys(d2[b], j[b]))
    border = best != none
    assert not (border & ~finite).any() and not (border & core).any()
    out[border] = out[(best[border] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    least = best >> np.uint64(32)
    at_least = np.zeros(n, np.int64)
    np.add.at(at_least, i[b], ((_keys(d2[b], j[b]) >> np.uint64(32)) == least[i[b]]).astype(np.int64))
    labelled = out >= 0
    return {"label": out, "core": core, "within": within,
            "count": np.bincount(out[labelled], minlength=c).astype(np.int64),
            "core_count": np.bincount(out[core], minlength=c).astype(np.int64), "first": first,
            "tied": border & (at_least > 1)}


OUTPUTS = CloudClusters._fields       # label, core, within, count, core_count, first: the restatement's keys are the call's


def cluster_mask_reference(ref, min_size=None, keep_largest=None, keep=None):
    """(N,) bool of cloud_cluster_mask: the (C,) choice by its rules on `count`, then read at the labels; noise False."""
    count, label = ref["count"], ref["label"]
    if keep is None:
        keep = np.ones(len(count), bool)
        if min_size is not None:
            keep &= count >= min_size
        if keep_largest is not None:
            passed = np.nonzero(keep)[0]
            order = sorted(passed.tolist(), key=lambda i: (-int(count[i]), i))      # ties to the lower id
            keep = np.zeros_like(keep)
            keep[order[:keep_largest]] = True
    keep = np.asarray(keep, bool)
    out = np.zeros(len(label), bool)
    has = label >= 0
    out[has] = keep[label[has]]
    return out


def same_partition(a, b):
    """Whether two label arrays (-1 = noise) describe the same noise set and the same partition of the rest."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.shape != b.shape or ((a < 0) != (b < 0)).any():
        return False
    has = a >= 0
    pairs = np.unique(np.stack([a[has], b[has]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- the cases ----------------------------------------------------------------------------------------------------------
H = 0.25


def _mixed(n, seed):
    """n points in a shuffled row order: half of them a jittered sheet of spacing 0.1 (a dozen neighbours within H), a
    third in blobs of about ten points 0.05 wide, the rest scattered over a box 12 wide (noise, and border points where
    they fall next to the sheet)."""
    rng = np.random.default_rng(seed)
    n_sheet, n_blob = n // 2, n // 3
    side = int(np.ceil(np.sqrt(max(n_sheet, 1))))
    g = np.arange(side, dtype=np.float64) * 0.1
    x, y = (a.reshape(-1)[:n_sheet] for a in np.meshgrid(g, g, indexing="ij"))
    sheet = np.column_stack([x + rng.uniform(-0.03, 0.03, n_sheet), y + rng.uniform(-0.03, 0.03, n_sheet),
                             0.2 * x + rng.normal(0, 0.01, n_sheet)])
    centres = rng.uniform(-5.0, -1.0, (max(n_blob // 10, 1), 3))
    blobs = centres[rng.integers(len(centres), size=n_blob)] + rng.uniform(-0.05, 0.05, (n_blob, 3))
    rest = rng.uniform(-6.0, 6.0, (n - n_sheet - n_blob, 3))
    p = np.concatenate([sheet, blobs, rest]).astype(np.float32)
    return p[rng.permutation(n)]


def _chain(n, order):
    """n points 0.2 apart on a line (only the next and the previous one are within H): the longest chains there are,
    across every workgroup boundary; rows ascending (+1), descending (-1) or permuted (0) along it."""
    x = (np.arange(n, dtype=np.float64) * 0.2).astype(np.float32)
    p = np.column_stack([x, np.full(n, 0.5, np.float32), np.full(n, -0.25, np.float32)]).astype(np.float32)
    if order == 0:
        return p[np.random.default_rng(311).permutation(n)]
    return p[::order].copy()


def _bridge(core_middle):
    """Two blobs of 60 points joined by a chain of links 0.2 apart (min_points = 6).  A link is a pair of points 0.01
    apart (6 within H: itself, its twin and the two links next to it), the links two away from the middle are triples,
    and the middle link is a pair (core: one cluster) or a single point (5 within H: not core, while the links next to it
    still have 6; so it is a border point that must not merge the two ends: two clusters)."""
    rng = np.random.default_rng(312)
    a = rng.uniform(-0.08, 0.08, (60, 3)) + [0.0, 0.0, 0.0]
    b = rng.uniform(-0.08, 0.08, (60, 3)) + [4.2, 0.0, 0.0]
    links = []
    for k in range(1, 21):                                   # x = 0.2 .. 4.0; the middle is link 10 at x = 2.0 (and 11)
        copies = 3 if k in (8, 12) else 2
        if k == 10:
            copies = 2 if core_middle else 1
        links += [[0.2 * k, 0.01 * c, 0.0] for c in range(copies)]
    p = np.concatenate([a, np.asarray(links), b]).astype(np.float32)
    return p[rng.permutation(len(p))]


TIE_POINTS = np.array([[0.25, 0.0, 0.0], [0.25, 0.0625, 0.0], [0.25, -0.0625, 0.0],          # rows 0-2: the right triple
                       [-0.25, 0.0, 0.0], [-0.25, 0.0625, 0.0], [-0.25, -0.0625, 0.0],       # rows 3-5: the left triple
                       [0.0, 0.0, 0.0]], np.float32)                                          # row 6: 0.25 from rows 0 and 3
# min_points = 4: rows 0 and 3 are core (their triple and row 6), the others border; row 6 is exactly H from both and
# goes to the lower core row, 0
TIE_LABELS = np.array([0, 0, 0, 1, 1, 1, 0], np.int64)


def _tie(flip):
    """The planted tie; with `flip` the rows of the two triples change places (row 6 then joins the LEFT triple, which
    holds the lower core row)."""
    p = TIE_POINTS.copy()
    if flip:
        p[[0, 1, 2, 3, 4, 5]] = p[[3, 4, 5, 0, 1, 2]]
    return p


def _nonfinite():
    p = _mixed(300, 313).copy()
    p[7] = [np.nan, 0.1, 0.1]
    p[8, 1] = -np.inf
    p[150] = [np.nan, np.nan, np.nan]
    p[299, 2] = np.inf
    p[255], p[256] = p[254], [np.inf, -np.inf, np.nan]
    return p


def _far():
    """21 points 1/16 apart at x = 125 000 = 5 * 10^5 cells of H (fp32 spacing 2^-7 there), 16 points 1/64 apart inside
    the last cell of the grid on +y (cell 2^20 - 1) and 16 inside the first one on -z (cell -2^20), and a loner."""
    k = np.arange(21, dtype=np.float64)
    a = np.column_stack([125000.0 + k / 16.0, np.zeros(21), np.zeros(21)])
    k = np.arange(16, dtype=np.float64)
    b = np.column_stack([np.zeros(16), 262143.75 + k / 64.0, np.ones(16)])
    c = np.column_stack([np.ones(16), np.zeros(16), -262144.0 + k / 64.0])
    p = np.concatenate([a, b, c, [[-125000.0, 7.0, 7.0]]]).astype(np.float32)
    return p[np.random.default_rng(314).permutation(len(p))]


def _tiny():
    """The 257-point mixed case times 2^-72 (a power of two: the fp32 differences scale exactly) with eps = H 2^-72:
    h = 2^-74, r2 < 2^-100, the two-cell reach; squares of differences are denormals."""
    return (_mixed(257, 305) * np.float32(2.0 ** -72)).astype(np.float32)


def _many_small():
    """700 clusters of 3 points 0.05 apart on a lattice of spacing 1, interleaved (point k of every cluster, then point
    k + 1) and permuted: 2100 rows over 9 workgroups, 700 roots to rank."""
    rng = np.random.default_rng(315)
    g = np.arange(700)
    centres = np.column_stack([g % 10, (g // 10) % 10, g // 100]).astype(np.float64)
    p = np.concatenate([centres + rng.uniform(-0.025, 0.025, (700, 3)) for _ in range(3)]).astype(np.float32)
    return p[rng.permutation(len(p))]


def _scene():
    """16 384 points: a sheet of 12 000 (the saddle z = 0.1 x y over [-3, 3]^2, about 7 points within 0.08 of a point),
    40 blobs of 50 points 0.1 wide (the floaters), and 2384 points scattered over a box 8 wide."""
    rng = np.random.default_rng(316)
    xy = rng.uniform(-3.0, 3.0, (12000, 2))
    sheet = np.column_stack([xy[:, 0], xy[:, 1], 0.1 * xy[:, 0] * xy[:, 1] + rng.normal(0.0, 0.005, 12000)])
    centres = rng.uniform(-3.5, 3.5, (40, 3)) + [0.0, 0.0, 2.5]
    blobs = np.repeat(centres, 50, axis=0) + rng.uniform(-0.05, 0.05, (2000, 3))
    rest = rng.uniform(-4.0, 4.0, (2384, 3))
    p = np.concatenate([sheet, blobs, rest]).astype(np.float32)
    return p[rng.permutation(len(p))]


def _lattice(side, spacing):
    g = np.arange(side, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def _ball():
    rng = np.random.default_rng(317)
    d = rng.normal(size=(600, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.3, (600, 1)) + [1.0, 2.0, 3.0]).astype(np.float32)


# name -> (points, eps, the values of min_points)
_CASES = {
    "n1": lambda: (np.array([[0.1, 0.2, 0.3]], np.float32), H, (1, 2)),
    "n255": lambda: (_mixed(255, 301), H, (4,)),
    "n256": lambda: (_mixed(256, 303), H, (4,)),
    "n257": lambda: (_mixed(257, 305), H, (1, 4, 12)),
    "all_noise": lambda: (_lattice(7, 1.0), H, (2,)),                    # 343 points a whole unit apart
    "one_cluster": lambda: (_ball(), H, (3,)),                           # 600 points in a ball of radius 0.3
    "duplicates": lambda: (np.tile(np.array([[0.3, -0.7, 1.1]], np.float32), (1027, 1)), H, (1, 1027, 1028)),
    "chain_up": lambda: (_chain(1029, 1), H, (2, 3)),
    "chain_down": lambda: (_chain(1029, -1), H, (2, 3)),
    "chain_permuted": lambda: (_chain(1029, 0), H, (2, 3)),
    "bridge_core": lambda: (_bridge(True), H, (6,)),
    "bridge_border": lambda: (_bridge(False), H, (6,)),
    "tie": lambda: (_tie(False), H, (4,)),
    "tie_flipped": lambda: (_tie(True), H, (4,)),
    "nonfinite": lambda: (_nonfinite(), H, (1, 4)),
    "far": lambda: (_far(), H, (3,)),
    "tiny": lambda: (_tiny(), H * 2.0 ** -72, (4,)),
    # cloud_nearest's two hard inputs at a few dozen points (cloud_reference.py): both clouds of the two-cell reach as one,
    # and the targets in the grid's last cells (a query beyond the edge has no cell to be indexed in)
    "reach2": lambda: (np.concatenate(reach2_clouds()[:2]), reach2_clouds()[2], (1,)),
    "grid_edge": lambda: (grid_edge_clouds()[1], grid_edge_clouds()[2], (1,)),
    "many_small": lambda: (_many_small(), H, (1, 3, 4)),
    "mixed_2000": lambda: (_mixed(2000, 307), H, (5, 14)),
    "scene": lambda: (_scene(), 0.08, (1, 4, 10)),                       # (at 10 the permutation case: no tied border distance)
}
CASE_IDS = tuple(_CASES)
PERMUTATION_CASE = ("scene", 10)


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, eps, min_points values): made once, never modified."""
    points, eps, mps = _CASES[name]()
    points.setflags(write=False)
    return points, eps, mps


RUNS = tuple((name, mp) for name in CASE_IDS for mp in case(name)[2])


@functools.lru_cache(maxsize=None)
def _case_pairs(name):
    points, eps, _ = case(name)
    return neighbour_pairs(points, eps)


@functools.lru_cache(maxsize=None)
def case_reference(name, min_points):
    points, eps, _ = case(name)
    ref = cloud_clusters_reference(points, eps, min_points, _case_pairs(name))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def permutation(n):
    return np.random.default_rng(318).permutation(n)
