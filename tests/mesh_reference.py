"""numpy restatement of the mesh components and the mesh filter (multi_view_stereonet_amd/mesh.py, csrc/mvsn_mesh.hip;
DESIGN.md section 18), the meshes both test files label, and the fixture "two spheres and a speck".  Everything is
integer work: the device is compared with this exactly."""
import functools

import numpy as np

from tsdf_reference import surface_nets_reference, voxel_centres


def components_reference(faces, m):
    """faces (F,3) integers, m vertex rows.  Min-label propagation over the sides of the faces with a pointer jump to a
    fixed point, then dense ids by lowest vertex row.  Returns a dict: vertex_label (m), face_label (F), vertex_count,
    face_count, first (C), all int64."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < m)).all(1)
    good = faces[ok]
    u = np.concatenate([good[:, 0], good[:, 1], good[:, 2]])
    v = np.concatenate([good[:, 1], good[:, 2], good[:, 0]])
    label = np.arange(m, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, u, label[v])
        np.minimum.at(new, v, label[u])
        while True:                                   # label[v] is a row of v's component, never above v: jump
            jump = new[new]
            if (jump == new).all():
                break
            new = jump
        if (new == label).all():
            break
        label = new
    first = np.nonzero(label == np.arange(m))[0].astype(np.int64)        # ascending
    vertex_label = np.searchsorted(first, label).astype(np.int64)
    face_label = np.full(faces.shape[0], -1, np.int64)
    face_label[ok] = vertex_label[good[:, 0]]
    c = first.shape[0]
    return {"vertex_label": vertex_label, "face_label": face_label,
            "vertex_count": np.bincount(vertex_label, minlength=c).astype(np.int64),
            "face_count": np.bincount(face_label[ok], minlength=c).astype(np.int64), "first": first}


def keep_reference(comp, min_faces=None, min_vertices=None, keep_largest=None):
    """The (C,) bool choice of filter_mesh's three rules."""
    keep = np.ones(comp["first"].shape[0], bool)
    if min_faces is not None:
        keep &= comp["face_count"] >= min_faces
    if min_vertices is not None:
        keep &= comp["vertex_count"] >= min_vertices
    if keep_largest is not None:
        passed = np.nonzero(keep)[0]
        order = sorted(passed.tolist(), key=lambda i: (-int(comp["face_count"][i]), i))    # ties to the lower id
        keep = np.zeros_like(keep)
        keep[order[:keep_largest]] = True
    return keep


def filter_reference(mesh, comp, keep):
    """mesh: a dict with vertices, normals, colors (or None), faces, cell; keep (C,) bool.  The gather of the kept
    vertices and faces in their input order, faces renumbered: the same keys plus vertex_rows and face_rows."""
    keep = np.asarray(keep, bool)
    vertex_rows = np.nonzero(keep[comp["vertex_label"]])[0].astype(np.int64)
    fl = comp["face_label"]
    face_rows = np.nonzero((fl >= 0) & keep[np.maximum(fl, 0)])[0].astype(np.int64)
    new_row = np.full(comp["vertex_label"].shape[0], -1, np.int64)
    new_row[vertex_rows] = np.arange(vertex_rows.shape[0])
    return {"vertices": mesh["vertices"][vertex_rows], "normals": mesh["normals"][vertex_rows],
            "colors": mesh["colors"][vertex_rows] if mesh["colors"] is not None else None,
            "cell": mesh["cell"][vertex_rows], "faces": new_row[np.asarray(mesh["faces"], np.int64)[face_rows]].reshape(-1, 3),
            "vertex_rows": vertex_rows, "face_rows": face_rows}


# ---- the meshes ------------------------------------------------------------------------------------------------------
def _strip(n_faces):
    i = np.arange(n_faces, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


def _grid(rows, cols):
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    a = (r * cols + c).reshape(-1).astype(np.int64)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)])


def _relabel(faces, m, seed):
    """The same graph with its rows under a seeded random permutation and its faces shuffled."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m).astype(np.int64)
    return perm[faces][rng.permutation(faces.shape[0])]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (faces (F,3) int64, m): made once, never modified."""
    out = {}
    out["no_faces"] = (np.zeros((0, 3), np.int64), 5)
    out["one_triangle"] = (np.array([[2, 0, 1]], np.int64), 3)
    # a fan around row 0 and a fan around row 5 that share row 4 and nothing else
    out["two_fans_one_vertex"] = (np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 6, 7], [5, 7, 8], [5, 8, 4]], np.int64), 9)
    # two triangles whose vertices would sit at the same three positions, in rows of their own
    out["coincident_positions"] = (np.array([[0, 1, 2], [3, 4, 5]], np.int64), 6)
    # 1027 triangles over 1029 rows: five workgroups of vertices, the last with five threads; the longest chains there
    # are, across every workgroup boundary
    strip = _strip(1027)
    out["strip_ascending"] = (strip, 1029)
    out["strip_descending"] = (1028 - strip, 1029)
    out["strip_permuted"] = (_relabel(strip, 1029, 11), 1029)
    # 1500 faces that share one row and nothing else: every thread works on one root
    i = np.arange(1500, dtype=np.int64)
    out["star_on_last_row"] = (np.stack([np.full(1500, 3000), 2 * i, 2 * i + 1], 1), 3001)
    out["star_on_row_0"] = (np.stack([np.zeros(1500, np.int64), 2 * i + 1, 2 * i + 2], 1), 3001)
    # 700 disjoint triangles and 700 rows no face uses, rows permuted: 1400 components over 11 workgroups
    j = 4 * np.arange(700, dtype=np.int64)
    out["many_small"] = (_relabel(np.stack([j, j + 1, j + 2], 1), 2800, 12), 2800)
    # a 256 x 256 grid and 50 detached triangles, rows permuted: 65 686 rows, 130 100 faces, 51 components
    k = 65536 + 3 * np.arange(50, dtype=np.int64)
    big = np.concatenate([_grid(256, 256), np.stack([k, k + 1, k + 2], 1)])
    out["grid_256_permuted"] = (_relabel(big, 65536 + 150, 13), 65536 + 150)
    # faces that take no part (-1, m and 2^40 as an index), repeated indices, duplicated faces, and rows only a bad face
    # names (7, 8: singletons)
    out["face_validity"] = (np.array([[0, 1, 2], [2, 3, -1], [3, 4, 5], [9, 4, 5], [3, 2 ** 40, 4], [4, 3, 5], [3, 4, 5],
                                      [6, 6, 6], [6, 6, 5], [7, 8, 9], [-2 ** 63, 0, 3], [1, 1, 0], [8, 7, 2 ** 31]],
                                     np.int64), 9)
    for faces, _ in out.values():
        faces.setflags(write=False)
    return out


# ---- the fixture: two spheres and a speck ----------------------------------------------------------------------------
SPHERES = dict(dims=(33, 19, 17), voxel_size=0.1, origin=(-1.62, -0.93, -0.81),
               spheres=(((-0.8, 0.02, -0.01), 0.62), ((0.75, -0.05, 0.03), 0.41), ((0.02, 0.6, 0.5), 0.13)))
SPHERES_M, SPHERES_F = 1080, 2148
SPHERES_VERTEX_COUNT, SPHERES_FACE_COUNT, SPHERES_FIRST = [730, 318, 32], [1456, 632, 60], [0, 154, 892]


def spheres_state():
    """(sdf_sum, weight, color_sum) fp32 in the layout (Nz,Ny,Nx): sdf_sum the minimum of the three sphere fields
    |p - c| - r, weight 1, and a smooth colour field."""
    cx, cy, cz = voxel_centres(SPHERES["dims"], SPHERES["voxel_size"], SPHERES["origin"])
    pz, py, px = np.meshgrid(cz, cy, cx, indexing="ij")
    d = np.minimum.reduce([np.sqrt((px - c[0]) ** 2 + (py - c[1]) ** 2 + (pz - c[2]) ** 2) - r
                           for c, r in SPHERES["spheres"]])
    col = np.stack([np.sin(1.3 * px + 0.2), np.cos(0.9 * py - 0.4), np.sin(0.7 * pz + 1.0) * 0.8])
    return d.astype(np.float32), np.ones(d.shape, np.float32), col.astype(np.float32)


@functools.lru_cache(maxsize=None)
def spheres_mesh():
    """The Surface Nets mesh of the fixture as fp32 / uint8 / int64 arrays (what a TSDFMesh holds): made once."""
    s, w, c = spheres_state()
    ref = surface_nets_reference(s, w, c, 1.0, SPHERES["voxel_size"], SPHERES["origin"])
    mesh = {"vertices": ref["vertices"].astype(np.float32), "normals": ref["normals"].astype(np.float32),
            "colors": ref["colors"], "faces": ref["faces"], "cell": ref["cell"]}
    for a in mesh.values():
        a.setflags(write=False)
    return mesh
