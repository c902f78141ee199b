"""Connected components of a triangle mesh on the device, and the mesh without its small ones (DESIGN.md section 18
states the semantics and the termination and visibility argument of the union-find; the kernels are
csrc/mvsn_mesh.hip).

What ``tsdf.extract_mesh`` gives is raw: every speck of the volume that two noisy views agreed on is a small closed
blob, every depth edge grows a detached sliver.  ``mesh_components`` labels the mesh, ``filter_mesh`` keeps the
components one asks for and renumbers the faces, and ``fusion.write_ply(..., faces=)`` saves the result.

The graph has the vertex rows as nodes and the sides of the faces as edges: two faces that share one vertex are
connected, two vertices at one position in different rows are not.  Everything is integer work and a pure function of
the mesh: the outputs do not depend on the order of the faces, on the order of a face's indices, or on any race.

Scoring a mesh (csrc/mvsn_mesh_sample.hip, csrc/mvsn_mesh_nearest.hip): ``mesh_sample`` draws an
area-uniform cloud from the surface, reproducibly, and ``mesh_nearest`` is the exact distance of points to the surface
within a radius, the mesh counterpart of ``fusion.cloud_nearest``; ``metrics.mesh_metrics`` is built on the two.

Rendering a mesh (csrc/mvsn_mesh_render.hip): ``mesh_render`` rasterises the faces into posed
cameras, the mesh counterpart of ``fusion.cloud_render`` without its holes: depth, face and barycentric maps, and the
interpolated normals and colours.

Making a mesh smaller (csrc/mvsn_mesh_simplify.hip): ``mesh_simplify`` clusters the vertices on
``fusion.voxel_merge``'s grid, remaps the faces, drops the collapsed and the repeated ones, and places each new vertex
by the quadric of the faces around it.

Edges, smoothing and normals (csrc/mvsn_mesh_edges.hip, csrc/mvsn_mesh_smooth.hip): ``mesh_edges``
is the unique edge set with its border, non-manifold and winding flags, ``mesh_smooth`` Taubin or Laplacian smoothing
over it with integer sums, ``mesh_normals`` the face normals, areas and area-weighted vertex normals of any mesh.
"""
from typing import NamedTuple, Optional

import torch

from . import _native
from .tsdf import TSDFMesh, _integer

MAX_ROWS = 2 ** 31 - 1               # vertices, and faces: a row is an int32 on the device


class MeshComponents(NamedTuple):
    vertex_label: torch.Tensor       # (M,) int64 component id of every vertex
    face_label: torch.Tensor         # (F,) int64 component id of every face, -1 for a face that takes no part
    vertex_count: torch.Tensor       # (C,) int64 vertices per component
    face_count: torch.Tensor         # (C,) int64 faces per component
    first: torch.Tensor              # (C,) int64 lowest vertex row of each component, ascending


class FilteredMesh(NamedTuple):
    mesh: TSDFMesh                   # the kept vertices and faces in their input order, faces renumbered
    vertex_rows: torch.Tensor        # (M',) int64 input row of every output vertex
    face_rows: torch.Tensor          # (F',) int64 input row of every output face
    components: MeshComponents       # of the INPUT mesh


def _check_faces(faces, num_vertices):
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise ValueError("faces must be a (F,3) int64 tensor")
    m = _integer(num_vertices, "num_vertices", 0)
    if m > MAX_ROWS or faces.shape[0] > MAX_ROWS:
        raise ValueError(f"at most 2^31 - 1 vertices and faces, got {m} and {faces.shape[0]}")
    return m, int(faces.shape[0])


def mesh_components(faces: torch.Tensor, num_vertices: int) -> MeshComponents:
    """The connected components of the graph whose nodes are the ``num_vertices`` = M vertex rows and whose edges are
    the sides of ``faces`` (F,3) int64.  Component ids are dense, 0..C-1, ordered by the component's lowest vertex row
    (``first``).  A vertex no face uses is a component of its own with ``face_count`` 0.  A face with an index outside
    [0, M) takes no part: its label is -1, it joins nothing and is counted nowhere.  A face with repeated indices is an
    ordinary face of their component; duplicated faces count once each.  M = 0 gives empties (every face -1) without a
    launch; F = 0 gives M singletons.  Bitwise reproducible.  The one host synchronisation is the read of C and the
    status word that size the outputs."""
    m, f = _check_faces(faces, num_vertices)
    dev = faces.device
    i64 = dict(dtype=torch.int64, device=dev)
    if m == 0:                         # no vertex, no component, nothing to launch
        return MeshComponents(torch.empty((0,), **i64), torch.full((f,), -1, **i64), torch.empty((0,), **i64),
                              torch.empty((0,), **i64), torch.empty((0,), **i64))
    if not faces.is_cuda:
        raise RuntimeError("mesh_components runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    fc = faces.detach().contiguous()
    ws_bytes = lib.mvsn_mesh_workspace_bytes(m, f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, **i64)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_components_label(_native.ptr(fc) if f else None, m, f, _native.ptr(head),
                                                     _native.ptr(ws), ws_bytes, st), "mvsn_mesh_components_label")
        c, status = head.tolist()      # the one host synchronisation: sizes the outputs
        if status != 0 or not 1 <= c <= m:
            raise RuntimeError(f"mesh_components: the union-find did not finish (status {status}, {c} components of {m} "
                               "vertices): its workspace was overwritten during the call")
        out = MeshComponents(torch.empty((m,), **i64), torch.empty((f,), **i64), torch.empty((c,), **i64),
                             torch.empty((c,), **i64), torch.empty((c,), **i64))
        _native.check(lib.mvsn_mesh_components_emit(
            _native.ptr(fc) if f else None, m, f, _native.ptr(ws), ws_bytes, c, _native.ptr(out.vertex_label),
            _native.ptr(out.face_label) if f else None, _native.ptr(out.vertex_count), _native.ptr(out.face_count),
            _native.ptr(out.first), st), "mvsn_mesh_components_emit")
    return out


def _check_mesh(mesh):
    if not isinstance(mesh, tuple) or len(mesh) != 5:
        raise ValueError("mesh must be a TSDFMesh (vertices, normals, colors, faces, cell)")
    vertices, normals, colors, faces, cell = mesh
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("mesh.vertices must be a (M,3) float32 tensor")
    m, dev = int(vertices.shape[0]), vertices.device
    for name, t, shape, dtype in (("normals", normals, (m, 3), torch.float32), ("cell", cell, (m,), torch.int64)) + \
            ((("colors", colors, (m, 3), torch.uint8),) if colors is not None else ()):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"mesh.{name} must be a {shape} {dtype} tensor like mesh.vertices")
        if t.device != dev:
            raise ValueError(f"mesh.{name} is on {t.device}, mesh.vertices on {dev}")
    _, f = _check_faces(faces, m)
    if faces.device != dev:
        raise ValueError(f"mesh.faces is on {faces.device}, mesh.vertices on {dev}")
    return m, f, dev


def _check_components(components, m, f, dev):
    if not isinstance(components, tuple) or len(components) != 5:
        raise ValueError("components must be a MeshComponents")
    c = int(components[2].shape[0]) if torch.is_tensor(components[2]) and components[2].dim() == 1 else -1
    for name, t, n in zip(MeshComponents._fields, components, (m, f, c, c, c)):
        if not torch.is_tensor(t) or tuple(t.shape) != (n,) or t.dtype != torch.int64:
            raise ValueError(f"components.{name} must be a ({max(n, 0)},) int64 tensor of this mesh")
        if t.device != dev:
            raise ValueError(f"components.{name} is on {t.device}, the mesh on {dev}")
    if c > m:
        raise ValueError(f"components holds {c} components for a mesh of {m} vertices")
    return c


def filter_mesh(mesh: TSDFMesh, *, min_faces: Optional[int] = None, min_vertices: Optional[int] = None,
                keep_largest: Optional[int] = None, keep: Optional[torch.Tensor] = None,
                components: Optional[MeshComponents] = None) -> FilteredMesh:
    """The mesh of the components of ``mesh`` one keeps.  A component is kept when ``face_count >= min_faces`` (if
    given) and ``vertex_count >= min_vertices`` (if given) and, with ``keep_largest`` = k, it is among the k with the
    most faces of those that passed, ties to the lower id.  ``keep``, a (C,) bool tensor, replaces the three rules
    (combining it with one of them, or giving none of the four, is a ValueError).  The result holds the vertices of the
    kept components and the faces labelled with them, in their input order, ``faces`` renumbered to the new rows,
    ``normals``, ``colors`` (or None) and ``cell`` carried along bit for bit; ``vertex_rows`` and ``face_rows`` give the
    input row of every output row; faces labelled -1 are dropped.  ``components`` describes the input mesh and is
    computed (``mesh_components``) unless handed in.  The choice is made on the device from the (C,) counts; the one
    further host read is (M', F').  Everything is validated here, before any launch."""
    m, f, dev = _check_mesh(mesh)
    rules = [r is not None for r in (min_faces, min_vertices, keep_largest)]
    if keep is not None and any(rules):
        raise ValueError("keep replaces min_faces, min_vertices and keep_largest: give it alone")
    if keep is None and not any(rules):
        raise ValueError("give one of min_faces, min_vertices, keep_largest or keep")
    lo_f = _integer(min_faces, "min_faces", 0) if min_faces is not None else None
    lo_v = _integer(min_vertices, "min_vertices", 0) if min_vertices is not None else None
    top = _integer(keep_largest, "keep_largest", 0) if keep_largest is not None else None
    if keep is not None and (not torch.is_tensor(keep) or keep.dim() != 1 or keep.dtype != torch.bool):
        raise ValueError("keep must be a (C,) bool tensor")
    if keep is not None and keep.device != dev:
        raise ValueError(f"keep is on {keep.device}, the mesh on {dev}")
    c = _check_components(components, m, f, dev) if components is not None else None
    if keep is not None and c is not None and keep.shape[0] != c:
        raise ValueError(f"keep must be a ({c},) bool tensor, one entry per component, got {tuple(keep.shape)}")
    if m > 0 and not mesh.vertices.is_cuda:
        raise RuntimeError("filter_mesh runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    if components is None:
        components = mesh_components(mesh.faces, m)
        c = int(components.first.shape[0])
        if keep is not None and keep.shape[0] != c:
            raise ValueError(f"keep must be a ({c},) bool tensor, one entry per component, got {tuple(keep.shape)}")

    def out(mo, fo):
        return FilteredMesh(TSDFMesh(torch.empty((mo, 3), dtype=torch.float32, device=dev),
                                     torch.empty((mo, 3), dtype=torch.float32, device=dev),
                                     torch.empty((mo, 3), dtype=torch.uint8, device=dev) if mesh.colors is not None else None,
                                     torch.empty((fo, 3), dtype=torch.int64, device=dev),
                                     torch.empty((mo,), dtype=torch.int64, device=dev)),
                            torch.empty((mo,), dtype=torch.int64, device=dev),
                            torch.empty((fo,), dtype=torch.int64, device=dev), components)
    if m == 0 or c == 0:               # no vertex, no component, nothing to launch
        return out(0, 0)

    if keep is None:                   # plumbing on (C,) tensors, no host read
        keep = torch.ones((c,), dtype=torch.bool, device=dev)
        if lo_f is not None:
            keep &= components.face_count >= lo_f
        if lo_v is not None:
            keep &= components.vertex_count >= lo_v
        if top is not None:
            # the passed components by falling face count, a stable sort: ties keep the order of the ids
            order = torch.argsort(torch.where(keep, components.face_count, -1), descending=True, stable=True)
            among = torch.zeros_like(keep)
            among[order[:top]] = True
            keep &= among
    lib = _native.load()
    keep_c = keep.detach().contiguous().view(torch.uint8)
    tensors = [t.detach().contiguous() if t is not None else None
               for t in (mesh.vertices, mesh.normals, mesh.colors, mesh.cell, mesh.faces, components.vertex_label,
                         components.face_label)]
    vertices, normals, colors, cell, faces, vertex_label, face_label = tensors
    ws_bytes = lib.mvsn_mesh_workspace_bytes(m, f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_select(_native.ptr(vertex_label), _native.ptr(face_label) if f else None,
                                           _native.ptr(keep_c), m, f, c, _native.ptr(head), _native.ptr(ws), ws_bytes, st),
                      "mvsn_mesh_select")
        mo, both = head.tolist()       # the one further host read: sizes the outputs
        fo = both - mo
        res = out(mo, fo)
        if mo == 0:                    # nothing kept
            return res
        _native.check(lib.mvsn_mesh_compact(
            _native.ptr(vertices), _native.ptr(normals), _native.ptr(colors), _native.ptr(cell),
            _native.ptr(faces) if f else None, _native.ptr(face_label) if f else None, _native.ptr(keep_c), m, f, c,
            _native.ptr(ws), ws_bytes, mo, fo, _native.ptr(res.mesh.vertices), _native.ptr(res.mesh.normals),
            _native.ptr(res.mesh.colors), _native.ptr(res.mesh.cell), _native.ptr(res.mesh.faces) if fo else None,
            _native.ptr(res.vertex_rows), _native.ptr(res.face_rows) if fo else None, st), "mvsn_mesh_compact")
    return res


# ---- scoring a mesh: surface samples and the point-to-mesh distance ---------------------------
NEAREST_BOX_CELLS = 512              # a face whose box of cells is larger goes on the list every query tests directly
MESH_SAMPLE_STATUS_NO_AREA = 1
MESH_NEAREST_STATUS_RANGE = 1


class MeshSamples(NamedTuple):
    points: torch.Tensor             # (n,3) fp32 the sample positions
    face: torch.Tensor               # (n,) int64 the face each sample was drawn from
    weights: torch.Tensor            # (n,3) fp32 barycentric weights
    normals: Optional[torch.Tensor]  # (n,3) fp32 interpolated vertex normals, or None
    colors: Optional[torch.Tensor]   # (n,3) uint8 interpolated vertex colours, or None


class MeshNearest(NamedTuple):
    dist2: torch.Tensor              # (N,) fp32 squared distance to the mesh, +inf where no face is within max_dist
    face: torch.Tensor               # (N,) int64 the nearest face's row, -1 where none
    point: torch.Tensor              # (N,3) fp32 the closest point on the mesh, 0 where none
    weights: torch.Tensor            # (N,3) fp32 its barycentric weights, 0 where none
    within: torch.Tensor             # (N,) int32 the number of faces within max_dist


def _check_surface(vertices, faces):
    """(M, F, device) of a mesh given as vertices (M,3) fp32 and faces (F,3) int64 on one device; ValueError otherwise."""
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError("vertices must be a (M,3) float32 tensor")
    m, f = _check_faces(faces, int(vertices.shape[0]))
    if faces.device != vertices.device:
        raise ValueError(f"faces are on {faces.device}, vertices on {vertices.device}")
    return m, f, vertices.device


def mesh_sample(vertices: torch.Tensor, faces: torch.Tensor, n: int, *, seed: int = 0,
                normals: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None) -> MeshSamples:
    """``n`` points drawn uniformly by area from the surface of the mesh ``vertices`` (M,3) fp32, ``faces`` (F,3) int64:
    what turns a mesh into a cloud for ``metrics.cloud_metrics`` (csrc/mvsn_mesh_sample.hip).

    The areas are taken in fp64 and turned into exact integers, ``q = floor(area * 2^(31 - ilogb(largest area)))``; their
    prefix is an integer scan, so it does not depend on any order of summation.  A face with an index outside [0, M) or
    a vertex that is not finite has area 0, and so has a face below 2^-31 of the largest face: none of them is ever
    drawn.  Sample i takes three splitmix64 draws of ``seed`` (an integer in [0, 2^64)): the first picks the face through
    the prefix, the other two are the barycentric pair (u, v), folded at u + v > 1; no square root is taken.  The point
    is ``a + u (b - a) + v (c - a)`` in fp64, rounded to fp32 once, and ``weights`` are ``((1 - u) - v, u, v)``.
    ``normals`` (M,3) fp32 gives the normalised weighted sum of the face's vertex normals, (0,0,0) where the sum has no
    direction; ``colors`` (M,3) uint8 the weighted sum rounded to nearest.

    The result is a bitwise-reproducible function of ``(vertices, faces, n, seed)``, and sample i does not depend on
    ``n``: ``mesh_sample(.., n)[:m]`` is ``mesh_sample(.., m)``.  It does depend on the order of the faces: a permuted
    mesh has another prefix, so the same draw lands in another face (the distribution is the same).  ``n`` = 0 is
    answered without a launch; ``n`` > 0 on a mesh without area is a ValueError.  Everything is validated here, before
    any launch; the one host synchronisation is the read of (total, status) between the prefix and the draws."""
    m, f, dev = _check_surface(vertices, faces)
    n = _integer(n, "n", 0)
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^31 - 1 samples, got n = {n}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    for name, t, dtype in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (m, 3) or t.dtype != dtype:
            raise ValueError(f"{name} must be a ({m},3) {dtype} tensor, one row per vertex")
        if t.device != dev:
            raise ValueError(f"{name} are on {t.device}, vertices on {dev}")
    out = MeshSamples(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int64, device=dev),
                      torch.empty((n, 3), dtype=torch.float32, device=dev),
                      torch.empty((n, 3), dtype=torch.float32, device=dev) if normals is not None else None,
                      torch.empty((n, 3), dtype=torch.uint8, device=dev) if colors is not None else None)
    if n == 0:                         # nothing to draw, nothing to launch
        return out
    if m == 0 or f == 0:               # no face, no area: known without a launch
        raise ValueError("the mesh has no area: nothing to draw samples from")
    if not vertices.is_cuda:
        raise RuntimeError("mesh_sample runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    v, fc = vertices.detach().contiguous(), faces.detach().contiguous()
    nor = normals.detach().contiguous() if normals is not None else None
    col = colors.detach().contiguous() if colors is not None else None
    ws_bytes = lib.mvsn_mesh_sample_workspace_bytes(f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_sample_prefix(_native.ptr(v), m, _native.ptr(fc), f, _native.ptr(head), _native.ptr(ws),
                                                  ws_bytes, st), "mvsn_mesh_sample_prefix")
        total, status = head.tolist()  # the one host synchronisation
        if status & MESH_SAMPLE_STATUS_NO_AREA or total <= 0:
            raise ValueError("the mesh has no area: nothing to draw samples from")
        _native.check(lib.mvsn_mesh_sample_draw(_native.ptr(v), m, _native.ptr(fc), f, _native.ptr(ws), ws_bytes, n, seed,
                                                _native.ptr(nor), _native.ptr(col), _native.ptr(out.points),
                                                _native.ptr(out.face), _native.ptr(out.weights), _native.ptr(out.normals),
                                                _native.ptr(out.colors), st), "mvsn_mesh_sample_draw")
    return out


def mesh_nearest(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, max_dist: float) -> MeshNearest:
    """For every row of ``points`` (N,3) fp32 the nearest face of the mesh ``vertices`` (M,3) fp32, ``faces`` (F,3) int64
    within ``max_dist``: the squared distance, the face's row, the closest point on it with its barycentric weights, and
    how many faces lie within ``max_dist``.  The mesh counterpart of ``fusion.cloud_nearest`` (DESIGN.md section 26,
    csrc/mvsn_mesh_nearest.hip), and the same contract: the result is exactly that of the brute force over every (point,
    face) pair in the stated arithmetic, ties to the lowest face row, bitwise reproducible, and independent of the order
    of the faces except that ``face`` follows the rows.

    The closest point x of a face is formed in fp64 (the plane's barycentric weights where all three are >= 0, else the
    nearest of the three sides; a collinear face degenerates to its sides, a face (v,v,v) to the point), rounded to fp32
    once and clamped to the face's box; the squared distance is ``cloud_nearest``'s fp32 ``(dx*dx + dy*dy) + dz*dz`` to
    it, within when ``<= float32(max_dist)**2``.  A face with an index outside [0, M) or a vertex that is not finite
    takes no part; a point that is not finite gets (+inf, -1, 0, 0, 0).  The faces go on a grid of cell size ``max_dist``
    anchored at (0,0,0), each into every cell of its box; a face of more than ``NEAREST_BOX_CELLS`` cells is tested by
    every point directly.  A finite vertex 2^20 cells or more from the origin raises ValueError, and so do more than
    2^31 - 1 (cell, face) pairs: ``max_dist`` is too small for the mesh.  N = 0, F = 0 or M = 0 gives the all-miss
    answer without a launch.  Everything is validated here, before any launch; the one host synchronisation is the read
    of (pairs, large faces, status) that sizes the workspace."""
    from .fusion import VOXEL_CELL_LIMIT, check_cloud, cloud_radius_scalars
    check_cloud("points", points)
    m, f, dev = _check_surface(vertices, faces)
    if points.device != dev:
        raise ValueError(f"points are on {points.device}, vertices on {dev}")
    h, inv, r2 = cloud_radius_scalars(max_dist)
    N = int(points.shape[0])
    out = MeshNearest(torch.empty((N,), dtype=torch.float32, device=dev), torch.empty((N,), dtype=torch.int64, device=dev),
                      torch.empty((N, 3), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.float32, device=dev),
                      torch.empty((N,), dtype=torch.int32, device=dev))

    def miss():
        out.dist2.fill_(float("inf")), out.face.fill_(-1), out.point.zero_(), out.weights.zero_(), out.within.zero_()
        return out
    if N == 0 or f == 0 or m == 0:     # nothing to find, nothing to launch
        return miss()
    if not points.is_cuda:
        raise RuntimeError("mesh_nearest runs on HIP devices only: make the points and the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    q, v, fc = points.detach().contiguous(), vertices.detach().contiguous(), faces.detach().contiguous()
    head = torch.empty(3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_nearest_count(_native.ptr(v), m, _native.ptr(fc), f, float(inv), _native.ptr(head), st),
                      "mvsn_mesh_nearest_count")
        pairs, large, status = head.tolist()   # the one host synchronisation: sizes the workspace
        if status & MESH_NEAREST_STATUS_RANGE:
            raise ValueError(f"max_dist too small for the mesh's extent: a vertex lies 2^20 = {VOXEL_CELL_LIMIT} "
                             f"cells of {float(h):g} or more from the origin")
        if pairs > MAX_ROWS:
            raise ValueError(f"max_dist ({float(h):g}) too small for the mesh's faces: {pairs} (cell, face) pairs, "
                             "at most 2^31 - 1")
        if pairs == 0 and large == 0:  # no face takes part
            return miss()
        ws_bytes = lib.mvsn_mesh_nearest_workspace_bytes(pairs, large)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _native.check(lib.mvsn_mesh_nearest_build(_native.ptr(v), m, _native.ptr(fc), f, float(inv), pairs, large,
                                                  _native.ptr(ws), ws_bytes, st), "mvsn_mesh_nearest_build")
        _native.check(lib.mvsn_mesh_nearest(_native.ptr(q), N, _native.ptr(v), m, _native.ptr(fc), f, float(inv), float(r2),
                                            pairs, large, _native.ptr(ws), ws_bytes, _native.ptr(out.dist2),
                                            _native.ptr(out.face), _native.ptr(out.point), _native.ptr(out.weights),
                                            _native.ptr(out.within), st), "mvsn_mesh_nearest")
    return out


# ---- a mesh rendered into posed cameras --------------------------------------------------------
RENDER_MAX_EXTENT = 2 ** 15          # rows and columns of a rendered map


class MeshRender(NamedTuple):
    depth: torch.Tensor              # (V,1,H,W) fp32: z-depth of the nearest face per pixel, 0 where no face hit
    face: torch.Tensor               # (V,H,W) int64: that face's row, -1 where none
    weights: torch.Tensor            # (V,3,H,W) fp32: perspective-correct barycentric weights in the face's vertex order
    normals: Optional[torch.Tensor]  # (V,3,H,W) fp32: the interpolated vertex normal (zeros where none), or None
    colors: Optional[torch.Tensor]   # (V,3,H,W) uint8: the interpolated vertex colour (zeros where none), or None
    clipped: torch.Tensor            # (V,) int64: faces in front of the camera that the view left out


def mesh_render(vertices: torch.Tensor, faces: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, size, *,
                normals: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None, min_depth: float = 0.0,
                max_depth: float = float("inf")) -> MeshRender:
    """Render the mesh ``vertices`` (M,3) fp32, ``faces`` (F,3) int64 into the V cameras ``K``, ``T_cam_in_world``
    (V,4,4) with maps of ``size`` = (H,W): per pixel the z-depth of the nearest face whose projection holds the pixel
    centre, that face's row and the perspective-correct barycentric weights of the centre in it, and with ``normals``
    (M,3) fp32 and ``colors`` (M,3) uint8 the interpolated vertex normal and colour; DESIGN.md section 27,
    csrc/mvsn_mesh_render.hip.  What turns a mesh -- one that went through ``filter_mesh``, was read back from a file,
    or is somebody's ground truth -- into depth maps for ``metrics.depth_metric_rows``, and into a hole-free occluder
    for ``fusion.cloud_visibility`` and ``fusion.cloud_colorize``.

    The camera and the projection are ``fusion.cloud_render``'s, step for step, and pixel centres are the integers.  A
    face takes part in a view when its rows lie in [0, M), its coordinates are finite, every vertex has a finite z >
    ``min_depth`` and projects within 2^16 pixels of the origin.  There is no near-plane clipping: a face that crosses
    the near plane or leaves that guard band is missing from the picture, and ``clipped[v]`` counts the faces view v
    lost that way (a face wholly behind the camera is not counted).  The projected vertices are snapped to 1/256 of a
    pixel and coverage is exact integer work on the snapped triangle: both sides of a face are rendered, a face without
    area covers nothing, and of two faces that share an edge exactly one owns a pixel centre on it, so a watertight
    mesh is rendered without gaps and without double hits.  The depth at a covered pixel is 1 / sum(lambda_k / z_k) in
    fp64, rounded once; the pixel takes the face when ``min_depth`` < z <= ``max_depth``; the nearest face wins, a tie
    on z goes to the lowest row.  ``weights`` are (lambda_k / z_k) z, and the gathers are ``mesh_sample``'s
    interpolation with them: the normal is the normalised weighted sum, (0,0,0) where it has no direction, the colour
    the weighted sum rounded to nearest.  Where no face lands the depth is 0, the face -1, everything else zero.

    Every output is a bitwise-reproducible function of the inputs: the only atomics are an integer minimum and an
    integer sum.  ``depth`` does not depend on the order of the faces.  F = 0 or M = 0 gives the all-miss render
    without a launch.  Everything is validated here, before any launch; no host synchronisation."""
    from .fusion import _check_render_cameras, _depth_limit_f32, _integer_in
    m, f, dev = _check_surface(vertices, faces)
    V = _check_render_cameras(K, T_cam_in_world, dev, "vertices")
    try:
        H, W = (_integer_in(x, "size", 1, RENDER_MAX_EXTENT) for x in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be two integers (H,W), each in [1, 2^15], got {size!r}") from None
    for name, t, dtype in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (m, 3) or t.dtype != dtype:
            raise ValueError(f"{name} must be a ({m},3) {dtype} tensor, one row per vertex")
        if t.device != dev:
            raise ValueError(f"{name} are on {t.device}, vertices on {dev}")
    lo = _depth_limit_f32(min_depth, "min_depth")
    hi = _depth_limit_f32(max_depth, "max_depth", infinite=True, positive=True)
    launch = f > 0 and m > 0
    make = torch.empty if launch else torch.zeros
    out = MeshRender(make((V, 1, H, W), dtype=torch.float32, device=dev), make((V, H, W), dtype=torch.int64, device=dev),
                     make((V, 3, H, W), dtype=torch.float32, device=dev),
                     make((V, 3, H, W), dtype=torch.float32, device=dev) if normals is not None else None,
                     make((V, 3, H, W), dtype=torch.uint8, device=dev) if colors is not None else None,
                     make((V,), dtype=torch.int64, device=dev))
    if not launch:                     # no face: every pixel is a miss, nothing to launch
        out.face.fill_(-1)
        return out
    if not vertices.is_cuda:
        raise RuntimeError("mesh_render runs on HIP devices only: move the mesh and the cameras to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
    dense = lambda t: t.detach().contiguous() if t is not None else None   # noqa: E731
    # (every converted copy is held until the launches are enqueued: a temporary's memory could be handed out again)
    v_c, f_c, nor_c, col_c, K_c, T_c = dense(vertices), dense(faces), dense(normals), dense(colors), f32(K), f32(T_cam_in_world)
    ws_bytes = lib.mvsn_mesh_render_workspace_bytes(V, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_mesh_render(
            _native.ptr(v_c), m, _native.ptr(f_c), f, _native.ptr(nor_c), _native.ptr(col_c), _native.ptr(K_c),
            _native.ptr(T_c), V, H, W, float(lo), float(hi), _native.ptr(ws), ws_bytes, _native.ptr(out.depth),
            _native.ptr(out.face), _native.ptr(out.weights), _native.ptr(out.normals), _native.ptr(out.colors),
            _native.ptr(out.clipped), _native.stream()), "mvsn_mesh_render")
    return out


# ---- a smaller mesh: vertex clustering with quadric placement ----------------------------------
SIMPLIFY_PLACEMENTS = {"mean": 0, "quadric": 1}
SIMPLIFY_LAMBDA = 2.0 ** -10         # the quadric's pull towards the mean, per incidence
MESH_SIMPLIFY_STATUS_TABLE = 1


class SimplifiedMesh(NamedTuple):
    vertices: torch.Tensor            # (M',3) fp32
    faces: torch.Tensor               # (F',3) int64, rows of `vertices`, winding of the input face kept
    normals: Optional[torch.Tensor]   # (M',3) fp32 or None
    colors: Optional[torch.Tensor]    # (M',3) uint8 or None
    count: torch.Tensor               # (M',) int32: input vertices merged into this one
    first: torch.Tensor               # (M',) int64: lowest input vertex row of the cluster, strictly ascending
    inverse: torch.Tensor             # (M,) int64: output row of every input vertex, -1 = none
    face_rows: torch.Tensor           # (F',) int64: input row of every output face, strictly ascending


def mesh_simplify(vertices: torch.Tensor, faces: torch.Tensor, voxel_size: float, *, origin=(0.0, 0.0, 0.0),
                  placement: str = "quadric", normals: Optional[torch.Tensor] = None,
                  colors: Optional[torch.Tensor] = None, drop_unreferenced: bool = True) -> SimplifiedMesh:
    """The mesh ``vertices`` (M,3) fp32, ``faces`` (F,3) int64 simplified by vertex clustering on the grid
    (``voxel_size``, ``origin``): the decimation step between ``filter_mesh`` and ``mesh_sample`` / ``mesh_render`` /
    ``write_ply`` (csrc/mvsn_mesh_simplify.hip).

    Two vertices become one output vertex exactly when ``fusion.voxel_merge`` puts them into one voxel: the cells are
    its cells, step for step.  A vertex with a non-finite coordinate is dropped (``inverse`` -1); a finite vertex 2^20
    cells or more from the origin raises ValueError.  Output vertices are ordered by ``first``, the lowest input row of
    their cluster.  A face is remapped through the clustering and dropped when a corner lies outside [0, M), a corner
    is a dropped vertex, or two of its remapped corners are equal.  Of the survivors, faces whose remapped triples are
    equal up to rotation are one face, and the one with the lowest input row stays; the opposite winding of the same
    three rows is a different face and is kept (a two-sided sheet stays two-sided).  Output faces keep the input order
    and their own corner order, renumbered to output rows; ``face_rows`` names their input rows.  With
    ``drop_unreferenced`` a cluster no surviving face uses is not output and its members' ``inverse`` is -1; without it
    every cluster is output and, for ``placement="mean"``, ``vertices``, ``colors``, ``count``, ``first`` and
    ``inverse`` are ``voxel_merge``'s bit for bit (wherever its mean lies in its own cell, below).

    ``placement="mean"`` puts the vertex at ``voxel_merge``'s mean.  ``placement="quadric"`` puts it at the point that
    minimises the summed squared distance to the planes of the input faces around the cluster's members, in cell-local
    voxel units: per (face, corner) incidence the unit normal n (fp64) and d = -n.u give n n^T, d n and 1, each
    quantised to 2^-30 and summed as integers; ``(A + lambda k I) x = -b + lambda k u_mean`` with lambda = 2^-10 is
    solved in fp64 by the closed-form inverse, x is clamped to the cell and rounded to fp32 once.  A face without area,
    with a non-finite corner or a corner out of range adds nothing; a cluster without incidences sits at its mean.
    Whatever the placement, the output vertex lies in its cluster's cell by the grid's own fp32 arithmetic: where the
    rounded position does not, the cluster's ``first`` member's position is taken instead.  So every vertex moves by
    less than the cell's diagonal, and simplifying the result again on the same grid changes neither M' nor F'.

    ``normals`` (M,3) fp32 give per output vertex the direction of ``voxel_normals``' integer sum over the members,
    (0,0,0) where it is zero; ``colors`` (M,3) uint8 give ``voxel_merge``'s integer mean.  Clustering can create
    non-manifold edges; ``mesh_components`` and ``filter_mesh`` take the result as any mesh.

    Every output is a bitwise-reproducible function of the inputs, and the vertex outputs do not depend on the order of
    the faces.  M = 0, or F = 0 with ``drop_unreferenced``, gives empties without a launch.  Everything is validated
    here, before any launch; there are two host reads, (clusters, status) and (M', F', status), to size the outputs."""
    from .fusion import VOXEL_CELL_LIMIT, VOXEL_STATUS_RANGE, _origin_f32, _positive_f32
    m, f, dev = _check_surface(vertices, faces)
    if not isinstance(placement, str) or placement not in SIMPLIFY_PLACEMENTS:
        raise ValueError(f"placement must be 'mean' or 'quadric', got {placement!r}")
    for name, t, dtype in (("normals", normals, torch.float32), ("colors", colors, torch.uint8)):
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (m, 3) or t.dtype != dtype:
            raise ValueError(f"{name} must be a ({m},3) {dtype} tensor, one row per vertex")
        if t.device != dev:
            raise ValueError(f"{name} are on {t.device}, vertices on {dev}")
    v, inv, _ = _positive_f32(voxel_size, "voxel_size", inverse=True)
    o = _origin_f32(origin)
    drop = bool(drop_unreferenced)

    def result(mo, fo):
        return SimplifiedMesh(torch.empty((mo, 3), dtype=torch.float32, device=dev),
                              torch.empty((fo, 3), dtype=torch.int64, device=dev),
                              torch.empty((mo, 3), dtype=torch.float32, device=dev) if normals is not None else None,
                              torch.empty((mo, 3), dtype=torch.uint8, device=dev) if colors is not None else None,
                              torch.empty((mo,), dtype=torch.int32, device=dev),
                              torch.empty((mo,), dtype=torch.int64, device=dev),
                              torch.empty((m,), dtype=torch.int64, device=dev),
                              torch.empty((fo,), dtype=torch.int64, device=dev))

    def nothing():
        out = result(0, 0)
        out.inverse.fill_(-1)
        return out
    if m == 0 or (f == 0 and drop):    # no vertex, or no face to keep one: nothing to launch
        return nothing()
    if not vertices.is_cuda:
        raise RuntimeError("mesh_simplify runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    dense = lambda t: t.detach().contiguous() if t is not None else None   # noqa: E731
    v_c, f_c, nor_c, col_c = dense(vertices), dense(faces), dense(normals), dense(colors)
    scalars = (float(v), float(inv), float(o[0]), float(o[1]), float(o[2]))
    ws_bytes = lib.mvsn_mesh_simplify_workspace_bytes(m, f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_simplify_assign(_native.ptr(v_c), m, *scalars, _native.ptr(head), _native.ptr(ws),
                                                    ws_bytes, st), "mvsn_mesh_simplify_assign")
        clusters, status = head[:2].tolist()   # the first host read: the clusters, with the status word
        if status & VOXEL_STATUS_RANGE:
            raise ValueError(f"voxel_size too small for the mesh's extent: a vertex lies 2^20 = {VOXEL_CELL_LIMIT} "
                             f"cells of {float(v):g} or more from the origin {tuple(float(x) for x in o)}")
        if status:
            raise RuntimeError(f"mesh_simplify: the hash grid overflowed (status {status})")
        if clusters == 0:              # every vertex dropped
            return nothing()
        _native.check(lib.mvsn_mesh_simplify_mark(
            _native.ptr(v_c), _native.ptr(nor_c), _native.ptr(col_c), m, _native.ptr(f_c) if f else None, f, *scalars,
            SIMPLIFY_PLACEMENTS[placement], int(drop), clusters, _native.ptr(head), _native.ptr(ws), ws_bytes, st),
            "mvsn_mesh_simplify_mark")
        mo, fo, status, _ = head.tolist()      # the second host read: sizes the outputs
        if status:
            raise RuntimeError(f"mesh_simplify: the face set overflowed (status {status})")
        out = result(mo, fo)
        _native.check(lib.mvsn_mesh_simplify_emit(
            _native.ptr(f_c) if f else None, m, f, clusters, _native.ptr(ws), ws_bytes, mo, fo,
            _native.ptr(out.vertices) if mo else None, _native.ptr(out.faces) if fo else None,
            _native.ptr(out.normals) if mo else None, _native.ptr(out.colors) if mo else None,
            _native.ptr(out.count) if mo else None, _native.ptr(out.first) if mo else None, _native.ptr(out.inverse),
            _native.ptr(out.face_rows) if fo else None, st), "mvsn_mesh_simplify_emit")
    return out


MAX_EDGE_FACES = (2 ** 31 - 1) // 3   # a side index 3 r + s is an int32 on the device
MESH_EDGES_STATUS_TABLE = 1
SMOOTH_METHODS = {"laplacian": 0, "taubin": 1}
SMOOTH_MAX_ITERATIONS = 10000


class MeshEdges(NamedTuple):
    edges: torch.Tensor               # (E,2) int64: the distinct unordered pairs, (low, high), in order of `first`
    first: torch.Tensor               # (E,) int64: the lowest side index 3 r + s that carries the edge, ascending
    face_count: torch.Tensor          # (E,) int32: sides that carry it: 1 border, 2 manifold interior, > 2 non-manifold
    winding: torch.Tensor             # (E,) int32: sides low -> high minus sides high -> low
    face_edge: torch.Tensor           # (F,3) int64: the edge row of every side, -1 for a side that takes no part
    vertex_degree: torch.Tensor       # (M,) int32: distinct edges at the vertex
    vertex_boundary: torch.Tensor     # (M,) bool: the vertex lies on an edge with face_count 1


class SmoothedMesh(NamedTuple):
    vertices: torch.Tensor            # (M,3) fp32
    edges: MeshEdges                  # of the mesh (the faces are the input's)


class MeshNormals(NamedTuple):
    face_normals: torch.Tensor        # (F,3) fp32 unit normals by the winding, zeros for a face without one
    face_area: torch.Tensor           # (F,) fp32
    vertex_normals: torch.Tensor      # (M,3) fp32 area-weighted unit normals, zeros for a vertex without one


def mesh_edges(faces: torch.Tensor, num_vertices: int) -> MeshEdges:
    """The unique edges of the mesh ``faces`` (F,3) int64 over ``num_vertices`` = M vertex rows (DESIGN.md section 29,
    csrc/mvsn_mesh_edges.hip): what a watertightness check, hole statistics or smoothing with a held border start from.

    Side s of face r = (v0, v1, v2) runs from v_s to v_(s+1)%3 and has the side index 3 r + s.  A face with any index
    outside [0, M) takes no part; a side with equal ends takes no part while the other sides of its face still do.  An
    edge is the unordered pair of a side's ends: ``edges`` holds the distinct ones as (low, high), ordered by ``first``,
    the lowest side index that carries the edge.  ``face_count`` is the number of sides that carry it (1: a border, 2: a
    manifold interior edge, more: non-manifold; the same face twice counts twice), ``winding`` the sides running
    low -> high minus those running high -> low (0 on a consistently wound interior edge), ``face_edge`` the edge row of
    every side (-1 for a side that takes no part), ``vertex_degree`` the number of distinct edges at a vertex and
    ``vertex_boundary`` whether it lies on an edge with ``face_count`` 1.

    Every output is a bitwise-reproducible function of ``faces``.  F = 0 or M = 0 gives E = 0 without a launch.  At most
    (2^31 - 1) / 3 faces.  The one host synchronisation is the read of (E, status) that sizes the outputs."""
    m, f = _check_faces(faces, num_vertices)
    if f > MAX_EDGE_FACES:
        raise ValueError(f"at most (2^31 - 1) / 3 = {MAX_EDGE_FACES} faces, got {f}")
    dev = faces.device

    def result(e):
        return MeshEdges(torch.empty((e, 2), dtype=torch.int64, device=dev), torch.empty((e,), dtype=torch.int64, device=dev),
                         torch.empty((e,), dtype=torch.int32, device=dev), torch.empty((e,), dtype=torch.int32, device=dev),
                         torch.empty((f, 3), dtype=torch.int64, device=dev), torch.empty((m,), dtype=torch.int32, device=dev),
                         torch.empty((m,), dtype=torch.bool, device=dev))
    if f == 0 or m == 0:               # no side takes part: nothing to launch
        out = result(0)
        out.face_edge.fill_(-1)
        out.vertex_degree.zero_()
        out.vertex_boundary.zero_()
        return out
    if not faces.is_cuda:
        raise RuntimeError("mesh_edges runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    fc = faces.detach().contiguous()
    ws_bytes = lib.mvsn_mesh_edges_workspace_bytes(m, f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_mesh_edges_mark(_native.ptr(fc), m, f, _native.ptr(head), _native.ptr(ws), ws_bytes, st),
                      "mvsn_mesh_edges_mark")
        e, status = head.tolist()      # the one host synchronisation: sizes the outputs
        if status != 0 or not 0 <= e <= 3 * f:
            raise RuntimeError(f"mesh_edges: the edge set overflowed (status {status}, {e} edges of {f} faces)")
        out = result(e)
        _native.check(lib.mvsn_mesh_edges_emit(
            m, f, _native.ptr(ws), ws_bytes, e, _native.ptr(out.edges) if e else None, _native.ptr(out.first) if e else None,
            _native.ptr(out.face_count) if e else None, _native.ptr(out.winding) if e else None, _native.ptr(out.face_edge),
            _native.ptr(out.vertex_degree), _native.ptr(out.vertex_boundary), st), "mvsn_mesh_edges_emit")
    return out


def _check_edges(edges, m, f, dev):
    if not isinstance(edges, tuple) or len(edges) != 7:
        raise ValueError("edges must be a MeshEdges")
    e = int(edges[0].shape[0]) if torch.is_tensor(edges[0]) and edges[0].dim() == 2 else -1
    for name, t, shape, dtype in zip(MeshEdges._fields, edges, ((e, 2), (e,), (e,), (e,), (f, 3), (m,), (m,)),
                                     (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32,
                                      torch.bool)):
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError(f"edges.{name} must be a {tuple(max(s, 0) for s in shape)} {dtype} tensor of this mesh")
        if t.device != dev:
            raise ValueError(f"edges.{name} is on {t.device}, the mesh on {dev}")
    return e


def _real(value, name, ok, rule):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not ok(float(value)):
        raise ValueError(f"{name} must be a number with {rule}, got {value!r}")
    return float(value)


def mesh_smooth(vertices: torch.Tensor, faces: torch.Tensor, iterations: int = 10, *, method: str = "taubin",
                lam: float = 0.5, mu: float = -0.53, fix_boundary: bool = False, pinned: Optional[torch.Tensor] = None,
                edges: Optional[MeshEdges] = None) -> SmoothedMesh:
    """The mesh ``vertices`` (M,3) fp32, ``faces`` (F,3) int64 smoothed with the uniform (umbrella) Laplacian over its
    unique edges: the step between ``filter_mesh`` and ``mesh_simplify`` that takes the voxel-pitch bumps of depth noise
    out of an extracted mesh (csrc/mvsn_mesh_smooth.hip).  The faces do not change.

    ``method="laplacian"`` takes ``iterations`` steps x <- x + lam L(x), L(x)_i the mean of x_j - x_i over the edges at
    i; ``method="taubin"`` takes ``iterations`` pairs of steps, with ``lam`` and then with ``mu`` (Taubin's lambda|mu
    filter: the second, negative step undoes the shrinkage of the first).  0 < lam <= 1, -2 <= mu < 0,
    0 <= iterations <= 10000.  ``edges`` takes the ``MeshEdges`` of this mesh to reuse; without it ``mesh_edges`` is
    called.  A vertex with a non-finite coordinate keeps its bits and its edges contribute to neither end; with
    ``fix_boundary`` every ``vertex_boundary`` vertex keeps its bits, and ``pinned`` (M,) bool adds the caller's own.  The
    degree that the mean divides by is the number of the vertex's edges that contribute; a vertex without one stays.

    The working positions are fp64.  With span, the largest per-axis extent of the finite vertices, written m 2^k with
    m in [0.5, 1), every edge (a, b) adds q = rint((x_b - x_a) 2^(30-k)), clamped to +-2^31, to a's integer sum and -q
    to b's; a vertex moves by f ((double)sum 2^(k-30)) / (double)degree; at the end the positions are rounded to fp32
    once.  The sums are integers, so the result is a bitwise-reproducible function of the inputs that does not depend on
    the order of the faces or of a face's corners.  Without a finite vertex, or with span 0, the result is the input's
    bits.  The steps are launched back to back: ``mesh_smooth`` itself reads nothing back (``mesh_edges`` reads once).
    M = 0, E = 0 or ``iterations`` = 0 gives a copy of the vertices without a launch of its own."""
    m, f, dev = _check_surface(vertices, faces)
    if not isinstance(method, str) or method not in SMOOTH_METHODS:
        raise ValueError(f"method must be 'laplacian' or 'taubin', got {method!r}")
    lam = _real(lam, "lam", lambda x: 0.0 < x <= 1.0, "0 < lam <= 1")
    mu = _real(mu, "mu", lambda x: -2.0 <= x < 0.0, "-2 <= mu < 0")
    iterations = _integer(iterations, "iterations", 0, SMOOTH_MAX_ITERATIONS)
    if not isinstance(fix_boundary, bool):
        raise ValueError(f"fix_boundary must be a bool, got {fix_boundary!r}")
    if pinned is not None:
        if not torch.is_tensor(pinned) or tuple(pinned.shape) != (m,) or pinned.dtype != torch.bool:
            raise ValueError(f"pinned must be a ({m},) bool tensor, one flag per vertex")
        if pinned.device != dev:
            raise ValueError(f"pinned is on {pinned.device}, vertices on {dev}")
    if edges is not None:
        _check_edges(edges, m, f, dev)
    else:
        edges = mesh_edges(faces, m)
    e = int(edges.edges.shape[0])
    if m == 0 or e == 0 or iterations == 0:    # nothing moves: nothing to launch
        return SmoothedMesh(vertices.detach().clone(memory_format=torch.contiguous_format), edges)
    if not vertices.is_cuda:
        raise RuntimeError("mesh_smooth runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    held = pinned.detach() if pinned is not None else None
    if fix_boundary:
        held = edges.vertex_boundary if held is None else held | edges.vertex_boundary
    held = held.contiguous() if held is not None else None
    v_c, e_c = vertices.detach().contiguous(), edges.edges.detach().contiguous()
    out = torch.empty((m, 3), dtype=torch.float32, device=dev)
    ws_bytes = lib.mvsn_mesh_smooth_workspace_bytes(m)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_mesh_smooth(_native.ptr(v_c), m, _native.ptr(e_c), e, _native.ptr(held),
                                           SMOOTH_METHODS[method], iterations, lam, mu, _native.ptr(ws), ws_bytes,
                                           _native.ptr(out), _native.stream()), "mvsn_mesh_smooth")
    return SmoothedMesh(out, edges)


def mesh_normals(vertices: torch.Tensor, faces: torch.Tensor) -> MeshNormals:
    """Face normals, face areas and area-weighted vertex normals of the mesh ``vertices`` (M,3) fp32, ``faces`` (F,3)
    int64: the normals that ``write_ply``, ``mesh_sample`` and ``mesh_render`` take, for a mesh whose own have gone stale
    (after ``mesh_smooth`` or ``mesh_simplify``) or that never had any (csrc/mvsn_mesh_smooth.hip).

    Per face c = (p1 - p0) x (p2 - p0) in fp64 from the fp32 vertices, with the lowest row rotated to the front so that
    the bits do not depend on the corner the face starts with: ``face_normals`` = c / |c|, by the winding, and
    ``face_area`` = |c| / 2, both zeros for a face with an index outside [0, M), a non-finite corner or no area.
    ``vertex_normals`` is the direction of the sum of c over the valid faces at the vertex, summed as exact integers (c
    quantised to 2^-31 of the largest component at that vertex), rounded to fp32 once; (0,0,0) where the sum is zero or
    no valid face uses the vertex.  Bitwise reproducible and independent of the order of the faces.  M = 0 gives zeros
    without a launch; there is no host read."""
    m, f, dev = _check_surface(vertices, faces)
    out = MeshNormals(torch.empty((f, 3), dtype=torch.float32, device=dev), torch.empty((f,), dtype=torch.float32, device=dev),
                      torch.empty((m, 3), dtype=torch.float32, device=dev))
    if m == 0:                         # no vertex, no valid face: nothing to launch
        out.face_normals.zero_()
        out.face_area.zero_()
        return out
    if not vertices.is_cuda:
        raise RuntimeError("mesh_normals runs on HIP devices only: make the mesh on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    v_c, f_c = vertices.detach().contiguous(), faces.detach().contiguous()
    ws_bytes = lib.mvsn_mesh_normals_workspace_bytes(m)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_mesh_normals(_native.ptr(v_c), m, _native.ptr(f_c) if f else None, f, _native.ptr(ws), ws_bytes,
                                            _native.ptr(out.face_normals) if f else None,
                                            _native.ptr(out.face_area) if f else None, _native.ptr(out.vertex_normals),
                                            _native.stream()), "mvsn_mesh_normals")
    return out
