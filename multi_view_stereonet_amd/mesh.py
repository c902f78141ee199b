"""Connected components of a triangle mesh on the device, and the mesh without its small ones (DESIGN.md section 18
states the semantics and the termination and visibility argument of the union-find; the kernels are
csrc/mvsn_mesh.hip).

What ``tsdf.extract_mesh`` gives is raw: every speck of the volume that two noisy views agreed on is a small closed
blob, every depth edge grows a detached sliver.  ``mesh_components`` labels the mesh, ``filter_mesh`` keeps the
components one asks for and renumbers the faces, and ``fusion.write_ply(..., faces=)`` saves the result.

The graph has the vertex rows as nodes and the sides of the faces as edges: two faces that share one vertex are
connected, two vertices at one position in different rows are not.  Everything is integer work and a pure function of
the mesh: the outputs do not depend on the order of the faces, on the order of a face's indices, or on any race.
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
