"""A dense TSDF volume on the device: posed depth maps integrated along their viewing rays, a triangle mesh taken
from the volume by Surface Nets (DESIGN.md section 15 states the semantics, every fp32 step and the error bounds; the
kernels are csrc/mvsn_tsdf.hip), and depth, normal, colour and weight maps of its surface ray-cast from any pose (section
16, csrc/mvsn_tsdf_raycast.hip).

Where ``fusion.fuse_depthmaps`` keeps or drops pixels, the volume averages: every voxel holds the weighted sum of the
truncated signed distances the views saw at it, so a surface that k views saw is in the result once, free space is
carved, and the gaps between pixels are filled.  ``TSDFVolume.integrate`` adds views, ``extract_mesh`` gives vertices
with normals and colours and the triangles between them, ``fusion.write_ply(..., faces=)`` saves them, ``raycast``
renders the surface as a camera sees it, and ``align`` refines the poses of depth maps against it (section 17,
csrc/mvsn_tsdf_align.hip).  ``integrate_cloud`` is the other way into the volume: oriented points instead of posed depth
maps (section 31, csrc/mvsn_tsdf_cloud.hip), so a cloud that was merged, cleaned, registered or read from a file becomes
a surface too, and ``TSDFVolume.around`` makes the volume that holds a cloud.

Conventions are ``fusion``'s: ``K`` (V,4,4) with the top-left 3x3 used and a bottom row of (0,0,1); ``T_cam_in_world``
(V,4,4) maps camera coordinates to world coordinates; pixel (x, y) = (column, row) with integer values at pixel
centres.  The signed distance is projective (depth minus the voxel's camera z) and positive towards the camera.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native
from .fusion import (_check_frames, _check_views, _cloud_index_build, _origin_f32, _positive_f32,
                     _raise_cloud_status, check_cloud, cloud_radius_scalars)

MAX_VOXELS = 2 ** 31 - 1
MAX_EXTENT = 2 ** 24                 # voxels along an axis, rows and columns of a map: every index is an exact float32
MAX_RAY_SAMPLES = 2 ** 20            # samples of one ray inside the volume's box


class TSDFMesh(NamedTuple):
    vertices: torch.Tensor           # (M,3) fp32 world coordinates, one per active cell
    normals: torch.Tensor            # (M,3) fp32 unit vectors pointing outwards (towards the cameras), or (0,0,0)
    colors: Optional[torch.Tensor]   # (M,3) uint8, or None for a volume without colour
    faces: torch.Tensor              # (F,3) int64 rows of `vertices`, counter-clockwise seen from the outside
    cell: torch.Tensor               # (M,) int64: the cell's linear index (k * Ny + j) * Nx + i, ascending


class TSDFRender(NamedTuple):
    depth: torch.Tensor              # (V,1,H,W) fp32 z-depth of the hit in the rendering camera, 0 without a hit
    normals: torch.Tensor            # (V,3,H,W) fp32 unit vectors in the world frame, pointing outwards, or (0,0,0)
    colors: Optional[torch.Tensor]   # (V,3,H,W) fp32 in the range of `images`, or None for a volume without colour
    weight: torch.Tensor             # (V,1,H,W) fp32 interpolated weight at the hit, 0 without one


class TSDFAlignment(NamedTuple):
    T_cam_in_world: torch.Tensor     # (V,4,4) fp32, the refined poses (each number rounded once from the fp64 pose)
    history: torch.Tensor            # (V, iterations+1, 3) fp64: count, sum_w, sum_w_r2 at the pose BEFORE update i; the last row at the final pose
    status: torch.Tensor             # (V,) int32: 0 ran all iterations, 1 stopped: fewer than min_pixels take part, 2 stopped: normal matrix not positive definite
    information: torch.Tensor        # (V,6,6) fp64: the normal matrix at the final pose (its inverse is the pose covariance up to the noise scale)


class TSDFVolume:
    """``dims`` = (Nx,Ny,Nz) voxels of ``voxel_size`` whose first centre is ``origin``: the centre of voxel (i,j,k) is
    ``origin + voxel_size * (i,j,k)``.  The state is three planar fp32 tensors in the layout (Nz,Ny,Nx), x fastest:
    ``sdf_sum`` (sum of w t), ``weight`` (sum of w) and, with ``color=True``, ``color_sum`` (3,Nz,Ny,Nx) (sum of w rgb).
    The volume stores sums, not a running mean, so views integrated one call at a time give the bits of one call with
    all of them; the value of a voxel is ``sdf_sum / weight`` (``values()``).  ``trunc`` is the truncation distance."""

    def __init__(self, dims: Sequence[int], voxel_size: float, origin: Sequence[float], trunc: float, device="cuda",
                 color: bool = False):
        try:
            d = tuple(int(x) for x in dims)
            if len(d) != 3 or any(x != y or isinstance(y, bool) for x, y in zip(d, dims)):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"dims must be three integers (Nx,Ny,Nz), got {dims!r}") from None
        if min(d) < 1:
            raise ValueError(f"dims must be at least 1 each, got {d}")
        if max(d) > MAX_EXTENT:
            raise ValueError(f"dims must be at most 2^24 each, got {d}")
        if d[0] * d[1] * d[2] > MAX_VOXELS:
            raise ValueError(f"at most 2^31 - 1 voxels, got {d[0]} x {d[1]} x {d[2]} = {d[0] * d[1] * d[2]}")
        self.voxel_size = _positive_f32(voxel_size, "voxel_size")[0]
        self.trunc = _positive_f32(trunc, "trunc")[0]
        o = _origin_f32(origin)
        self.dims, self.origin, self.device = d, o, torch.device(device)
        nx, ny, nz = d
        self.sdf_sum = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color_sum = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self.device = self.sdf_sum.device          # (with its index: tensors are compared against it)

    def reset(self) -> None:
        """Zero the volume."""
        self.sdf_sum.zero_()
        self.weight.zero_()
        if self.color_sum is not None:
            self.color_sum.zero_()

    def values(self) -> torch.Tensor:
        """(Nz,Ny,Nx) fp32: ``sdf_sum / weight``, NaN where ``weight == 0``."""
        return torch.where(self.weight == 0, torch.full_like(self.sdf_sum, float("nan")), self.sdf_sum / self.weight)

    def integrate(self, depth: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, *,
                  images: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                  weights: Optional[torch.Tensor] = None, min_depth: float = 0.0) -> None:
        """Integrate ``depth`` (V,1,H,W) fp32, V <= 65535.  For every voxel centre p and every view in index order:
        Xc = T_cam_in_world^-1 p, skipped unless z = Xc.z > ``min_depth``; the pixel is the one nearest to the projection
        of Xc, skipped unless it lies in the map; D is the depth there, skipped unless it is finite and > 0, ``valid``
        (V,1,H,W) bool / uint8 is set and the weight w there (``weights`` (V,1,H,W) fp32; 1 without) is finite and > 0;
        sdf = D - z, skipped if sdf < -trunc; then ``sdf_sum += w * min(sdf, trunc)``, ``weight += w`` and, with
        ``images`` (V,3,H,W) fp32 (which needs ``color=True``, and the reverse), ``color_sum += w * rgb``.  A voxel no view
        updates keeps its bits.  ``K`` and ``T_cam_in_world`` may be of any floating-point dtype: the kernel reads their
        float32 values (and forms the inverses from those in fp64).  Everything is validated here, before the launch; no
        host synchronisation."""
        def limits(V, H, W, dev):
            if V > 65535 or H * W > 2 ** 31 - 1 or max(H, W) > MAX_EXTENT:
                raise ValueError(f"at most 65535 views of 2^31 - 1 pixels and 2^24 rows or columns, got {V} of {H} x {W}")
            if dev != self.device:
                raise ValueError(f"depth is on {dev}, the volume on {self.device}")
        V, H, W, dev = _check_views(depth, K, T_cam_in_world, limits=limits, floating=True)
        if (images is not None) != (self.color_sum is not None):
            raise ValueError("images need a volume made with color=True, and such a volume needs images")
        if images is not None:
            _check_frames("images", images, V, H, W, 3, (torch.float32,), dev)
        if valid is not None:
            _check_frames("valid", valid, V, H, W, 1, (torch.bool, torch.uint8), dev)
        if weights is not None:
            _check_frames("weights", weights, V, H, W, 1, (torch.float32,), dev)
        with np.errstate(all="ignore"):
            try:
                md = np.float32(min_depth)
            except (TypeError, ValueError):
                raise ValueError(f"min_depth must be a finite number, got {min_depth!r}") from None
        if not np.isfinite(md):
            raise ValueError(f"min_depth must be a finite number, got {min_depth!r}")

        if not depth.is_cuda:
            raise RuntimeError("TSDFVolume.integrate runs on HIP devices only: make the volume and the depth maps on "
                               "'cuda' (there is no CPU implementation)")
        lib = _native.load()
        f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
        valid_c = valid.detach().contiguous().view(torch.uint8) if valid is not None else None
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            _native.check(lib.mvsn_tsdf_integrate(
                _native.ptr(depth.detach().contiguous()), _native.ptr(valid_c),
                _native.ptr(weights.detach().contiguous() if weights is not None else None),
                _native.ptr(images.detach().contiguous() if images is not None else None), _native.ptr(f32(K)),
                _native.ptr(f32(T_cam_in_world)), V, H, W, nx, ny, nz, float(self.voxel_size), float(self.origin[0]),
                float(self.origin[1]), float(self.origin[2]), float(self.trunc), float(md), _native.ptr(self.sdf_sum),
                _native.ptr(self.weight), _native.ptr(self.color_sum), _native.stream()), "mvsn_tsdf_integrate")

    @classmethod
    def around(cls, points: torch.Tensor, voxel_size: float, trunc: float, *, padding: Optional[float] = None,
               color: bool = False) -> "TSDFVolume":
        """The smallest volume on the ``voxel_size`` lattice (voxel centres at integer multiples of ``voxel_size``) that
        holds the finite rows of ``points`` (N,3) fp32 plus ``padding`` (a finite number >= 0; None: ``trunc``) on every
        side, on the points' device.  The origin is rounded once to fp32.  One host read: the bounding box.  ValueError
        where no row is finite or the box exceeds the volume's limits (2^31 - 1 voxels, 2^24 along an axis)."""
        check_cloud("points", points)
        v = _positive_f32(voxel_size, "voxel_size")[0]
        tr = _positive_f32(trunc, "trunc")[0]
        with np.errstate(all="ignore"):
            try:
                pad = np.float32(tr if padding is None else padding)
            except (TypeError, ValueError):
                raise ValueError(f"padding must be a finite number >= 0, got {padding!r}") from None
        if not (np.isfinite(pad) and pad >= 0):
            raise ValueError(f"padding must be a finite number >= 0, got {padding!r}")
        box = None
        if int(points.shape[0]) > 0:
            p = points.detach()
            finite = torch.isfinite(p).all(dim=1, keepdim=True)
            lo = torch.where(finite, p, torch.full_like(p, float("inf"))).amin(dim=0)
            hi = torch.where(finite, p, torch.full_like(p, float("-inf"))).amax(dim=0)
            box = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()     # the one host read
        if box is None or not np.isfinite(box).all():
            raise ValueError("points hold no finite row: there is nothing to put a volume around")
        vs, pd = float(v), float(pad)
        first = np.floor((box[0] - pd) / vs)
        last = np.ceil((box[1] + pd) / vs)
        with np.errstate(all="ignore"):
            origin = (first * vs).astype(np.float32)
        if not np.isfinite(origin).all() or not (np.abs(first) < 2.0 ** 52).all() or not (np.abs(last) < 2.0 ** 52).all():
            raise ValueError(f"the box of the points, {box[0]} to {box[1]}, has no lattice of voxel_size {vs:g}")
        # (the rounding of the origin to fp32 may have moved it past the box: one more voxel on that side)
        first = first - (origin.astype(np.float64) > box[0] - pd)
        with np.errstate(all="ignore"):
            origin = (first * vs).astype(np.float32)
        dims = last - first + 1.0
        dims = dims + (origin.astype(np.float64) + (dims - 1.0) * vs < box[1] + pd)
        if (dims > MAX_EXTENT).any() or float(dims[0]) * float(dims[1]) * float(dims[2]) > MAX_VOXELS:
            raise ValueError(f"the box of the points plus padding needs {int(dims[0])} x {int(dims[1])} x {int(dims[2])} "
                             f"voxels of {vs:g}: at most 2^31 - 1 voxels and 2^24 along an axis")
        return cls(tuple(int(d) for d in dims), v, origin, tr, device=points.device, color=color)

    def integrate_cloud(self, points: torch.Tensor, normals: torch.Tensor, radius: float, *,
                        weights: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None) -> None:
        """Add the oriented cloud ``points`` (N,3) fp32 with ``normals`` (N,3) fp32 to the volume: the implicit
        moving-least-squares distance (Hoppe's weighted tangent planes), so a cloud that ``voxel_merge`` merged, a filter
        cleaned, ``cloud_register`` moved or ``read_ply`` read becomes a surface that ``extract_mesh``, ``raycast`` and
        ``align`` work on.  ``integrate_cloud`` (module level) states every step; DESIGN.md section 31 has the rest.
        The call adds to whatever the volume holds: depth maps and clouds can go into one volume."""
        integrate_cloud(self.sdf_sum, self.weight, self.color_sum, self.voxel_size, self.origin, self.trunc, points,
                        normals, radius, weights=weights, colors=colors)

    def extract_mesh(self, min_weight: float = 1.0) -> TSDFMesh:
        """The surface of the volume by Surface Nets, a pure function of the state tensors.  A voxel is observed when
        ``weight >= min_weight`` and inside when its value is < 0 (exactly 0 counts as outside); a cell of 2x2x2 voxels
        whose corners are all observed and not all of one sign gets one vertex, the mean of the zero crossings on its
        edges, with the normalised gradient of the values as its normal (pointing outwards, towards the cameras) and the
        interpolated colour; every grid edge with a sign change whose four cells all have a vertex gives a quad, split
        into two triangles.  Vertices come ordered by ``cell``, faces by (voxel, axis) of their edge; the outputs are
        bitwise reproducible.  A volume with a dimension < 2, or with no active cell, gives empties.  The one host
        synchronisation is the read of the two counts that size the outputs."""
        return extract_mesh(self.sdf_sum, self.weight, self.color_sum, self.voxel_size, self.origin, min_weight)

    def raycast(self, K: torch.Tensor, T_cam_in_world: torch.Tensor, size: Sequence[int], *, min_weight: float = 1.0,
                min_depth: float = 0.0, max_depth: Optional[float] = None, step: Optional[float] = None) -> TSDFRender:
        """The surface of the volume as cameras (``K``, ``T_cam_in_world``) (V,4,4) see it, in maps of ``size`` = (H, W):
        ``depth`` is the z-depth in the rendering camera (what ``integrate`` consumes), ``normals`` the unit gradient of
        the interpolated values in the world frame (outwards, as the mesh's), ``colors`` the interpolated
        ``color_sum / weight`` and ``weight`` the interpolated weight; a pixel without a hit holds zeros in all of them.
        The ray of a pixel is sampled at the depths k * ``step``, k = 1, 2, ..., inside (``min_depth``, ``max_depth``]
        (``step`` None: min(voxel_size, trunc / 4); ``max_depth`` None: no far limit); a sample is defined where the 8
        voxels around it have ``weight >= min_weight`` and its value is their trilinear interpolant; the hit is the
        first change from >= 0 to < 0 between two consecutive defined samples, placed by linear interpolation; a change
        from < 0 to >= 0 (a surface seen from behind) ends the ray.  Bitwise reproducible, a view's maps do not depend on
        the other views of the call, no host synchronisation.  DESIGN.md section 16 has every fp32 step."""
        if step is None:
            with np.errstate(all="ignore"):
                step = min(self.voxel_size, self.trunc / np.float32(4))
        return raycast(self.sdf_sum, self.weight, self.color_sum, self.voxel_size, self.origin, K, T_cam_in_world, size,
                       min_weight=min_weight, min_depth=min_depth, max_depth=max_depth, step=step)

    def align(self, depth: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, *,
              valid: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, min_weight: float = 1.0,
              band: Optional[float] = None, iterations: int = 10, stride: int = 1, min_pixels: int = 6,
              min_pivot: float = 1e-9) -> TSDFAlignment:
        """Refine the poses ``T_cam_in_world`` (V,4,4) of the depth maps ``depth`` (V,1,H,W) fp32 against the volume:
        Gauss-Newton on the point-to-TSDF residual, no data association and no render.  A pixel with depth D is the
        point ``ray * D`` of its view; it takes part when it lies on the ``stride`` lattice (x % stride == 0 and
        y % stride == 0), D is finite and > 0, ``valid`` is set, its weight w (``weights`` (V,1,H,W) fp32; 1 without) is
        finite and > 0, the 8 voxels around the point have ``weight >= min_weight`` (``raycast``'s "defined"), the
        trilinear value f there has |f| <= ``band`` and its gradient is finite.  The residual is r = f / voxel_size;
        every iteration solves the 6 x 6 normal equations of sum w r^2 for a rigid update about the volume's centre and
        applies it to the pose, which is carried in fp64.  A view stops, and keeps its pose, when fewer than
        ``min_pixels`` pixels take part (status 1) or when the normal matrix, scaled to a unit diagonal, has a Cholesky
        pivot below ``min_pivot`` (status 2: the scene does not constrain all six degrees of freedom); the remaining
        rows of its ``history`` repeat.  ``band`` None is ``trunc / 2``: a default, not a measured constant -- values at
        +-trunc are clamped and carry no gradient, so the band must stay inside the truncation.  ``iterations`` is an
        integer in [0, 1000]; with 0 the result holds the float32 values of the input poses and one history row.  Every
        view is aligned on its own; bitwise reproducible; everything is validated here, before any launch; no host
        synchronisation whatever ``iterations`` is.  DESIGN.md section 17 has every step."""
        if band is None:
            with np.errstate(all="ignore"):
                band = self.trunc / np.float32(2)
        return align(self.sdf_sum, self.weight, self.voxel_size, self.origin, depth, K, T_cam_in_world, band=band,
                     valid=valid, weights=weights, min_weight=min_weight, iterations=iterations, stride=stride,
                     min_pixels=min_pixels, min_pivot=min_pivot)


def _check_state(sdf_sum, weight, color_sum):
    """ValueError unless the three are state tensors of one volume on one device; returns (nx, ny, nz, device)."""
    if not torch.is_tensor(sdf_sum) or sdf_sum.dim() != 3 or sdf_sum.dtype != torch.float32:
        raise ValueError("sdf_sum must be a (Nz,Ny,Nx) float32 tensor")
    nz, ny, nx = (int(x) for x in sdf_sum.shape)
    dev = sdf_sum.device
    if not torch.is_tensor(weight) or tuple(weight.shape) != (nz, ny, nx) or weight.dtype != torch.float32:
        raise ValueError(f"weight must be a ({nz},{ny},{nx}) float32 tensor like sdf_sum")
    if weight.device != dev:
        raise ValueError(f"weight is on {weight.device}, sdf_sum on {dev}")
    if color_sum is not None:
        if not torch.is_tensor(color_sum) or tuple(color_sum.shape) != (3, nz, ny, nx) or color_sum.dtype != torch.float32:
            raise ValueError(f"color_sum must be a (3,{nz},{ny},{nx}) float32 tensor")
        if color_sum.device != dev:
            raise ValueError(f"color_sum is on {color_sum.device}, sdf_sum on {dev}")
    if nx * ny * nz > MAX_VOXELS or max(nx, ny, nz) > MAX_EXTENT:
        raise ValueError(f"at most 2^31 - 1 voxels and 2^24 along an axis, got {nx} x {ny} x {nz}")
    return nx, ny, nz, dev


def extract_mesh(sdf_sum: torch.Tensor, weight: torch.Tensor, color_sum: Optional[torch.Tensor], voxel_size: float,
                 origin: Sequence[float], min_weight: float = 1.0) -> TSDFMesh:
    """``TSDFVolume.extract_mesh`` on state tensors of any origin: ``sdf_sum`` and ``weight`` (Nz,Ny,Nx) fp32,
    ``color_sum`` (3,Nz,Ny,Nx) fp32 or None."""
    nx, ny, nz, dev = _check_state(sdf_sum, weight, color_sum)
    v = _positive_f32(voxel_size, "voxel_size")[0]
    mw = _positive_f32(min_weight, "min_weight")[0]
    o = _origin_f32(origin)

    def mesh(m, f):
        return TSDFMesh(torch.empty((m, 3), dtype=torch.float32, device=dev),
                        torch.empty((m, 3), dtype=torch.float32, device=dev),
                        torch.empty((m, 3), dtype=torch.uint8, device=dev) if color_sum is not None else None,
                        torch.empty((f, 3), dtype=torch.int64, device=dev),
                        torch.empty((m,), dtype=torch.int64, device=dev))
    if min(nx, ny, nz) < 2:            # no cell, nothing to launch: empties on the state's device
        return mesh(0, 0)
    if not sdf_sum.is_cuda:
        raise RuntimeError("extract_mesh runs on HIP devices only: make the volume on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    s, w = sdf_sum.detach().contiguous(), weight.detach().contiguous()
    c = color_sum.detach().contiguous() if color_sum is not None else None
    ws_bytes = lib.mvsn_tsdf_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_tsdf_classify(_native.ptr(s), _native.ptr(w), nx, ny, nz, float(mw), _native.ptr(head),
                                             _native.ptr(ws), ws_bytes, st), "mvsn_tsdf_classify")
        m, both = head.tolist()        # the one host synchronisation: sizes the outputs
        quads = both - m
        out = mesh(m, 2 * quads)
        if m == 0:                     # no active cell
            return out
        _native.check(lib.mvsn_tsdf_extract(_native.ptr(s), _native.ptr(w), _native.ptr(c), nx, ny, nz, float(v),
                                            float(o[0]), float(o[1]), float(o[2]), float(mw), _native.ptr(ws), ws_bytes,
                                            m, quads, _native.ptr(out.vertices), _native.ptr(out.normals),
                                            _native.ptr(out.colors), _native.ptr(out.faces), _native.ptr(out.cell), st),
                      "mvsn_tsdf_extract")
    return out


def raycast(sdf_sum: torch.Tensor, weight: torch.Tensor, color_sum: Optional[torch.Tensor], voxel_size: float,
            origin: Sequence[float], K: torch.Tensor, T_cam_in_world: torch.Tensor, size: Sequence[int], *,
            min_weight: float = 1.0, min_depth: float = 0.0, max_depth: Optional[float] = None,
            step: Optional[float] = None) -> TSDFRender:
    """``TSDFVolume.raycast`` on state tensors of any origin (``extract_mesh``'s).  ``step`` None: ``voxel_size``."""
    nx, ny, nz, dev = _check_state(sdf_sum, weight, color_sum)
    for name, m in (("K", K), ("T_cam_in_world", T_cam_in_world)):
        if not torch.is_tensor(m) or m.dim() != 3 or tuple(m.shape[1:]) != (4, 4) or m.shape[0] != K.shape[0]:
            raise ValueError(f"{name} must be a (V,4,4) tensor" + ("" if m is K else " like K"))
        if not m.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {m.dtype}")
        if m.device != dev:
            raise ValueError(f"{name} is on {m.device}, the volume on {dev}")
    V = int(K.shape[0])
    if V < 1:
        raise ValueError("K must hold at least one view")
    try:
        H, W = (int(x) for x in size)
        if any(x != y or isinstance(y, bool) for x, y in zip((H, W), size)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"size must be two integers (H, W), got {size!r}") from None
    if H < 1 or W < 1:
        raise ValueError(f"size must be at least 1 x 1, got {H} x {W}")
    if V > 65535 or H * W > 2 ** 31 - 1 or max(H, W) > MAX_EXTENT:
        raise ValueError(f"at most 65535 views of 2^31 - 1 pixels and 2^24 rows or columns, got {V} of {H} x {W}")
    v = _positive_f32(voxel_size, "voxel_size")[0]
    mw = _positive_f32(min_weight, "min_weight")[0]
    st = _positive_f32(v if step is None else step, "step")[0]
    o = _origin_f32(origin)
    with np.errstate(all="ignore"):
        try:
            lo = np.float32(min_depth)
            hi = np.float32(np.inf if max_depth is None else max_depth)
        except (TypeError, ValueError):
            raise ValueError(f"min_depth and max_depth must be numbers, got {min_depth!r} and {max_depth!r}") from None
    if not np.isfinite(lo):
        raise ValueError(f"min_depth must be a finite number, got {min_depth!r}")
    if (max_depth is not None and not np.isfinite(hi)) or not hi > lo:
        raise ValueError(f"max_depth must be a finite number above min_depth = {lo}, or None, got {max_depth!r}")
    # no ray holds more samples inside the box: its length in depth is at most its metric length, at most the diagonal
    samples = float(v) * float(np.sqrt(float((nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2))) / float(st) + 2.0
    if samples > MAX_RAY_SAMPLES:
        raise ValueError(f"a ray can hold {samples:.0f} samples inside the volume, at most 2^20: choose a larger step "
                         f"than {st}")

    def maps(make):
        return TSDFRender(make((V, 1, H, W), dtype=torch.float32, device=dev),
                          make((V, 3, H, W), dtype=torch.float32, device=dev),
                          make((V, 3, H, W), dtype=torch.float32, device=dev) if color_sum is not None else None,
                          make((V, 1, H, W), dtype=torch.float32, device=dev))
    if min(nx, ny, nz) < 2:            # no cell, no sample is ever defined, nothing to launch
        return maps(torch.zeros)
    if not sdf_sum.is_cuda:
        raise RuntimeError("raycast runs on HIP devices only: make the volume on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    s, w = sdf_sum.detach().contiguous(), weight.detach().contiguous()
    c = color_sum.detach().contiguous() if color_sum is not None else None
    # (held in names until the launch is queued: a converted copy must not be freed and its block handed out again)
    K32, T32 = (t.detach().to(torch.float32).contiguous() for t in (K, T_cam_in_world))
    ws_bytes = lib.mvsn_tsdf_raycast_workspace_bytes(nx, ny, nz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = maps(torch.empty)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_tsdf_raycast(
            _native.ptr(s), _native.ptr(w), _native.ptr(c), nx, ny, nz, float(v), float(o[0]), float(o[1]), float(o[2]),
            _native.ptr(K32), _native.ptr(T32), V, H, W, float(mw), float(lo), float(hi), float(st),
            _native.ptr(ws), ws_bytes, _native.ptr(out.depth), _native.ptr(out.normals), _native.ptr(out.colors),
            _native.ptr(out.weight), _native.stream()), "mvsn_tsdf_raycast")
    return out


def _integer(value, name, lo, hi=None):
    """``value`` as an int; ValueError unless it is an integer (not a bool) in [lo, hi]."""
    try:
        i = int(value)
        if i != value or isinstance(value, bool):
            raise TypeError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name} must be an integer, got {value!r}") from None
    if i < lo or (hi is not None and i > hi):
        raise ValueError(f"{name} must be an integer " + (f"in [{lo}, {hi}]" if hi is not None else f">= {lo}") + f", got {value!r}")
    return i


def _check_align(sdf_sum, weight, voxel_size, origin, depth, K, T_cam_in_world, valid, weights, min_weight, band, stride):
    """The validation ``align`` and ``align_system`` share; returns the checked scalars and sizes."""
    nx, ny, nz, dev = _check_state(sdf_sum, weight, None)

    def limits(V, H, W, d):
        if V > 65535 or H * W > 2 ** 31 - 1 or max(H, W) > MAX_EXTENT:
            raise ValueError(f"at most 65535 views of 2^31 - 1 pixels and 2^24 rows or columns, got {V} of {H} x {W}")
        if d != dev:
            raise ValueError(f"depth is on {d}, the volume on {dev}")
    V, H, W, _ = _check_views(depth, K, T_cam_in_world, limits=limits, floating=True)
    if valid is not None:
        _check_frames("valid", valid, V, H, W, 1, (torch.bool, torch.uint8), dev)
    if weights is not None:
        _check_frames("weights", weights, V, H, W, 1, (torch.float32,), dev)
    v = _positive_f32(voxel_size, "voxel_size")[0]
    mw = _positive_f32(min_weight, "min_weight")[0]
    bd = _positive_f32(band, "band")[0]
    o = _origin_f32(origin)
    st = min(_integer(stride, "stride", 1), max(H, W))     # (a longer stride leaves pixel (0, 0), as max(H, W) does)
    return nx, ny, nz, dev, V, H, W, v, mw, bd, o, st


def _align_inputs(sdf_sum, weight, depth, K, T_cam_in_world, valid, weights):
    # (held in names until the launches are queued: a converted copy must not be freed and its block handed out again)
    return (sdf_sum.detach().contiguous(), weight.detach().contiguous(), depth.detach().contiguous(),
            valid.detach().contiguous().view(torch.uint8) if valid is not None else None,
            weights.detach().contiguous() if weights is not None else None,
            K.detach().to(torch.float32).contiguous(), T_cam_in_world.detach().to(torch.float32).contiguous())


def align_system(sdf_sum: torch.Tensor, weight: torch.Tensor, voxel_size: float, origin: Sequence[float],
                 depth: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, *, band: float,
                 valid: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, min_weight: float = 1.0,
                 stride: int = 1, with_residual: bool = False):
    """One evaluation of ``align``'s Gauss-Newton system at the float32 values of ``T_cam_in_world``, on state tensors
    of any origin: ``(H (V,6,6) fp64, b (V,6) fp64, count (V,) int64, sum_w (V,) fp64, sum_w_r2 (V,) fp64, residual)``
    with H = sum w J J^T, b = sum w J r over the pixels that take part, J = (n, q x n) the derivative of r with respect
    to the update (v, omega) about the volume's centre, in voxel units.  ``residual`` (V,1,H,W) fp32, with
    ``with_residual``, is r per pixel and NaN where the pixel does not take part; None without.  ``band`` is required
    (the state has no ``trunc``).  What ``align`` iterates; the covariance of a pose is H^-1 times the noise scale."""
    nx, ny, nz, dev, V, H, W, v, mw, bd, o, st = _check_align(sdf_sum, weight, voxel_size, origin, depth, K, T_cam_in_world,
                                                               valid, weights, min_weight, band, stride)
    f64 = dict(dtype=torch.float64, device=dev)
    if min(nx, ny, nz) < 2:            # no cell, no point is ever defined, nothing to launch
        res = torch.full((V, 1, H, W), float("nan"), dtype=torch.float32, device=dev) if with_residual else None
        return (torch.zeros((V, 6, 6), **f64), torch.zeros((V, 6), **f64), torch.zeros((V,), dtype=torch.int64, device=dev),
                torch.zeros((V,), **f64), torch.zeros((V,), **f64), res)
    if not depth.is_cuda:
        raise RuntimeError("align_system runs on HIP devices only: make the volume and the depth maps on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    s, w, d, vd, wt, K32, T32 = _align_inputs(sdf_sum, weight, depth, K, T_cam_in_world, valid, weights)
    ws_bytes = lib.mvsn_tsdf_align_workspace_bytes(nx, ny, nz, V, H, W, st)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    Hm, b, sums = torch.empty((V, 6, 6), **f64), torch.empty((V, 6), **f64), torch.empty((V, 3), **f64)
    res = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev) if with_residual else None
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_tsdf_align_system(
            _native.ptr(s), _native.ptr(w), nx, ny, nz, float(v), float(o[0]), float(o[1]), float(o[2]), _native.ptr(d),
            _native.ptr(vd), _native.ptr(wt), _native.ptr(K32), _native.ptr(T32), V, H, W, st, float(mw), float(bd),
            _native.ptr(ws), ws_bytes, _native.ptr(Hm), _native.ptr(b), _native.ptr(sums), _native.ptr(res),
            _native.stream()), "mvsn_tsdf_align_system")
    dense = lambda t: t.clone(memory_format=torch.contiguous_format)   # noqa: E731  (unit strides for V = 1 too)
    return Hm, b, dense(sums[:, 0]).to(torch.int64), dense(sums[:, 1]), dense(sums[:, 2]), res


def align(sdf_sum: torch.Tensor, weight: torch.Tensor, voxel_size: float, origin: Sequence[float], depth: torch.Tensor,
          K: torch.Tensor, T_cam_in_world: torch.Tensor, *, band: float, valid: Optional[torch.Tensor] = None,
          weights: Optional[torch.Tensor] = None, min_weight: float = 1.0, iterations: int = 10, stride: int = 1,
          min_pixels: int = 6, min_pivot: float = 1e-9) -> TSDFAlignment:
    """``TSDFVolume.align`` on state tensors of any origin (``extract_mesh``'s).  ``band`` is required: the state has
    no ``trunc``; keep it inside the truncation the state was integrated with."""
    nx, ny, nz, dev, V, H, W, v, mw, bd, o, st = _check_align(sdf_sum, weight, voxel_size, origin, depth, K, T_cam_in_world,
                                                               valid, weights, min_weight, band, stride)
    it = _integer(iterations, "iterations", 0, 1000)
    mp = _integer(min_pixels, "min_pixels", 1, 2 ** 62)
    try:
        pv = float(min_pivot)
    except (TypeError, ValueError):
        raise ValueError(f"min_pivot must be a number inside (0, 1), got {min_pivot!r}") from None
    if not 0.0 < pv < 1.0:
        raise ValueError(f"min_pivot must be a number inside (0, 1), got {min_pivot!r}")
    if min(nx, ny, nz) < 2:            # no cell, no point is ever defined, nothing to launch: every view stops at once
        return TSDFAlignment(T_cam_in_world.detach().to(torch.float32).clone(),
                             torch.zeros((V, it + 1, 3), dtype=torch.float64, device=dev),
                             torch.ones((V,), dtype=torch.int32, device=dev),
                             torch.zeros((V, 6, 6), dtype=torch.float64, device=dev))
    if not depth.is_cuda:
        raise RuntimeError("align runs on HIP devices only: make the volume and the depth maps on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    s, w, d, vd, wt, K32, T32 = _align_inputs(sdf_sum, weight, depth, K, T_cam_in_world, valid, weights)
    ws_bytes = lib.mvsn_tsdf_align_workspace_bytes(nx, ny, nz, V, H, W, st)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = TSDFAlignment(torch.empty((V, 4, 4), dtype=torch.float32, device=dev),
                        torch.empty((V, it + 1, 3), dtype=torch.float64, device=dev),
                        torch.empty((V,), dtype=torch.int32, device=dev),
                        torch.empty((V, 6, 6), dtype=torch.float64, device=dev))
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_tsdf_align(
            _native.ptr(s), _native.ptr(w), nx, ny, nz, float(v), float(o[0]), float(o[1]), float(o[2]), _native.ptr(d),
            _native.ptr(vd), _native.ptr(wt), _native.ptr(K32), _native.ptr(T32), V, H, W, st, float(mw), float(bd), it, mp,
            pv, _native.ptr(ws), ws_bytes, _native.ptr(out.T_cam_in_world), _native.ptr(out.history),
            _native.ptr(out.status), _native.ptr(out.information), _native.stream()), "mvsn_tsdf_align")
    return out


def integrate_cloud(sdf_sum: torch.Tensor, weight: torch.Tensor, color_sum: Optional[torch.Tensor], voxel_size: float,
                    origin: Sequence[float], trunc: float, points: torch.Tensor, normals: torch.Tensor, radius: float, *,
                    weights: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None) -> None:
    """``TSDFVolume.integrate_cloud`` on state tensors of any origin, updated in place (they must be contiguous).

    ``normals`` point outwards, are expected to be unit length and are used as given; the volume is positive towards
    the cameras, so ``n . (x - p)`` is positive outside.  ``weights`` (N,) fp32 (1 without), ``colors`` (N,3) uint8
    (which need ``color_sum``, and the reverse, as ``images`` in ``integrate``).  A row takes part when its point is
    finite, its normal is finite and not (0,0,0) (this project's "no normal") and its weight is finite and in (0, 256];
    any other row is skipped.  With h = float32(radius), r2 = h*h and the voxel centre ``x = origin + float32(i) *
    voxel_size`` (a multiply, then an add), a row reaches the voxel when ``d2 = (dx*dx + dy*dy) + dz*dz <= r2`` for the
    fp32 differences ``dx = x - p``: ``cloud_nearest``'s relation.  Per accepted row, every step one fp32 operation:
    ``phi = (1 - d2/r2)^2``, ``A = rint(phi*w * 2^16)``, ``s = (dx*nx + dy*ny) + dz*nz``, ``t = min(max(s, -trunc),
    trunc)``, ``T = rint(t/trunc * 2^20)``.  The count, sum A, sum A*T and sum A*c per colour channel are exact 64-bit
    integers, so no byte of the state depends on the order of the rows, and the call is bitwise reproducible.  A voxel
    with sum A > 0 gets, each number formed in fp64 and rounded once to fp32: ``weight += sum A * 2^-16``, ``sdf_sum +=
    sum A*T * trunc * 2^-36`` and ``color_sum += (sum A*c * 2^-16) / 127.5 - sum A * 2^-16``; every other voxel keeps its
    bits, and so does a voxel with more than 2^19 - 1 accepted rows (the sums could overflow).  Because each call rounds
    the state once, two calls are not bit-identical to one call on the concatenated clouds.  Two sheets of points closer
    than ``radius`` blend into one.

    The points go on ``cloud_nearest``'s grid with cell = ``radius``: the time grows with (rows per cell) x (cells
    visited, 27 almost always) per voxel near the cloud, voxels in bricks of 8 x 8 x 8 far from every row cost a byte,
    and a finite point more than 2^20 cells of ``radius`` from the origin raises ValueError.  Everything is validated
    here, before any launch; the one host synchronisation is the read of the index build's status word, after
    everything is enqueued."""
    nx, ny, nz, dev = _check_state(sdf_sum, weight, color_sum)
    for name, t in (("sdf_sum", sdf_sum), ("weight", weight), ("color_sum", color_sum)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: it is updated in place")
    v = _positive_f32(voxel_size, "voxel_size")[0]
    tr = _positive_f32(trunc, "trunc")[0]
    o = _origin_f32(origin)
    check_cloud("points", points)
    N = int(points.shape[0])
    if points.device != dev:
        raise ValueError(f"points is on {points.device}, the volume on {dev}")
    if not torch.is_tensor(normals) or tuple(normals.shape) != (N, 3) or normals.dtype != torch.float32:
        raise ValueError(f"normals must be a ({N},3) float32 tensor like points")
    if normals.device != dev:
        raise ValueError(f"normals is on {normals.device}, the volume on {dev}")
    h, inv, r2 = cloud_radius_scalars(radius, "radius")
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) != (N,) or weights.dtype != torch.float32:
            raise ValueError(f"weights must be a ({N},) float32 tensor, one per point")
        if weights.device != dev:
            raise ValueError(f"weights is on {weights.device}, the volume on {dev}")
    if (colors is not None) != (color_sum is not None):
        raise ValueError("colors need a volume made with color=True, and such a volume needs colors")
    if colors is not None:
        if not torch.is_tensor(colors) or tuple(colors.shape) != (N, 3) or colors.dtype != torch.uint8:
            raise ValueError(f"colors must be a ({N},3) uint8 tensor like points")
        if colors.device != dev:
            raise ValueError(f"colors is on {colors.device}, the volume on {dev}")
    if N == 0:                         # nothing to add, nothing to launch
        return
    if not points.is_cuda:
        raise RuntimeError("integrate_cloud runs on HIP devices only: make the volume and the cloud on 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    # (held in names until the launches are queued: a copy must not be freed and its block handed out again)
    p, nr = points.detach().contiguous(), normals.detach().contiguous()
    w = weights.detach().contiguous() if weights is not None else None
    c = colors.detach().contiguous() if colors is not None else None
    flag_bytes = lib.mvsn_tsdf_cloud_workspace_bytes(nx, ny, nz)
    flags = torch.empty(flag_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        ws, ws_bytes, status = _cloud_index_build(lib, p, N, h, inv, dev, st)
        _native.check(lib.mvsn_tsdf_cloud_integrate(
            _native.ptr(p), _native.ptr(nr), _native.ptr(w), _native.ptr(c), N, _native.ptr(ws), ws_bytes, float(h),
            float(inv), float(r2), nx, ny, nz, float(v), float(o[0]), float(o[1]), float(o[2]), float(tr),
            _native.ptr(sdf_sum.detach()), _native.ptr(weight.detach()),
            _native.ptr(color_sum.detach() if color_sum is not None else None), _native.ptr(flags), flag_bytes, st),
            "mvsn_tsdf_cloud_integrate")
        bits = int(status.item())      # the one host synchronisation, after everything is enqueued
    _raise_cloud_status(bits, h, "integrate_cloud")   # (cloud_nearest's errors: the points are the index's target, radius its max_dist)
