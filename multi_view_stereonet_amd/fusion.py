"""Depth-map fusion: from per-view depth maps to one geometric-consistency-filtered, coloured point cloud.

Each reference view's depth is checked against its neighbours' depths; the pixels enough neighbours confirm are
averaged with the confirming depths and back-projected into world coordinates (DESIGN.md section 10 states the
semantics; the kernels are csrc/mvsn_fusion.hip).  ``fuse_depthmaps`` runs that on depth maps already on the device,
``reconstruct`` runs the network over posed frames first, and ``write_ply`` saves the result.  A per-pixel confidence
(``net.options.confidence``) can gate the fusion before the geometric check (``min_confidence``)
and be read at the kept points (``point_values``).  ``voxel_merge`` (csrc/mvsn_voxel.hip) merges a
cloud on a voxel grid: a surface that k views saw is in the fused cloud k times, and in the merged one once.
``depth_normals`` (csrc/mvsn_normals.hip) gives every pixel of a depth map its normal, facing the
camera; ``point_normals`` reads those maps at the points of a fused cloud and ``voxel_normals`` takes them through a merge.
``cloud_nearest`` (csrc/mvsn_cloud.hip) finds, for every point of one cloud, the nearest point of
another within a radius, exactly; ``radius_outlier_mask`` is the same query of a cloud against itself
(``metrics.cloud_metrics`` builds accuracy / completeness / F-score on it).  ``cloud_register`` (DESIGN.md section 20,
csrc/mvsn_cloud_register.hip) moves one cloud onto another by ICP on that query, point-to-plane or point-to-point, and
``cloud_register_system`` is one evaluation of its normal equations; ``cloud_normals`` (DESIGN.md section 21,
csrc/mvsn_cloud_normals.hip) gives a bare cloud the normals that the point-to-plane mode needs, from the covariance of
every point's neighbours within a radius.  ``cloud_knn`` (csrc/mvsn_cloud_knn.hip) returns the k
nearest neighbours within a radius themselves, and ``statistical_outlier_mask`` is the statistical outlier filter on it,
whose threshold follows the cloud's own spacing.  ``cloud_register_global`` registers two clouds
from unrelated frames, the start that ``cloud_register`` needs: ``cloud_fpfh`` (csrc/mvsn_cloud_fpfh.hip) describes every
point by its FPFH histogram, ``feature_nearest`` (csrc/mvsn_cloud_match.hip) matches the descriptors, and ``cloud_ransac``
(csrc/mvsn_cloud_ransac.hip) finds the pose that most correspondences agree on.  ``cloud_clusters`` (DESIGN.md section
24, csrc/mvsn_cloud_cluster.hip) splits a cloud into its density-connected pieces (DBSCAN on the same radius query) and
``cloud_cluster_mask`` keeps the pieces one asks for: the detached floaters that both local filters pass go.
``cloud_render`` (csrc/mvsn_cloud_render.hip) renders a cloud into posed cameras, the nearest point
per pixel; ``cloud_visibility`` tests every point against depth maps for occlusion and reads per-view maps at the points
that are seen, and ``cloud_colorize`` colours a bare cloud that way.  A dense TSDF volume that integrates the same
depth maps and a mesh from it are in ``tsdf``; ``write_ply(faces=)`` writes such a mesh and
``read_ply`` reads back what ``write_ply`` wrote, or an ASCII cloud from elsewhere, for ``tsdf.integrate_cloud``
 to turn into a surface.

Conventions: ``K`` (V,4,4) with the top-left 3x3 used and a bottom row of (0,0,1); ``T_cam_in_world`` (V,4,4) maps camera
coordinates to world coordinates; pixel (x, y) = (column, row) with integer values at pixel centres.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native

MAX_NEIGHBOURS = 32


class FusionResult(NamedTuple):
    points: torch.Tensor             # (M,3) fp32 world coordinates
    colors: Optional[torch.Tensor]   # (M,3) uint8, or None without images
    view: torch.Tensor               # (M,) int32: the reference view each point comes from
    pixel: torch.Tensor              # (M,) int32: its row-major pixel index
    depth: torch.Tensor              # (R,1,H,W) fp32: fused depth, 0 where not kept
    count: torch.Tensor              # (R,1,H,W) uint8: consistent neighbours per pixel


def _host_index_array(a, name) -> np.ndarray:
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integers, got {a.dtype}")
    return a.astype(np.int64)


def _check_frames(name, t, V, H, W, channels, dtypes, device):
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor")
    if tuple(t.shape) != (V, channels, H, W):
        raise ValueError(f"{name} must be ({V},{channels},{H},{W}), got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, depth on {device}")


def _check_views(depth, K, T_cam_in_world, *, limits=None, T_optional=False, floating=False):
    """ValueError unless ``depth`` is a (V,1,H,W) float32 tensor of at least one view of at least one pixel and ``K`` and
    ``T_cam_in_world`` (which may be None with ``T_optional``) are (V,4,4) tensors on its device (floating-point ones
    with ``floating``).  ``limits(V, H, W, dev)``: the caller's own size and device limits, checked after the depth and
    before the matrices.  Returns (V, H, W, dev)."""
    if not torch.is_tensor(depth) or depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError("depth must be a (V,1,H,W) tensor")
    V, _, H, W = depth.shape
    dev = depth.device
    if V < 1 or H * W < 1:
        raise ValueError("depth must hold at least one view of at least one pixel")
    if depth.dtype != torch.float32:
        raise ValueError(f"depth must be float32, got {depth.dtype}")
    if limits is not None:
        limits(V, H, W, dev)
    for name, m in (("K", K), ("T_cam_in_world", T_cam_in_world)):
        if m is None and T_optional and name != "K":
            continue
        if not torch.is_tensor(m) or tuple(m.shape) != (V, 4, 4):
            raise ValueError(f"{name} must be a ({V},4,4) tensor")
        if floating and not m.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {m.dtype}")
        if m.device != dev:
            raise ValueError(f"{name} is on {m.device}, depth on {dev}")
    return V, H, W, dev


def _positive_f32(value, name, inverse=False, square=False):
    """(v, 1/v, v*v) with v = np.float32(value), each formed once in fp32 on the host, None for what was not asked for;
    ValueError unless every one of them is finite and > 0."""
    with np.errstate(all="ignore"):
        try:
            v = np.float32(value)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a positive finite number, got {value!r}") from None
        inv = np.float32(1) / v if inverse else None
        sq = v * v if square else None
    if not all(np.isfinite(x) and x > 0 for x in (v, inv, sq) if x is not None):
        how = " in float32" if not inverse else " (in float32, with a finite inverse)" if not square else \
            " (in float32, with a finite inverse and a finite non-zero square)"
        raise ValueError(f"{name} must be finite and > 0{how}, got {value!r}")
    return v, inv, sq


def _origin_f32(origin):
    """``origin`` as three np.float32; ValueError unless they are three finite numbers."""
    try:
        o = np.asarray(origin, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"origin must be three finite numbers, got {origin!r}") from None
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be three finite numbers, got {origin!r}")
    return o


def fuse_depthmaps(depth: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, neighbours, *,
                   images: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                   ref_views: Optional[Sequence[int]] = None, max_reproj_px: float = 1.0,
                   max_rel_depth: float = 0.01, min_consistent: int = 2, confidence: Optional[torch.Tensor] = None,
                   min_confidence: Optional[float] = None) -> FusionResult:
    """Fuse ``depth`` (V,1,H,W) into a point cloud.

    ``neighbours`` is a host (R,M) integer array, 1 <= M <= 32: row i lists the views that check ``ref_views[i]``
    (default ``range(V)``), -1 skips a slot.  A pixel of a reference view is kept when at least ``min_consistent``
    neighbours confirm it (reprojection error < ``max_reproj_px`` pixels and relative depth difference <
    ``max_rel_depth``, both strictly).  A depth that is <= 0 or NaN is no depth, as a candidate and under a neighbour's
    bilinear taps, where it fails the slot.  ``+inf`` passes "> 0": as a candidate it can never be confirmed, so it is
    kept (as ``inf``, with a point that is not finite) only with ``min_consistent=0``; as a tap it makes its slot
    inconsistent for every pixel whose four taps hold it.  No such value changes any other pixel.  In a uint8 ``valid``
    every non-zero byte is "valid".  Points come ordered by position in ``ref_views``, then row-major pixel.  Everything
    is validated here, before any launch; the one host synchronisation is the read of the number of kept pixels (to
    size the outputs).

    ``confidence`` (V,1,H,W) fp32 with ``min_confidence``: the call is this function with ``valid`` and-ed with
    ``confidence >= min_confidence`` (formed on the device; a pixel at the threshold is kept, a NaN confidence is not).
    The gate applies, as ``valid`` does, to the candidate pixel and to every neighbour tap."""
    V, H, W, dev = _check_views(depth, K, T_cam_in_world)
    if images is not None:
        _check_frames("images", images, V, H, W, 3, (torch.float32,), dev)
    if valid is not None:
        _check_frames("valid", valid, V, H, W, 1, (torch.bool, torch.uint8), dev)
    if min_confidence is not None and confidence is None:
        raise ValueError("min_confidence needs the confidence maps")
    if confidence is not None:
        _check_frames("confidence", confidence, V, H, W, 1, (torch.float32,), dev)
    if min_confidence is not None and not float(min_confidence) >= 0:
        raise ValueError(f"min_confidence must be a non-negative number, got {min_confidence}")
    nb = _host_index_array(neighbours, "neighbours")
    if nb.ndim != 2:
        raise ValueError(f"neighbours must be (R, M), got shape {nb.shape}")
    R, M = nb.shape
    if not 1 <= M <= MAX_NEIGHBOURS:
        raise ValueError(f"neighbours must have 1..{MAX_NEIGHBOURS} slots per reference view, got {M}")
    refs = np.arange(V, dtype=np.int64) if ref_views is None else _host_index_array(ref_views, "ref_views").reshape(-1)
    if refs.shape[0] != R:
        raise ValueError(f"neighbours has {R} rows for {refs.shape[0]} reference views")
    if R < 1 or R > 65535:
        raise ValueError(f"1..65535 reference views, got {R}")
    if ((refs < 0) | (refs >= V)).any():
        raise ValueError(f"ref_views must lie in [0, {V})")
    if ((nb < -1) | (nb >= V)).any():
        raise ValueError(f"neighbour indices must lie in [-1, {V})")
    if (nb == refs[:, None]).any():
        raise ValueError("a view cannot be its own neighbour")
    if not (max_reproj_px >= 0 and max_rel_depth >= 0 and min_consistent >= 0):
        raise ValueError("thresholds must be non-negative")

    if not depth.is_cuda:
        raise RuntimeError("fuse_depthmaps runs on HIP devices only: move the depth maps to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
    depth_c, K_c, T_c = f32(depth), f32(K), f32(T_cam_in_world)
    valid_c = valid.detach().contiguous().view(torch.uint8) if valid is not None else None
    if confidence is not None and min_confidence is not None:
        gated = torch.empty((V, 1, H, W), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.mvsn_confidence_mask(_native.ptr(confidence.detach().contiguous()), _native.ptr(valid_c),
                                                   V * H * W, float(min_confidence), _native.ptr(gated),
                                                   _native.stream()), "mvsn_confidence_mask")
        valid_c = gated
    refs_d = torch.from_numpy(refs.astype(np.int32)).to(dev)
    nb_d = torch.from_numpy(np.ascontiguousarray(nb.astype(np.int32))).to(dev)
    ws_bytes = lib.mvsn_fusion_workspace_bytes(R, M, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    fused = torch.empty((R, 1, H, W), dtype=torch.float32, device=dev)
    count = torch.empty((R, 1, H, W), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_fusion_consistency(
            _native.ptr(depth_c), _native.ptr(valid_c), _native.ptr(K_c), _native.ptr(T_c), _native.ptr(refs_d),
            _native.ptr(nb_d), V, R, M, H, W, float(max_reproj_px), float(max_rel_depth), int(min_consistent),
            _native.ptr(fused), _native.ptr(count), _native.ptr(total), _native.ptr(ws), ws_bytes, st),
            "mvsn_fusion_consistency")
        n = int(total.item())          # the one host synchronisation: sizes the outputs
        points = torch.empty((n, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev) if images is not None else None
        view = torch.empty((n,), dtype=torch.int32, device=dev)
        pixel = torch.empty((n,), dtype=torch.int32, device=dev)
        images_c = f32(images) if images is not None else None
        _native.check(lib.mvsn_fusion_emit(
            _native.ptr(fused), _native.ptr(images_c), _native.ptr(refs_d), R, H, W, M, _native.ptr(ws), ws_bytes, n,
            _native.ptr(points), _native.ptr(colors), _native.ptr(view), _native.ptr(pixel), st), "mvsn_fusion_emit")
    return FusionResult(points, colors, view, pixel, fused, count)


def point_values(result: FusionResult, maps: torch.Tensor, ref_views: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The value of ``maps`` (V,1,H,W) fp32 -- a confidence pyramid's level 0, say -- at every point of ``result``:
    (M,) fp32, ``maps[result.view[i]]`` at row-major pixel ``result.pixel[i]``.  ``ref_views``: the fusion's, when
    ``maps`` holds only those views, in that order (``maps`` is then (R,1,H,W))."""
    return _gather_at_points(result, maps, 1, ref_views, "maps")


def _gather_at_points(result, maps, channels, ref_views, name):
    """``point_values`` (channels 1, (M,)) and ``point_normals`` (channels 3, (M,3)): the checks, the table from a view
    to its row of ``maps`` when ``ref_views`` is given, and the launch.  An empty cloud returns before point_normals asks
    for a HIP device and after point_values does."""
    func, entry, empty_first = {1: ("point_values", "mvsn_fusion_gather", False),
                                3: ("point_normals", "mvsn_normals_gather", True)}[channels]
    if not torch.is_tensor(maps) or maps.dim() != 4 or maps.shape[1] != channels:
        raise ValueError(f"{name} must be a (V,{channels},H,W) tensor")
    if maps.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {maps.dtype}")
    if tuple(maps.shape[-2:]) != tuple(result.depth.shape[-2:]):
        raise ValueError(f"{name} are {tuple(maps.shape[-2:])}, the fusion ran on {tuple(result.depth.shape[-2:])}")
    if maps.device != result.view.device:
        raise ValueError(f"{name} are on {maps.device}, the points on {result.view.device}")
    view = result.view
    if ref_views is not None:
        refs = _host_index_array(ref_views, "ref_views").reshape(-1)
        if refs.shape[0] != maps.shape[0]:
            raise ValueError(f"{name} hold {maps.shape[0]} views for {refs.shape[0]} reference views")
        row = np.full(int(refs.max()) + 1 if refs.size else 1, -1, dtype=np.int32)
        row[refs] = np.arange(refs.shape[0], dtype=np.int32)
        lut = torch.from_numpy(row).to(view.device)
        view = lut[view.long().clamp(0, lut.shape[0] - 1)].contiguous()
    M = int(view.shape[0])
    shape = (M,) if channels == 1 else (M, channels)
    if M == 0 and empty_first:         # no points: nothing to launch
        return torch.empty(shape, dtype=torch.float32, device=maps.device)
    if not maps.is_cuda:
        raise RuntimeError(f"{func} runs on HIP devices only (there is no CPU implementation)")
    out = torch.empty(shape, dtype=torch.float32, device=maps.device)
    if M == 0:
        return out
    lib = _native.load()
    with torch.cuda.device(maps.device):
        _native.check(getattr(lib, entry)(_native.ptr(maps.detach().contiguous()), _native.ptr(view.contiguous()),
                                          _native.ptr(result.pixel.contiguous()), maps.shape[0],
                                          maps.shape[2] * maps.shape[3], M, _native.ptr(out), _native.stream()), entry)
    return out


def depth_normals(depth: torch.Tensor, K: torch.Tensor, *, valid: Optional[torch.Tensor] = None,
                  T_cam_in_world: Optional[torch.Tensor] = None, max_rel_step: float = 0.05) -> torch.Tensor:
    """The normal of every pixel of ``depth`` (V,1,H,W), from differences of its back-projected neighbours: (V,3,H,W)
    fp32 unit vectors that face the camera (n . X < 0), in the camera frame, or in the world frame when
    ``T_cam_in_world`` (V,4,4) is given (its top-left 3x3 is taken to be a rotation).

    A pixel is usable when its depth is > 0 (and ``valid`` (V,1,H,W) is set); a neighbour counts when it is usable and
    its depth differs by at most ``max_rel_step`` of the pixel's (``inf``: no such test), so a depth edge is not
    differenced across.  Each tangent is the central difference where both neighbours count and the one-sided one where
    one does; the normal is (0,0,0) where the pixel is not usable or a tangent has no neighbour (DESIGN.md section 13
    states every step).  Everything is validated here, before the launch; no host synchronisation."""
    def limits(V, H, W, dev):
        if V > 65535 or H * W > 2 ** 31 - 1:
            raise ValueError(f"at most 65535 views of 2^31 - 1 pixels, got {V} of {H * W}")
    V, H, W, dev = _check_views(depth, K, T_cam_in_world, limits=limits, T_optional=True)
    if valid is not None:
        _check_frames("valid", valid, V, H, W, 1, (torch.bool, torch.uint8), dev)
    try:
        step = float(max_rel_step)
    except (TypeError, ValueError):
        raise ValueError(f"max_rel_step must be a non-negative number, got {max_rel_step!r}") from None
    if not step >= 0:
        raise ValueError(f"max_rel_step must be a non-negative number, got {max_rel_step!r}")

    if not depth.is_cuda:
        raise RuntimeError("depth_normals runs on HIP devices only: move the depth maps to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
    valid_c = valid.detach().contiguous().view(torch.uint8) if valid is not None else None
    T_c = f32(T_cam_in_world) if T_cam_in_world is not None else None
    normals = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_depth_normals(_native.ptr(f32(depth)), _native.ptr(valid_c), _native.ptr(f32(K)),
                                             _native.ptr(T_c), V, H, W, step, _native.ptr(normals), _native.stream()),
                      "mvsn_depth_normals")
    return normals


def point_normals(result: FusionResult, normals: torch.Tensor, ref_views: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The normal maps ``normals`` (V,3,H,W) fp32 of ``depth_normals`` at every point of ``result``: (M,3) fp32,
    ``normals[result.view[i], :, pixel]`` at row-major pixel ``result.pixel[i]`` (``point_values`` for a three-channel
    map).  ``ref_views``: the fusion's, when ``normals`` holds only those views, in that order (then (R,3,H,W))."""
    return _gather_at_points(result, normals, 3, ref_views, "normals")


class VoxelCloud(NamedTuple):
    points: torch.Tensor             # (M,3) fp32: mean position of each occupied voxel
    colors: Optional[torch.Tensor]   # (M,3) uint8 mean colour, or None
    count: torch.Tensor              # (M,) int32: points merged into the voxel
    first: torch.Tensor              # (M,) int64: lowest input index among the voxel's points
    inverse: torch.Tensor            # (N,) int64: output row of every input point, -1 = dropped


VOXEL_CELL_LIMIT = 1 << 20           # cells of a finite point lie in [-2^20, 2^20) on every axis
VOXEL_STATUS_RANGE, VOXEL_STATUS_TABLE = 1, 2


def voxel_merge(points: torch.Tensor, voxel_size: float, *, colors: Optional[torch.Tensor] = None,
                origin: Sequence[float] = (0.0, 0.0, 0.0)) -> VoxelCloud:
    """Merge ``points`` (N,3) fp32 on a regular grid of ``voxel_size`` anchored at ``origin``: the points of one cell
    become one point, at the mean of their positions (and of ``colors`` (N,3) uint8), ordered by the lowest input index
    of each voxel -- a cloud of ``fuse_depthmaps`` keeps its "reference, then row-major pixel" order.  ``first`` and
    ``inverse`` carry the provenance: ``res.view[vc.first]`` / ``res.pixel[vc.first]`` name a representative pixel,
    and any per-point attribute reduces through ``inverse`` with ordinary torch.

    The cell of a point is floor((p - origin) * (1 / voxel_size)) in fp32 (DESIGN.md section 12 states every step); a
    point with a non-finite coordinate is dropped (``inverse`` -1, counted nowhere); a finite point more than 2^20
    cells from the origin raises ValueError.  Every output is a bitwise-reproducible function of the inputs, and the
    means do not depend on the order of the points.  Everything is validated here, before any launch; the one host
    synchronisation is the read of the number of voxels (with the status word beside it)."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be an (N,3) tensor")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    N, dev = int(points.shape[0]), points.device
    if N > 2 ** 31 - 1:
        raise ValueError(f"at most 2^31 - 1 points, got {N}")
    if colors is not None:
        if not torch.is_tensor(colors) or tuple(colors.shape) != (N, 3):
            raise ValueError(f"colors must be an ({N},3) tensor like points")
        if colors.dtype != torch.uint8:
            raise ValueError(f"colors must be uint8, got {colors.dtype}")
        if colors.device != dev:
            raise ValueError(f"colors are on {colors.device}, points on {dev}")
    v, inv, _ = _positive_f32(voxel_size, "voxel_size", inverse=True)
    o = _origin_f32(origin)

    def result(m):
        return VoxelCloud(torch.empty((m, 3), dtype=torch.float32, device=dev),
                          torch.empty((m, 3), dtype=torch.uint8, device=dev) if colors is not None else None,
                          torch.empty((m,), dtype=torch.int32, device=dev),
                          torch.empty((m,), dtype=torch.int64, device=dev),
                          torch.empty((N,), dtype=torch.int64, device=dev))
    if N == 0:                         # nothing to merge, nothing to launch: empties on the points' device
        return result(0)
    if not points.is_cuda:
        raise RuntimeError("voxel_merge runs on HIP devices only: move the points to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    pts = points.detach().contiguous()
    cols = colors.detach().contiguous() if colors is not None else None
    scalars = (float(v), float(inv), float(o[0]), float(o[1]), float(o[2]))
    ws_bytes = lib.mvsn_voxel_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        _native.check(lib.mvsn_voxel_assign(_native.ptr(pts), N, *scalars, _native.ptr(head), _native.ptr(ws), ws_bytes,
                                            st), "mvsn_voxel_assign")
        m, status = head.tolist()      # the one host synchronisation: sizes the outputs, carries the status word
        if status & VOXEL_STATUS_RANGE:
            raise ValueError(f"voxel_size too small for the cloud's extent: a point lies 2^20 = {VOXEL_CELL_LIMIT} "
                             f"cells of {float(v):g} or more from the origin {tuple(float(x) for x in o)}")
        if status:
            raise RuntimeError(f"voxel_merge: the hash grid overflowed (status {status})")
        vc = result(m)
        if m == 0:                     # every point dropped
            vc.inverse.fill_(-1)
            return vc
        accum = torch.empty((m, 8), dtype=torch.int64, device=dev)
        _native.check(lib.mvsn_voxel_merge(_native.ptr(pts), _native.ptr(cols), N, *scalars, _native.ptr(ws), ws_bytes,
                                           m, _native.ptr(accum), _native.ptr(vc.points), _native.ptr(vc.colors),
                                           _native.ptr(vc.count), _native.ptr(vc.first), _native.ptr(vc.inverse), st),
                      "mvsn_voxel_merge")
    return vc


def voxel_normals(vc: VoxelCloud, normals: torch.Tensor) -> torch.Tensor:
    """The normal of every voxel of ``vc``: (len(vc.count),3) fp32, the direction of the sum of the ``normals`` (N,3)
    fp32 of its points (N = len(vc.inverse): ``point_normals`` of the cloud that was merged).  Each component is
    quantised to 2^-20 and the sums are integers, so the result does not depend on the order of the points and is
    bitwise reproducible.  A point the merge dropped, a non-finite normal and the (0,0,0) of an undefined pixel add
    nothing; a voxel whose sum is zero gets (0,0,0)."""
    N, M = int(vc.inverse.shape[0]), int(vc.count.shape[0])
    dev = vc.inverse.device
    if not torch.is_tensor(normals) or tuple(normals.shape) != (N, 3):
        raise ValueError(f"normals must be an ({N},3) tensor, one row per merged point")
    if normals.dtype != torch.float32:
        raise ValueError(f"normals must be float32, got {normals.dtype}")
    if normals.device != dev:
        raise ValueError(f"normals are on {normals.device}, the cloud on {dev}")
    if M == 0:                         # no voxels, nothing to launch
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    if N == 0:                         # (voxels without points: not a cloud voxel_merge returns)
        return torch.zeros((M, 3), dtype=torch.float32, device=dev)
    if not normals.is_cuda:
        raise RuntimeError("voxel_normals runs on HIP devices only (there is no CPU implementation)")
    lib = _native.load()
    out = torch.empty((M, 3), dtype=torch.float32, device=dev)
    accum = torch.empty((M, 3), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_voxel_normals(_native.ptr(normals.detach().contiguous()),
                                             _native.ptr(vc.inverse.contiguous()), N, M, _native.ptr(accum),
                                             _native.ptr(out), _native.stream()), "mvsn_voxel_normals")
    return out


class CloudNeighbours(NamedTuple):
    dist2: torch.Tensor              # (N,) fp32: squared distance to the nearest target point, +inf where none within max_dist
    index: torch.Tensor              # (N,) int64: that target point's row, -1 where none
    within: torch.Tensor             # (N,) int32: number of target points within max_dist


CLOUD_STATUS_RANGE, CLOUD_STATUS_TABLE = 1, 2


def check_cloud(name, t):
    """ValueError unless ``t`` is an (N,3) float32 tensor of at most 2^31 - 1 rows (any device)."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be an (N,3) tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if int(t.shape[0]) > 2 ** 31 - 1:
        raise ValueError(f"at most 2^31 - 1 {name} points, got {int(t.shape[0])}")


def cloud_radius_scalars(max_dist, name="max_dist"):
    """(h, 1/h, h*h) as np.float32, each formed once in fp32 on the host; ValueError unless all three are finite and
    > 0."""
    return _positive_f32(max_dist, name, inverse=True, square=True)


def _require_hip(who, t, noun="clouds"):
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs on HIP devices only: move the {noun} to 'cuda' "
                           "(there is no CPU implementation)")


def _raise_cloud_status(bits, h, who):
    if bits & CLOUD_STATUS_RANGE:
        raise ValueError(f"max_dist too small for the target's extent: a target point lies 2^20 = {VOXEL_CELL_LIMIT} "
                         f"cells of {float(h):g} or more from the origin")
    if bits:
        raise RuntimeError(f"{who}: the hash grid overflowed (status {bits})")


def _cloud_index_build(lib, target, n, h, inv, dev, st, status=None):
    """``(ws, ws_bytes, status)``: the hash-grid index of ``target`` (n,3) fp32, contiguous on ``dev``, enqueued on
    stream ``st`` in a workspace made here.  The build's status word goes to ``status`` (an int64 word on ``dev``; made
    here without one): the caller reads it after its own launches, its one host synchronisation, and hands it to
    ``_raise_cloud_status``."""
    ws_bytes = lib.mvsn_cloud_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if status is None:
        status = torch.empty(1, dtype=torch.int64, device=dev)
    _native.check(lib.mvsn_cloud_index_build(_native.ptr(target), n, float(h), float(inv), _native.ptr(status),
                                             _native.ptr(ws), ws_bytes, st), "mvsn_cloud_index_build")
    return ws, ws_bytes, status


def cloud_nearest(query: torch.Tensor, target: torch.Tensor, max_dist: float) -> CloudNeighbours:
    """For every row of ``query`` (N,3) fp32 the nearest row of ``target`` (T,3) fp32 within ``max_dist``: its squared
    distance, its row, and how many target points lie within ``max_dist``.  Neither cloud needs any order.

    With h = float32(max_dist) the squared distance is ``(dx*dx + dy*dy) + dz*dz`` of the fp32 differences, each step
    one fp32 operation; a target is within when that is ``<= h*h``; ties for the nearest go to the lowest target row.
    The result is exactly that of the brute force over every target point (DESIGN.md section 14 has the proof).  A
    target with a non-finite coordinate is nobody's neighbour, a query with one gets (+inf, -1, 0), and a query may lie
    anywhere.  The target goes on a grid of cell size h anchored at (0,0,0): a finite target more than 2^20 cells from
    the origin raises ValueError.  The time grows with (targets per cell) x (cells visited, 27 almost always): a
    ``max_dist`` far above the sampling distance is quadratic within a neighbourhood.  Everything is validated here,
    before any launch; the one host synchronisation is the read of the status word, after the query is enqueued."""
    check_cloud("query", query)
    check_cloud("target", target)
    if query.device != target.device:
        raise ValueError(f"query is on {query.device}, target on {target.device}")
    h, inv, r2 = cloud_radius_scalars(max_dist)
    N, T, dev = int(query.shape[0]), int(target.shape[0]), query.device
    if N == 0 or T == 0:               # nothing to find, nothing to launch
        return CloudNeighbours(torch.full((N,), float("inf"), dtype=torch.float32, device=dev),
                               torch.full((N,), -1, dtype=torch.int64, device=dev),
                               torch.zeros((N,), dtype=torch.int32, device=dev))
    _require_hip("cloud_nearest", query)
    lib = _native.load()
    q, t = query.detach().contiguous(), target.detach().contiguous()
    out = CloudNeighbours(torch.empty((N,), dtype=torch.float32, device=dev),
                          torch.empty((N,), dtype=torch.int64, device=dev),
                          torch.empty((N,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        st = _native.stream()
        ws, ws_bytes, status = _cloud_index_build(lib, t, T, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_nearest(_native.ptr(q), N, float(inv), float(r2), _native.ptr(ws), ws_bytes, T,
                                             _native.ptr(out.dist2), _native.ptr(out.index), _native.ptr(out.within),
                                             st), "mvsn_cloud_nearest")
        bits = int(status.item())      # the one host synchronisation (the query never leaves its buffers, whatever the table holds)
    _raise_cloud_status(bits, h, "cloud_nearest")
    return out


class CloudNormals(NamedTuple):
    normals: torch.Tensor            # (N,3) fp32: unit normal, (0,0,0) where the direction is not defined
    eigenvalues: torch.Tensor        # (N,3) fp32: of the neighbourhood's covariance, ascending, squared world units
    count: torch.Tensor              # (N,) int32: support points within the radius (cloud_nearest's `within`)


def _check_viewpoint(viewpoint, N, dev):
    """None, or the viewpoint as a (1,3) or (N,3) float32 tensor (three numbers stay where they are until the launch);
    ValueError for anything that is neither three numbers nor an (N,3) float32 tensor on the points' device."""
    if viewpoint is None:
        return None
    if torch.is_tensor(viewpoint) and viewpoint.dim() == 2:
        if tuple(viewpoint.shape) != (N, 3) or viewpoint.dtype != torch.float32:
            raise ValueError(f"viewpoint must be three numbers or a ({N},3) float32 tensor")
        if viewpoint.device != dev:
            raise ValueError(f"viewpoint is on {viewpoint.device}, points on {dev}")
        return viewpoint.detach().contiguous()
    if torch.is_tensor(viewpoint):     # a (3,) tensor stays where it is until the launch: nothing waits for the device
        if tuple(viewpoint.shape) != (3,) or viewpoint.dtype == torch.bool or viewpoint.is_complex() or \
                viewpoint.device.type == "meta":
            raise ValueError(f"viewpoint must be three numbers or a ({N},3) float32 tensor")
        return viewpoint.detach().to(torch.float32).reshape(1, 3)
    try:
        with np.errstate(all="ignore"):
            v = np.asarray(viewpoint, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"viewpoint must be three numbers or a ({N},3) float32 tensor, got {viewpoint!r}") from None
    if v.shape != (3,):
        raise ValueError(f"viewpoint must be three numbers or a ({N},3) float32 tensor, got {viewpoint!r}")
    return torch.from_numpy(v.reshape(1, 3))


def cloud_normals(points: torch.Tensor, radius: float, *, support: Optional[torch.Tensor] = None, viewpoint=None,
                  min_neighbours: int = 3, min_gap: float = 2.0 ** -20) -> CloudNormals:
    """A normal for every row of ``points`` (N,3) fp32 from the covariance of the rows of ``support`` (M,3) fp32 within
    ``radius`` of it (PCA; DESIGN.md section 21, csrc/mvsn_cloud_normals.hip).  ``support`` defaults to ``points``
    itself: a point is then its own neighbour, as in ``radius_outlier_mask``.  Neither cloud needs depth maps, a
    volume or any order: this is where ``cloud_register``'s ``target_normals`` come from for a bare cloud.

    ``count`` is exactly ``cloud_nearest(points, support, radius).within``.  ``eigenvalues`` are those of the
    neighbourhood's covariance, ascending, in squared world units.  ``normals`` is the unit eigenvector of the smallest,
    and (0,0,0) where ``count < min_neighbours`` (an integer >= 3), where the point is not finite, and where
    ``lambda_1 - lambda_0 <= min_gap * lambda_2`` (``min_gap`` in [0, 1)): collinear or coincident neighbours or an
    isotropic blob, which define no direction.

    The sign: with ``viewpoint`` (three numbers, a (3,) tensor, or an (N,3) fp32 tensor such as
    ``T_cam_in_world[res.view, :3, 3]``) every normal is flipped so that ``n . (viewpoint - p) >= 0``.  Without one,
    where that product is 0 and where a viewpoint row is not finite the sign is canonical: the component of largest
    magnitude is positive, ties going to the lowest axis.  Point-to-plane registration does not care about the sign.

    The differences of the neighbours are quantised to 2^-20 of the radius and summed as exact integers; the
    covariance, six cyclic Jacobi sweeps and the sign rule run in fp64, and every output number is rounded to fp32
    once.  Every output is a bitwise-reproducible function of the inputs and does not depend on the order of
    ``support``'s rows.  A point with more than 2^20 support points within ``radius`` gets the zero normal and zero
    eigenvalues (the sums could overflow; its count is still exact).  As for ``cloud_nearest``, the time grows with
    (support points per cell) x (cells visited, 27 almost always): a ``radius`` far above the sampling distance is
    quadratic within a neighbourhood, and a finite support point more than 2^20 cells of ``radius`` from the origin
    raises ValueError.  Everything is validated here, before any launch; the one host synchronisation is the read of
    the index build's status word, after everything is enqueued."""
    check_cloud("points", points)
    own = support is None
    if own:
        support = points
    check_cloud("support", support)
    dev = points.device
    if support.device != dev:
        raise ValueError(f"support is on {support.device}, points on {dev}")
    h, inv, r2 = cloud_radius_scalars(radius, "radius")
    N, M = int(points.shape[0]), int(support.shape[0])
    k = _integer_in(min_neighbours, "min_neighbours", 3, 2 ** 62)
    try:
        gap = float(min_gap)
    except (TypeError, ValueError):
        raise ValueError(f"min_gap must be a number in [0, 1), got {min_gap!r}") from None
    if not 0.0 <= gap < 1.0:
        raise ValueError(f"min_gap must be a number in [0, 1), got {min_gap!r}")
    view = _check_viewpoint(viewpoint, N, dev)
    if N == 0 or M == 0:               # no neighbourhood, nothing to launch
        return CloudNormals(torch.zeros((N, 3), dtype=torch.float32, device=dev),
                            torch.zeros((N, 3), dtype=torch.float32, device=dev),
                            torch.zeros((N,), dtype=torch.int32, device=dev))
    _require_hip("cloud_normals", points)
    lib = _native.load()
    q = points.detach().contiguous()
    t = q if own else support.detach().contiguous()
    if view is not None:
        view = view.to(dev).contiguous()
    rows = 0 if view is None else int(view.shape[0])
    out = CloudNormals(torch.empty((N, 3), dtype=torch.float32, device=dev),
                       torch.empty((N, 3), dtype=torch.float32, device=dev),
                       torch.empty((N,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        st = _native.stream()
        ws, ws_bytes, status = _cloud_index_build(lib, t, M, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_normals(_native.ptr(q), N, _native.ptr(view), rows, float(h), float(inv), float(r2),
                                             k, gap, _native.ptr(ws), ws_bytes, M, _native.ptr(out.normals),
                                             _native.ptr(out.eigenvalues), _native.ptr(out.count), st),
                      "mvsn_cloud_normals")
        bits = int(status.item())      # the one host synchronisation, after everything is enqueued
    _raise_cloud_status(bits, h, "cloud_normals")   # (cloud_nearest's errors: the support is the index's target, radius its max_dist)
    return out


class CloudRegistration(NamedTuple):
    T: torch.Tensor                  # (4,4) fp32: source coordinates -> the target's frame, each number rounded once
    history: torch.Tensor            # (iterations+1,3) fp64: (count, sum w, sum w r^2) before update i; the last row at T
    status: torch.Tensor             # () int32: 0, 1 = fewer than min_points took part, 2 = the normal matrix was singular
    information: torch.Tensor        # (6,6) fp64: H = sum w J J^T at T


def _integer_in(value, name, lo, hi):
    try:
        i = int(value)
        if i != value or isinstance(value, bool):
            raise TypeError
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{name} must be an integer, got {value!r}") from None
    if i < lo or i > hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {value!r}")
    return i


def _pose_f32(T, name, dev):
    """``T`` as a contiguous (4,4) float32 tensor on ``dev``; ValueError unless it is a finite (4,4) floating-point
    tensor.  Its values are looked at where it lives: pass a host tensor and nothing waits for the device."""
    if not torch.is_tensor(T) or tuple(T.shape) != (4, 4):
        raise ValueError(f"{name} must be a (4,4) tensor")
    if not T.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {T.dtype}")
    if T.device.type == "meta":
        raise ValueError(f"{name} is on {T.device}")
    T32 = T.detach().to(torch.float32)
    if not bool(torch.isfinite(T32).all()):
        raise ValueError(f"{name} must be finite (as float32)")
    return T32.to(dev).contiguous()


def _check_register(source, target, max_dist, target_normals, weights, centre):
    """The validation ``cloud_register`` and ``cloud_register_system`` share: (N, M, dev, h, inv, r2, centre) with centre
    None (the default: the target's mean) or three np.float32."""
    check_cloud("source", source)
    check_cloud("target", target)
    dev = source.device
    if target.device != dev:
        raise ValueError(f"target is on {target.device}, source on {dev}")
    N, M = int(source.shape[0]), int(target.shape[0])
    if target_normals is not None:
        if not torch.is_tensor(target_normals) or tuple(target_normals.shape) != (M, 3) or \
                target_normals.dtype != torch.float32:
            raise ValueError(f"target_normals must be a ({M},3) float32 tensor")
        if target_normals.device != dev:
            raise ValueError(f"target_normals is on {target_normals.device}, source on {dev}")
    if weights is not None:
        if not torch.is_tensor(weights) or tuple(weights.shape) != (N,) or weights.dtype != torch.float32:
            raise ValueError(f"weights must be a ({N},) float32 tensor")
        if weights.device != dev:
            raise ValueError(f"weights is on {weights.device}, source on {dev}")
    h, inv, r2 = cloud_radius_scalars(max_dist)
    c = None
    if centre is not None:
        try:
            if torch.is_tensor(centre):
                if centre.device.type == "meta":
                    raise TypeError
                centre = centre.detach().cpu().numpy()
            with np.errstate(all="ignore"):
                c = np.asarray(centre, dtype=np.float64).astype(np.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"centre must be three finite numbers, got {centre!r}") from None
        if c.shape != (3,) or not np.isfinite(c).all():
            raise ValueError(f"centre must be three finite numbers (as float32), got {centre!r}")
    return N, M, dev, h, inv, r2, c


def _register_centre(c, target, dev):
    """(3,) float32 on ``dev``: the given centre, or the fp64 mean of the finite rows of ``target`` rounded once (formed
    on the device, nothing read back; (0,0,0) where no row is finite)."""
    if c is not None:
        return torch.from_numpy(c).to(dev)
    t = target.detach()
    ok = torch.isfinite(t).all(dim=1, keepdim=True)
    total = torch.where(ok, t, torch.zeros((), dtype=t.dtype, device=dev)).to(torch.float64).sum(dim=0)
    return (total / ok.sum().clamp(min=1).to(torch.float64)).to(torch.float32).contiguous()


def cloud_register_system(source: torch.Tensor, target: torch.Tensor, max_dist: float, T: torch.Tensor, *,
                          target_normals: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                          centre=None, with_matches: bool = False):
    """One evaluation of what ``cloud_register`` iterates, at the float32 values of ``T``:
    ``(H (6,6) fp64, b (6,) fp64, count () int64, sum_w () fp64, sum_w_r2 () fp64, index, residual)`` with
    H = sum w J J^T and b = sum w J r over the source points that take part.  With ``with_matches``, ``index`` (N,) int64
    is the matched target row and ``residual`` (N,) fp32 is r (point-to-plane) or the squared distance (point-to-point);
    -1 and NaN where the point takes no part; both None without.  The covariance of the pose is H^-1 times the noise
    scale."""
    N, M, dev, h, inv, r2, c = _check_register(source, target, max_dist, target_normals, weights, centre)
    T32 = _pose_f32(T, "T", dev)
    f64 = dict(dtype=torch.float64, device=dev)
    if N == 0 or M == 0:               # nothing to match, nothing to launch
        index = torch.full((N,), -1, dtype=torch.int64, device=dev) if with_matches else None
        res = torch.full((N,), float("nan"), dtype=torch.float32, device=dev) if with_matches else None
        return (torch.zeros((6, 6), **f64), torch.zeros((6,), **f64), torch.zeros((), dtype=torch.int64, device=dev),
                torch.zeros((), **f64), torch.zeros((), **f64), index, res)
    _require_hip("cloud_register_system", source)
    lib = _native.load()
    s, t = source.detach().contiguous(), target.detach().contiguous()
    nm = target_normals.detach().contiguous() if target_normals is not None else None
    wt = weights.detach().contiguous() if weights is not None else None
    cen = _register_centre(c, t, dev)
    ws_bytes = lib.mvsn_cloud_register_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    Hm, b, sums = torch.empty((6, 6), **f64), torch.empty((6,), **f64), torch.empty((3,), **f64)
    index = torch.empty((N,), dtype=torch.int64, device=dev) if with_matches else None
    res = torch.empty((N,), dtype=torch.float32, device=dev) if with_matches else None
    with torch.cuda.device(dev):
        st = _native.stream()
        idx_ws, idx_bytes, status = _cloud_index_build(lib, t, M, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_register_system(
            _native.ptr(s), N, _native.ptr(wt), _native.ptr(t), _native.ptr(nm), M, float(inv), float(r2),
            _native.ptr(idx_ws), idx_bytes, _native.ptr(T32), _native.ptr(cen), _native.ptr(ws), ws_bytes, _native.ptr(Hm),
            _native.ptr(b), _native.ptr(sums), _native.ptr(index), _native.ptr(res), st), "mvsn_cloud_register_system")
        bits = int(status.item())      # the one host synchronisation
    _raise_cloud_status(bits, h, "cloud_register_system")
    return Hm, b, sums[0].to(torch.int64), sums[1].clone(), sums[2].clone(), index, res


def cloud_register(source: torch.Tensor, target: torch.Tensor, max_dist: float, *,
                   target_normals: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                   T_init: Optional[torch.Tensor] = None, centre=None, iterations: int = 20, min_points: int = 6,
                   min_pivot: float = 1e-9) -> CloudRegistration:
    """Register ``source`` (N,3) fp32 to ``target`` (M,3) fp32 (ICP; DESIGN.md section 20, csrc/mvsn_cloud_register.hip):
    the rigid ``T`` with p' = R p + t that brings the source points onto their nearest target points within
    ``max_dist``, by ``iterations`` Gauss-Newton steps from ``T_init`` (the identity by default).

    With ``target_normals`` (M,3) fp32 the residual is point-to-plane, r = (p' - target_j) . n_j; without, point-to-point,
    the three differences.  The match j of a source point is exactly ``cloud_nearest(p', target, max_dist)``; a point
    takes part iff its row and p' are finite, its weight (``weights`` (N,) fp32, 1 without) is finite and > 0, it has a
    match and, in plane mode, the match's normal is finite.  ``centre`` (three numbers or a (3,) tensor) is the point the
    rotation update turns about; the default is the mean of the target's finite rows, formed on the device.

    Every iteration forms H = sum w J J^T and b = sum w J r in fp64 in a fixed order (bitwise reproducible), solves
    H (v, omega) = -b through a Jacobi-scaled Cholesky factor and applies R <- exp([omega]x) R,
    t <- exp([omega]x) (t - c) + c + v to the fp64 pose.  The run stops, keeping its pose, with status 1 when fewer
    than ``min_points`` points take part and with status 2 when H has a diagonal entry that is not positive and finite
    or a scaled pivot below ``min_pivot``; ``history`` rows then repeat.  ``cloud_register_system(..., T=result.T)``
    reproduces the last history row and ``information`` bit for bit.  Point-to-plane converges in a few iterations from
    a start within ``max_dist``; point-to-point lowers the distances every step but slides along surfaces slowly.

    Everything is validated here, before any launch; ``T_init`` and ``centre`` are checked where they live (pass host
    tensors and nothing waits for the device).  The one host synchronisation is the read of the index build's status
    word, after the whole loop is enqueued."""
    N, M, dev, h, inv, r2, c = _check_register(source, target, max_dist, target_normals, weights, centre)
    it = _integer_in(iterations, "iterations", 0, 1000)
    mp = _integer_in(min_points, "min_points", 1, 2 ** 62)
    try:
        pv = float(min_pivot)
    except (TypeError, ValueError):
        raise ValueError(f"min_pivot must be a number inside (0, 1), got {min_pivot!r}") from None
    if not 0.0 < pv < 1.0:
        raise ValueError(f"min_pivot must be a number inside (0, 1), got {min_pivot!r}")
    T32 = _pose_f32(torch.eye(4, dtype=torch.float32) if T_init is None else T_init, "T_init", dev)
    f64 = dict(dtype=torch.float64, device=dev)
    if N == 0 or M == 0:               # nothing to match, nothing to launch: the run stops at once
        return CloudRegistration(T32.clone(), torch.zeros((it + 1, 3), **f64),
                                 torch.ones((), dtype=torch.int32, device=dev), torch.zeros((6, 6), **f64))
    _require_hip("cloud_register", source)
    lib = _native.load()
    s, t = source.detach().contiguous(), target.detach().contiguous()
    nm = target_normals.detach().contiguous() if target_normals is not None else None
    wt = weights.detach().contiguous() if weights is not None else None
    cen = _register_centre(c, t, dev)
    ws_bytes = lib.mvsn_cloud_register_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    run = torch.empty(1, dtype=torch.int32, device=dev)
    out = CloudRegistration(torch.empty((4, 4), dtype=torch.float32, device=dev), torch.empty((it + 1, 3), **f64),
                            run[0], torch.empty((6, 6), **f64))
    with torch.cuda.device(dev):
        st = _native.stream()
        idx_ws, idx_bytes, status = _cloud_index_build(lib, t, M, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_register(
            _native.ptr(s), N, _native.ptr(wt), _native.ptr(t), _native.ptr(nm), M, float(inv), float(r2),
            _native.ptr(idx_ws), idx_bytes, _native.ptr(T32), _native.ptr(cen), it, mp, pv, _native.ptr(ws), ws_bytes,
            _native.ptr(out.T), _native.ptr(out.history), _native.ptr(run), _native.ptr(out.information), st),
            "mvsn_cloud_register")
        bits = int(status.item())      # the one host synchronisation, after the whole loop is enqueued
    _raise_cloud_status(bits, h, "cloud_register")
    return out


def radius_outlier_mask(points: torch.Tensor, radius: float, min_neighbours: int) -> torch.Tensor:
    """(N,) bool: True where at least ``min_neighbours`` OTHER points of ``points`` (N,3) fp32 lie within ``radius``
    (``cloud_nearest`` of the cloud against itself; the point itself is not counted, its exact duplicates are).  A
    point with a non-finite coordinate gets False."""
    try:
        k = int(min_neighbours)
        if k != min_neighbours or isinstance(min_neighbours, bool):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"min_neighbours must be an integer, got {min_neighbours!r}") from None
    check_cloud("points", points)
    cloud_radius_scalars(radius, "radius")
    if int(points.shape[0]) == 0:
        return torch.zeros((0,), dtype=torch.bool, device=points.device)
    nn = cloud_nearest(points, points, radius)
    return (nn.within - 1 >= k) & torch.isfinite(points).all(dim=1)


class CloudKNN(NamedTuple):
    dist2: torch.Tensor              # (N,k) fp32: squared distances to the k nearest target points, ascending; +inf past the last
    index: torch.Tensor              # (N,k) int64: their rows, -1 past the last
    within: torch.Tensor             # (N,) int32: number of candidates (target points within max_dist, less the point itself with exclude_self)


class CloudOutliers(NamedTuple):
    keep: torch.Tensor               # (N,) bool: mean_dist <= mean + std_ratio * std
    mean_dist: torch.Tensor          # (N,) fp64: mean distance to the k nearest other points, NaN with fewer than k within max_dist
    mean: torch.Tensor               # () fp64, on the device: mean of mean_dist over the points that have one
    std: torch.Tensor                # () fp64, on the device: their sample standard deviation


CLOUD_KNN_MAX = 64


def _check_knn(query, target, k, max_dist, exclude_self, names=("query", "target")):
    """The validation of ``cloud_knn``: (N, T, dev, k, h, inv, r2)."""
    check_cloud(names[0], query)
    check_cloud(names[1], target)
    if query.device != target.device:
        raise ValueError(f"{names[0]} is on {query.device}, {names[1]} on {target.device}")
    h, inv, r2 = cloud_radius_scalars(max_dist)
    kk = _integer_in(k, "k", 1, CLOUD_KNN_MAX)
    N, T = int(query.shape[0]), int(target.shape[0])
    if exclude_self and N != T:
        raise ValueError(f"exclude_self needs query and target to be the same cloud: {N} query rows, {T} target rows")
    return N, T, query.device, kk, h, inv, r2


def _cloud_knn(who, query, target, N, T, dev, k, h, inv, r2, exclude_self, with_mean):
    """(CloudKNN, mean (N,) fp64 or None): the launches of ``cloud_knn`` after its validation."""
    if N == 0 or T == 0:               # nothing to find, nothing to launch
        out = CloudKNN(torch.full((N, k), float("inf"), dtype=torch.float32, device=dev),
                       torch.full((N, k), -1, dtype=torch.int64, device=dev),
                       torch.zeros((N,), dtype=torch.int32, device=dev))
        return out, (torch.full((N,), float("nan"), dtype=torch.float64, device=dev) if with_mean else None)
    _require_hip(who, query)
    lib = _native.load()
    q = query.detach().contiguous()
    t = q if target is query else target.detach().contiguous()
    out = CloudKNN(torch.empty((N, k), dtype=torch.float32, device=dev),
                   torch.empty((N, k), dtype=torch.int64, device=dev),
                   torch.empty((N,), dtype=torch.int32, device=dev))
    mean = torch.empty((N,), dtype=torch.float64, device=dev) if with_mean else None
    with torch.cuda.device(dev):
        st = _native.stream()
        ws, ws_bytes, status = _cloud_index_build(lib, t, T, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_knn(_native.ptr(q), N, k, 1 if exclude_self else 0, float(h), float(inv), float(r2),
                                         _native.ptr(ws), ws_bytes, T, _native.ptr(out.dist2), _native.ptr(out.index),
                                         _native.ptr(out.within), _native.ptr(mean), st), "mvsn_cloud_knn")
        bits = int(status.item())      # the one host synchronisation, after the query is enqueued
    _raise_cloud_status(bits, h, who)
    return out, mean


def cloud_knn(query: torch.Tensor, target: torch.Tensor, k: int, max_dist: float = None, *,
              exclude_self: bool = False) -> CloudKNN:
    """For every row of ``query`` (N,3) fp32 the ``k`` (1 to 64) nearest rows of ``target`` (T,3) fp32 within
    ``max_dist`` (PCL's and Open3D's hybrid search; DESIGN.md section 22, csrc/mvsn_cloud_knn.hip): their squared
    distances in ascending order, their rows, and how many candidates there were.  Neither cloud needs any order.

    A target is a candidate exactly when ``cloud_nearest`` counts it: ``(dx*dx + dy*dy) + dz*dz <= h*h`` of the fp32
    differences with h = float32(max_dist).  With ``exclude_self`` (``query`` and ``target`` must then have the same
    number of rows: the same cloud) the target row equal to the query's row is no candidate; its exact duplicates are.
    Ties in the distance go to the lowest target row.  The result is exactly that of the brute force over every target
    point and a stable sort on (distance, row): it is a bitwise-reproducible function of the inputs, and permuting the
    target's rows changes nothing but the rows reported.  Slots from the number of candidates on hold (+inf, -1).
    ``cloud_knn(q, t, 1, h)`` is ``cloud_nearest(q, t, h)`` bit for bit.  A target with a non-finite coordinate is
    nobody's neighbour, a query with one gets all (+inf, -1) and 0, and a query may lie anywhere.

    As for ``cloud_nearest``, the time grows with (targets per cell) x (cells visited, 27 almost always): a ``max_dist``
    far above the sampling distance is quadratic within a neighbourhood, and a finite target more than 2^20 cells of
    ``max_dist`` from the origin raises ValueError.  ``max_dist`` is required: leaving it out is a ValueError like any
    other bad radius.  Everything is validated here, before any launch; the one host synchronisation is the read of the
    index build's status word, after the query is enqueued."""
    N, T, dev, kk, h, inv, r2 = _check_knn(query, target, k, max_dist, exclude_self)
    return _cloud_knn("cloud_knn", query, target, N, T, dev, kk, h, inv, r2, bool(exclude_self), False)[0]


def statistical_outlier_mask(points: torch.Tensor, k: int, std_ratio: float, max_dist: float = None) -> CloudOutliers:
    """The statistical outlier filter of PCL (``StatisticalOutlierRemoval``) and Open3D (``remove_statistical_outlier``)
    on ``points`` (N,3) fp32: ``mean_dist`` is every point's mean distance to its ``k`` (1 to 64) nearest OTHER points
    (``cloud_knn(points, points, k, max_dist, exclude_self=True)``: exact duplicates count, at distance 0, as in
    ``radius_outlier_mask``), ``mean`` and ``std`` are the mean and the sample standard deviation of ``mean_dist`` over
    the cloud, and ``keep = mean_dist <= mean + std_ratio * std`` (``std_ratio`` a finite number >= 0).  Unlike
    ``radius_outlier_mask`` the threshold follows the cloud's own spacing.

    A point with fewer than ``k`` other points within ``max_dist``, or with a non-finite coordinate, has ``mean_dist``
    NaN: it gets ``keep`` False and enters neither ``mean`` nor ``std``.  ``max_dist`` bounds the search (and its cost,
    as for ``cloud_nearest``); choose it several times the spacing of the sparsest part that should be kept.

    ``mean_dist`` is the fp64 sum of the k fp64 square roots in order of distance, over k; ``mean`` and ``std`` are
    two-pass fp64 sums in an order that N alone fixes; the comparison runs on the device in fp64.  Nothing is read on
    the host but the index build's status word: every output is a bitwise-reproducible function of the inputs.
    Everything is validated here, before any launch."""
    N, _, dev, kk, h, inv, r2 = _check_knn(points, points, k, max_dist, True, names=("points", "points"))
    try:
        ratio = float(std_ratio)
        if isinstance(std_ratio, (bool, str)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"std_ratio must be a finite number >= 0, got {std_ratio!r}") from None
    if not (np.isfinite(ratio) and ratio >= 0.0):
        raise ValueError(f"std_ratio must be a finite number >= 0, got {std_ratio!r}")
    if N == 0:
        return CloudOutliers(torch.zeros((0,), dtype=torch.bool, device=dev),
                             torch.zeros((0,), dtype=torch.float64, device=dev),
                             torch.full((), float("nan"), dtype=torch.float64, device=dev),
                             torch.zeros((), dtype=torch.float64, device=dev))
    _, mean_dist = _cloud_knn("statistical_outlier_mask", points, points, N, N, dev, kk, h, inv, r2, True, True)
    lib = _native.load()
    ws_bytes = lib.mvsn_cloud_mean_stats_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stats = torch.empty((3,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_cloud_mean_stats(_native.ptr(mean_dist), N, _native.ptr(ws), ws_bytes, _native.ptr(stats),
                                                _native.stream()), "mvsn_cloud_mean_stats")
    keep = mean_dist <= stats[1] + ratio * stats[2]          # (a NaN compares false)
    return CloudOutliers(keep, mean_dist, stats[1], stats[2])


class CloudClusters(NamedTuple):
    label: torch.Tensor              # (N,) int64: cluster id of every point, -1 for noise
    core: torch.Tensor               # (N,) bool: a finite point with at least min_points points within eps, itself included
    within: torch.Tensor             # (N,) int32: points within eps of the point, itself included (cloud_nearest's `within`)
    count: torch.Tensor              # (C,) int64: points per cluster, border points included
    core_count: torch.Tensor         # (C,) int64: core points per cluster
    first: torch.Tensor              # (C,) int64: lowest core row of each cluster, ascending


CLUSTER_STATUS_WORKSPACE = 1


def cloud_clusters(points: torch.Tensor, eps: float, min_points: int) -> CloudClusters:
    """The density-based clusters (DBSCAN: Open3D's ``cluster_dbscan``, scikit-learn's ``DBSCAN``) of ``points`` (N,3)
    fp32, and with ``min_points=1`` its Euclidean clusters (PCL's ``EuclideanClusterExtraction``); DESIGN.md section
    24, csrc/mvsn_cloud_cluster.hip.  The cloud needs no order.

    Row j is a *neighbour* of row i exactly when ``cloud_nearest(points, points, eps)`` counts it: both rows finite and
    ``(dx*dx + dy*dy) + dz*dz <= h*h`` of the fp32 differences with h = float32(eps).  A point is its own neighbour,
    exact duplicates are neighbours at distance 0, and the relation is symmetric bit for bit.  A point is *core* when
    ``within >= min_points`` (``min_points`` an integer >= 1; the point itself is counted, as in Open3D and
    scikit-learn).  A *cluster* is a connected component of the graph on the core points whose edges are the neighbour
    relation.  A finite point that is not core but has a core neighbour is a *border* point and joins the cluster of its
    nearest core neighbour, ties in the distance to the lowest row (the minimum of (d2 bits, row), the tie rule of
    ``cloud_nearest``): a border point never connects two clusters, and which cluster it joins is a function of the
    input, not of a visiting order.  Every other point, and every row with a non-finite coordinate, is *noise*: label
    -1, never core, nobody's neighbour.  Cluster ids are dense, 0..C-1, ordered by ``first``, the lowest core row of
    the cluster; C may be 0.  ``count`` includes the border points; ``within`` is ``cloud_nearest``'s bit for bit.

    Every output is a bitwise-reproducible function of the inputs: integer work on top of the exact radius query, and
    permuting the rows permutes ``core`` and ``within`` and leaves the partition alone (but for border points at
    exactly tied distances).  N = 0 gives empties without a launch.  The time is ``cloud_nearest``'s, (points per cell)
    x (cells visited, 27 almost always), paid three times, plus the unions: keep ``eps`` at a few sampling distances;
    far above them it is quadratic within a neighbourhood.  A finite point more than 2^20 cells of ``eps`` from the
    origin raises ValueError.  Everything is validated here, before any launch; the one host synchronisation is the
    read of (C, the union-find's status, the index build's status) that sizes the outputs."""
    check_cloud("points", points)
    h, inv, r2 = cloud_radius_scalars(eps, "eps")
    k = _integer_in(min_points, "min_points", 1, 2 ** 31 - 1)
    N, dev = int(points.shape[0]), points.device
    i64 = dict(dtype=torch.int64, device=dev)
    if N == 0:                         # no point, no cluster, nothing to launch
        return CloudClusters(torch.empty((0,), **i64), torch.empty((0,), dtype=torch.bool, device=dev),
                             torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), **i64),
                             torch.empty((0,), **i64), torch.empty((0,), **i64))
    _require_hip("cloud_clusters", points, "cloud")
    lib = _native.load()
    p = points.detach().contiguous()
    ws_bytes = lib.mvsn_cloud_cluster_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    head = torch.empty(3, **i64)       # (C, the union-find's status, the index build's status)
    within = torch.empty((N,), dtype=torch.int32, device=dev)
    core = torch.empty((N,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _native.stream()
        index_ws, index_bytes, _ = _cloud_index_build(lib, p, N, h, inv, dev, st, status=head[2:])
        _native.check(lib.mvsn_cloud_cluster_label(_native.ptr(p), N, float(inv), float(r2), k, _native.ptr(index_ws),
                                                   index_bytes, _native.ptr(within), _native.ptr(core), _native.ptr(head),
                                                   _native.ptr(ws), ws_bytes, st), "mvsn_cloud_cluster_label")
        c, status, bits = head.tolist()    # the one host synchronisation: sizes the outputs
        _raise_cloud_status(bits, h, "cloud_clusters")     # (eps is the index's max_dist, the cloud its target)
        if status != 0 or not 0 <= c <= N:
            raise RuntimeError(f"cloud_clusters: the union-find did not finish (status {status}, {c} clusters of {N} "
                               "points): its workspace was overwritten during the call")
        out = CloudClusters(torch.empty((N,), **i64), core.view(torch.bool), within, torch.empty((c,), **i64),
                            torch.empty((c,), **i64), torch.empty((c,), **i64))
        _native.check(lib.mvsn_cloud_cluster_emit(
            _native.ptr(p), N, float(inv), float(r2), _native.ptr(index_ws), index_bytes, _native.ptr(core), _native.ptr(ws),
            ws_bytes, c, _native.ptr(out.label), _native.ptr(out.count) if c else None,
            _native.ptr(out.core_count) if c else None, _native.ptr(out.first) if c else None, st),
            "mvsn_cloud_cluster_emit")
    return out


def _check_clusters(clusters):
    """(N, C, dev) of a well-formed ``CloudClusters``; ValueError for anything else."""
    if not isinstance(clusters, tuple) or len(clusters) != 6:
        raise ValueError("clusters must be a CloudClusters (label, core, within, count, core_count, first)")
    label, count = clusters[0], clusters[3]
    if not torch.is_tensor(label) or label.dim() != 1:
        raise ValueError("clusters.label must be a (N,) int64 tensor")
    n, dev = int(label.shape[0]), label.device
    c = int(count.shape[0]) if torch.is_tensor(count) and count.dim() == 1 else -1
    dtypes = (torch.int64, torch.bool, torch.int32, torch.int64, torch.int64, torch.int64)
    for name, t, size, dtype in zip(CloudClusters._fields, clusters, (n, n, n, c, c, c), dtypes):
        if not torch.is_tensor(t) or tuple(t.shape) != (size,) or t.dtype != dtype:
            raise ValueError(f"clusters.{name} must be a ({max(size, 0)},) {dtype} tensor of this cloud")
        if t.device != dev:
            raise ValueError(f"clusters.{name} is on {t.device}, clusters.label on {dev}")
    if c > n:
        raise ValueError(f"clusters holds {c} clusters for a cloud of {n} points")
    return n, c, dev


def cloud_cluster_mask(clusters: CloudClusters, *, min_size: Optional[int] = None, keep_largest: Optional[int] = None,
                       keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N,) bool: the points of the clusters of ``clusters`` (what ``cloud_clusters`` returned) one keeps, by
    ``filter_mesh``'s rules on ``count``.  A cluster is kept when ``count >= min_size`` (if given) and, with
    ``keep_largest`` = k, it is among the k largest of those that passed, by a stable descending sort: ties go to the
    lower id.  ``keep``, a (C,) bool tensor, replaces both (combining it with one of them, or giving none of the three,
    is a ValueError).  Noise is always False.  ``points[mask]`` is the cloud without its floaters.  Torch operations on
    the tensors' own device, no host read."""
    n, c, dev = _check_clusters(clusters)
    rules = [r is not None for r in (min_size, keep_largest)]
    if keep is not None and any(rules):
        raise ValueError("keep replaces min_size and keep_largest: give it alone")
    if keep is None and not any(rules):
        raise ValueError("give one of min_size, keep_largest or keep")
    lo = _integer_in(min_size, "min_size", 0, 2 ** 63 - 1) if min_size is not None else None
    top = _integer_in(keep_largest, "keep_largest", 0, 2 ** 63 - 1) if keep_largest is not None else None
    if keep is not None:
        if not torch.is_tensor(keep) or tuple(keep.shape) != (c,) or keep.dtype != torch.bool:
            raise ValueError(f"keep must be a ({c},) bool tensor, one entry per cluster")
        if keep.device != dev:
            raise ValueError(f"keep is on {keep.device}, the clusters on {dev}")
    if c == 0:                         # no cluster: every point is noise
        return torch.zeros((n,), dtype=torch.bool, device=dev)
    if keep is None:
        keep = torch.ones((c,), dtype=torch.bool, device=dev)
        if lo is not None:
            keep &= clusters.count >= lo
        if top is not None:
            # the passed clusters by falling size, a stable sort: ties keep the order of the ids
            order = torch.argsort(torch.where(keep, clusters.count, -1), descending=True, stable=True)
            among = torch.zeros_like(keep)
            among[order[:top]] = True
            keep &= among
    label = clusters.label
    return (label >= 0) & (label < c) & keep[label.clamp(0, c - 1)]


class CloudRender(NamedTuple):
    depth: torch.Tensor              # (V,1,H,W) fp32: z-depth of the nearest point per pixel, 0 where no point hit
    index: torch.Tensor              # (V,H,W) int64: that point's row, -1 where none
    colors: Optional[torch.Tensor]   # (V,3,H,W) uint8: its colour (zeros where none), or None without colors
    normals: Optional[torch.Tensor]  # (V,3,H,W) fp32: its normal (zeros where none), or None without normals


class CloudVisibility(NamedTuple):
    visible: torch.Tensor            # (N,V) bool: view v sees point i
    count: torch.Tensor              # (N,) int32: the views that see the point
    values: Optional[torch.Tensor]   # (N,C) fp32: the mean of maps over those views (0 where none), or None without maps


RENDER_MAX_RADIUS = 8
VISIBILITY_MAX_CHANNELS = 16
_RENDER_MAX_EXTENT, _RENDER_MAX_PIXELS, _RENDER_MAX_VIEWS = 2 ** 24, 2 ** 31 - 1, 65535


def _depth_limit_f32(value, name, *, infinite=False, positive=False):
    """``value`` as np.float32: a finite number >= 0 (> 0 with ``positive``; +inf allowed with ``infinite``);
    ValueError for anything else, a NaN included."""
    what = f"{name} must be a {'number > 0 (inf: no limit)' if positive else 'finite number >= 0'}, got {value!r}"
    if isinstance(value, (bool, str)) or value is None:
        raise ValueError(what)
    with np.errstate(all="ignore"):
        try:
            v = np.float32(value)
        except (TypeError, ValueError):
            raise ValueError(what) from None
    if np.ndim(v) != 0 or not (v > 0 if positive else v >= 0) or (not infinite and not np.isfinite(v)):
        raise ValueError(what)
    return v


def _check_render_cameras(K, T_cam_in_world, dev, what):
    """V of the (V,4,4) floating-point tensors ``K`` and ``T_cam_in_world`` on ``dev``, 1 <= V <= 65535."""
    if not torch.is_tensor(K) or K.dim() != 3 or tuple(K.shape[1:]) != (4, 4):
        raise ValueError("K must be a (V,4,4) tensor")
    V = int(K.shape[0])
    if not 1 <= V <= _RENDER_MAX_VIEWS:
        raise ValueError(f"1..65535 views, got {V}")
    for name, m in (("K", K), ("T_cam_in_world", T_cam_in_world)):
        if not torch.is_tensor(m) or tuple(m.shape) != (V, 4, 4):
            raise ValueError(f"{name} must be a ({V},4,4) tensor")
        if not m.is_floating_point():
            raise ValueError(f"{name} must be a floating-point tensor, got {m.dtype}")
        if m.device != dev:
            raise ValueError(f"{name} is on {m.device}, {what} on {dev}")
    return V


def _check_rows(name, t, N, dtype, dev):
    if not torch.is_tensor(t) or tuple(t.shape) != (N, 3) or t.dtype != dtype:
        raise ValueError(f"{name} must be a ({N},3) {dtype} tensor, one row per point")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, points on {dev}")


def cloud_render(points: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, size, *, radius: int = 0,
                 colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, min_depth: float = 0.0,
                 max_depth: float = float("inf")) -> CloudRender:
    """Render ``points`` (N,3) fp32 into the V cameras ``K``, ``T_cam_in_world`` (V,4,4) with maps of ``size`` = (H,W):
    per pixel the z-depth and the row of the nearest point that lands on it, and that point's ``colors`` (N,3) uint8 and
    ``normals`` (N,3) fp32 if given; DESIGN.md section 25, csrc/mvsn_cloud_render.hip.  The cloud needs no order.

    The camera is ``TSDFVolume.integrate``'s: P = K T^-1 formed in fp64 from the float32 values and rounded once, z = P
    row 2 . (p,1), the pixel (c, r) = floor((u, v) + 0.5) with (u, v) = rows 0, 1 over z, every step one fp32 operation.
    A point takes part in a view when its coordinates and z are finite, ``min_depth`` < z <= ``max_depth`` and its pixel
    is within ``radius`` of the map; it covers the flat, screen-aligned square of 2 ``radius`` + 1 pixels around its
    pixel, clipped to the map.  A pixel takes the least (z, row) of the points that cover it: the nearest point, a tie
    on z to the lowest row.  ``radius=0`` is the exact point render; ``radius`` up to 8 closes the holes between the
    points through which a farther surface would show, at a price: a covered neighbour pixel takes the point's own z, so
    a slanted surface comes forward by up to ``radius`` pixels' worth of its depth gradient and silhouettes grow by
    ``radius`` pixels.  Where no point lands the depth is 0, the index -1 and colour and normal are zero.

    Every output is a bitwise-reproducible function of the inputs whatever the order of the points: the only atomic is
    an integer minimum.  N = 0 gives the all-miss render without a launch.  Everything is validated here, before any
    launch; no host synchronisation."""
    check_cloud("points", points)
    N, dev = int(points.shape[0]), points.device
    V = _check_render_cameras(K, T_cam_in_world, dev, "points")
    try:
        H, W = (_integer_in(x, "size", 1, _RENDER_MAX_EXTENT) for x in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be two integers (H,W), each in [1, 2^24], got {size!r}") from None
    if H * W > _RENDER_MAX_PIXELS:
        raise ValueError(f"at most 2^31 - 1 pixels per map, got {H} x {W}")
    R = _integer_in(radius, "radius", 0, RENDER_MAX_RADIUS)
    if colors is not None:
        _check_rows("colors", colors, N, torch.uint8, dev)
    if normals is not None:
        _check_rows("normals", normals, N, torch.float32, dev)
    lo = _depth_limit_f32(min_depth, "min_depth")
    hi = _depth_limit_f32(max_depth, "max_depth", infinite=True, positive=True)
    if N == 0:                         # no point: every pixel is a miss, nothing to launch
        return CloudRender(torch.zeros((V, 1, H, W), dtype=torch.float32, device=dev),
                           torch.full((V, H, W), -1, dtype=torch.int64, device=dev),
                           torch.zeros((V, 3, H, W), dtype=torch.uint8, device=dev) if colors is not None else None,
                           torch.zeros((V, 3, H, W), dtype=torch.float32, device=dev) if normals is not None else None)
    if not points.is_cuda:
        raise RuntimeError("cloud_render runs on HIP devices only: move the cloud and the cameras to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
    dense = lambda t: t.detach().contiguous() if t is not None else None   # noqa: E731
    # (every converted copy is held until the launches are enqueued: a temporary's memory could be handed out again)
    p_c, col_c, nor_c, K_c, T_c = dense(points), dense(colors), dense(normals), f32(K), f32(T_cam_in_world)
    ws_bytes = lib.mvsn_cloud_render_workspace_bytes(V, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = CloudRender(torch.empty((V, 1, H, W), dtype=torch.float32, device=dev),
                      torch.empty((V, H, W), dtype=torch.int64, device=dev),
                      torch.empty((V, 3, H, W), dtype=torch.uint8, device=dev) if colors is not None else None,
                      torch.empty((V, 3, H, W), dtype=torch.float32, device=dev) if normals is not None else None)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_cloud_render(
            _native.ptr(p_c), N, _native.ptr(col_c), _native.ptr(nor_c), _native.ptr(K_c), _native.ptr(T_c), V, H, W, R,
            float(lo), float(hi), _native.ptr(ws), ws_bytes,
            _native.ptr(out.depth), _native.ptr(out.index), _native.ptr(out.colors), _native.ptr(out.normals),
            _native.stream()), "mvsn_cloud_render")
    return out


def cloud_visibility(points: torch.Tensor, depth: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, *,
                     rel_tol: float = 0.01, maps: Optional[torch.Tensor] = None,
                     min_depth: float = 0.0) -> CloudVisibility:
    """Which of the V views ``depth`` (V,1,H,W) fp32 with cameras ``K``, ``T_cam_in_world`` (V,4,4) sees each of
    ``points`` (N,3) fp32 (hidden-point removal), and with ``maps`` (V,C,H,W) fp32, 1 <= C <= 16, the mean of the maps at
    the point over the views that see it; DESIGN.md section 25, csrc/mvsn_cloud_render.hip.

    Point i is visible in view v when it takes part in ``cloud_render`` at ``radius=0`` (finite, z > ``min_depth``, its
    nearest pixel inside the map: the same fp32 steps, the same bits of z), the depth D at that pixel is finite and > 0
    and z <= fma(rel_tol, D, D) in fp32: the point is not behind what the view sees there, by more than ``rel_tol`` of
    it.  ``depth`` is any z-depth map: a render (with ``rel_tol=0`` every row in ``cloud_render(...).index[v]`` at
    ``radius=0`` is visible in v against that render's depth, exactly), the network's output, ``TSDFVolume.raycast``'s.
    ``values`` is the sum of ``maps[v, :, r, c]`` over the visible views in view order, plain fp32 additions, divided
    once by ``count``; 0 where no view sees the point.  The sample is the nearest pixel's, not a bilinear one, and a
    visible sample that is not finite is added like any other: mask the maps' holes in ``depth``.

    No atomics: every output is a bitwise-reproducible function of the inputs.  N = 0 gives empties without a launch.
    Everything is validated here, before the launch; no host synchronisation."""
    check_cloud("points", points)
    N = int(points.shape[0])

    def limits(V, H, W, dev):
        if V > _RENDER_MAX_VIEWS or H * W > _RENDER_MAX_PIXELS or max(H, W) > _RENDER_MAX_EXTENT:
            raise ValueError(f"at most 65535 views of 2^31 - 1 pixels and 2^24 rows or columns, got {V} of {H} x {W}")
        if dev != points.device:
            raise ValueError(f"depth is on {dev}, points on {points.device}")
    V, H, W, dev = _check_views(depth, K, T_cam_in_world, limits=limits, floating=True)
    C = None
    if maps is not None:
        if not torch.is_tensor(maps) or maps.dim() != 4 or not 1 <= maps.shape[1] <= VISIBILITY_MAX_CHANNELS:
            raise ValueError(f"maps must be a ({V},C,{H},{W}) tensor with 1 <= C <= {VISIBILITY_MAX_CHANNELS}")
        C = int(maps.shape[1])
        _check_frames("maps", maps, V, H, W, C, (torch.float32,), dev)
    tol = _depth_limit_f32(rel_tol, "rel_tol")
    lo = _depth_limit_f32(min_depth, "min_depth")
    if N == 0:                         # no point, nothing to launch
        return CloudVisibility(torch.empty((0, V), dtype=torch.bool, device=dev),
                               torch.empty((0,), dtype=torch.int32, device=dev),
                               torch.empty((0, C), dtype=torch.float32, device=dev) if C else None)
    if not points.is_cuda:
        raise RuntimeError("cloud_visibility runs on HIP devices only: move the cloud and the depth maps to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()   # noqa: E731
    # (every converted copy is held until the launch is enqueued: a temporary's memory could be handed out again)
    p_c, d_c, K_c, T_c = points.detach().contiguous(), depth.detach().contiguous(), f32(K), f32(T_cam_in_world)
    m_c = maps.detach().contiguous() if C else None
    visible = torch.empty((N, V), dtype=torch.uint8, device=dev)
    count = torch.empty((N,), dtype=torch.int32, device=dev)
    values = torch.empty((N, C), dtype=torch.float32, device=dev) if C else None
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_cloud_visibility(
            _native.ptr(p_c), N, _native.ptr(d_c), _native.ptr(m_c), C or 0, _native.ptr(K_c), _native.ptr(T_c), V, H, W,
            float(tol), float(lo), _native.ptr(visible), _native.ptr(count),
            _native.ptr(values), _native.stream()), "mvsn_cloud_visibility")
    return CloudVisibility(visible.view(torch.bool), count, values)


def cloud_colorize(points: torch.Tensor, images: torch.Tensor, depth: torch.Tensor, K: torch.Tensor,
                   T_cam_in_world: torch.Tensor, *, rel_tol: float = 0.01):
    """Colours for a bare cloud -- one that was merged, registered or read back from a file and has lost the pixels it
    came from: (colors (N,3) uint8, count (N,) int32).  ``cloud_visibility(points, depth, ..., maps=images)`` with
    ``images`` (V,3,H,W) fp32 in [-1,1], then the conversion ``fuse_depthmaps`` applies, rint((c + 1) * 127.5) in fp64
    clamped to 0..255: the mean colour over the views that see the point, so a point never takes the colour of what
    stands in front of it.  A point no view sees gets (0,0,0) and ``count`` 0."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("images must be a (V,3,H,W) tensor")
    vis = cloud_visibility(points, depth, K, T_cam_in_world, rel_tol=rel_tol, maps=images)
    q = torch.round((vis.values.to(torch.float64) + 1.0) * 127.5)         # (ties to even, as rint)
    q = torch.nan_to_num(q, nan=0.0).clamp_(0.0, 255.0)                  # (a NaN gives 0, as mvsn_fusion_emit's)
    q = torch.where((vis.count > 0)[:, None], q, torch.zeros_like(q))
    return q.to(torch.uint8), vis.count


class CloudFeatures(NamedTuple):
    features: torch.Tensor           # (N,33) fp32: the FPFH descriptor, each 11-bin block summing to 100; zero where undefined
    spfh: torch.Tensor               # (N,33) int32: the point's own pair histogram (f1's 11 bins, f2's, f3's)
    pairs: torch.Tensor              # (N,) int32: K_i, the number of pairs counted (the sum of each block of spfh)


class FeatureMatches(NamedTuple):
    index: torch.Tensor              # (Q,) int64: the nearest target row in descriptor space, -1 where none
    dist2: torch.Tensor              # (Q,) fp32: its squared descriptor distance, +inf where none
    second_dist2: torch.Tensor       # (Q,) fp32: the runner-up's, +inf where there is none (for a ratio test)
    mutual: Optional[torch.Tensor]   # (Q,) bool: the match's own nearest query row is this row; None unless asked


class CloudRansac(NamedTuple):
    T: torch.Tensor                  # (4,4) fp32: source coordinates -> the target's frame; the identity unless status is 0
    hypothesis: torch.Tensor         # () int64: the winning hypothesis, -1 where none
    inliers: torch.Tensor            # () int64: its number of inlier correspondences
    status: torch.Tensor             # () int64: 0, 1 = fewer than 3 usable correspondences, 2 = every hypothesis rejected
    inlier: torch.Tensor             # (C,) bool: the winner's inliers


class GlobalRegistration(NamedTuple):
    T: torch.Tensor                  # (4,4) fp32: the refined pose with refine, else the coarse one
    coarse: CloudRansac              # the RANSAC result
    correspondences: torch.Tensor    # (C,2) int64: (source row, target row) handed to RANSAC
    refined: Optional[CloudRegistration]   # cloud_register's result from coarse.T; None without refine


FEATURE_DIM = 33
RANSAC_MAX_HYPOTHESES = 2 ** 24


def _check_normals(normals, name, N, dev, what="points"):
    if not torch.is_tensor(normals) or tuple(normals.shape) != (N, 3) or normals.dtype != torch.float32:
        raise ValueError(f"{name} must be a ({N},3) float32 tensor")
    if normals.device != dev:
        raise ValueError(f"{name} is on {normals.device}, {what} on {dev}")


def _check_fpfh(points, normals, radius, min_neighbours, names=("points", "normals")):
    check_cloud(names[0], points)
    N, dev = int(points.shape[0]), points.device
    _check_normals(normals, names[1], N, dev, names[0])
    h, inv, r2 = cloud_radius_scalars(radius, "radius")
    return N, dev, h, inv, r2, _integer_in(min_neighbours, "min_neighbours", 1, 2 ** 62)


def cloud_fpfh(points: torch.Tensor, normals: torch.Tensor, radius: float, *, min_neighbours: int = 3) -> CloudFeatures:
    """The Fast Point Feature Histogram (Rusu et al., ICRA 2009; PCL's ``FPFHEstimation``, Open3D's
    ``compute_fpfh_feature``) of every row of ``points`` (N,3) fp32 with ``normals`` (N,3) fp32 from its neighbours
    within ``radius``: 33 bins, three blocks of 11 (csrc/mvsn_cloud_fpfh.hip).

    A neighbour j of i is one that ``cloud_nearest(points, points, radius)`` counts, other than i itself and not at
    distance 0, with both normals finite and not (0,0,0) (what ``cloud_normals`` writes where it is undefined).  ``spfh``
    holds the counts of the pair's three Darboux-frame features, each in 11 equal bins, and ``pairs`` their number K_i.
    ``features`` adds to the point's own histogram the mean of its neighbours' histograms, weighted by
    ``radius^2 / max(d^2, radius^2 2^-20)`` (scale-free, unlike the paper's 1/distance), and scales each block to sum 100;
    a point with ``K_i < min_neighbours`` (an integer >= 1), or with more than 2^20 neighbours, gets an all-zero row.

    Every step up to the bins is a single fp32 operation (no atan2: the angle's bin comes from sign tests), the counts
    and the weighted sums are exact integers, the rest is fp64 rounded to fp32 once: every output is a
    bitwise-reproducible function of the inputs, and permuting the rows permutes the outputs (a tie between the two
    angles of a pair, which goes to the lower row, aside).  As for ``cloud_nearest``, the time grows with (points per
    cell) x 27 cells, and a finite point more than 2^20 cells of ``radius`` from the origin raises ValueError.
    Everything is validated here, before any launch; the one host synchronisation is the read of the index build's
    status word, after everything is enqueued."""
    N, dev, h, inv, r2, k = _check_fpfh(points, normals, radius, min_neighbours)
    if N == 0:                         # no neighbourhood, nothing to launch
        return CloudFeatures(torch.zeros((0, FEATURE_DIM), dtype=torch.float32, device=dev),
                             torch.zeros((0, FEATURE_DIM), dtype=torch.int32, device=dev),
                             torch.zeros((0,), dtype=torch.int32, device=dev))
    _require_hip("cloud_fpfh", points)
    lib = _native.load()
    p, nm = points.detach().contiguous(), normals.detach().contiguous()
    out = CloudFeatures(torch.empty((N, FEATURE_DIM), dtype=torch.float32, device=dev),
                        torch.empty((N, FEATURE_DIM), dtype=torch.int32, device=dev),
                        torch.empty((N,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        st = _native.stream()
        ws, ws_bytes, status = _cloud_index_build(lib, p, N, h, inv, dev, st)
        _native.check(lib.mvsn_cloud_fpfh(_native.ptr(p), _native.ptr(nm), N, float(h), float(inv), float(r2), k,
                                          _native.ptr(ws), ws_bytes, _native.ptr(out.spfh), _native.ptr(out.pairs),
                                          _native.ptr(out.features), st), "mvsn_cloud_fpfh")
        bits = int(status.item())      # the one host synchronisation, after everything is enqueued
    _raise_cloud_status(bits, h, "cloud_fpfh")
    return out


def _check_features(name, t):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != FEATURE_DIM:
        raise ValueError(f"{name} must be an (N,{FEATURE_DIM}) tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if int(t.shape[0]) > 2 ** 31 - 1:
        raise ValueError(f"at most 2^31 - 1 {name} rows, got {int(t.shape[0])}")


def feature_nearest(query_features: torch.Tensor, target_features: torch.Tensor, *, mutual: bool = False) -> FeatureMatches:
    """For every row of ``query_features`` (Q,33) fp32 the nearest row of ``target_features`` (T,33) fp32 in descriptor
    space, by brute force (csrc/mvsn_cloud_match.hip): its row, its squared distance, and the
    squared distance of the runner-up (for a ratio test).

    The distance is ``sum_b (q_b - t_b)^2`` from b = 0 upwards, each step one fp32 operation; ties go to the lowest
    target row.  A row of either side takes part iff its 33 values are finite and not all zero (``cloud_fpfh`` writes
    zeros where the descriptor is undefined); a query row that takes no part, or finds no target, gets (-1, +inf, +inf).
    With ``mutual`` the same search runs with the roles swapped and ``mutual[i]`` says whether the match's own nearest
    query row is i.  Every output is a bitwise-reproducible function of the inputs; nothing is read on the host.  The
    time is Q x T x 33: meant for clouds merged to 10^4 - 10^5 points (``voxel_merge``)."""
    _check_features("query_features", query_features)
    _check_features("target_features", target_features)
    dev = query_features.device
    if target_features.device != dev:
        raise ValueError(f"query_features is on {dev}, target_features on {target_features.device}")
    Q, T = int(query_features.shape[0]), int(target_features.shape[0])
    want = bool(mutual)
    if Q == 0 or T == 0:               # nothing to find, nothing to launch
        return FeatureMatches(torch.full((Q,), -1, dtype=torch.int64, device=dev),
                              torch.full((Q,), float("inf"), dtype=torch.float32, device=dev),
                              torch.full((Q,), float("inf"), dtype=torch.float32, device=dev),
                              torch.zeros((Q,), dtype=torch.bool, device=dev) if want else None)
    if not query_features.is_cuda:
        raise RuntimeError("feature_nearest runs on HIP devices only: move the descriptors to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    q, t = query_features.detach().contiguous(), target_features.detach().contiguous()

    def search(a, na, b, nb):
        index = torch.empty((na,), dtype=torch.int64, device=dev)
        d2, second = torch.empty((na,), dtype=torch.float32, device=dev), torch.empty((na,), dtype=torch.float32, device=dev)
        _native.check(lib.mvsn_cloud_feature_nearest(_native.ptr(a), na, _native.ptr(b), nb, FEATURE_DIM, _native.ptr(index),
                                                     _native.ptr(d2), _native.ptr(second), _native.stream()),
                      "mvsn_cloud_feature_nearest")
        return index, d2, second

    with torch.cuda.device(dev):
        index, d2, second = search(q, Q, t, T)
        both = None
        if want:
            back, _, _ = search(t, T, q, Q)
            both = torch.empty((Q,), dtype=torch.bool, device=dev)
            _native.check(lib.mvsn_cloud_feature_mutual(_native.ptr(index), Q, _native.ptr(back), T, _native.ptr(both),
                                                        _native.stream()), "mvsn_cloud_feature_mutual")
    return FeatureMatches(index, d2, second, both)


def _check_ransac(source, target, max_dist, hypotheses, seed, edge_similarity):
    """The validation ``cloud_ransac`` and ``cloud_register_global`` share: (N, M, dev, r2, hypotheses, seed, es)."""
    check_cloud("source", source)
    check_cloud("target", target)
    dev = source.device
    if target.device != dev:
        raise ValueError(f"target is on {target.device}, source on {dev}")
    _, _, r2 = cloud_radius_scalars(max_dist)
    hyp = _integer_in(hypotheses, "hypotheses", 1, RANSAC_MAX_HYPOTHESES)
    sd = _integer_in(seed, "seed", 0, 2 ** 64 - 1)
    try:
        es = float(edge_similarity)
        if isinstance(edge_similarity, (bool, str)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"edge_similarity must be a number inside (0, 1], got {edge_similarity!r}") from None
    if not 0.0 < es <= 1.0:
        raise ValueError(f"edge_similarity must be a number inside (0, 1], got {edge_similarity!r}")
    return int(source.shape[0]), int(target.shape[0]), dev, r2, hyp, sd, es


def _no_pose(C, status, dev):
    return CloudRansac(torch.eye(4, dtype=torch.float32, device=dev), torch.full((), -1, dtype=torch.int64, device=dev),
                       torch.zeros((), dtype=torch.int64, device=dev), torch.full((), status, dtype=torch.int64, device=dev),
                       torch.zeros((C,), dtype=torch.bool, device=dev))


def _cloud_ransac(source, target, corr, N, M, dev, r2, hyp, sd, es):
    C = int(corr.shape[0])
    if N == 0 or M == 0 or C == 0:     # fewer than 3 usable correspondences, nothing to launch
        return _no_pose(C, 1, dev)
    if not source.is_cuda:
        raise RuntimeError("cloud_ransac runs on HIP devices only: move the clouds to 'cuda' "
                           "(there is no CPU implementation)")
    lib = _native.load()
    s, t, c = source.detach().contiguous(), target.detach().contiguous(), corr.detach().contiguous()
    ws_bytes = lib.mvsn_cloud_ransac_workspace_bytes()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    T, T64 = torch.empty((4, 4), dtype=torch.float32, device=dev), torch.empty((4, 4), dtype=torch.float64, device=dev)
    best = torch.empty((3,), dtype=torch.int64, device=dev)
    inlier = torch.empty((C,), dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        _native.check(lib.mvsn_cloud_ransac(_native.ptr(s), N, _native.ptr(t), M, _native.ptr(c), C, float(r2), es, hyp, sd,
                                            _native.ptr(ws), ws_bytes, _native.ptr(T), _native.ptr(T64), _native.ptr(best),
                                            _native.ptr(inlier), _native.stream()), "mvsn_cloud_ransac")
    return CloudRansac(T, best[0], best[1], best[2], inlier)


def _check_correspondences(corr, dev):
    if not torch.is_tensor(corr) or corr.dim() != 2 or corr.shape[1] != 2 or corr.dtype != torch.int64:
        raise ValueError("correspondences must be a (C,2) int64 tensor of (source row, target row)")
    if corr.device != dev:
        raise ValueError(f"correspondences is on {corr.device}, source on {dev}")
    if int(corr.shape[0]) > 2 ** 31 - 1:
        raise ValueError(f"at most 2^31 - 1 correspondences, got {int(corr.shape[0])}")


def cloud_ransac(source: torch.Tensor, target: torch.Tensor, correspondences: torch.Tensor, max_dist: float, *,
                 hypotheses: int = 100000, seed: int = 0, edge_similarity: float = 0.9) -> CloudRansac:
    """The rigid pose that brings the most of ``correspondences`` (C,2) int64, rows of ``source`` (N,3) fp32 paired with
    rows of ``target`` (M,3) fp32, within ``max_dist`` of each other: RANSAC over ``hypotheses`` (1 to 2^24) triples
    (csrc/mvsn_cloud_ransac.hip; Open3D's ``registration_ransac_based_on_correspondence``).

    Hypothesis h draws three correspondences from a counter-based generator (splitmix64 of ``seed`` and h: integer
    operations only).  It is rejected when two draws coincide, a drawn row lies outside its cloud or is not finite, two
    edges of the triangles differ in length by more than ``edge_similarity`` (inside (0, 1]; Open3D's edge-length
    checker) or a triangle is degenerate.  Its pose comes from the two triangles' orthonormal frames in fp64, its score
    is the number of correspondences within ``max_dist`` after the pose.  The winner has the most inliers, ties going
    to the lowest h: the result is a bitwise-reproducible function of the inputs, ``seed`` included, and nothing is
    read on the host.  ``status`` is 0, 1 where fewer than 3 correspondences are usable, 2 where every hypothesis was
    rejected; ``T`` is then the identity.  A correspondence with a row outside its cloud takes no part.  The time is
    hypotheses x C.  Everything is validated here, before any launch."""
    N, M, dev, r2, hyp, sd, es = _check_ransac(source, target, max_dist, hypotheses, seed, edge_similarity)
    _check_correspondences(correspondences, dev)
    return _cloud_ransac(source, target, correspondences, N, M, dev, r2, hyp, sd, es)


def cloud_register_global(source: torch.Tensor, target: torch.Tensor, max_dist: float, *, feature_radius: float = None,
                          source_normals: Optional[torch.Tensor] = None, target_normals: Optional[torch.Tensor] = None,
                          normal_radius: Optional[float] = None, mutual: bool = True, hypotheses: int = 100000,
                          seed: int = 0, edge_similarity: float = 0.9, refine: bool = True,
                          refine_iterations: int = 20) -> GlobalRegistration:
    """Register ``source`` (N,3) fp32 to ``target`` (M,3) fp32 from unrelated frames: the start that ``cloud_register``
    needs and ``cloud_metrics`` presumes.  Normals come from
    ``cloud_normals(., normal_radius or feature_radius / 2)`` where they are not given; ``cloud_fpfh`` describes both
    clouds at ``feature_radius``; ``feature_nearest(mutual=mutual)`` matches source rows to target rows; the rows with
    a match (a mutual one where asked) are the correspondences of ``cloud_ransac`` with ``max_dist``, ``hypotheses``,
    ``seed`` and ``edge_similarity``; with ``refine``, ``cloud_register(source, target, max_dist,
    target_normals=..., T_init=coarse.T, iterations=refine_iterations)`` finishes the job.

    Callers bring the clouds to 10^4 - 10^5 points first (``voxel_merge``): matching is brute force.  Every stage is a
    bitwise-reproducible function of its inputs, so the whole result is one of (source, target, the arguments).  The
    boolean selection of the matched rows is the composition's one extra host read (the size of the list), next to the
    status words of the index builds.  Every argument is validated here, before any launch."""
    N, M, dev, r2, hyp, sd, es = _check_ransac(source, target, max_dist, hypotheses, seed, edge_similarity)
    fh = cloud_radius_scalars(feature_radius, "feature_radius")[0]
    nh = cloud_radius_scalars(float(fh) / 2 if normal_radius is None else normal_radius, "normal_radius")[0]
    if source_normals is not None:
        _check_normals(source_normals, "source_normals", N, dev, "source")
    if target_normals is not None:
        _check_normals(target_normals, "target_normals", M, dev, "source")
    it = _integer_in(refine_iterations, "refine_iterations", 0, 1000)
    if N == 0 or M == 0:               # nothing to describe or to match, nothing to launch
        coarse = _no_pose(0, 1, dev)
        refined = cloud_register(source, target, max_dist, target_normals=target_normals, T_init=coarse.T,
                                 iterations=it) if refine else None
        return GlobalRegistration(coarse.T, coarse, torch.zeros((0, 2), dtype=torch.int64, device=dev), refined)
    if not source.is_cuda:
        raise RuntimeError("cloud_register_global runs on HIP devices only: move the clouds to 'cuda' "
                           "(there is no CPU implementation)")
    sn = cloud_normals(source, float(nh)).normals if source_normals is None else source_normals
    tn = cloud_normals(target, float(nh)).normals if target_normals is None else target_normals
    fs, ft = cloud_fpfh(source, sn, float(fh)), cloud_fpfh(target, tn, float(fh))
    m = feature_nearest(fs.features, ft.features, mutual=bool(mutual))
    keep = (m.index >= 0) & m.mutual if mutual else m.index >= 0
    rows = torch.nonzero(keep).reshape(-1)               # the one extra host read: the length of the list
    corr = torch.stack([rows, m.index[rows]], dim=1).contiguous()
    coarse = _cloud_ransac(source, target, corr, N, M, dev, r2, hyp, sd, es)
    refined = None
    if refine:
        refined = cloud_register(source, target, max_dist, target_normals=tn, T_init=coarse.T, iterations=it)
    return GlobalRegistration(refined.T if refine else coarse.T, coarse, corr, refined)


def frame_pair_poses(T_cam_in_world: torch.Tensor, ref: Sequence[int], src: Sequence[int]) -> torch.Tensor:
    """T_right_in_left = T_left_in_world^-1 T_right_in_world for every (ref[i], src[i]): (len(ref),1,4,4) fp32, formed
    in fp64 on the host (a handful of 4x4s: the DataLoader-side pose arithmetic)."""
    T = T_cam_in_world.detach().to("cpu", torch.float64)
    ref, src = list(ref), list(src)
    return (torch.linalg.inv(T[ref]) @ T[src]).to(torch.float32).unsqueeze(1).contiguous()


def reconstruct(net, images: torch.Tensor, K: torch.Tensor, T_cam_in_world: torch.Tensor, neighbours, *,
                num_idepth_samples: int = 64, batch: int = 8, cost_volume_filter: bool = True,
                refiners: Sequence[bool] = (True,) * 5, with_confidence: bool = False,
                min_confidence: Optional[float] = None, with_normals: bool = False,
                normals_max_rel_step: float = 0.05, **fusion_kwargs):
    """Posed frames -> point cloud: the network's depth map for every view, then ``fuse_depthmaps`` over all of them.

    ``images`` (V,3,H,W) fp32 in [-1,1] on the network's device, ``K`` / ``T_cam_in_world`` (V,4,4), ``neighbours`` (V,S)
    without -1: the S source views of each reference view, the first of which sets the baseline (a zero baseline
    raises, as ``multi_view_unpack_batch`` does).  The network runs over the reference views ``batch`` at a time; its
    finest idepth map is converted to depth in the units of the poses (``metrics.idepth_to_depth``).  The same
    ``neighbours`` (and ``fusion_kwargs``) drive the fusion.  Returns ``(FusionResult, depth (V,1,H,W))``.

    ``with_confidence`` or a ``min_confidence``: the forwards run with ``net.options.confidence`` on (restored
    afterwards, also when a forward raises), the finest confidence map of every view goes, with ``min_confidence``, to
    the fusion, and the return value is ``(FusionResult, depth, confidence (V,1,H,W))``.

    ``with_normals``: the world-frame normals of the points, ``point_normals(result, depth_normals(depth, K,
    T_cam_in_world=T_cam_in_world, max_rel_step=normals_max_rel_step))`` (M,3), come as one more, last element."""
    from . import metrics
    from . import multi_view_stereonet_utils as snu

    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("images must be a (V,3,H,W) tensor")
    V = images.shape[0]
    nb = _host_index_array(neighbours, "neighbours")
    if nb.ndim != 2 or nb.shape[0] != V or nb.shape[1] < 1:
        raise ValueError(f"neighbours must be ({V}, S) with S >= 1")
    if ((nb < 0) | (nb >= V)).any():
        raise ValueError(f"the network needs S real source views per reference view: indices in [0, {V})")
    if batch < 1:
        raise ValueError("batch must be >= 1")
    # checked on the camera centres, before any launch (T_right_in_left of two coincident cameras can keep a rounding
    # residue in its translation)
    centres = T_cam_in_world.detach().to("cpu", torch.float64)[:, :3, 3]
    if ((centres - centres[nb[:, 0]]).norm(dim=1) <= 0).any():
        raise AssertionError("baseline to the first source view must be positive")
    dev = images.device
    Kc = K.detach().to("cpu", torch.float32)
    params = {"num_idepth_samples": int(num_idepth_samples), "cost_volume_filter": bool(cost_volume_filter),
              "refiners": list(refiners)}
    want_conf = bool(with_confidence) or min_confidence is not None
    depths, confs = [], []
    old_conf = net.options.confidence
    net.options.confidence = want_conf or old_conf
    try:
        with torch.no_grad():
            for lo in range(0, V, batch):
                ref = list(range(lo, min(lo + batch, V)))
                frames = {"left_image": images[ref],
                          "right_image": [images[nb[ref, s].tolist()] for s in range(nb.shape[1])],
                          "K": Kc[ref].unsqueeze(1).contiguous(),
                          "T_right_in_left": [frame_pair_poses(T_cam_in_world, ref, nb[ref, s])
                                              for s in range(nb.shape[1])]}
                inputs = snu.multi_view_unpack_batch(frames, dev, net.num_levels)
                out = snu.multi_view_forward(net, inputs, params)
                depths.append(metrics.idepth_to_depth(out["left_idepthmap_pyr"][0], inputs["baseline"]))
                if want_conf:
                    confs.append(out["left_confidence_pyr"][0])
    finally:
        net.options.confidence = old_conf
    with torch.no_grad():
        depth = torch.cat(depths, 0)
        if not want_conf:
            result = fuse_depthmaps(depth, K.to(dev), T_cam_in_world.to(dev), nb, images=images, **fusion_kwargs)
            out = (result, depth)
        else:
            confidence = torch.cat(confs, 0)
            result = fuse_depthmaps(depth, K.to(dev), T_cam_in_world.to(dev), nb, images=images,
                                    confidence=confidence, min_confidence=min_confidence, **fusion_kwargs)
            out = (result, depth, confidence)
        if with_normals:
            maps = depth_normals(depth, K.to(dev), T_cam_in_world=T_cam_in_world.to(dev),
                                 max_rel_step=normals_max_rel_step)
            out += (point_normals(result, maps),)
    return out


def write_ply(path: str, points, colors=None, confidence=None, normals=None, faces=None) -> None:
    """Binary little-endian PLY: float x, y, z per vertex, plus float nx, ny, nz (right after the position) when
    ``normals`` (N,3) is given, plus uchar red, green, blue when ``colors`` is given, plus float confidence (after the
    colours) when ``confidence`` (N,) is given.  ``faces`` (F,3) integers (a mesh of ``tsdf.TSDFVolume.extract_mesh``)
    adds ``element face F`` with ``property list uchar int vertex_indices`` after the vertex block; an index outside
    [0, N) raises ValueError.  Without ``faces`` the file is what it was before the argument existed, byte for byte."""
    pts = (points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)).astype("<f4")
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N,3)")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = (normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)).astype("<f4")
        if nrm.shape != pts.shape:
            raise ValueError("normals must be (N,3) like points")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        if col.shape != pts.shape:
            raise ValueError("colors must be (N,3) like points")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if confidence is not None:
        conf = (confidence.detach().cpu().numpy() if torch.is_tensor(confidence) else np.asarray(confidence)).astype("<f4")
        if conf.shape != (pts.shape[0],):
            raise ValueError("confidence must be (N,) like the points")
        fields += [("confidence", "<f4")]
    if faces is not None:
        tri = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
            raise ValueError("faces must be (F,3) integers")
        if tri.size and (tri.min() < 0 or tri.max() >= pts.shape[0]):
            raise ValueError(f"faces must index the {pts.shape[0]} points: indices in [0, {pts.shape[0]})")
    rec = np.empty(pts.shape[0], dtype=fields)
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        col = col.astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    if confidence is not None:
        rec["confidence"] = conf
    props = "".join(f"property {'float' if t == '<f4' else 'uchar'} {n}\n" for n, t in fields)
    face_props = f"element face {tri.shape[0]}\nproperty list uchar int vertex_indices\n" if faces is not None else ""
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {pts.shape[0]}\n{props}{face_props}end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        if faces is not None:
            frec = np.empty(tri.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
            frec["n"], frec["v"] = 3, tri
            f.write(frec.tobytes())


class PlyData(NamedTuple):
    points: torch.Tensor             # (N,3) fp32
    normals: Optional[torch.Tensor]  # (N,3) fp32, or None where the file has no nx, ny, nz
    colors: Optional[torch.Tensor]   # (N,3) uint8, or None where the file has no red, green, blue
    confidence: Optional[torch.Tensor]   # (N,) fp32, or None where the file has no confidence
    faces: Optional[torch.Tensor]    # (F,3) int64, or None where the file has no face element


_PLY_FLOATS = ("x", "y", "z", "nx", "ny", "nz", "confidence")
_PLY_BYTES = ("red", "green", "blue")


def _ply_header(data, path):
    """(format, vertex count, vertex property names, face count or None, face index type or None, offset of the body)."""
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' line or no 'end_header' line)")
    try:
        lines = data[:end].decode("ascii").split("\n")[1:]
    except UnicodeDecodeError:
        raise ValueError(f"{path}: the header is not ASCII") from None
    fmt, n, names, nf, face_type, element = None, None, [], None, None, None
    for line in lines:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if tok[1:] not in (["binary_little_endian", "1.0"], ["ascii", "1.0"]):
                raise ValueError(f"{path}: format {' '.join(tok[1:])!r} is not understood (binary_little_endian 1.0 or "
                                 "ascii 1.0)")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError(f"{path}: header line {line!r} is not understood")
            element = tok[1]
            if element == "vertex" and n is None and nf is None:
                n = int(tok[2])
            elif element == "face" and n is not None and nf is None:
                nf = int(tok[2])
            else:
                raise ValueError(f"{path}: element {element!r} is not understood (one 'vertex', then at most one 'face')")
        elif tok[0] == "property" and element == "vertex":
            if len(tok) != 3 or (tok[2] in _PLY_FLOATS and tok[1] not in ("float", "float32")) or \
                    (tok[2] in _PLY_BYTES and tok[1] not in ("uchar", "uint8")) or tok[2] not in _PLY_FLOATS + _PLY_BYTES:
                raise ValueError(f"{path}: vertex property {' '.join(tok[1:])!r} is not understood (float x y z nx ny nz "
                                 "confidence, uchar red green blue)")
            if tok[2] in names:
                raise ValueError(f"{path}: vertex property {tok[2]!r} appears twice")
            names.append(tok[2])
        elif tok[0] == "property" and element == "face":
            if len(tok) != 5 or tok[1] != "list" or tok[2] not in ("uchar", "uint8") or \
                    tok[3] not in ("int", "int32", "uint", "uint32") or tok[4] not in ("vertex_indices", "vertex_index") or \
                    face_type is not None:
                raise ValueError(f"{path}: face property {' '.join(tok[1:])!r} is not understood (list uchar int|uint "
                                 "vertex_indices)")
            face_type = "<u4" if tok[3].startswith("u") else "<i4"
        else:
            raise ValueError(f"{path}: header line {line!r} is not understood")
    if fmt is None or n is None:
        raise ValueError(f"{path}: the header has no format line or no vertex element")
    for group in (("x", "y", "z"), ("nx", "ny", "nz"), _PLY_BYTES):
        have = [g in names for g in group]
        if any(have) != all(have) or (group[0] == "x" and not all(have)):
            raise ValueError(f"{path}: vertex properties {names} are not understood: {', '.join(group)} go together"
                             + (" and are required" if group[0] == "x" else ""))
    if nf is not None and face_type is None:
        raise ValueError(f"{path}: the face element has no vertex_indices property")
    return fmt, n, names, nf, face_type, end + len(b"end_header\n")


def read_ply(path: str) -> PlyData:
    """Read what ``write_ply`` writes, as CPU tensors: ``format binary_little_endian 1.0``; per vertex float ``x y z``,
    optionally float ``nx ny nz``, uchar ``red green blue`` and float ``confidence``, in any order; optionally an
    ``element face`` with ``property list uchar int|uint vertex_indices`` whose faces are all triangles.  ``format ascii
    1.0`` with the same properties is read too (ground-truth clouds are often ASCII).  Anything else raises ValueError
    with a message that names what was not understood: other elements, other properties or property types, big-endian
    data, a face that is no triangle, an index outside the vertices, a file that ends early or goes on after its last
    element.  Host only, pure numpy."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, n, names, nf, face_type, at = _ply_header(data, path)
    dtype = np.dtype([(name, "u1" if name in _PLY_BYTES else "<f4") for name in names])
    tri = None
    if fmt == "ascii":
        tok = data[at:].split()
        need = n * len(names)
        if len(tok) < need:
            raise ValueError(f"{path}: truncated: {len(tok)} numbers, the {n} vertices need {need}")
        try:
            table = np.array(tok[:need], dtype=np.float64).reshape(n, len(names))
        except ValueError:
            raise ValueError(f"{path}: a vertex value is not a number") from None
        rec = np.empty(n, dtype=dtype)
        for c, name in enumerate(names):
            col = table[:, c]
            if name in _PLY_BYTES and not ((col >= 0) & (col <= 255) & (col == np.floor(col))).all():
                raise ValueError(f"{path}: a {name} value is not an integer in [0, 255]")
            with np.errstate(all="ignore"):
                rec[name] = col
        rest = tok[need:]
        if nf is not None:
            if len(rest) < 4 * nf:
                raise ValueError(f"{path}: truncated: {len(rest)} numbers, the {nf} faces need {4 * nf}")
            try:
                ftab = np.array(rest[:4 * nf], dtype=np.int64).reshape(nf, 4)
            except (ValueError, OverflowError):
                raise ValueError(f"{path}: a face value is not an integer") from None
            if (ftab[:, 0] != 3).any():
                raise ValueError(f"{path}: face {int(np.argmax(ftab[:, 0] != 3))} has {int(ftab[np.argmax(ftab[:, 0] != 3), 0])} "
                                 "vertices: only triangles are understood")
            tri, rest = ftab[:, 1:], rest[4 * nf:]
        if rest:
            raise ValueError(f"{path}: {len(rest)} numbers after the last element")
    else:
        body = n * dtype.itemsize
        if len(data) < at + body:
            raise ValueError(f"{path}: truncated: {len(data) - at} bytes, the {n} vertices need {body}")
        rec = np.frombuffer(data, dtype=dtype, count=n, offset=at)
        at += body
        if nf is not None:
            fdtype = np.dtype([("n", "u1"), ("v", face_type, (3,))])
            got = np.frombuffer(data, dtype=fdtype, count=min(nf, (len(data) - at) // fdtype.itemsize), offset=at)
            if (got["n"] != 3).any():
                bad = int(np.argmax(got["n"] != 3))
                raise ValueError(f"{path}: face {bad} has {int(got['n'][bad])} vertices: only triangles are understood")
            if len(got) < nf:
                raise ValueError(f"{path}: truncated: {len(data) - at} bytes, the {nf} faces need {nf * fdtype.itemsize}")
            tri = got["v"].astype(np.int64)
            at += nf * fdtype.itemsize
        if at != len(data):
            raise ValueError(f"{path}: {len(data) - at} bytes after the last element")
    if tri is not None and tri.size and (tri.min() < 0 or tri.max() >= n):
        raise ValueError(f"{path}: a face indexes outside the {n} vertices")

    def columns(group):
        if group[0] not in names:
            return None
        return torch.from_numpy(np.stack([rec[g] for g in group], axis=1).copy() if n else
                                np.zeros((0, len(group)), rec.dtype[group[0]]))
    conf = torch.from_numpy(rec["confidence"].copy()) if "confidence" in names else None
    return PlyData(columns(("x", "y", "z")), columns(("nx", "ny", "nz")), columns(_PLY_BYTES), conf,
                   torch.from_numpy(np.ascontiguousarray(tri).reshape(-1, 3)) if tri is not None else None)
