"""Time fuse_depthmaps (multi_view_stereonet_amd/fusion.py) on two synthetic analytic scenes (synthetic.fusion_scene):
V = 64 at 512x256 with M = 4 neighbours, and V = 16 at 1024x512 with M = 8.

Per call: ms between two device events around the whole call (four launches and the one host read of the kept-point
count), warm-up excluded, and the bytes each kernel must move: the consistency kernel reads the reference depth and
writes the fused depth and the count map (its neighbour taps are gathered through L2 / MALL and listed separately as
the logical gather volume), the emit kernel reads the fused depth and writes the points, colours, view and pixel
arrays.  Prints one JSON line per scene.  The kernel split comes from a rocprofv3 --kernel-trace --stats run of this
tool.  --confidence: also times the call gated by a seeded random confidence at min_confidence = 0.25 (one more launch,
mvsn_confidence_mask, in front of the four) and reports it as "gated".  --voxel: also merges each scene's cloud on a
voxel grid (fusion.voxel_merge; the voxel is one pixel's footprint at the median fused depth, about one point per
surface element of a single view) and reports, as "voxel", N, M and ms per call next to the same merge composed from
torch ops on the device (torch.unique(dim=0, return_inverse=True) on the integer cells + index_add_), timed the same
way.  --normals: also times depth_normals on each scene's depth maps (one launch; world frame) and reports, as
"normals", ms per call next to the same map composed from torch ops on the device (shifted slices, torch.cross,
F.normalize), the bytes per second the call achieves against the 16 bytes per pixel the algorithm must move (4 read, 12
written; 17 with a validity mask), how far the two maps are apart, and ms per point_normals / voxel_normals call on the
fused cloud.  --cloud-metrics: also fuses each scene's depths with a seeded relative perturbation into a
prediction, scores it against the cloud of the true depths (metrics.cloud_metrics; threshold = max_dist = one pixel's
footprint at the median fused depth) and reports, as "cloud", the metrics, ms per cloud_nearest call (prediction against
truth) with the index build and the query timed separately between device events, and the same query composed from torch
ops on the device -- torch.cdist + min over chunks of the target -- for the first TORCH_QUERIES queries only (the full
composition forms N x T distances: 7e13 at these sizes), with its extrapolation to all queries.  --tsdf: also integrates
each scene's V views into a 256^3 volume (tsdf.TSDFVolume; 2 cm voxels around the scene, truncation 4 voxels) with and
without colour and reports, as "tsdf", ms per integrate call next to the same integration composed from torch ops on the
device (projection, nearest gather, masked accumulate, a view at a time), the bytes of state the call must move (read
once, written once) over its time as a share of STREAMING_BYTES_PER_S (the 6.3 TB/s a streaming kernel reaches on this
device) and of DEPTH_NORMALS_BYTES_PER_S (the 2.95 TB/s depth_normals_kernel reached), ms per extract_mesh call with M and F, and the
mesh vertices scored by metrics.cloud_metrics against the fused cloud of the true depths (points on the analytic
surfaces; threshold one voxel).  --raycast: also renders that volume (with colour) back into the scene's V input views
(TSDFVolume.raycast at the default step, one voxel) and reports, as "raycast", ms per call, the share of pixels with a
hit, the ms of a call of one pixel (the preparation pass that every call pays, whatever V is), how far the rendered depth
is from the input depth, and the same fixed-step march for depth alone composed from torch ops (grid_sample on values(),
one step of all rays at a time) on the first TORCH_RAYCAST_VIEWS views, with the share of the samples inside the box that
were not defined.  --align: also perturbs the scene's poses by a fixed seeded twist (ALIGN_SHIFT, ALIGN_ANGLE), aligns
all V views against that volume (TSDFVolume.align, ALIGN_ITERATIONS iterations, the default band trunc / 2) and reports,
as "align", ms per call and per iteration, the ms of a call with no iteration (the preparation pass and one evaluation),
the pose errors before and after, the status counts, and one iteration (the evaluation of the 6 x 6 system and its solve)
composed from torch ops on the first TORCH_ALIGN_VIEWS views.  --mesh: also extracts the mesh of that volume (with colour)
and reports, as "mesh", M, F, the number of components C and the largest one's share, ms per mesh_components call and per
filter_mesh(min_faces=MESH_MIN_FACES) call (labelling included, and with the components handed in), and the labelling
composed from torch ops -- scatter_reduce(amin) over the sides of the faces plus a pointer jump, repeated to a fixed point
with a host read per round -- with its rounds and whether it finds the same partition.  --register: also registers each scene's fused cloud, moved
by a fixed seeded twist (REGISTER_ANGLE, REGISTER_SHIFT about the cloud's mean), back onto itself
(fusion.cloud_register against the fused cloud with its point_normals, REGISTER_ITERATIONS iterations, max_dist
REGISTER_MAX_DIST) point-to-plane and point-to-point and reports, as "register", ms per call and per iteration (call
minus the call with no iteration, over the iterations), ms of one cloud_nearest query at the same max_dist, the pose
errors before and after, the status and the history's first and last rows, and one iteration composed from torch ops
(torch.cdist over chunks of the target, gathers, J, the sums as einsums in fp64, a Cholesky solve) on the first
TORCH_QUERIES source points, with its extrapolation to all of them.  --cloud-normals: also estimates the normals of each
scene's fused cloud from the bare points (fusion.cloud_normals at radius NORMALS_RADIUS, facing every point's own camera)
and reports, as "cloud_normals", ms per call, the share of points that got a normal, the angle to point_normals of the same
cloud (mean and p99), ms of one cloud_nearest query of the cloud against itself at the same radius (the walk is the same:
the difference is the cost of the moments and the eigen-solve), and the composition from torch ops (torch.cdist over
chunks of the cloud, the moments as fp64 matrix products, torch.linalg.eigh) on the first TORCH_QUERIES points, with its
extrapolation to all of them.  --knn: also searches each scene's fused cloud for every point's k nearest other points
(fusion.cloud_knn of the cloud against itself, exclude_self, within KNN_RADIUS) at k = 8 and 32 and filters it
(fusion.statistical_outlier_mask, k = 8, std_ratio 2) and reports, as "knn", ms per call, ms of one cloud_nearest query of
the cloud against itself at the same radius (the same walk: the floor), the share of points with fewer than k neighbours,
ms per statistical_outlier_mask call and the share kept, and the search composed from torch ops (torch.cdist over chunks of
the cloud, topk per chunk, topk over the chunks' winners) on the first TORCH_QUERIES points, with its extrapolation to
all of them.  --clusters: also splits each scene's fused cloud, merged on a voxel grid of one pixel's footprint
(fusion.voxel_merge), into its density-connected pieces (fusion.cloud_clusters at eps = CLUSTER_EPS_VOXELS voxels,
min_points = CLUSTER_MIN_POINTS) and reports, as "clusters", N, the number of clusters C, the share of noise, the largest
cluster's share, ms per call, ms of one cloud_nearest query of the cloud against itself at the same radius (the walk that
the call makes three times), and the same labelling composed from torch ops -- the edge list of fusion.cloud_knn at k = 64,
min-label propagation over the core edges with scatter_reduce(amin) plus a pointer jump, repeated to a fixed point with a
host read per round, the border points from the first core entry of their sorted neighbour list -- with its rounds, how
many points have more than 64 neighbours (their edge lists are cut short), and whether it finds the same labelling.
--render: also renders each scene's fused cloud back into the scene's views (fusion.cloud_render) and reports, as
"render", N, V, the map size, the share of pixels hit and ms per call at radius 0 and 1, ms per fusion.cloud_visibility of
the cloud against the scene's depth maps with and without the images as maps, whether every rendered row is visible
against its own render with no tolerance, and the radius-0 render composed from torch ops (the projection as nested
addcmul, then scatter_reduce_(amin) on int64 keys, view by view) with the pixels whose depth bits differ from the
kernel's, and its exact form (every fused multiply-add of a row formed in fp64 and rounded once) with whether that gives
the same depth bits; with a library built with -DMVSN_RENDER_COUNT (MVSN_HIPCC_FLAGS) also the splat's candidates and the
atomics it issued.
--global: also registers two samplings of an asymmetric height field from unrelated frames and prints, on a
line of its own as "global", the points per cloud, ms for fusion.cloud_fpfh (each cloud), fusion.feature_nearest (one way
and mutual) and fusion.cloud_ransac, ms of the match composed from torch ops (torch.cdist + min) and in how many rows its
index differs, ms of the whole fusion.cloud_register_global, and the pose error before and after the refinement.
--mesh-metrics: also scores the mesh of each scene's --tsdf volume against the fused cloud (metrics.mesh_metrics at a
threshold of one voxel) and reports, as "mesh_metrics", M, F, the (cell, face) pairs and the large faces of the index, ms
per mesh.mesh_sample of MESH_SAMPLES points, per mesh.mesh_nearest of the N fused points against the mesh and per
mesh_metrics, ms of fusion.cloud_nearest of the same N points against the mesh's vertices (for scale), the same distance by
brute force from torch ops (fp64, every face against the first TORCH_QUERIES points, in chunks of faces) with the rows whose
dist2 bits or face differ, and the scores next to cloud_metrics of the vertices.
--mesh-render: also renders the mesh of each scene's --tsdf volume into the scene's own views (mesh.mesh_render) and
reports, as "mesh_render", M, F, ms per call with and without the normal and colour gathers, ms of fusion.cloud_render of
the vertices and its share of pixels hit (for scale: the holes a vertex render leaves), the share of pixels hit, the sum
of clipped, and against TSDFVolume.raycast at the same poses the share of pixels both hit and the median and the 99th
percentile of |depth - raycast depth| over them, in voxels.
--simplify: also simplifies the mesh of each scene's --tsdf volume (mesh.mesh_simplify on the volume's own grid, at
SIMPLIFY_VOXELS volume voxels per cell, both placements, normals and colours carried) and reports, as "simplify", per
cell size and placement M and F before and after, ms per call, the positions that fell back to a member's, and the
one-sided distance of MESH_SAMPLES mesh_sample points of the simplified mesh to the original surface by mesh_nearest
(mean and maximum, in volume voxels), next to the same clustering composed from torch ops (voxel_merge, an index through
its inverse, torch.unique over the canonical triples, a renumbering) with its ms and whether it keeps as many faces.
--smooth: also finds the edges of the mesh of each scene's --tsdf volume (mesh.mesh_edges), smooths it (mesh.mesh_smooth,
Taubin, SMOOTH_ITERATIONS iterations, the edges reused) and recomputes its normals (mesh.mesh_normals), and reports, as
"smooth", M, F, E and the border and non-manifold edge counts, ms per mesh_edges, ms per smoothing call and per step
(a call takes 2 SMOOTH_ITERATIONS steps), ms per mesh_normals, and next to them the same smoothing composed from torch
ops (torch.unique over the sorted pairs of the sides, then per step index_add_ of the neighbour differences in fp64) with
its ms for the edges, per call and per step, and how far its vertices are from the device's.
--cloud-volume: also meshes the cloud: the fused cloud merged by voxel_merge, its normals by voxel_normals, added by
tsdf.TSDFVolume.integrate_cloud to the --tsdf volume with a radius of CLOUD_VOLUME_RADIUS_VOXELS voxels, then
extract_mesh; reports, as "cloud_volume", N, the flagged bricks out of all bricks, ms per call (and of the entry alone,
on a built index), M and F of the mesh, metrics.mesh_metrics of that mesh against the fused cloud next to those of the
mesh of the same views through integrate, and the same sums composed from torch ops (chunks of the cloud through
torch.cdist) at TORCH_VOXELS of the updated voxels with its ms, its extrapolation to the voxels of the flagged bricks and
its largest difference from the device's state.  Nothing asserts a time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_view_stereonet_amd import _native, synthetic  # noqa: E402
from multi_view_stereonet_amd.fusion import (cloud_render, cloud_visibility, cloud_clusters, cloud_knn, cloud_nearest, cloud_normals, cloud_radius_scalars,  # noqa: E402
                                             cloud_fpfh, cloud_ransac, cloud_register_global, feature_nearest,
                                             cloud_register, statistical_outlier_mask, depth_normals, fuse_depthmaps, point_normals, voxel_merge, voxel_normals)
from multi_view_stereonet_amd.mesh import filter_mesh, mesh_components, mesh_edges, mesh_nearest, mesh_normals, mesh_render, mesh_sample, mesh_simplify, mesh_smooth  # noqa: E402
from multi_view_stereonet_amd.metrics import cloud_metrics, mesh_metrics  # noqa: E402
from multi_view_stereonet_amd.tsdf import TSDFVolume  # noqa: E402

SCENES = [(64, 256, 512, 4), (16, 512, 1024, 8)]


def neighbours(views, slots):
    return np.array([sorted((w for w in range(views) if w != v), key=lambda w: (abs(w - v), w))[:slots]
                     for v in range(views)])


def timed(call, steps, warmup):
    for _ in range(warmup):
        res = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return res, times


def torch_voxel_merge(points, colors, voxel):
    """The merge from torch ops: the same fp32 cells, then unique over the int64 cell rows and index_add_ sums (float
    sums in arrival order, rows in cell order, no `first`: what a caller had to write without voxel_merge)."""
    cells = torch.floor(points * float(np.float32(1) / np.float32(voxel))).to(torch.int64)
    uniq, inverse = torch.unique(cells, dim=0, return_inverse=True)
    m = uniq.shape[0]
    count = torch.zeros(m, dtype=torch.float32, device=points.device).index_add_(
        0, inverse, torch.ones(points.shape[0], dtype=torch.float32, device=points.device))
    pos = torch.zeros(m, 3, dtype=torch.float32, device=points.device).index_add_(0, inverse, points)
    col = torch.zeros(m, 3, dtype=torch.float32, device=points.device).index_add_(0, inverse, colors.to(torch.float32))
    return pos / count[:, None], (col / count[:, None] + 0.5).to(torch.uint8), count, inverse


def run_voxel(res, fx, steps, warmup):
    voxel = float(np.float32(float(res.depth[res.depth > 0].median()) / fx))    # one pixel's footprint at the median depth
    vc, times = timed(lambda: voxel_merge(res.points, voxel, colors=res.colors), steps, warmup)
    tc, ttimes = timed(lambda: torch_voxel_merge(res.points, res.colors, voxel), steps, warmup)
    N, M = int(res.points.shape[0]), int(vc.points.shape[0])
    assert int(tc[0].shape[0]) == M and int(vc.count.sum()) == N
    return {"voxel": {"voxel_size": voxel, "N": N, "M": M, "ms_per_call_median": float(np.median(times)),
                      "ms_per_call_min": float(np.min(times)), "torch_ms_per_call_median": float(np.median(ttimes)),
                      "torch_ms_per_call_min": float(np.min(ttimes))}}


def torch_depth_normals(depth, K, T, step):
    """depth_normals from torch ops: the same neighbour test and tangents on shifted copies of the maps (every
    intermediate a (V,H,W,3) tensor in HBM: what a caller had to write without the kernel)."""
    import torch.nn.functional as F
    V, _, H, W = depth.shape
    d = depth[:, 0]
    Ki = torch.linalg.inv(K[:, :3, :3].double()).float()
    ys, xs = torch.meshgrid(torch.arange(H, device=d.device, dtype=torch.float32),
                            torch.arange(W, device=d.device, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    X = d[..., None] * torch.einsum("vij,hwj->vhwi", Ki, pix)
    ok = d > 0
    bound = step * d

    def neighbour(dy, dx):
        inside = torch.ones(H, W, dtype=torch.bool, device=d.device)
        if dx:
            inside[:, 0 if dx < 0 else W - 1] = False
        if dy:
            inside[0 if dy < 0 else H - 1, :] = False
        dn = torch.roll(d, (-dy, -dx), (1, 2))
        counts = ok & torch.roll(ok, (-dy, -dx), (1, 2)) & inside & ((dn - d).abs() <= bound)
        return counts, torch.roll(X, (-dy, -dx), (1, 2))

    (left, Xl), (right, Xr), (up, Xu), (down, Xd) = neighbour(0, -1), neighbour(0, 1), neighbour(-1, 0), neighbour(1, 0)
    tu = torch.where(right[..., None], Xr, X) - torch.where(left[..., None], Xl, X)
    tv = torch.where(down[..., None], Xd, X) - torch.where(up[..., None], Xu, X)
    c = torch.einsum("vij,vhwj->vhwi", T[:, :3, :3], torch.cross(tv, tu, dim=-1))
    n = F.normalize(c, dim=-1)
    defined = ok & (left | right) & (up | down) & (c != 0).any(-1)
    return torch.where(defined[..., None], n, torch.zeros_like(n)).permute(0, 3, 1, 2).contiguous()


def run_normals(sc, res, steps, warmup):
    depth, K, T = sc["depth"], sc["K"], sc["T_cam_in_world"]
    V, _, H, W = depth.shape
    maps, times = timed(lambda: depth_normals(depth, K, T_cam_in_world=T), steps, warmup)
    tmaps, ttimes = timed(lambda: torch_depth_normals(depth, K, T, 0.05), steps, warmup)
    both = (maps != 0).any(1) & (tmaps != 0).any(1)
    cosine = (maps * tmaps).sum(1)[both].clamp(-1, 1)
    pn, gtimes = timed(lambda: point_normals(res, maps), steps, warmup)
    fx = float(K[0, 0, 0])
    vc = voxel_merge(res.points, float(np.float32(float(res.depth[res.depth > 0].median()) / fx)), colors=res.colors)
    vn, vtimes = timed(lambda: voxel_normals(vc, pn), steps, warmup)
    nbytes = 16 * V * H * W
    return {"normals": {"ms_per_call_median": float(np.median(times)), "ms_per_call_min": float(np.min(times)),
                        "torch_ms_per_call_median": float(np.median(ttimes)),
                        "torch_ms_per_call_min": float(np.min(ttimes)), "algorithmic_bytes": nbytes,
                        "bytes_per_s_at_median": nbytes / (float(np.median(times)) * 1e-3),
                        "bytes_per_s_at_min": nbytes / (float(np.min(times)) * 1e-3),
                        "defined_fraction": float((maps != 0).any(1).float().mean()),
                        "defined_mask_differs_from_torch": int(((maps != 0).any(1) != (tmaps != 0).any(1)).sum()),
                        "max_angle_to_torch_rad": float(torch.acos(cosine).max()) if cosine.numel() else 0.0,
                        "point_normals_ms_median": float(np.median(gtimes)), "points": int(pn.shape[0]),
                        "voxel_normals_ms_median": float(np.median(vtimes)), "voxels": int(vn.shape[0])}}


TORCH_QUERIES = 1024
TORCH_TARGET_CHUNK = 1 << 20


def torch_cloud_nearest(query, target, max_dist):
    """The query from torch ops: chunks of the target through torch.cdist, the running minimum and the count (what a
    caller had to write without cloud_nearest; cdist's own arithmetic, so the last bits of a distance may differ)."""
    best = torch.full((query.shape[0],), float("inf"), device=query.device)
    index = torch.full((query.shape[0],), -1, dtype=torch.int64, device=query.device)
    within = torch.zeros(query.shape[0], dtype=torch.int64, device=query.device)
    for a in range(0, target.shape[0], TORCH_TARGET_CHUNK):
        d = torch.cdist(query, target[a:a + TORCH_TARGET_CHUNK])
        d = torch.where(d <= max_dist, d, torch.full_like(d, float("inf")))
        within += torch.isfinite(d).sum(dim=1)
        m, i = d.min(dim=1)
        closer = m < best
        best, index = torch.where(closer, m, best), torch.where(closer, i + a, index)
    return best * best, index, within


def run_cloud(sc, nb, res, steps, warmup):
    steps, warmup = min(steps, 5), min(warmup, 1)           # (the calls are long: milliseconds to seconds)
    depth, K, T = sc["depth"], sc["K"], sc["T_cam_in_world"]
    noise = torch.randn(depth.shape, generator=torch.Generator().manual_seed(1)).to(depth.device)
    pred = fuse_depthmaps(depth * (1.0 + 0.002 * noise), K, T, nb).points
    truth = res.points
    threshold = float(np.float32(float(res.depth[res.depth > 0].median()) / float(K[0, 0, 0])))
    metrics = cloud_metrics(pred, truth, threshold)
    nn, times = timed(lambda: cloud_nearest(pred, truth, threshold), steps, warmup)
    # the two entries on their own, between device events
    lib = _native.load()
    h, inv, r2 = cloud_radius_scalars(threshold)
    N, Tn = int(pred.shape[0]), int(truth.shape[0])
    ws_bytes = lib.mvsn_cloud_workspace_bytes(Tn)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pred.device)
    status = torch.empty(1, dtype=torch.int64, device=pred.device)
    out = (torch.empty(N, device=pred.device), torch.empty(N, dtype=torch.int64, device=pred.device),
           torch.empty(N, dtype=torch.int32, device=pred.device))

    def build():
        _native.check(lib.mvsn_cloud_index_build(_native.ptr(truth), Tn, float(h), float(inv), _native.ptr(status),
                                                 _native.ptr(ws), ws_bytes, _native.stream()), "mvsn_cloud_index_build")

    def query():
        _native.check(lib.mvsn_cloud_nearest(_native.ptr(pred), N, float(inv), float(r2), _native.ptr(ws), ws_bytes, Tn,
                                             _native.ptr(out[0]), _native.ptr(out[1]), _native.ptr(out[2]),
                                             _native.stream()), "mvsn_cloud_nearest")

    _, btimes = timed(build, steps, warmup)
    _, qtimes = timed(query, steps, warmup)
    assert torch.equal(out[1], nn.index) and torch.equal(out[2], nn.within)
    sub = pred[:TORCH_QUERIES].contiguous()
    (tb, ti, tw), ttimes = timed(lambda: torch_cloud_nearest(sub, truth, threshold), steps, 1)
    found = nn.index[:TORCH_QUERIES] >= 0
    scale = N / float(sub.shape[0])
    return {"cloud": {"threshold": threshold, "n_pred": N, "n_truth": Tn, "workspace_bytes": int(ws_bytes),
                      "metrics": metrics, "within_mean": float(nn.within.float().mean()),
                      "ms_per_call_median": float(np.median(times)), "ms_per_call_min": float(np.min(times)),
                      "build_ms_median": float(np.median(btimes)), "query_ms_median": float(np.median(qtimes)),
                      "torch_queries": int(sub.shape[0]), "torch_ms_median": float(np.median(ttimes)),
                      "torch_ms_extrapolated_to_all_queries": float(np.median(ttimes)) * scale,
                      "torch_found_differs": int((found != (ti >= 0)).sum()),
                      "torch_max_abs_dist2_difference": float((tb - nn.dist2[:TORCH_QUERIES])[found & (ti >= 0)].abs().max())
                      if bool((found & (ti >= 0)).any()) else 0.0}}


TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN = (256, 256, 256), 0.02, (-2.56, -2.56, 3.2)
# what a streaming kernel reaches on this device, and what depth_normals_kernel itself reached
STREAMING_BYTES_PER_S, DEPTH_NORMALS_BYTES_PER_S = 6.3e12, 2.95e12


def torch_tsdf_integrate(state, depth, images, K, T, voxel, origin, trunc):
    """The integration from torch ops, a view at a time: the same projection, nearest gather and masked accumulate, every
    intermediate a volume-sized tensor in HBM (what a caller had to write without the kernel)."""
    s, w, c = state
    nz, ny, nx = s.shape
    dev = s.device
    ax = [torch.arange(n, device=dev, dtype=torch.float32) * voxel + o for n, o in zip((nx, ny, nz), origin)]
    pz, py, px = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    P = (K[:, :3, :3].double() @ torch.linalg.inv(T.double())[:, :3, :]).float()
    H, W = depth.shape[-2:]
    for v in range(depth.shape[0]):
        a = [P[v, r, 0] * px + P[v, r, 1] * py + P[v, r, 2] * pz + P[v, r, 3] for r in range(3)]
        z = a[2]
        col, row = torch.floor(a[0] / z + 0.5), torch.floor(a[1] / z + 0.5)
        ok = (z > 0) & (col >= 0) & (col <= W - 1) & (row >= 0) & (row <= H - 1)
        pix = torch.where(ok, row * W + col, torch.zeros_like(col)).long()
        D = depth[v, 0].reshape(-1)[pix]
        sdf = D - z
        ok &= (D > 0) & ~(sdf < -trunc)
        s += torch.where(ok, sdf.clamp(max=trunc), torch.zeros_like(sdf))
        w += ok
        if c is not None:
            c += torch.where(ok, images[v].reshape(3, -1)[:, pix], torch.zeros_like(c))


def run_tsdf(sc, res, steps, warmup):
    steps, warmup = min(steps, 5), min(warmup, 1)           # (the torch composition takes seconds)
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    dev = depth.device
    trunc = 4 * TSDF_VOXEL
    out = {"dims": list(TSDF_DIMS), "voxel_size": TSDF_VOXEL, "trunc": trunc, "views": int(depth.shape[0])}
    n = TSDF_DIMS[0] * TSDF_DIMS[1] * TSDF_DIMS[2]
    for color in (False, True):
        vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, trunc, device=dev, color=color)
        kw = {"images": images} if color else {}
        _, times = timed(lambda: vol.integrate(depth, K, T, **kw), steps, warmup)
        state_bytes = 2 * 4 * n * (5 if color else 2)        # every plane read once and written once
        _, ttimes = timed(lambda: torch_tsdf_integrate(
            (torch.zeros_like(vol.sdf_sum), torch.zeros_like(vol.weight), torch.zeros_like(vol.color_sum) if color else None),
            depth, images, K, T, float(vol.voxel_size), [float(x) for x in vol.origin], float(vol.trunc)), 2, 1)
        # one integration each into fresh volumes: where the two count different views
        vol.reset()
        vol.integrate(depth, K, T, **kw)
        tstate = (torch.zeros_like(vol.sdf_sum), torch.zeros_like(vol.weight),
                  torch.zeros_like(vol.color_sum) if color else None)
        torch_tsdf_integrate(tstate, depth, images, K, T, float(vol.voxel_size), [float(x) for x in vol.origin],
                             float(vol.trunc))
        differs = float((vol.weight != tstate[1]).float().mean())
        rate = state_bytes / (float(np.median(times)) * 1e-3)
        out["colour" if color else "plain"] = {
            "ms_per_call_median": float(np.median(times)), "ms_per_call_min": float(np.min(times)),
            "torch_ms_per_call_median": float(np.median(ttimes)), "state_bytes": state_bytes,
            "state_bytes_per_s_at_median": rate, "share_of_streaming_rate": rate / STREAMING_BYTES_PER_S,
            "share_of_depth_normals_rate": rate / DEPTH_NORMALS_BYTES_PER_S,
            "voxels_whose_view_count_differs_from_torch": differs}
        if color:
            mesh, etimes = timed(lambda: vol.extract_mesh(), steps, warmup)
            out["extract"] = {"ms_per_call_median": float(np.median(etimes)), "ms_per_call_min": float(np.min(etimes)),
                              "M": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0]),
                              "observed_fraction": float((vol.weight >= 1).float().mean())}
            out["mesh_against_surface"] = cloud_metrics(mesh.vertices, res.points, TSDF_VOXEL)
    return {"tsdf": out}


TORCH_RAYCAST_VIEWS = 4


def torch_raycast(vol, K, T, size, step):
    """The march for depth alone from torch ops: every ray of every view advanced one step at a time through
    grid_sample on values() (trilinear, a NaN where a corner is unobserved), every intermediate a (V,H,W) tensor in
    HBM.  Returns (depth (V,H,W), samples inside the box, undefined ones among them)."""
    import torch.nn.functional as F
    H, W = size
    dev = K.device
    nx, ny, nz = vol.dims
    vs = float(vol.voxel_size)
    o = torch.tensor([float(x) for x in vol.origin], dtype=torch.float64, device=dev)
    A = (T[:, :3, :3].double() @ torch.linalg.inv(K[:, :3, :3].double()) / vs).float()
    g0 = ((T[:, :3, 3].double() - o) / vs).float()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    dirs = torch.einsum("vij,hwj->vhwi", A, torch.stack([xs, ys, torch.ones_like(xs)], -1))
    g0 = g0[:, None, None, :]
    values = vol.values()[None, None]
    top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=dev)
    # the depths of the box: between the camera z of its corners
    corners = torch.tensor([[i, j, k] for i in (0, nx - 1) for j in (0, ny - 1) for k in (0, nz - 1)],
                           dtype=torch.float64, device=dev) * vs + o
    z = torch.einsum("vj,cvj->vc", T[:, :3, 2].double(), corners[:, None, :] - T[None, :, :3, 3].double())
    k0, k1 = max(1, int(z.min() / step) - 1), int(z.max() / step) + 2
    shape = dirs.shape[:3]
    f_prev = torch.full(shape, float("nan"), device=dev)
    alive = torch.ones(shape, dtype=torch.bool, device=dev)
    depth = torch.zeros(shape, device=dev)
    inside_n = torch.zeros((), dtype=torch.int64, device=dev)
    undefined_n = torch.zeros((), dtype=torch.int64, device=dev)
    t_prev = 0.0
    for k in range(k0, k1 + 1):
        t = float(np.float32(k) * np.float32(step))
        g = t * dirs + g0
        inside = ((g >= 0) & (g < top)).all(-1)
        f = F.grid_sample(values, (2 * g / top - 1)[None], mode="bilinear", padding_mode="border", align_corners=True)[0, 0]
        f = torch.where(inside, f, torch.full_like(f, float("nan")))
        inside_n += (alive & inside).sum()
        undefined_n += (alive & inside & torch.isnan(f)).sum()
        hit = alive & (f_prev >= 0) & (f < 0)
        depth = torch.where(hit, t_prev + step * f_prev / (f_prev - f), depth)
        alive &= ~(hit | ((f_prev < 0) & (f >= 0)))
        f_prev, t_prev = f, t
    return depth, inside_n, undefined_n


def run_raycast(sc, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    V, _, H, W = depth.shape
    trunc = 4 * TSDF_VOXEL
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, trunc, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    step = float(min(vol.voxel_size, vol.trunc / np.float32(4)))
    r, times = timed(lambda: vol.raycast(K, T, (H, W)), steps, warmup)
    _, ptimes = timed(lambda: vol.raycast(K[:1], T[:1], (1, 1)), steps, warmup)
    hit = r.depth > 0
    both = hit & (depth > 0)
    diff = (r.depth - depth).abs()[both]
    sub = min(V, TORCH_RAYCAST_VIEWS)
    (tdepth, inside_n, undefined_n), ttimes = timed(lambda: torch_raycast(vol, K[:sub], T[:sub], (H, W), step), 2, 1)
    thit = tdepth > 0
    same = thit == hit[:sub, 0]
    tboth = thit & hit[:sub, 0]
    return {"raycast": {
        "dims": list(TSDF_DIMS), "voxel_size": TSDF_VOXEL, "step": step, "views": V, "rays": V * H * W,
        "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
        "ns_per_ray_at_mean": 1e6 * float(np.mean(times)) / (V * H * W),
        "one_pixel_call_ms_mean": float(np.mean(ptimes)), "one_pixel_call_ms_min": float(np.min(ptimes)),
        "preparation_share_of_call": float(np.mean(ptimes)) / float(np.mean(times)),
        "hit_share": float(hit.float().mean()), "defined_hit_share": float((r.weight > 0).float().mean()),
        "abs_rendered_minus_input_depth_median": float(diff.median()), "abs_rendered_minus_input_depth_max": float(diff.max()),
        "torch_views": sub, "torch_ms_per_call_mean": float(np.mean(ttimes)), "torch_ms_per_call_min": float(np.min(ttimes)),
        "torch_ms_per_call_all_views": float(np.mean(ttimes)) * V / sub,
        "torch_hit_mask_agreement": float(same.float().mean()),
        "torch_depth_difference_max": float((tdepth - r.depth[:sub, 0]).abs()[tboth].max()) if bool(tboth.any()) else 0.0,
        "samples_inside_box_undefined_share": float(undefined_n) / max(int(inside_n), 1)}}


TORCH_ALIGN_VIEWS = 4
ALIGN_ITERATIONS = 10
ALIGN_SHIFT = 0.02            # one voxel
ALIGN_ANGLE = 0.004           # radians: 0.23 degrees


def align_twists(V, device):
    """T_cam_in_world <- [exp([w]x) R, t + s]: w of length ALIGN_ANGLE and s of length ALIGN_SHIFT in seeded directions."""
    gen = torch.Generator().manual_seed(17)
    w = torch.nn.functional.normalize(torch.randn(V, 3, generator=gen, dtype=torch.float64), dim=1) * ALIGN_ANGLE
    s = torch.nn.functional.normalize(torch.randn(V, 3, generator=gen, dtype=torch.float64), dim=1) * ALIGN_SHIFT
    Wx = torch.zeros(V, 3, 3, dtype=torch.float64)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    return torch.linalg.matrix_exp(Wx).to(device), s.to(device)


def pose_errors(T, T_true):
    """(translation distances, rotation angles) (V,) between poses, fp64."""
    T, T_true = T.double(), T_true.double()
    dR = T[:, :3, :3] @ T_true[:, :3, :3].transpose(1, 2)
    cos = ((dR.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)
    return (T[:, :3, 3] - T_true[:, :3, 3]).norm(dim=1), torch.acos(cos)


def torch_align_iteration(vol, depth, K, T, band):
    """One iteration from torch ops: the points, the 8 corners of their cells gathered from values(), the trilinear value
    and gradient, J, the sums as einsums in fp64, a Cholesky solve and the update; every intermediate a (V,H,W) tensor
    in HBM.  Returns (new poses (V,4,4) fp64, count (V,), sum w r^2 (V,))."""
    dev = K.device
    V, _, H, W = depth.shape
    nx, ny, nz = vol.dims
    vs = float(vol.voxel_size)
    o = torch.tensor([float(x) for x in vol.origin], dtype=torch.float64, device=dev)
    A = (T[:, :3, :3].double() @ torch.linalg.inv(K[:, :3, :3].double()) / vs).float()
    g0 = ((T[:, :3, 3].double() - o) / vs).float()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    dirs = torch.einsum("vij,hwj->vhwi", A, torch.stack([xs, ys, torch.ones_like(xs)], -1))
    g = depth[:, 0, :, :, None] * dirs + g0[:, None, None, :]
    c = torch.floor(g)
    top = torch.tensor([nx - 2, ny - 2, nz - 2], dtype=torch.float32, device=dev)
    ok = ((c >= 0) & (c <= top)).all(-1) & torch.isfinite(depth[:, 0]) & (depth[:, 0] > 0)
    ci = torch.where(ok[..., None], c, torch.zeros_like(c)).long()
    fr = g - c
    d = vol.values().reshape(-1)
    at = (ci[..., 2] * ny + ci[..., 1]) * nx + ci[..., 0]
    v = [d[at + (k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nx * ny] for k in range(8)]
    lerp = lambda f, a, b: a + f * (b - a)   # noqa: E731
    fx, fy, fz = fr[..., 0], fr[..., 1], fr[..., 2]
    f = lerp(fz, lerp(fy, lerp(fx, v[0], v[1]), lerp(fx, v[2], v[3])), lerp(fy, lerp(fx, v[4], v[5]), lerp(fx, v[6], v[7])))
    n = torch.stack([lerp(fz, lerp(fy, v[1] - v[0], v[3] - v[2]), lerp(fy, v[5] - v[4], v[7] - v[6])),
                     lerp(fz, lerp(fx, v[2] - v[0], v[3] - v[1]), lerp(fx, v[6] - v[4], v[7] - v[5])),
                     lerp(fy, lerp(fx, v[4] - v[0], v[5] - v[1]), lerp(fx, v[6] - v[2], v[7] - v[3]))], -1) / vs
    ok = ok & (f.abs() <= band) & torch.isfinite(n).all(-1)
    c0 = torch.tensor([(nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2], dtype=torch.float32, device=dev)
    J = torch.cat([n, torch.cross(g - c0, n, dim=-1)], -1)
    J = torch.where(ok[..., None], J, torch.zeros_like(J)).double().reshape(V, -1, 6)
    r = torch.where(ok, f / vs, torch.zeros_like(f)).double().reshape(V, -1)
    Hm = torch.einsum("vpi,vpj->vij", J, J)
    b = torch.einsum("vpi,vp->vi", J, r)
    s = Hm.diagonal(dim1=1, dim2=2).rsqrt()
    L = torch.linalg.cholesky_ex(Hm * s[:, :, None] * s[:, None, :]).L      # (no host read: a failed factor gives NaNs)
    delta = torch.cholesky_solve(-(b * s)[..., None], L)[..., 0] * s
    w = delta[:, 3:]
    Wx = torch.zeros(V, 3, 3, dtype=torch.float64, device=dev)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    Rd = torch.linalg.matrix_exp(Wx)
    cw = o + vs * c0.double()
    out = T.double().clone()
    out[:, :3, :3] = Rd @ out[:, :3, :3]
    out[:, :3, 3] = torch.einsum("vij,vj->vi", Rd, T[:, :3, 3].double() - cw) + cw + vs * delta[:, :3]
    return out, ok.reshape(V, -1).sum(1), (r * r).sum(1)


def run_align(sc, steps, warmup):
    depth, K, T = sc["depth"], sc["K"], sc["T_cam_in_world"]
    V, _, H, W = depth.shape
    trunc = 4 * TSDF_VOXEL
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, trunc, device=depth.device)
    vol.integrate(depth, K, T)
    Rd, shift = align_twists(V, depth.device)
    off = T.double().clone()
    off[:, :3, :3] = Rd @ off[:, :3, :3]
    off[:, :3, 3] += shift
    off = off.float()
    r, times = timed(lambda: vol.align(depth, K, off, iterations=ALIGN_ITERATIONS), steps, warmup)
    _, ztimes = timed(lambda: vol.align(depth, K, off, iterations=0), steps, warmup)
    before, after = pose_errors(off, T), pose_errors(r.T_cam_in_world, T)
    sub = min(V, TORCH_ALIGN_VIEWS)
    band = float(vol.trunc / np.float32(2))
    (tT, tcount, tcost), ttimes = timed(lambda: torch_align_iteration(vol, depth[:sub], K[:sub], off[:sub], band), 2, 1)
    one = vol.align(depth[:sub], K[:sub], off[:sub], iterations=1)
    per_iteration = (float(np.mean(times)) - float(np.mean(ztimes))) / ALIGN_ITERATIONS
    hist = r.history
    return {"align": {
        "dims": list(TSDF_DIMS), "voxel_size": TSDF_VOXEL, "band": band, "views": V, "pixels": V * H * W,
        "iterations": ALIGN_ITERATIONS, "shift": ALIGN_SHIFT, "angle": ALIGN_ANGLE,
        "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
        "zero_iteration_call_ms_mean": float(np.mean(ztimes)), "ms_per_iteration": per_iteration,
        "ns_per_pixel_and_iteration": 1e6 * per_iteration / (V * H * W),
        "translation_error_before_mean": float(before[0].mean()), "translation_error_after_mean": float(after[0].mean()),
        "translation_error_after_max": float(after[0].max()),
        "rotation_error_before_mean": float(before[1].mean()), "rotation_error_after_mean": float(after[1].mean()),
        "rotation_error_after_max": float(after[1].max()),
        "status_counts": [int((r.status == k).sum()) for k in range(3)],
        "share_of_pixels_taking_part_first_last": [float(hist[:, 0, 0].sum()) / (V * H * W), float(hist[:, -1, 0].sum()) / (V * H * W)],
        "sum_w_r2_first_last": [float(hist[:, 0, 2].sum()), float(hist[:, -1, 2].sum())],
        "torch_views": sub, "torch_ms_per_iteration_mean": float(np.mean(ttimes)), "torch_ms_per_iteration_min": float(np.min(ttimes)),
        "torch_ms_per_iteration_all_views": float(np.mean(ttimes)) * V / sub,
        "torch_count_equal": bool((tcount == one.history[:, 0, 0].long()).all()),
        "torch_pose_difference_max": float((tT - one.T_cam_in_world.double()).abs().max())}}


REGISTER_ANGLE, REGISTER_SHIFT, REGISTER_ITERATIONS, REGISTER_MAX_DIST = 0.004, 0.02, 10, 0.04


def torch_register_iteration(source, target, normals, T, centre, max_dist):
    """One iteration from torch ops: the moved points, their nearest targets through torch_cloud_nearest (N x M
    distances in chunks), the gathers, J, the sums as einsums in fp64, a Cholesky solve and the update.  `normals` None:
    point-to-point.  Returns (new pose (4,4) fp64, count, sum r^2)."""
    dev = source.device
    p = source @ T[:3, :3].T + T[:3, 3]
    _, index, _ = torch_cloud_nearest(p, target, max_dist)
    ok = index >= 0
    j = index.clamp(min=0)
    d, q = p - target[j], p - centre
    if normals is not None:
        n = normals[j]
        J = torch.cat([n, torch.cross(q, n, dim=-1)], -1)[:, None, :]
        r = (d * n).sum(-1)[:, None]
    else:
        eye = torch.eye(3, device=dev).expand(p.shape[0], 3, 3)
        J = torch.cat([eye, torch.cross(q[:, None, :].expand(-1, 3, -1), eye, dim=-1)], -1)
        r = d
    J = torch.where(ok[:, None, None], J, torch.zeros_like(J)).double().reshape(-1, 6)
    r = torch.where(ok[:, None], r, torch.zeros_like(r)).double().reshape(-1)
    Hm, b = J.T @ J, J.T @ r
    s = Hm.diagonal().rsqrt()
    L = torch.linalg.cholesky_ex(Hm * s[:, None] * s[None, :]).L           # (no host read: a failed factor gives NaNs)
    delta = torch.cholesky_solve(-(b * s)[:, None], L)[:, 0] * s
    w = delta[3:]
    Wx = torch.zeros(3, 3, dtype=torch.float64, device=dev)
    Wx[0, 1], Wx[0, 2], Wx[1, 0], Wx[1, 2], Wx[2, 0], Wx[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    Rd = torch.linalg.matrix_exp(Wx)
    c = centre.double()
    out = T.double().clone()
    out[:3, :3] = Rd @ out[:3, :3]
    out[:3, 3] = Rd @ (T[:3, 3].double() - c) + c + delta[:3]
    return out, ok.sum(), (r * r).sum()


def run_register(sc, res, steps, warmup):
    steps, warmup = min(steps, 2), min(warmup, 1)           # (the calls are long: a second or more)
    depth, K, T = sc["depth"], sc["K"], sc["T_cam_in_world"]
    dev = depth.device
    target = res.points
    normals = point_normals(res, depth_normals(depth, K, T_cam_in_world=T))
    centre = target.double().mean(dim=0)
    gen = torch.Generator().manual_seed(23)
    w = torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0) * REGISTER_ANGLE
    shift = (torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0) * REGISTER_SHIFT).to(dev)
    Wx = torch.zeros(3, 3, dtype=torch.float64)
    Wx[0, 1], Wx[0, 2], Wx[1, 0], Wx[1, 2], Wx[2, 0], Wx[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    Rd = torch.linalg.matrix_exp(Wx).to(dev)
    source = ((target.double() - centre) @ Rd.T + centre + shift).float()
    T_true = torch.eye(4, dtype=torch.float64, device=dev)          # the pose that undoes the twist
    T_true[:3, :3], T_true[:3, 3] = Rd.T, centre - Rd.T @ (centre + shift)
    start = torch.eye(4, dtype=torch.float32)
    N, M = int(source.shape[0]), int(target.shape[0])
    _, qtimes = timed(lambda: cloud_nearest(source, target, REGISTER_MAX_DIST), steps, warmup)
    out = {"n_source": N, "n_target": M, "max_dist": REGISTER_MAX_DIST, "iterations": REGISTER_ITERATIONS,
           "angle": REGISTER_ANGLE, "shift": REGISTER_SHIFT, "cloud_nearest_ms_mean": float(np.mean(qtimes)),
           "torch_points": min(N, TORCH_QUERIES)}
    before = pose_errors(start[None].to(dev), T_true[None])
    sub = source[:TORCH_QUERIES].contiguous()
    cen32 = centre.float()
    for mode, nm in (("plane", normals), ("point", None)):
        kw = dict(target_normals=nm, centre=cen32.cpu(), T_init=start)
        r, times = timed(lambda: cloud_register(source, target, REGISTER_MAX_DIST, iterations=REGISTER_ITERATIONS, **kw),
                         steps, warmup)
        _, ztimes = timed(lambda: cloud_register(source, target, REGISTER_MAX_DIST, iterations=0, **kw), steps, warmup)
        after = pose_errors(r.T[None], T_true[None])
        per_iteration = (float(np.mean(times)) - float(np.mean(ztimes))) / REGISTER_ITERATIONS
        (tT, tcount, tcost), ttimes = timed(
            lambda: torch_register_iteration(sub, target, nm, start.to(dev), cen32, REGISTER_MAX_DIST), 2, 1)
        one = cloud_register(sub, target, REGISTER_MAX_DIST, iterations=1, **kw)
        out[mode] = {
            "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
            "zero_iteration_call_ms_mean": float(np.mean(ztimes)), "ms_per_iteration": per_iteration,
            "ns_per_point_and_iteration": 1e6 * per_iteration / N,
            "translation_error_before": float(before[0][0]), "translation_error_after": float(after[0][0]),
            "rotation_error_before": float(before[1][0]), "rotation_error_after": float(after[1][0]),
            "status": int(r.status), "history_first": r.history[0].tolist(), "history_last": r.history[-1].tolist(),
            "information_diagonal": r.information.diagonal().tolist(),
            "torch_ms_per_iteration_mean": float(np.mean(ttimes)),
            "torch_ms_per_iteration_extrapolated_to_all_points": float(np.mean(ttimes)) * N / float(sub.shape[0]),
            "torch_count_equal": bool(int(tcount) == int(one.history[0, 0])),
            "torch_pose_difference_max": float((tT - one.T.double()).abs().max())}
    return {"register": out}


NORMALS_RADIUS = REGISTER_MAX_DIST                      # the radius the registration above matches within
TORCH_NORMALS_CHUNK = 1 << 17


def torch_cloud_normals(query, cloud, radius):
    """The normals from torch ops (what a caller had to write without cloud_normals): the neighbours through torch.cdist
    over chunks of the cloud, the count and the first and second moments as fp64 matrix products with the 0/1 mask, the
    covariance, torch.linalg.eigh.  Returns (unit eigenvector of the smallest eigenvalue (Q,3) fp64, count (Q,))."""
    Q = query.shape[0]
    cnt = torch.zeros(Q, dtype=torch.float64, device=query.device)
    S = torch.zeros(Q, 3, dtype=torch.float64, device=query.device)
    SS = torch.zeros(Q, 9, dtype=torch.float64, device=query.device)
    for a in range(0, cloud.shape[0], TORCH_NORMALS_CHUNK):
        part = cloud[a:a + TORCH_NORMALS_CHUNK]
        w = (torch.cdist(query, part) <= radius).double()
        p = part.double()
        cnt += w.sum(dim=1)
        S += w @ p
        SS += w @ (p[:, :, None] * p[:, None, :]).reshape(-1, 9)
    n = cnt.clamp(min=1.0)[:, None]
    m = S / n
    C = (SS / n).reshape(Q, 3, 3) - m[:, :, None] * m[:, None, :]
    _, E = torch.linalg.eigh(C)
    return E[:, :, 0], cnt


def _angles(a, b, line=False):
    a, b = a.double(), b.double()
    ang = torch.atan2(torch.linalg.cross(a, b).norm(dim=1), (a * b).sum(dim=1))
    return torch.minimum(ang, np.pi - ang) if line else ang


def run_cloud_normals(sc, res, steps, warmup):
    steps, warmup = min(steps, 3), min(warmup, 1)           # (the calls are long: a tenth of a second or more)
    depth, K, T = sc["depth"], sc["K"], sc["T_cam_in_world"]
    points = res.points
    N = int(points.shape[0])
    centres = T[res.view.long(), :3, 3].float().contiguous()
    got, times = timed(lambda: cloud_normals(points, NORMALS_RADIUS, viewpoint=centres), steps, warmup)
    nn, qtimes = timed(lambda: cloud_nearest(points, points, NORMALS_RADIUS), steps, warmup)
    assert torch.equal(nn.within, got.count)
    truth = point_normals(res, depth_normals(depth, K, T_cam_in_world=T))
    has = (got.normals != 0).any(dim=1)
    both = has & (truth != 0).any(dim=1)
    ang = _angles(got.normals[both], truth[both]).sort().values
    sub = points[:TORCH_QUERIES].contiguous()
    (tn, tcount), ttimes = timed(lambda: torch_cloud_normals(sub, points, NORMALS_RADIUS), 2, 1)
    sub_has = has[:TORCH_QUERIES]
    scale = N / float(sub.shape[0])
    return {"cloud_normals": {
        "n_points": N, "radius": NORMALS_RADIUS, "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
        "ns_per_point": 1e6 * float(np.mean(times)) / N, "cloud_nearest_ms_mean": float(np.mean(qtimes)),
        "neighbours_mean": float(got.count.float().mean()), "neighbours_max": int(got.count.max()),
        "share_with_normal": float(has.float().mean()), "compared_with_point_normals": int(both.sum()),
        "angle_to_point_normals_mean": float(ang.mean()), "angle_to_point_normals_p99": float(ang[int(0.99 * (len(ang) - 1))]),
        "torch_points": int(sub.shape[0]), "torch_ms_mean": float(np.mean(ttimes)),
        "torch_ms_extrapolated_to_all_points": float(np.mean(ttimes)) * scale,
        "torch_count_differs": int((tcount.long() != got.count[:TORCH_QUERIES].long()).sum()),
        "torch_line_angle_max": float(_angles(tn[sub_has], got.normals[:TORCH_QUERIES][sub_has], line=True).max())
        if bool(sub_has.any()) else 0.0}}


KNN_RADIUS = NORMALS_RADIUS
KNN_K = (8, 32)
KNN_STD_RATIO = 2.0


def torch_cloud_knn(query, cloud, k, radius):
    """The k nearest other points from torch ops (what a caller had to write without cloud_knn): torch.cdist over chunks of
    the cloud, the point itself masked, topk per chunk, topk over the chunks' winners.  cdist's own arithmetic: at these sizes
    it takes the matrix-product form, whose error in d^2 (about 1e-7 of the coordinates' squares) is of the size of a nearest
    neighbour's d^2 itself, so its distances and with them its neighbours differ from the exact ones (the result reports by
    how much); its other form refuses a launch of this size.  The first rows of `cloud` are `query`.  Returns (dist (Q,k), index (Q,k))."""
    Q = query.shape[0]
    own = torch.arange(Q, device=query.device)
    best_d = torch.full((Q, k), float("inf"), device=query.device)
    best_i = torch.full((Q, k), -1, dtype=torch.int64, device=query.device)
    for a in range(0, cloud.shape[0], TORCH_NORMALS_CHUNK):
        d = torch.cdist(query, cloud[a:a + TORCH_NORMALS_CHUNK])
        if a < Q:
            rows = own[a:a + d.shape[1]]
            d[rows, rows - a] = float("inf")
        d = torch.where(d <= radius, d, torch.full((), float("inf"), device=d.device))
        cd, ci = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        md, mi = torch.cat([best_d, cd], dim=1), torch.cat([best_i, ci + a], dim=1)
        best_d, pick = torch.topk(md, k, dim=1, largest=False)
        best_i = torch.gather(mi, 1, pick)
    return best_d, torch.where(torch.isinf(best_d), torch.full_like(best_i, -1), best_i)


def run_knn(res, steps, warmup):
    steps, warmup = min(steps, 3), min(warmup, 1)           # (the calls are long: a tenth of a second or more)
    points = res.points
    N = int(points.shape[0])
    nn, qtimes = timed(lambda: cloud_nearest(points, points, KNN_RADIUS), steps, warmup)
    out = {"n_points": N, "radius": KNN_RADIUS, "cloud_nearest_ms_mean": float(np.mean(qtimes)),
           "neighbours_mean": float(nn.within.float().mean()) - 1.0, "neighbours_max": int(nn.within.max()) - 1}
    sub = points[:TORCH_QUERIES].contiguous()
    scale = N / float(sub.shape[0])
    for k in KNN_K:
        got, times = timed(lambda: cloud_knn(points, points, k, KNN_RADIUS, exclude_self=True), steps, warmup)
        assert torch.equal(got.within, nn.within - torch.isfinite(points).all(dim=1).int())
        (td, ti), ttimes = timed(lambda: torch_cloud_knn(sub, points, k, KNN_RADIUS), 2, 1)
        mine = got.dist2[:TORCH_QUERIES].sqrt()
        both = torch.isfinite(mine) & torch.isfinite(td)
        out["k%d" % k] = {
            "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
            "ns_per_point": 1e6 * float(np.mean(times)) / N, "share_with_fewer_than_k": float((got.within < k).float().mean()),
            "torch_points": int(sub.shape[0]), "torch_ms_mean": float(np.mean(ttimes)),
            "torch_ms_extrapolated_to_all_points": float(np.mean(ttimes)) * scale,
            "torch_distance_differs_max": float((mine[both] - td[both]).abs().max()) if bool(both.any()) else 0.0,
            "torch_index_differs": int((ti != got.index[:TORCH_QUERIES]).sum())}
    sor, stimes = timed(lambda: statistical_outlier_mask(points, KNN_K[0], KNN_STD_RATIO, KNN_RADIUS), steps, warmup)
    out["statistical_outlier_mask"] = {
        "k": KNN_K[0], "std_ratio": KNN_STD_RATIO, "ms_per_call_mean": float(np.mean(stimes)), "ms_per_call_min": float(np.min(stimes)),
        "share_kept": float(sor.keep.float().mean()), "share_without_k_neighbours": float(torch.isnan(sor.mean_dist).float().mean()),
        "mean": float(sor.mean), "std": float(sor.std)}
    return {"knn": out}


CLUSTER_EPS_VOXELS = 2.5
CLUSTER_MIN_POINTS = 8


def torch_cloud_clusters(points, eps, min_points):
    """The labelling of cloud_clusters composed from torch ops on top of cloud_knn's edge list (k = 64, the most it
    returns: a point with more neighbours loses edges): (root (N,) int64: the lowest core row of the point's cluster, -1
    for noise; rounds)."""
    N = points.shape[0]
    knn = cloud_knn(points, points, 64, eps, exclude_self=True)
    finite = torch.isfinite(points).all(dim=1)
    core = finite & (knn.within + 1 >= min_points)
    valid = knn.index >= 0
    to = knn.index.clamp(min=0)
    rows = torch.arange(N, device=points.device)
    edge = valid & core[:, None] & core[to]
    u, v = rows[:, None].expand_as(to)[edge], to[edge]
    label = rows.clone()
    rounds = 0
    while True:
        new = label.scatter_reduce(0, u, label[v], "amin")
        new = new[new]
        rounds += 1
        if bool(torch.equal(new, label)):          # the host read of the round
            break
        label = new
    near_core = valid & core[to]                  # the lists are sorted by (d2, row): the first core entry is the nearest
    pos = near_core.int().argmax(dim=1)
    joins = label[to[rows, pos]]
    border = finite & ~core & near_core.any(dim=1)
    return torch.where(core, label, torch.where(border, joins, torch.full_like(label, -1))), rounds


def run_clusters(res, fx, steps, warmup):
    voxel = float(np.float32(float(res.depth[res.depth > 0].median()) / fx))    # one pixel's footprint at the median depth
    points = voxel_merge(res.points, voxel, colors=res.colors).points.contiguous()
    eps = CLUSTER_EPS_VOXELS * voxel
    N = int(points.shape[0])
    got, times = timed(lambda: cloud_clusters(points, eps, CLUSTER_MIN_POINTS), steps, warmup)
    nn, qtimes = timed(lambda: cloud_nearest(points, points, eps), steps, warmup)
    assert torch.equal(got.within, nn.within)
    (troot, rounds), ttimes = timed(lambda: torch_cloud_clusters(points, eps, CLUSTER_MIN_POINTS), min(steps, 3), 1)
    C = int(got.first.shape[0])
    root = torch.where(got.label >= 0, got.first[got.label.clamp(min=0)], got.label) if C else got.label
    return {"clusters": {
        "voxel_size": voxel, "eps": eps, "min_points": CLUSTER_MIN_POINTS, "N": N, "C": C,
        "share_noise": float((got.label < 0).float().mean()), "share_core": float(got.core.float().mean()),
        "largest_cluster_share": float(got.count.max()) / N if C else 0.0,
        "neighbours_mean": float(got.within.float().mean()) - 1.0, "neighbours_max": int(got.within.max()) - 1,
        "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
        "cloud_nearest_ms_mean": float(np.mean(qtimes)),
        "torch_ms_per_call_mean": float(np.mean(ttimes)), "torch_ms_per_call_min": float(np.min(ttimes)),
        "torch_rounds": rounds, "points_with_more_than_64_neighbours": int((got.within > 65).sum()),
        "torch_labelling_equal": bool(torch.equal(troot, root)),
        "torch_rows_that_differ": int((troot != root).sum())}}


def torch_cloud_render(points, K, T, H, W, exact=False):
    """cloud_render at radius 0 composed from torch ops on the same device: per view the same camera (K T^-1 in fp64,
    rounded once), the rows as nested addcmul, the same pixel rule, then scatter_reduce_(amin) on int64 keys
    (bits of z << 32) | row -- what a caller had to write without the kernel.  addcmul rounds the product before the sum,
    so its z differs from the kernel's fused multiply-add in the last bit at many pixels; with ``exact`` every step of a
    row is formed in fp64 (the product of two fp32 numbers is exact there) and rounded to fp32 once: the kernel's fused
    multiply-add but for a double rounding, about once in 2^29 operations.  Returns (depth (V,H,W), index (V,H,W))."""
    V, N = K.shape[0], points.shape[0]
    Ti = torch.linalg.inv(T.double())
    P = torch.cat([K[:, :2, :3].double() @ Ti[:, :3, :], Ti[:, 2:3, :]], dim=1).float()             # (V,3,4)
    x, y, z = (points[:, k].contiguous() for k in range(3))
    rows = torch.arange(N, dtype=torch.int64, device=points.device)
    finite = torch.isfinite(points).all(dim=1)
    keys = torch.full((V, H * W), torch.iinfo(torch.int64).max, dtype=torch.int64, device=points.device)

    xd, yd, zd = (x.double(), y.double(), z.double()) if exact else (None, None, None)

    def row(p):
        if not exact:
            return torch.addcmul(torch.addcmul(torch.addcmul(p[3].expand(N), z, p[2]), y, p[1]), x, p[0])
        acc = p[3].double().expand(N)
        for coord, entry in ((zd, p[2]), (yd, p[1]), (xd, p[0])):
            acc = (coord * entry.double() + acc).float().double()
        return acc.float()
    for v in range(V):
        zc = row(P[v, 2])
        fc, fr = torch.floor(row(P[v, 0]) / zc + 0.5), torch.floor(row(P[v, 1]) / zc + 0.5)
        ok = finite & torch.isfinite(zc) & (zc > 0) & (fc >= 0) & (fc < W) & (fr >= 0) & (fr < H)
        pix = (fr[ok].to(torch.int64) * W + fc[ok].to(torch.int64))
        key = (zc[ok].view(torch.int32).to(torch.int64) << 32) | rows[ok]
        keys[v].scatter_reduce_(0, pix, key, "amin")
    hit = keys != torch.iinfo(torch.int64).max
    depth = torch.where(hit, (keys >> 32).to(torch.int32).view(torch.float32), torch.zeros((), device=points.device))
    index = torch.where(hit, keys & 0xFFFFFFFF, torch.full_like(keys, -1))
    return depth.reshape(V, H, W), index.reshape(V, H, W)


def render_debug_counts():
    """(candidates, atomics) so far of a library built with -DMVSN_RENDER_COUNT, None of the usual build."""
    import ctypes
    fn = getattr(_native.load(), "mvsn_cloud_render_debug_counts", None)
    if fn is None:
        return None
    out = (ctypes.c_uint64 * 2)()
    torch.cuda.synchronize()
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
    if fn(out) != 0:
        return None
    return int(out[0]), int(out[1])


def run_render(sc, res, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    V, _, H, W = depth.shape
    points = res.points
    N = int(points.shape[0])
    out = {"N": N, "V": V, "rows": H, "cols": W,
           "workspace_bytes": int(_native.load().mvsn_cloud_render_workspace_bytes(V, H, W))}
    for radius in (0, 1):
        before = render_debug_counts()
        r = cloud_render(points, K, T, (H, W), radius=radius)
        after = render_debug_counts()
        if before is not None and after is not None:
            cand, atom = after[0] - before[0], after[1] - before[1]
            out[f"radius{radius}_candidates"], out[f"radius{radius}_atomics"] = cand, atom
            out[f"radius{radius}_atomics_per_candidate"] = atom / max(cand, 1)
        _, times = timed(lambda: cloud_render(points, K, T, (H, W), radius=radius), steps, warmup)
        out[f"radius{radius}_ms_mean"], out[f"radius{radius}_ms_min"] = float(np.mean(times)), float(np.min(times))
        out[f"radius{radius}_share_of_pixels_hit"] = float((r.index >= 0).float().mean())
        if radius == 0:
            exact = r
    _, times = timed(lambda: cloud_render(points, K, T, (H, W), colors=res.colors), steps, warmup)
    out["radius0_with_colors_ms_mean"] = float(np.mean(times))
    vis, times = timed(lambda: cloud_visibility(points, depth, K, T), steps, warmup)
    out["visibility_ms_mean"], out["visibility_ms_min"] = float(np.mean(times)), float(np.min(times))
    out["views_per_point_mean"] = float(vis.count.float().mean())
    _, times = timed(lambda: cloud_visibility(points, depth, K, T, maps=images), steps, warmup)
    out["visibility_with_maps_ms_mean"], out["visibility_with_maps_ms_min"] = float(np.mean(times)), float(np.min(times))
    own = cloud_visibility(points, exact.depth, K, T, rel_tol=0.0)
    out["rendered_rows_visible_with_no_tolerance"] = all(      # (section 25's exact property, at the workload's size)
        bool(own.visible[exact.index[v][exact.index[v] >= 0], v].all()) for v in range(V))
    (tdepth, tindex), ttimes = timed(lambda: torch_cloud_render(points, K, T, H, W), min(steps, 3), 1)
    out["torch_ms_mean"], out["torch_ms_min"] = float(np.mean(ttimes)), float(np.min(ttimes))
    same = tdepth.view(torch.int32) == exact.depth[:, 0].view(torch.int32)
    out["torch_pixels_whose_depth_bits_differ"] = int((~same).sum())
    out["torch_pixels_whose_index_differs"] = int((tindex != exact.index).sum())
    # the same composition with every fused multiply-add formed exactly: the check that both compute the same thing
    (edepth, eindex), etimes = timed(lambda: torch_cloud_render(points, K, T, H, W, exact=True), min(steps, 3), 1)
    same = edepth.view(torch.int32) == exact.depth[:, 0].view(torch.int32)
    out["torch_exact_ms_mean"] = float(np.mean(etimes))
    out["torch_exact_depth_bits_equal"] = bool(same.all())
    out["torch_exact_pixels_whose_depth_bits_differ"] = int((~same).sum())
    out["torch_exact_pixels_whose_index_differs"] = int((eindex != exact.index).sum())
    return {"render": out}


GLOBAL_GRID = 128                     # the target is a GLOBAL_GRID^2 sampling of a height field over [-1,1]^2
GLOBAL_BUMPS = ((0.45, 0.50, 0.22, 0.55), (-0.50, 0.35, 0.35, -0.40), (-0.30, -0.55, 0.15, 0.45), (0.55, -0.40, 0.28, 0.30))
GLOBAL_FEATURE_RADIUS, GLOBAL_MAX_DIST, GLOBAL_EDGE_SIMILARITY, GLOBAL_HYPOTHESES = 0.25, 0.15, 0.98, 100000


def global_scene(dev):
    """(source, target, T_true): an asymmetric height field (four Gaussian bumps and a step edge) sampled on a grid (target)
    and on the same grid shifted by half a spacing with every fourth row dropped (source), the source moved by 2.5 rad
    about (1, 2, -1.5) and by (3, -2, 5); T_true (4,4) fp64 takes it back."""
    def height(x, y):
        z = torch.zeros_like(x)
        for cx, cy, width, h in GLOBAL_BUMPS:
            z = z + h * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * width * width))
        return z + 0.12 * torch.tanh((x + 0.4 * y - 0.15) / (4.0 / (GLOBAL_GRID - 1)))
    g = torch.linspace(-1.0, 1.0, GLOBAL_GRID, dtype=torch.float64, device=dev)
    Y, X = torch.meshgrid(g, g, indexing="ij")
    target = torch.stack([X, Y, height(X, Y)], dim=-1).reshape(-1, 3)
    keep = torch.arange(GLOBAL_GRID, device=dev) % 4 != 3
    half = 1.0 / (GLOBAL_GRID - 1)
    Xs, Ys = X[keep] + half, Y[keep] + half
    src = torch.stack([Xs, Ys, height(Xs, Ys)], dim=-1).reshape(-1, 3)
    w = torch.nn.functional.normalize(torch.tensor([1.0, 2.0, -1.5], dtype=torch.float64), dim=0) * 2.5
    Wx = torch.zeros(3, 3, dtype=torch.float64)
    Wx[0, 1], Wx[0, 2], Wx[1, 0], Wx[1, 2], Wx[2, 0], Wx[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3], M[:3, 3] = torch.linalg.matrix_exp(Wx), torch.tensor([3.0, -2.0, 5.0], dtype=torch.float64)
    M = M.to(dev)
    source = (src @ M[:3, :3].T + M[:3, 3]).float()
    return source.contiguous(), target.float().contiguous(), torch.linalg.inv(M)


def run_global(steps, warmup):
    """Global registration stage by stage (fusion.cloud_register_global's own composition), the descriptor match also from
    torch ops (torch.cdist + min: what a caller had to write without feature_nearest)."""
    steps, warmup = min(steps, 3), min(warmup, 1)
    dev = torch.device("cuda:0")
    source, target, T_true = global_scene(dev)
    nr = GLOBAL_FEATURE_RADIUS / 2
    sn, tn = cloud_normals(source, nr).normals, cloud_normals(target, nr).normals
    fs, ftimes = timed(lambda: cloud_fpfh(source, sn, GLOBAL_FEATURE_RADIUS), steps, warmup)
    ft, gtimes = timed(lambda: cloud_fpfh(target, tn, GLOBAL_FEATURE_RADIUS), steps, warmup)
    m, mtimes = timed(lambda: feature_nearest(fs.features, ft.features, mutual=True), steps, warmup)
    one, otimes = timed(lambda: feature_nearest(fs.features, ft.features), steps, warmup)
    (td, ti), ttimes = timed(lambda: torch.cdist(fs.features, ft.features).min(dim=1), steps, warmup)
    rows = torch.nonzero((m.index >= 0) & m.mutual).reshape(-1)
    corr = torch.stack([rows, m.index[rows]], dim=1).contiguous()
    kw = dict(hypotheses=GLOBAL_HYPOTHESES, seed=0, edge_similarity=GLOBAL_EDGE_SIMILARITY)
    coarse, rtimes = timed(lambda: cloud_ransac(source, target, corr, GLOBAL_MAX_DIST, **kw), steps, warmup)
    whole, wtimes = timed(lambda: cloud_register_global(source, target, GLOBAL_MAX_DIST, feature_radius=GLOBAL_FEATURE_RADIUS, **kw),
                          steps, warmup)
    before, after = pose_errors(coarse.T[None], T_true[None]), pose_errors(whole.T[None], T_true[None])
    return {"global": {
        "n_source": int(source.shape[0]), "n_target": int(target.shape[0]), "feature_radius": GLOBAL_FEATURE_RADIUS,
        "max_dist": GLOBAL_MAX_DIST, "edge_similarity": GLOBAL_EDGE_SIMILARITY, "hypotheses": GLOBAL_HYPOTHESES,
        "pairs_mean": float(fs.pairs.float().mean()), "pairs_max": int(fs.pairs.max()),
        "fpfh_source_ms_mean": float(np.mean(ftimes)), "fpfh_target_ms_mean": float(np.mean(gtimes)),
        "match_mutual_ms_mean": float(np.mean(mtimes)), "match_one_way_ms_mean": float(np.mean(otimes)),
        "torch_cdist_min_ms_mean": float(np.mean(ttimes)), "torch_index_differs": int((ti != one.index).sum()),
        "correspondences": int(corr.shape[0]), "ransac_ms_mean": float(np.mean(rtimes)), "ransac_inliers": int(coarse.inliers),
        "ransac_status": int(coarse.status), "coarse_equals_the_stages": bool(torch.equal(whole.coarse.T, coarse.T)),
        "cloud_register_global_ms_mean": float(np.mean(wtimes)),
        "translation_error_coarse": float(before[0][0]), "rotation_error_coarse": float(before[1][0]),
        "translation_error_refined": float(after[0][0]), "rotation_error_refined": float(after[1][0]),
        "refine_status": int(whole.refined.status)}}


MESH_MIN_FACES = 200


def torch_mesh_components(faces, m):
    """The labelling from torch ops: every vertex takes the lowest label across the sides of its faces
    (scatter_reduce amin), then one pointer jump, repeated to a fixed point with a host read per round (what a caller had
    to write without mesh_components).  Returns (the lowest row of every vertex's component (m,), rounds)."""
    u = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2]])
    v = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0]])
    label = torch.arange(m, dtype=torch.int64, device=faces.device)
    rounds = 0
    while True:
        rounds += 1
        new = label.scatter_reduce(0, u, label[v], "amin").scatter_reduce(0, v, label[u], "amin")
        new = new[new]
        if bool((new == label).all()):                      # the host read of the round
            return label, rounds
        label = new


def run_mesh(sc, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, 4 * TSDF_VOXEL, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    m, f = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    comp, times = timed(lambda: mesh_components(mesh.faces, m), steps, warmup)
    clean, ftimes = timed(lambda: filter_mesh(mesh, min_faces=MESH_MIN_FACES), steps, warmup)
    _, stimes = timed(lambda: filter_mesh(mesh, min_faces=MESH_MIN_FACES, components=comp), steps, warmup)
    (tlabel, rounds), ttimes = timed(lambda: torch_mesh_components(mesh.faces, m), min(steps, 3), 1)
    c = int(comp.first.shape[0])
    return {"mesh": {
        "dims": list(TSDF_DIMS), "voxel_size": TSDF_VOXEL, "M": m, "F": f, "C": c,
        "largest_component_share_of_faces": float(comp.face_count.max()) / max(f, 1),
        "largest_component_share_of_vertices": float(comp.vertex_count.max()) / max(m, 1),
        "workspace_bytes": int(_native.load().mvsn_mesh_workspace_bytes(m, f)),
        "components_ms_per_call_mean": float(np.mean(times)), "components_ms_per_call_min": float(np.min(times)),
        "min_faces": MESH_MIN_FACES, "filter_ms_per_call_mean": float(np.mean(ftimes)),
        "filter_ms_per_call_min": float(np.min(ftimes)),
        "filter_with_components_handed_in_ms_mean": float(np.mean(stimes)),
        "kept_components": int((comp.face_count >= MESH_MIN_FACES).sum()),
        "kept_vertices": int(clean.mesh.vertices.shape[0]), "kept_faces": int(clean.mesh.faces.shape[0]),
        "torch_ms_per_call_mean": float(np.mean(ttimes)), "torch_ms_per_call_min": float(np.min(ttimes)),
        "torch_rounds": rounds, "torch_partition_equal": bool(torch.equal(tlabel, comp.first[comp.vertex_label]))}}


MESH_SAMPLES = 1 << 20
TORCH_FACE_CHUNK = 1 << 14


def torch_mesh_nearest(query, vertices, faces, max_dist):
    """mesh_nearest's distance from torch ops, every face against every query in chunks of faces: the normative fp64
    steps, one torch op each, then the fp32 clamp and d2; the running minimum over
    (d2, face).  Returns (dist2, face)."""
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]      # noqa: E731
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],                # noqa: E731
                                      a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    h = torch.tensor(max_dist, dtype=torch.float32, device=query.device)
    r2 = h * h
    best = torch.full((query.shape[0],), float("inf"), device=query.device)
    index = torch.full((query.shape[0],), -1, dtype=torch.int64, device=query.device)
    qd = query.double()[:, None, :]
    for s0 in range(0, faces.shape[0], TORCH_FACE_CHUNK):
        p32 = vertices[faces[s0:s0 + TORCH_FACE_CHUNK]][None]                # (1, f, 3, 3)
        P = p32.double()
        a = P[..., 0, :]
        ab, ac, aq = P[..., 1, :] - a, P[..., 2, :] - a, qd - a
        n = cross(ab, ac)
        nn = dot(n, n)
        wb, wc = dot(cross(aq, ac), n) / nn, dot(cross(ab, aq), n) / nn
        wa = (1.0 - wb) - wc
        inside = (nn > 0) & (wb >= 0) & (wc >= 0) & (wa >= 0)
        x = (a + wb[..., None] * ab) + wc[..., None] * ac
        bestd, xe = None, None
        for k in range(3):
            p0 = P[..., k, :]
            e, d = P[..., (k + 1) % 3, :] - p0, qd - p0
            ee = dot(e, e)
            r = dot(d, e) / ee
            t = torch.where(ee > 0, torch.where(r > 0, torch.where(r < 1, r, torch.ones_like(r)), torch.zeros_like(r)),
                            torch.zeros_like(r))
            xs = p0 + t[..., None] * e
            d = qd - xs
            dd = dot(d, d)
            take = dd < bestd if bestd is not None else None
            bestd = dd if take is None else torch.where(take, dd, bestd)
            xe = xs if take is None else torch.where(take[..., None], xs, xe)
        x = torch.where(inside[..., None], x, xe).float()
        x = torch.maximum(torch.minimum(x, p32.amax(dim=-2)), p32.amin(dim=-2))
        df = query[:, None, :] - x
        d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
        d2 = torch.where(d2 <= r2, d2, torch.full_like(d2, float("inf")))
        m, i = d2.min(dim=1)
        closer = m < best
        best, index = torch.where(closer, m, best), torch.where(closer, i + s0, index)
    return best, index


def run_mesh_metrics(sc, res, steps, warmup):
    steps, warmup = min(steps, 5), min(warmup, 1)           # (the calls are long: milliseconds)
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, 4 * TSDF_VOXEL, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    v, f, truth = mesh.vertices, mesh.faces, res.points
    m, nf, n = int(v.shape[0]), int(f.shape[0]), int(truth.shape[0])
    _, inv, _ = cloud_radius_scalars(TSDF_VOXEL)
    head = torch.empty(3, dtype=torch.int64, device=v.device)
    _native.check(_native.load().mvsn_mesh_nearest_count(_native.ptr(v), m, _native.ptr(f), nf, float(inv),
                                                         _native.ptr(head), _native.stream()), "mvsn_mesh_nearest_count")
    pairs, large, _ = head.tolist()
    _, stimes = timed(lambda: mesh_sample(v, f, MESH_SAMPLES, normals=mesh.normals, colors=mesh.colors), steps, warmup)
    near, ntimes = timed(lambda: mesh_nearest(truth, v, f, TSDF_VOXEL), steps, warmup)
    scores, mtimes = timed(lambda: mesh_metrics(v, f, truth, TSDF_VOXEL, samples=MESH_SAMPLES), steps, warmup)
    _, ctimes = timed(lambda: cloud_nearest(truth, v, TSDF_VOXEL), steps, warmup)
    q = truth[:TORCH_QUERIES]
    (td2, tface), ttimes = timed(lambda: torch_mesh_nearest(q, v, f, TSDF_VOXEL), 2, 1)
    found = torch.isfinite(near.dist2)
    return {"mesh_metrics": {
        "M": m, "F": nf, "N": n, "pairs": pairs, "large_faces": large, "max_dist": TSDF_VOXEL, "samples": MESH_SAMPLES,
        "workspace_bytes": int(_native.load().mvsn_mesh_nearest_workspace_bytes(pairs, large)),
        "sample_ms_per_call_mean": float(np.mean(stimes)), "sample_ms_per_call_min": float(np.min(stimes)),
        "nearest_ms_per_call_mean": float(np.mean(ntimes)), "nearest_ms_per_call_min": float(np.min(ntimes)),
        "metrics_ms_per_call_mean": float(np.mean(mtimes)), "metrics_ms_per_call_min": float(np.min(mtimes)),
        "cloud_nearest_against_vertices_ms_mean": float(np.mean(ctimes)),
        "found_fraction": float(found.float().mean()), "within_mean_where_found": float(near.within[found].float().mean()),
        "torch_queries": int(q.shape[0]), "torch_ms_per_call_mean": float(np.mean(ttimes)),
        "torch_extrapolated_ms_all_queries": float(np.mean(ttimes)) * n / max(int(q.shape[0]), 1),
        "torch_rows_whose_dist2_bits_differ": int((td2.view(torch.int32) != near.dist2[:TORCH_QUERIES].view(torch.int32)).sum()),
        "torch_rows_whose_face_differs": int((tface != near.face[:TORCH_QUERIES]).sum()),
        "scores": scores, "vertices_as_a_cloud": cloud_metrics(v, truth, TSDF_VOXEL)}}


def run_mesh_render(sc, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    V, _, H, W = depth.shape
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, 4 * TSDF_VOXEL, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    v, f = mesh.vertices, mesh.faces
    r, times = timed(lambda: mesh_render(v, f, K, T, (H, W)), steps, warmup)
    full, gtimes = timed(lambda: mesh_render(v, f, K, T, (H, W), normals=mesh.normals, colors=mesh.colors), steps, warmup)
    cloud, ctimes = timed(lambda: cloud_render(v, K, T, (H, W)), steps, warmup)
    ray = vol.raycast(K, T, (H, W))
    hit, rhit = r.depth > 0, ray.depth > 0
    both = hit & rhit
    diff = ((r.depth - ray.depth).abs()[both] / TSDF_VOXEL).double()
    return {"mesh_render": {
        "M": int(v.shape[0]), "F": int(f.shape[0]), "views": V, "pixels": V * H * W,
        "workspace_bytes": int(_native.load().mvsn_mesh_render_workspace_bytes(V, H, W)),
        "small_pixels": int(_native.load().mvsn_mesh_render_small_pixels()),
        "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
        "with_gathers_ms_per_call_mean": float(np.mean(gtimes)), "with_gathers_ms_per_call_min": float(np.min(gtimes)),
        "cloud_render_of_vertices_ms_per_call_mean": float(np.mean(ctimes)),
        "cloud_render_of_vertices_hit_share": float((cloud.depth > 0).float().mean()),
        "hit_share": float(hit.float().mean()), "clipped_sum": int(r.clipped.sum()),
        "gathers_same_depth": bool(torch.equal(full.depth, r.depth)),
        "raycast_hit_share": float(rhit.float().mean()), "both_hit_share": float(both.float().mean()),
        "hit_mask_agreement": float((hit == rhit).float().mean()),
        "abs_depth_minus_raycast_voxels_median": float(diff.median()) if diff.numel() else 0.0,
        "abs_depth_minus_raycast_voxels_p99": float(torch.quantile(diff[:: max(1, diff.numel() // (1 << 22))], 0.99))
        if diff.numel() else 0.0}}


SIMPLIFY_VOXELS = (1, 2, 4)         # cell sizes of --simplify, in volume voxels


def torch_mesh_simplify(v, f, voxel, origin):
    """The clustering from torch ops: voxel_merge for the vertex side (the mean), the faces through its inverse, the
    collapsed ones masked out, torch.unique over the canonical triples (which sorts them: the faces come out in triple
    order, not in input order, and without their input rows), the used clusters renumbered."""
    vc = voxel_merge(v, voxel, origin=origin)
    g = vc.inverse[f]
    g = g[(g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2]) & (g >= 0).all(dim=1)]
    k = g.argmin(dim=1, keepdim=True)
    canon = torch.cat([g.gather(1, k), g.gather(1, (k + 1) % 3), g.gather(1, (k + 2) % 3)], dim=1)
    faces = torch.unique(canon, dim=0)
    used = torch.zeros(vc.points.shape[0], dtype=torch.bool, device=v.device)
    used[faces.reshape(-1)] = True
    row = torch.cumsum(used, 0) - 1
    return vc.points[used], row[faces]


def simplify_fallbacks(v, f, size, origin, placement):
    """The fourth result word of mvsn_mesh_simplify_mark: the clusters whose position fell back to a member's."""
    lib, m, nf = _native.load(), int(v.shape[0]), int(f.shape[0])
    s = np.float32(size)
    scalars = (float(s), float(np.float32(1) / s)) + tuple(float(np.float32(x)) for x in origin)
    ws_bytes = lib.mvsn_mesh_simplify_workspace_bytes(m, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
    head = torch.empty(4, dtype=torch.int64, device=v.device)
    _native.check(lib.mvsn_mesh_simplify_assign(_native.ptr(v), m, *scalars, _native.ptr(head), _native.ptr(ws), ws_bytes,
                                                _native.stream()), "mvsn_mesh_simplify_assign")
    clusters = int(head[0])
    _native.check(lib.mvsn_mesh_simplify_mark(_native.ptr(v), None, None, m, _native.ptr(f), nf, *scalars,
                                              {"mean": 0, "quadric": 1}[placement], 1, clusters, _native.ptr(head),
                                              _native.ptr(ws), ws_bytes, _native.stream()), "mvsn_mesh_simplify_mark")
    return int(head[3])


def run_simplify(sc, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, 4 * TSDF_VOXEL, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    v, f = mesh.vertices, mesh.faces
    m, nf = int(v.shape[0]), int(f.shape[0])
    lib = _native.load()
    out = {"M": m, "F": nf, "samples": MESH_SAMPLES, "workspace_bytes": int(lib.mvsn_mesh_simplify_workspace_bytes(m, nf))}
    for cells in SIMPLIFY_VOXELS:
        size = cells * TSDF_VOXEL
        diagonal = float(np.sqrt(3.0) * size)
        row = {}
        for placement in ("mean", "quadric"):
            call = lambda: mesh_simplify(v, f, size, origin=TSDF_ORIGIN, placement=placement, normals=mesh.normals,  # noqa: E731
                                         colors=mesh.colors)
            small, times = timed(call, steps, warmup)
            bare, btimes = timed(lambda: mesh_simplify(v, f, size, origin=TSDF_ORIGIN, placement=placement), steps, warmup)
            pts = mesh_sample(small.vertices, small.faces, MESH_SAMPLES, seed=1).points
            near = mesh_nearest(pts, v, f, diagonal)
            d = near.dist2[torch.isfinite(near.dist2)].double().sqrt() / TSDF_VOXEL
            row[placement] = {"M_out": int(small.vertices.shape[0]), "F_out": int(small.faces.shape[0]),
                              "ms_per_call_mean": float(np.mean(times)), "ms_per_call_min": float(np.min(times)),
                              "without_attributes_ms_per_call_mean": float(np.mean(btimes)),
                              "same_mesh_without_attributes": bool(torch.equal(bare.vertices, small.vertices) and
                                                                   torch.equal(bare.faces, small.faces)),
                              "fallbacks": simplify_fallbacks(v, f, size, TSDF_ORIGIN, placement),
                              "samples_within_the_cell_diagonal": float(torch.isfinite(near.dist2).float().mean()),
                              "distance_voxels_mean": float(d.mean()), "distance_voxels_max": float(d.max())}
        (tv, tf), ttimes = timed(lambda: torch_mesh_simplify(v, f, size, TSDF_ORIGIN), steps, warmup)
        row["torch"] = {"M_out": int(tv.shape[0]), "F_out": int(tf.shape[0]), "ms_per_call_mean": float(np.mean(ttimes)),
                        "ms_per_call_min": float(np.min(ttimes)),
                        "same_counts_as_mean": bool(tv.shape[0] == row["mean"]["M_out"] and tf.shape[0] == row["mean"]["F_out"])}
        row["device_call_beats_torch"] = bool(row["mean"]["without_attributes_ms_per_call_mean"] < row["torch"]["ms_per_call_mean"])
        out["cells_%d" % cells] = row
    return {"simplify": out}


SMOOTH_ITERATIONS = 10               # Taubin iterations of --smooth: 20 steps per call


def torch_mesh_edges(f, m):
    """The distinct unordered pairs of the sides from torch ops: sorted pairs packed into one int64, torch.unique (which
    sorts them: the edges come out in pair order, without first, counts per side or windings)."""
    sides = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    sides = sides[((f >= 0) & (f < m)).all(dim=1).repeat(3) & (sides[:, 0] != sides[:, 1])]
    key = torch.unique((sides.min(dim=1).values << 32) | sides.max(dim=1).values)
    return torch.stack([key >> 32, key & 0xffffffff], dim=1)


def torch_mesh_smooth(v, edges, iterations, lam, mu):
    """Taubin smoothing over `edges` from torch ops, in fp64 (float sums: the result depends on the order index_add_
    happens to add in)."""
    a, b = edges[:, 0], edges[:, 1]
    x = v.double()
    degree = torch.zeros(v.shape[0], dtype=torch.float64, device=v.device)
    degree.index_add_(0, a, torch.ones_like(a, dtype=torch.float64))
    degree.index_add_(0, b, torch.ones_like(b, dtype=torch.float64))
    degree = degree.clamp_(min=1.0)[:, None]
    for _ in range(iterations):
        for factor in (lam, mu):
            d = x[b] - x[a]
            total = torch.zeros_like(x)
            total.index_add_(0, a, d)
            total.index_add_(0, b, -d)
            x = x + factor * (total / degree)
    return x.float()


def run_smooth(sc, steps, warmup):
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, 4 * TSDF_VOXEL, device=depth.device, color=True)
    vol.integrate(depth, K, T, images=images)
    mesh = vol.extract_mesh()
    v, f = mesh.vertices, mesh.faces
    m, nf = int(v.shape[0]), int(f.shape[0])
    lib = _native.load()
    edges, etimes = timed(lambda: mesh_edges(f, m), steps, warmup)
    smooth, stimes = timed(lambda: mesh_smooth(v, f, SMOOTH_ITERATIONS, edges=edges), steps, warmup)
    _, wtimes = timed(lambda: mesh_smooth(v, f, SMOOTH_ITERATIONS), steps, warmup)
    normals, ntimes = timed(lambda: mesh_normals(smooth.vertices, f), steps, warmup)
    tedges, tetimes = timed(lambda: torch_mesh_edges(f, m), steps, warmup)
    tsmooth, tstimes = timed(lambda: torch_mesh_smooth(v, tedges, SMOOTH_ITERATIONS, 0.5, -0.53), steps, warmup)
    finite = torch.isfinite(v).all(dim=1)
    moved = (smooth.vertices - v)[finite].double().norm(dim=1) / TSDF_VOXEL
    apart = (smooth.vertices - tsmooth)[finite].double().norm(dim=1) / TSDF_VOXEL
    outwards = (normals.vertex_normals * mesh.normals).sum(dim=1)
    n_steps = 2 * SMOOTH_ITERATIONS
    return {"smooth": {
        "M": m, "F": nf, "E": int(edges.edges.shape[0]), "iterations": SMOOTH_ITERATIONS, "steps_per_call": n_steps,
        "border_edges": int((edges.face_count == 1).sum()), "non_manifold_edges": int((edges.face_count > 2).sum()),
        "inconsistent_interior_edges": int(((edges.face_count == 2) & (edges.winding != 0)).sum()),
        "border_vertices": int(edges.vertex_boundary.sum()),
        "workspace_bytes": {"edges": int(lib.mvsn_mesh_edges_workspace_bytes(m, nf)) if nf else 0,
                            "smooth": int(lib.mvsn_mesh_smooth_workspace_bytes(m)),
                            "normals": int(lib.mvsn_mesh_normals_workspace_bytes(m))},
        "edges_ms_per_call_mean": float(np.mean(etimes)), "edges_ms_per_call_min": float(np.min(etimes)),
        "smooth_ms_per_call_mean": float(np.mean(stimes)), "smooth_ms_per_call_min": float(np.min(stimes)),
        "smooth_ms_per_step_mean": float(np.mean(stimes)) / n_steps,
        "smooth_with_its_own_edges_ms_per_call_mean": float(np.mean(wtimes)),
        "normals_ms_per_call_mean": float(np.mean(ntimes)), "normals_ms_per_call_min": float(np.min(ntimes)),
        "moved_voxels_mean": float(moved.mean()) if m else 0.0, "moved_voxels_max": float(moved.max()) if m else 0.0,
        "vertex_normals_along_the_tsdf_gradient": float((outwards > 0).float().mean()) if m else 0.0,
        "torch": {"E": int(tedges.shape[0]), "edges_ms_per_call_mean": float(np.mean(tetimes)),
                  "smooth_ms_per_call_mean": float(np.mean(tstimes)), "smooth_ms_per_call_min": float(np.min(tstimes)),
                  "smooth_ms_per_step_mean": float(np.mean(tstimes)) / n_steps,
                  "same_edge_count": bool(tedges.shape[0] == edges.edges.shape[0]),
                  "vertices_apart_voxels_max": float(apart.max()) if m else 0.0},
        "device_edges_beat_torch": bool(np.mean(etimes) < np.mean(tetimes)),
        "device_smooth_beats_torch": bool(np.mean(stimes) < np.mean(tstimes))}}


CLOUD_VOLUME_RADIUS_VOXELS, TORCH_VOXELS, TORCH_POINT_CHUNK = 3, 1024, 1 << 16


def torch_integrate_cloud(centres, points, normals, radius, trunc):
    """The sums of integrate_cloud at the voxel centres `centres` (Q,3) from torch ops: chunks of the cloud through
    torch.cdist (its own arithmetic, so a row at the edge of the reach may fall on the other side), the weights
    (1 - d2 / r2)^2 and the clamped plane distances as (Q, chunk) tensors in HBM, float sums in arrival order (what a
    caller had to write without the kernel): (weight (Q,), sdf_sum (Q,))."""
    w = torch.zeros(centres.shape[0], dtype=torch.float32, device=centres.device)
    s = torch.zeros_like(w)
    r2 = radius * radius
    for a in range(0, points.shape[0], TORCH_POINT_CHUNK):
        p, n = points[a:a + TORCH_POINT_CHUNK], normals[a:a + TORCH_POINT_CHUNK]
        d2 = torch.cdist(centres, p) ** 2
        ok = (d2 <= r2) & (n != 0).any(1)[None, :]
        phi = torch.where(ok, (1 - d2 / r2) ** 2, torch.zeros_like(d2))
        dist = (centres[:, None, :] - p[None, :, :]).mul(n[None, :, :]).sum(2).clamp(-trunc, trunc)
        w += phi.sum(1)
        s += (phi * dist).sum(1)
    return w, s


def run_cloud_volume(sc, res, steps, warmup):
    steps, warmup = min(steps, 5), min(warmup, 1)           # (the calls are long: milliseconds)
    depth, K, T, images = sc["depth"], sc["K"], sc["T_cam_in_world"], sc["images"]
    dev = depth.device
    trunc, radius = 4 * TSDF_VOXEL, CLOUD_VOLUME_RADIUS_VOXELS * TSDF_VOXEL
    maps = depth_normals(depth, K, T_cam_in_world=T)
    vc = voxel_merge(res.points, float(np.float32(float(res.depth[res.depth > 0].median()) / float(K[0, 0, 0]))), colors=res.colors)
    vn = voxel_normals(vc, point_normals(res, maps))
    pts = vc.points.contiguous()
    n = int(pts.shape[0])
    vol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, trunc, device=dev)
    _, times = timed(lambda: vol.integrate_cloud(pts, vn, radius), steps, warmup)
    vol.reset()
    vol.integrate_cloud(pts, vn, radius)
    mesh, etimes = timed(lambda: vol.extract_mesh(), steps, warmup)
    # the brick flags of one more call, through the entries, into a scratch state
    lib = _native.load()
    h, inv, r2 = cloud_radius_scalars(radius)
    nx, ny, nz = TSDF_DIMS
    flag_bytes = lib.mvsn_tsdf_cloud_workspace_bytes(nx, ny, nz)
    flags = torch.empty(flag_bytes, dtype=torch.uint8, device=dev)
    scratch = (torch.zeros_like(vol.sdf_sum), torch.zeros_like(vol.weight))
    ws_bytes = lib.mvsn_cloud_workspace_bytes(n)
    ws, status = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    st = _native.stream()
    _native.check(lib.mvsn_cloud_index_build(_native.ptr(pts), n, float(h), float(inv), _native.ptr(status), _native.ptr(ws),
                                             ws_bytes, st), "mvsn_cloud_index_build")
    _, itimes = timed(lambda: _native.check(lib.mvsn_tsdf_cloud_integrate(
        _native.ptr(pts), _native.ptr(vn), None, None, n, _native.ptr(ws), ws_bytes, float(h), float(inv), float(r2), nx, ny, nz,
        float(vol.voxel_size), *(float(o) for o in vol.origin), float(vol.trunc), _native.ptr(scratch[0]), _native.ptr(scratch[1]),
        None, _native.ptr(flags), flag_bytes, st), "mvsn_tsdf_cloud_integrate"), steps, warmup)
    bricks = -(-nx // 8) * -(-ny // 8) * -(-nz // 8)
    flagged = int(flags[:bricks].sum())
    # the torch composition at a sample of the voxels the device updated
    seen = torch.nonzero(vol.weight.reshape(-1) > 0)[:, 0]
    pick = seen[torch.randperm(seen.shape[0], generator=torch.Generator().manual_seed(0))[:TORCH_VOXELS].to(dev)]
    k, j, i = pick // (nx * ny), (pick // nx) % ny, pick % nx
    centres = torch.stack([i, j, k], 1).to(torch.float32) * float(vol.voxel_size) + torch.tensor(vol.origin, device=dev)
    (tw, ts), ttimes = timed(lambda: torch_integrate_cloud(centres, pts, vn, float(h), float(vol.trunc)), 2, 1)
    dw, dsum = vol.weight.reshape(-1)[pick], vol.sdf_sum.reshape(-1)[pick]
    strong = dw >= 1
    # the same views through integrate, for the scores next to each other
    dvol = TSDFVolume(TSDF_DIMS, TSDF_VOXEL, TSDF_ORIGIN, trunc, device=dev)
    dvol.integrate(depth, K, T)
    dmesh = dvol.extract_mesh()
    score = lambda m: mesh_metrics(m.vertices, m.faces, res.points, TSDF_VOXEL, samples=MESH_SAMPLES)   # noqa: E731
    return {"cloud_volume": {
        "N": n, "radius": radius, "trunc": trunc, "bricks": bricks, "flagged_bricks": flagged,
        "voxels_updated": int(seen.shape[0]), "ms_per_call_median": float(np.median(times)),
        "ms_per_call_min": float(np.min(times)), "entry_only_ms_per_call_median": float(np.median(itimes)),
        "extract_ms_per_call_median": float(np.median(etimes)), "M": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0]),
        "scores": score(mesh), "scores_of_the_depth_map_volume": score(dmesh),
        "M_of_the_depth_map_volume": int(dmesh.vertices.shape[0]), "F_of_the_depth_map_volume": int(dmesh.faces.shape[0]),
        "torch_voxels": int(pick.shape[0]), "torch_ms_per_call_mean": float(np.mean(ttimes)),
        "torch_extrapolated_ms_all_flagged_voxels": float(np.mean(ttimes)) * flagged * 512 / max(int(pick.shape[0]), 1),
        "torch_max_abs_weight_difference": float((tw - dw).abs().max()),
        "torch_max_abs_value_difference_where_weight_at_least_1":
            float((ts[strong] / tw[strong] - dsum[strong] / dw[strong]).abs().max()) if bool(strong.any()) else 0.0}}


def run(V, H, W, M, steps, warmup, confidence=False, voxel=False, normals=False, cloud=False, tsdf=False, raycast=False,
        align=False, mesh=False, register=False, cloud_normals_too=False, knn=False, clusters=False, render=False, mesh_metrics_too=False, mesh_render_too=False,
        simplify_too=False, smooth_too=False, cloud_volume_too=False):
    dev = torch.device("cuda:0")
    sc = synthetic.fusion_scene(V, H, W, arc=0.02 * (V - 1), device=dev)
    nb = neighbours(V, M)
    args = (sc["depth"], sc["K"], sc["T_cam_in_world"], nb)
    res, times = timed(lambda: fuse_depthmaps(*args, images=sc["images"]), steps, warmup)
    P, N = H * W, int(res.points.shape[0])
    gated = {}
    if confidence:
        conf = torch.rand(V, 1, H, W, generator=torch.Generator().manual_seed(0)).to(dev)
        gres, gtimes = timed(lambda: fuse_depthmaps(*args, images=sc["images"], confidence=conf, min_confidence=0.25),
                             steps, warmup)
        gated = {"gated": {"min_confidence": 0.25, "ms_per_call_median": float(np.median(gtimes)),
                           "ms_per_call_min": float(np.min(gtimes)), "points": int(gres.points.shape[0]),
                           "mask_bytes": 5 * V * P + V * P}}
    merged = run_voxel(res, float(sc["K"][0, 0, 0]), steps, warmup) if voxel else {}
    oriented = run_normals(sc, res, steps, warmup) if normals else {}
    scored = run_cloud(sc, nb, res, steps, warmup) if cloud else {}
    volume = run_tsdf(sc, res, steps, warmup) if tsdf else {}
    rendered = run_raycast(sc, steps, warmup) if raycast else {}
    aligned = run_align(sc, steps, warmup) if align else {}
    cleaned = run_mesh(sc, steps, warmup) if mesh else {}
    registered = run_register(sc, res, steps, warmup) if register else {}
    estimated = run_cloud_normals(sc, res, steps, warmup) if cloud_normals_too else {}
    searched = run_knn(res, steps, warmup) if knn else {}
    split = run_clusters(res, float(sc["K"][0, 0, 0]), steps, warmup) if clusters else {}
    drawn = run_render(sc, res, steps, warmup) if render else {}
    mesh_scored = run_mesh_metrics(sc, res, steps, warmup) if mesh_metrics_too else {}
    rasterised = run_mesh_render(sc, steps, warmup) if mesh_render_too else {}
    simplified = run_simplify(sc, steps, warmup) if simplify_too else {}
    smoothed = run_smooth(sc, steps, warmup) if smooth_too else {}
    meshed = run_cloud_volume(sc, res, steps, warmup) if cloud_volume_too else {}
    return {**meshed, **smoothed, **simplified, **rasterised, **mesh_scored, **drawn, **split, **gated, **merged, **oriented, **scored, **volume, **rendered, **aligned, **cleaned, **registered, **estimated, **searched, "scene": f"V{V}_{W}x{H}_M{M}", "ms_per_call_median": float(np.median(times)),
            "ms_per_call_min": float(np.min(times)), "steps": steps, "points": N,
            "kept_fraction": N / (V * P),
            "bytes": {"consistency_ref_depth_read": 4 * V * P, "consistency_maps_written": 5 * V * P,
                      "consistency_gather_logical": 16 * V * P * M,
                      "emit_fused_read": 4 * V * P, "emit_points_written": N * (12 + 3 + 4 + 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--confidence", action="store_true", help="also time the call gated by a confidence map")
    ap.add_argument("--voxel", action="store_true", help="also time voxel_merge of the fused cloud, and its torch form")
    ap.add_argument("--normals", action="store_true", help="also time depth_normals, and its torch form")
    ap.add_argument("--cloud-metrics", action="store_true",
                    help="also score a perturbed fusion against the true one (cloud_metrics) and time cloud_nearest")
    ap.add_argument("--tsdf", action="store_true",
                    help="also integrate the views into a 256^3 TSDF volume, extract its mesh and score it")
    ap.add_argument("--raycast", action="store_true",
                    help="also render the TSDF volume back into the input views (raycast), and the torch form of the march")
    ap.add_argument("--align", action="store_true",
                    help="also align the views from perturbed poses to the TSDF volume, and the torch form of one iteration")
    ap.add_argument("--mesh", action="store_true",
                    help="also label the components of the volume's mesh and drop the small ones, and the torch form")
    ap.add_argument("--register", action="store_true",
                    help="also register the fused cloud, moved by a small twist, back onto itself, and the torch form")
    ap.add_argument("--cloud-normals", action="store_true",
                    help="also estimate the fused cloud's normals from its bare points (cloud_normals), and the torch form")
    ap.add_argument("--global", dest="global_too", action="store_true",
                    help="also register two samplings of an asymmetric surface from unrelated frames (cloud_fpfh, "
                         "feature_nearest, cloud_ransac, cloud_register_global), and the torch form of the match; its own line")
    ap.add_argument("--knn", action="store_true",
                    help="also search the fused cloud for every point's k nearest others (cloud_knn) and filter it "
                         "(statistical_outlier_mask), and the torch form of the search")
    ap.add_argument("--clusters", action="store_true",
                    help="also split the merged fused cloud into its density-connected pieces (cloud_clusters), and the "
                         "torch form of the labelling")
    ap.add_argument("--render", action="store_true",
                    help="also render the fused cloud back into the input views (cloud_render at radius 0 and 1), test its "
                         "points for occlusion (cloud_visibility, with and without maps), and the torch form of the render")
    ap.add_argument("--mesh-metrics", action="store_true",
                    help="also score the volume's mesh against the fused cloud (mesh_metrics) and time mesh_sample and "
                         "mesh_nearest, cloud_nearest against the vertices, and the torch brute force of the distance")
    ap.add_argument("--mesh-render", action="store_true",
                    help="also render the volume's mesh into the input views (mesh_render, with and without gathers), next "
                         "to cloud_render of its vertices, and compare the depth with the volume's raycast")
    ap.add_argument("--simplify", action="store_true",
                    help="also simplify the volume's mesh (mesh_simplify at 1, 2 and 4 voxels per cell, both placements), "
                         "measure how far the result is from the original surface, and the torch form of the clustering")
    ap.add_argument("--smooth", action="store_true",
                    help="also find the edges of the volume's mesh (mesh_edges), smooth it (mesh_smooth, Taubin) and recompute "
                         "its normals (mesh_normals), and the torch form of the edges and of the smoothing")
    ap.add_argument("--cloud-volume", action="store_true",
                    help="also mesh the merged fused cloud through integrate_cloud and extract_mesh, score it next to the "
                         "mesh of the depth-map volume, and the torch form of the sums at a sample of the voxels")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    for V, H, W, M in SCENES:
        print(json.dumps(run(V, H, W, M, a.steps, a.warmup, a.confidence, a.voxel, a.normals, a.cloud_metrics,
                             a.tsdf, a.raycast, a.align, a.mesh, a.register, a.cloud_normals, a.knn, a.clusters,
                             a.render, a.mesh_metrics, a.mesh_render, a.simplify, a.smooth, a.cloud_volume)), flush=True)
    if a.global_too:
        print(json.dumps(run_global(a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
