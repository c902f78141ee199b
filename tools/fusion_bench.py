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
way."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_view_stereonet_amd import synthetic  # noqa: E402
from multi_view_stereonet_amd.fusion import fuse_depthmaps, voxel_merge  # noqa: E402

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


def run(V, H, W, M, steps, warmup, confidence=False, voxel=False):
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
    return {**gated, **merged, "scene": f"V{V}_{W}x{H}_M{M}", "ms_per_call_median": float(np.median(times)),
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
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    for V, H, W, M in SCENES:
        print(json.dumps(run(V, H, W, M, a.steps, a.warmup, a.confidence, a.voxel)), flush=True)


if __name__ == "__main__":
    main()
