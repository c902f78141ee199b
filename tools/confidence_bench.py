"""Time the confidence-producing soft-argmin launch against mvsn_soft_argmin on the same volume, and a batch-1 forward
with EngineOptions.confidence on against off.

Launch time: device events around 20 calls after 3 warm-up calls, on 512 chains x 64 x 16x32 (the headline step) and
2 chains x 64 x 16x32 (batch 1); the two launches alternate, three rounds, medians printed.  The volume's bytes over the
time is the achieved read rate (the kernel reads the volume twice; the second pass and the window reads are cache hits
where the volume of a workgroup's pixels stays resident).  Forward time: 512x256, D = 64, 2 source views, batch 1,
recorded plan replayed as a hipGraph, 50 forwards per window after 10, three alternating rounds.  One JSON line each."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_view_stereonet_amd import MultiViewStereoNet, synthetic  # noqa: E402
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu  # noqa: E402
from multi_view_stereonet_amd.weights import load_weights  # noqa: E402

DEV = torch.device("cuda:0")


def per_call_ms(fn, calls=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def launch_times(eng, n, D=64, rows=16, cols=32, rounds=3):
    g = torch.Generator().manual_seed(n)
    cost = torch.randn(n, D, rows, cols, generator=g).to(DEV)
    samples = torch.sort(torch.rand(n, D, generator=g), dim=1).values.to(DEV).contiguous()
    plain, conf = [], []
    for _ in range(rounds):
        plain.append(per_call_ms(lambda: eng.soft_argmin(cost, samples)))
        conf.append(per_call_ms(lambda: eng.soft_argmin_confidence(cost, samples)))
    a, b = eng.soft_argmin(cost, samples), eng.soft_argmin_confidence(cost, samples)
    nbytes = 4.0 * cost.numel()
    return {"what": "launch", "chains": n, "D": D, "grid": [rows, cols], "volume_MB": nbytes / 1e6,
            "soft_argmin_us": [round(1e3 * t, 2) for t in plain], "soft_argmin_confidence_us": [round(1e3 * t, 2) for t in conf],
            "median_us": [round(1e3 * float(np.median(plain)), 2), round(1e3 * float(np.median(conf)), 2)],
            "volume_TBps": [round(nbytes / (1e9 * float(np.median(plain))), 3), round(nbytes / (1e9 * float(np.median(conf))), 3)],
            "idepth_bit_identical": bool(torch.equal(a, b[0]))}


def forward_times(net, rounds=3):
    batch = synthetic.make_batch(256, 512, 2, batch=1, seed=1)
    x = snu.multi_view_unpack_batch(batch, DEV, 5)
    args = (x["left_image_pyr"], x["K_pyr"], x["T_right_in_left"], x["right_image_pyr"], 64, True, [True] * 5)
    res = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            net.options.confidence = on
            res[on].append(per_call_ms(lambda: net(*args), calls=50, warmup=10))
    net.options.confidence = False
    launches = {}
    for on in (False, True):       # the call list of an eager forward
        net.options.confidence, net.options.plan_max_chains = on, 0
        eng = net.engine()
        eng.timeline = []
        net(*args)
        launches[on] = len(eng.timeline)
        eng.timeline = None
    net.options.confidence, net.options.plan_max_chains = False, 16
    return {"what": "batch-1 forward 512x256 D=64 S=2 (hipGraph replay)", "off_ms": [round(t, 4) for t in res[False]],
            "on_ms": [round(t, 4) for t in res[True]],
            "median_ms": [round(float(np.median(res[False])), 4), round(float(np.median(res[True])), 4)],
            "launches": [launches[False], launches[True]]}


def main():
    torch.set_grad_enabled(False)
    net = MultiViewStereoNet()
    net.load_state_dict(load_weights("gta_sfm_150epochs"), strict=True)
    net = net.to(DEV).eval()
    eng = net.engine()
    for n in (512, 2):
        print(json.dumps(launch_times(eng, n)), flush=True)
    print(json.dumps(forward_times(net)), flush=True)


if __name__ == "__main__":
    main()
