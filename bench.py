#!/usr/bin/env python3
"""depthmaps/sec of the MI355X plane-sweep forward at 512x256, 64 hypotheses, 2 source views.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one MultiViewStereoNet.forward() over a batch of B synthetic reference images (each
with 2 source views) already resident in HBM; every rank runs its own B images (weak scaling,
images are independent -- SURVEY 8e).
Rank 0 prints ONE JSON line, LAST and < 4 KB (`final_line`); the full record goes to `bench_detail.json` and a
`DETAIL <json>` stdout line before it.  A plain run sets up, runs W untimed and K timed steps, writes the last step's
outputs if `--dump-outputs DIR` is given (`dump_outputs`) and prints the line: `value` (depthmaps/s), `ms_per_step`
and the run's description.  `--full` adds everything else -- the all-gather of one metric row per image, the per-kernel
rooflines, the other configurations, tier legs and latencies, and
  roofline      the dominant kernel's algorithmic flops / measured launch time (device events on the
                stream the kernels run on) against the fp32 MFMA peak, plus the fused chain kernel
                against both peaks,
  cpu_baseline  the CPU oracle (the build's restatement of the reference forward) timed on the host,
  l1_vs_ref     L1 / relative error of image 0 against the reference-generated golden depth map.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from multi_view_stereonet_amd import MultiViewStereoNet, synthetic  # noqa: E402
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu  # noqa: E402
from multi_view_stereonet_amd import distributed as mdist  # noqa: E402
from multi_view_stereonet_amd.weights import load_weights  # noqa: E402

ROWS, COLS, D, S = 256, 512, 64, 2
WEIGHTS = "gta_sfm_150epochs"
GOLDEN = os.path.join(ROOT, "tests", "golden", "g2_gta_512x256_d64_s2.npz")
GOLDEN_SEED = 7
# BASELINE.json's configs (config 1 is the CPU plumbing case).  `--config` selects the workload of the timed region;
# the default line (headline = the configuration the metric is quoted on) also carries the others as `other_configs`.
# `batch` = reference images per GPU per step; config 3 is stated as batch 8 over 8 GPUs = ONE image per rank.
# Headline: 256 images = 512 chains = two rounds of one chain per CU, 35 GB of the 288 (measured 128 / 256 / 384 / 512
# images: 3400-3428 / 3459-3493 / 3528 / 3491-3530 depthmaps/s; the persistent kernels' prologues and tails amortise).
# Every config has a reference-generated fixture whose input is image 0 of rank 0 (seed = the fixture's).
CONFIGS = {
    "headline": dict(rows=256, cols=512, D=64, S=2, weights="gta_sfm_150epochs", golden="g2_gta_512x256_d64_s2.npz",
                     batch=256, what="GTA-SfM-shaped 512x256, D=64 hypotheses, 2 source views, cost-volume filter + 5 refiners"),
    "config2": dict(rows=256, cols=512, D=64, S=1, weights="gta_sfm_150epochs", golden="gc2_gta_512x256_d64_s1.npz",
                    batch=128, what="BASELINE config 2: GTA-SfM 2-view, 512x256, D=64, 1 source view"),
    "config3": dict(rows=256, cols=512, D=64, S=5, weights="gta_sfm_150epochs", golden="gc3_gta_512x256_d64_s5.npz",
                    batch=1, what="BASELINE config 3: GTA-SfM 5-cmp, 512x256, D=64, 5 source views, ONE image per GPU "
                                  "(batch 8 over 8 GPUs)"),
    "config4": dict(rows=480, cols=640, D=96, S=1, weights="demon_45epochs", golden="g3_demon_640x480_d96_s1.npz",
                    batch=32, more_batches=(128,),
                    what="BASELINE config 4: DeMoN 640x480, D=96, 1 source view, demon_45epochs weights"),
    "config5": dict(rows=512, cols=1024, D=128, S=4, weights="gta_sfm_150epochs", golden="gc5_gta_1024x512_d128_s4.npz",
                    batch=8, more_batches=(32,),
                    what="BASELINE config 5 geometry: 1024x512, D=128, 4 source views (fp32 throughout; the bf16 "
                                  "tiers are reported by the headline line)"),
}


_FRAMES = {}     # (rows, cols, S, seed, smooth, jitter) -> one synthetic (image, S sources) set on the host


def one_set(rows, cols, S, seed, smooth=False, jitter=0.0):
    """One seeded synthetic set, generated once per process: the side legs of the default line (other batch sizes, the
    host-fed and evaluate rates, the oracle checks) reuse the timed region's images instead of re-drawing ~2000 frames."""
    key = (rows, cols, S, seed, bool(smooth), float(jitter))
    if key not in _FRAMES:
        _FRAMES[key] = synthetic.make_batch(rows, cols, S, batch=1, seed=seed, smooth=smooth, pose_jitter=jitter)
    return _FRAMES[key]


def config_inputs(cfg, batch, rank, device):
    """B independent (image, S sources) sets of a config; image 0 of rank 0 is the golden fixture's input."""
    import numpy as np
    fix = np.load(os.path.join(ROOT, "tests", "golden", cfg["golden"]))
    seed0, smooth = int(fix["meta"][5]), bool(fix["smooth"]) if "smooth" in fix.files else False
    jitter = float(fix["jitter"]) if "jitter" in fix.files else 0.0
    parts = [one_set(cfg["rows"], cfg["cols"], cfg["S"], seed0 + rank * batch + i, smooth, jitter) for i in range(batch)]
    merged = {"left_image": torch.cat([p["left_image"] for p in parts], 0),
              "right_image": [torch.cat([p["right_image"][s] for p in parts], 0) for s in range(cfg["S"])],
              "K": torch.cat([p["K"] for p in parts], 0),
              "T_right_in_left": [torch.cat([p["T_right_in_left"][s] for p in parts], 0) for s in range(cfg["S"])]}
    return merged, snu.multi_view_unpack_batch(merged, device, 5), torch.from_numpy(fix["idepth_0"])


def per_pixel_rel(ref0, got0):
    """The contract's reading of "within 1e-3 relative on the final depthmap": |a - ref| / max(|ref|, 1e-3 * mean|ref|)
    per pixel over ref > 0 (the refiner's final relu clamps the rest to exactly 0); (max, p99.9)."""
    ref, got = ref0.double().reshape(-1), got0.double().reshape(-1)
    sel = ref > 0
    if not bool(sel.any()):
        return 0.0, 0.0
    e = ((got - ref).abs() / ref.abs().clamp_min(1e-3 * float(ref.abs().mean())))[sel].sort().values
    return float(e[-1]), float(e[int(0.999 * (e.numel() - 1))])


def l1_against(ref0, got0, golden=None):
    l1 = float((got0 - ref0).abs().mean())
    mx, p999 = per_pixel_rel(ref0, got0)
    res = {"l1": l1, "mean_rel": l1 / float(ref0.abs().mean()),
           "max_rel": float((got0 - ref0).abs().max() / ref0.abs().max()),
           "max_rel_per_pixel": mx, "p999_rel_per_pixel": p999,
           "rel_definitions": "mean_rel = mean|a-b| / mean|ref|; max_rel = max|a-b| / max|ref|; *_per_pixel = "
                              "|a-b| / max(|ref|, 1e-3 mean|ref|) over ref > 0 (contract: < 1e-3)"}
    if golden:
        res["reference"] = f"tests/golden/{golden} (reference PyTorch-CPU forward)"
    return res
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2 dense peak
PEAK_HBM_GBS = 8000.0
PMC_TRAFFIC_FILE = "r*_pmc_traffic.json"   # FETCH_SIZE / WRITE_SIZE passes of the bench command (tools/prof_round.sh)
FEATURE_TIER_PMC_FILE = "r*_bf16_feature_tier_pmc.json"   # FETCH / WRITE of the chain and the regulariser's layers per tier (tools/prof_feature_tier.sh)
LEVEL_PMC_FILE = "r*_level_pmc.json"       # ... of the refiner towers level by level (tools/level_profile.py)


FINAL_LINE_LIMIT = 4096      # the driver keeps a bounded tail of stdout: the line it parses must fit well inside it
DETAIL_FILE = os.path.join(ROOT, "bench_detail.json")
_ROOFLINE_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "frac_per_rank", "traffic", "launches_per_step",
                  "avg_launch_ms", "share_of_step", "direct_form_equivalent_TFLOPs")
_CPU_KEYS = ("value", "unit", "cores", "kind", "sample", "cpu_model", "logical_cpus", "physical_cores")
_TOP_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "world_size", "backend",
             "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _numbers(d, digits=6):
    """The numeric leaves of a flat dict (floats to `digits` significant figures); prose stays in the DETAIL record."""
    out = {}
    for k, v in (d or {}).items():
        if isinstance(v, bool) or v is None or isinstance(v, int):
            out[k] = v
        elif isinstance(v, float):
            out[k] = float(f"{v:.{digits}g}")
        elif isinstance(v, (list, tuple)) and all(isinstance(x, (int, float)) for x in v):
            out[k] = [float(f"{x:.{digits}g}") if isinstance(x, float) else x for x in v]
    return out


def final_line(full):
    """The ONE line the driver parses, from the full record: the contract's keys, `roofline` and `cpu_baseline` without
    prose, the parity figures as numbers.  Everything else (per-kernel rooflines, the other configurations, the tier
    legs, batch latency, PCIe-inclusive and evaluate rates) is the DETAIL record (`emit`).  VERDICT r5 item 1: the
    22 KB line of round 5 outgrew the driver's capture and the headline went unparsed."""
    line = {k: full[k] for k in _TOP_KEYS if k in full}
    for k in ("value", "ms_per_step"):
        if isinstance(line.get(k), float):
            line[k] = float(f"{line[k]:.7g}")
    if isinstance(full.get("config"), dict):
        line["config"] = {k: v for k, v in full["config"].items() if not isinstance(v, str) or len(v) <= 160}
    if isinstance(full.get("l1_vs_ref"), dict):
        line["l1_vs_ref"] = _numbers(full["l1_vs_ref"]) or full["l1_vs_ref"]
    if isinstance(full.get("roofline"), dict):
        r = full["roofline"]
        line["roofline"] = {k: (float(f"{r[k]:.6g}") if isinstance(r[k], float) else
                                [float(f"{x:.6g}") for x in r[k]] if isinstance(r[k], list) else r[k])
                            for k in _ROOFLINE_KEYS if k in r}
        if r.get("stand_in"):
            line["roofline"]["stand_in"] = True
    if isinstance(full.get("chain_kernel"), dict):
        line["chain_kernel"] = _numbers(full["chain_kernel"]) or full["chain_kernel"]
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        line["cpu_baseline"] = {k: cb[k] for k in _CPU_KEYS if k in cb} or cb
        if isinstance(line["cpu_baseline"].get("value"), float):
            line["cpu_baseline"]["value"] = float(f"{cb['value']:.5g}")
        for k in ("one_thread", "all_physical_cores"):
            if isinstance(cb.get(k), dict):
                line["cpu_baseline"][k] = _numbers(cb[k])
    for k, v in full.items():
        if k.startswith("l1_vs_oracle"):
            line[k] = _numbers(v) if isinstance(v, dict) else (float(f"{v:.6g}") if isinstance(v, float) else v)
    for k in ("per_rank_ms_per_step", "mean_idepth", "rows_gathered", "rank_sum", "selftest", "engine_options_override"):
        if k in full:
            line[k] = full[k]
    line["detail"] = "bench_detail.json + the `DETAIL ` stdout line before this one"
    text = json.dumps(line)
    if len(text) >= FINAL_LINE_LIMIT:       # never again an unparsable line: shed optional groups, keep the contract
        for k in ("chain_kernel", "l1_vs_oracle_last", "l1_vs_oracle_slice_b", "per_rank_ms_per_step"):
            line.pop(k, None)
            text = json.dumps(line)
            if len(text) < FINAL_LINE_LIMIT:
                break
    assert len(text) < FINAL_LINE_LIMIT, len(text)
    return text


def emit(full, stream=None):
    """Full record -> `bench_detail.json` next to this script and a `DETAIL <json>` stdout line; then, LAST, the compact
    JSON line (`final_line`) -- the only stdout line that starts with `{`."""
    if stream is None:
        # RCCL writes its NCCL_DEBUG=VERSION banner with C stdio: on a pipe it sits in libc's buffer until exit and
        # would land AFTER the JSON line (seen on the GPU box, whose environment sets NCCL_DEBUG=VERSION) -- push
        # whatever C code has buffered out first, so the compact line stays the last thing on stdout
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
    stream = stream or sys.stdout
    blob = json.dumps(full)
    try:
        with open(DETAIL_FILE, "w") as f:
            f.write(blob + "\n")
    except OSError:
        pass
    stream.write("DETAIL " + blob + "\n")
    stream.write(final_line(full) + "\n")
    stream.flush()


DUMP_LIMIT = 60 * 2 ** 20      # bytes of array data in all the files `--dump-outputs` writes (< 64 MB with headers)
DUMP_SEED = 20261016           # the element sample of an output too large to keep whole


def dump_outputs(out, path):
    """`--dump-outputs DIR`: the arrays the forward of the last timed step returned to its caller, as
    DIR/<key>_<level>.npy (float32; the bool masks as 0 / 1).  Each output gets an equal share of DUMP_LIMIT: one that
    fits is written whole in its own shape, a larger one as a fixed sample of its flattened elements (seeded indices,
    in increasing order: the same elements on every run with the same arguments).  Returns {name: shape written}."""
    import numpy as np
    arrays = []
    for key in sorted(out):
        val = out[key]
        for lvl, t in enumerate(val if isinstance(val, (list, tuple)) else [val]):
            if isinstance(t, torch.Tensor):
                arrays.append((f"{key}_{lvl}" if isinstance(val, (list, tuple)) else key, t))
    os.makedirs(path, exist_ok=True)
    written, total = {}, 0
    for name, t in arrays:
        dtype = torch.float64 if t.dtype == torch.float64 else torch.float32
        cap = DUMP_LIMIT // len(arrays) // (8 if dtype == torch.float64 else 4)
        if t.numel() > cap:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(t.numel(), cap, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        a = t.to(dtype).cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a)
        written[name] = list(a.shape)
        total += a.nbytes
    assert total <= DUMP_LIMIT, total
    return written


def make_inputs(batch, first_seed, device):
    """B independent (image, 2 sources) sets; set i uses seed first_seed+i, so image 0 of rank 0 is
    the golden fixture's input."""
    parts = [one_set(ROWS, COLS, S, first_seed + i) for i in range(batch)]
    merged = {"left_image": torch.cat([p["left_image"] for p in parts], 0),
              "right_image": [torch.cat([p["right_image"][s] for p in parts], 0) for s in range(S)],
              "K": torch.cat([p["K"] for p in parts], 0),
              "T_right_in_left": [torch.cat([p["T_right_in_left"][s] for p in parts], 0) for s in range(S)]}
    return merged, snu.multi_view_unpack_batch(merged, device, 5)


def run_forward(net, inp, d=D):
    return net(inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"], inp["right_image_pyr"], d, True,
               [True] * 5)


def headline_by_batch(net, dev, batches=(128, 384, 512)):
    """The headline forward at other batch sizes (images per step), same protocol as other_configs: the timed region's
    256 images are two rounds of one chain per CU; rounds 1-2 quoted 128 images, and the persistent kernels' prologues
    and tails keep amortising beyond 256 (memory: 17 / 52 / 70 GB)."""
    cfg, res = CONFIGS["headline"], {}
    for b in batches:
        _, inp, _ = config_inputs(cfg, b, 0, dev)
        for _ in range(2):
            run_forward(net, inp, cfg["D"])
        torch.cuda.synchronize()
        blocks = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(2):
                run_forward(net, inp, cfg["D"])
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / 2 * 1e3)
        ms = sorted(blocks)[1]
        res[f"B={b}"] = {"ms_per_step": round(ms, 2), "depthmaps_per_s": round(b / ms * 1e3, 1)}
        del inp
        torch.cuda.empty_cache()
    return res


def other_configs(dev, skip):
    """BASELINE configs 2-5 at their stated sizes on this GPU: ms per forward at batch 1 and at the config's batch,
    and the depth error of image 0 against the reference-generated fixture (same contract as the headline)."""
    res = {}
    for name, cfg in CONFIGS.items():
        if name in skip:
            continue
        net = MultiViewStereoNet()
        net.load_state_dict(load_weights(cfg["weights"]), strict=True)
        net = net.to(dev).eval()
        entry = {"workload": cfg["what"]}
        for b in sorted({1, cfg["batch"]} | set(cfg.get("more_batches", ()))):
            _, inp, ref0 = config_inputs(cfg, b, 0, dev)
            for _ in range(5):      # (record, list replay, graph instantiation of a planned forward; allocator pools)
                out = run_forward(net, inp, cfg["D"])
            torch.cuda.synchronize()
            # median of five blocks: a one-off host hiccup (a 60 ms pause inside 20 batch-1 forwards once read as
            # 5.8 instead of 2.7 ms per forward) must not become the configuration's figure
            reps, blocks = (8, []) if b == 1 else (2, [])
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(reps):
                    out = run_forward(net, inp, cfg["D"])
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / reps * 1e3)
            ms = sorted(blocks)[2]
            eng = net.engine()
            form = {1: "direct", 2: "winograd", 3: "stepwise", 4: "banded"}.get(eng.last_chain_form, "?")
            if form == "banded":        # which plan: thin bands (15 / 16 / 8 / 4 workgroups per chain) or slabs (3 / 4)
                n_ch, r4, c4 = eng.last_chain_shape
                form += f" ({eng.lib.mvsn_incremental_cost_volume_banded_groups(n_ch, r4, c4)} workgroups per chain)"
            entry[f"B={b}"] = {"ms_per_forward": round(ms, 3), "depthmaps_per_s": round(b / ms * 1e3, 1),
                               "chain_form": form}
            if b == 1:
                entry["l1_vs_ref"] = l1_against(ref0, out["left_idepthmap_pyr"][0][:1].cpu(), cfg["golden"])
            del inp, out
        res[name] = entry
        del net
        torch.cuda.empty_cache()
    return res


def kernel_breakdown(net, inp, d=D):
    """One instrumented forward: per-kernel launch counts, device time, algorithmic flops/bytes."""
    eng = net.engine()
    eng.timeline = []
    run_forward(net, inp, d)
    torch.cuda.synchronize()
    tl, eng.timeline = eng.timeline, None
    agg = {}
    for name, a, b, flops, nbytes in tl:
        e = agg.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] += a.elapsed_time(b)
        e["flops"] += flops
        e["bytes"] += nbytes
    return agg


def host_cpu_info():
    """(model name, logical cpus, physical cores) from /proc/cpuinfo (physical = distinct (physical id, core id) pairs)."""
    model, cores, phys, cur = "unknown", os.cpu_count() or 1, set(), {}
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ":" not in ln:
                    if cur:
                        phys.add((cur.get("physical id", "0"), cur.get("core id", str(len(phys)))))
                    cur = {}
                    continue
                k, v = (x.strip() for x in ln.split(":", 1))
                cur[k] = v
                if k == "model name":
                    model = v
        if cur:
            phys.add((cur.get("physical id", "0"), cur.get("core id", str(len(phys)))))
    except OSError:
        pass
    return model, cores, (len(phys) or cores)


def roofline_by_kernel(agg, total_ms, top=14, wino_names=()):
    """Every arithmetic kernel of the step (refiner launches by LEVEL and dilation, ` L<level>` in the name) against both
    roofs: launch time from this run's device events; executed flops (Winograd forms: 4/9 of the direct count) against
    the fp32 MFMA peak; ALGORITHMIC bytes (each tensor of the launch -- and of the pass it carries -- once) against the
    HBM peak; `binds` = the roof the launch sits closer to.  Counter-measured bytes of the same launches, where a PMC
    pass of THIS library is committed: profiles/<round>_level_pmc.json (tools/level_profile.py), keyed alike."""
    pmc = load_profile_json(LEVEL_PMC_FILE) or {}
    rows = {}
    for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        if v["flops"] <= 0 or len(rows) >= top:
            continue
        sec = v["ms"] * 1e-3
        # executed / direct-form flops: F(2x2,3x3) 16 / 36; the 5x5 stride-2 layers on their four phases 392 / 800
        ex = v["flops"] * ((0.49 if "k5s2" in k else 4.0 / 9.0) if (" wino" in k or k in wino_names) else 1.0) / sec / 1e12
        gbs = v["bytes"] / sec / 1e9
        row = {"launches": v["launches"], "ms_per_step": round(v["ms"], 3), "ms_per_launch": round(v["ms"] / v["launches"], 4),
               "share_of_step": round(v["ms"] / total_ms, 4), "executed_TFLOPs": round(ex, 1),
               "frac_of_fp32_mfma_peak": round(ex / PEAK_FP32_MFMA_TFLOPS, 3), "algorithmic_GBps": round(gbs, 0),
               "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 3)}
        row["binds"] = "mfma" if row["frac_of_fp32_mfma_peak"] >= row["frac_of_hbm_peak"] else "hbm"
        t = pmc.get(k)
        if t:
            row["pmc"] = t
        rows[k] = row
    return rows


def load_profile_json(name):
    """A committed counter file under profiles/ -- only if it was taken with THIS library (its `_library_digest` equals
    multi_view_stereonet_amd/libmvsn_hip.so.sources); a stale file is refused, never scaled.  `name` may hold a `*`
    (round prefix): the newest round's file whose digest matches is the one used."""
    import glob
    try:
        with open(os.path.join(ROOT, "multi_view_stereonet_amd", "libmvsn_hip.so.sources")) as f:
            digest = f.read().strip()
    except OSError:
        return None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", name)), reverse=True):
        try:
            with open(path) as f:
                data = json.load(f)
        except (OSError, ValueError):
            continue
        if data.get("_library_digest") == digest:
            data["_file"] = os.path.basename(path)
            return data
    return None


def cpu_baseline(cfg, budget_s=15.0):
    """The oracle (CPU restatement of the reference forward) on the host cores, B=1, same workload (one
    thread, all physical cores, and the best thread count of a short sweep -- the latter is `value`)."""
    from oracle import mvsn_oracle as oracle
    w = load_weights(cfg["weights"])
    _, inp, _ = config_inputs(cfg, 1, 0, torch.device("cpu"))
    model, cores, physical = host_cpu_info()

    def once():
        t0 = time.time()
        out = oracle.forward(w, inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"], inp["right_image_pyr"],
                             cfg["D"])
        return time.time() - t0, out

    def at(threads, reps):
        torch.set_num_threads(threads)
        once()
        ts = [once()[0] for _ in range(reps)]
        return {"threads": threads, "forwards": reps, "mean_ms": round(sum(ts) / reps * 1e3, 1),
                "depthmaps_per_s": round(reps / sum(ts), 3)}

    one = at(1, 2)
    # torch's intra-op scaling on this small per-image problem peaks well below the core count; take the
    # best of a short sweep and report the thread count actually used
    best, threads = None, 1
    for cand in [c for c in (8, 16, 32, 64) if c <= cores] or [cores]:
        torch.set_num_threads(cand)
        once()
        dt = min(once()[0] for _ in range(2))
        if best is None or dt < best:
            best, threads = dt, cand
    allp = at(physical, 2) if physical not in (1, threads) else None
    torch.set_num_threads(threads)
    once()  # warm-up
    times, t_start = [], time.time()
    while len(times) < 3 or (time.time() - t_start < budget_s and len(times) < 50):
        dt, out = once()
        times.append(dt)
    mean = sum(times) / len(times)
    res = {"value": 1.0 / mean, "unit": "depthmaps/s", "cores": threads, "kind": "port",
           "sample": f"{len(times)} forwards of 1 image ({cfg['cols']}x{cfg['rows']}, D={cfg['D']}, S={cfg['S']}, fp32, "
                     f"torch CPU, {threads} threads of {cores} host cpus), mean {mean * 1e3:.1f} ms",
           "cpu_model": model, "logical_cpus": cores, "physical_cores": physical, "one_thread": one,
           "all_physical_cores": allp if allp is not None else {"threads": physical, "note": "same as `cores`"}}
    return res, out


def oracle_check(cfg, index, got):
    """Image `index` of rank 0's step (seed = the fixture's + index) through the CPU oracle, against the GPU's depth map of
    that image: same fields as l1_vs_ref (the contract: max_rel_per_pixel < 1e-3)."""
    from oracle import mvsn_oracle as oracle
    w = load_weights(cfg["weights"])
    _, inp, _ = config_inputs(cfg, 1, index, torch.device("cpu"))      # (rank * batch + i = index)
    ref = oracle.forward(w, inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"], inp["right_image_pyr"],
                         cfg["D"])["left_idepthmap_pyr"][0]
    res = {k: v for k, v in l1_against(ref, got).items() if k != "rel_definitions"}
    res["image"] = index
    res["reference"] = "oracle/mvsn_oracle.py on the same seeded input (CPU)"
    return res


def self_launch(n):
    """Re-execute this command line under torch.distributed.run with n local ranks (one per GPU)."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def mask_mean(mask):
    """Per-image fraction of set voxels of a (B, D, H, W) bool volume: an integer sum, no fp32 copy.  The metric rows take
    it over the level-4 mask (a few MB): over the level-0 volume (8.6 GB at config 5 / B = 32) ATen's reduction was 10 % of
    the traced kernel time as `.float().mean()` and 20 % as an int64 sum -- bench bookkeeping, outside the
    timed region, but it polluted the kernel percentages of the traces kept as evidence."""
    return (mask.sum(dim=(1, 2, 3), dtype=torch.int64).to(torch.float64) / (mask[0].numel() or 1)).float()


def timed_steps(step, steps, warmup, world, sync, reduce_device):
    """The timing protocol: `warmup` untimed steps, then exactly `steps` steps between barrier + device sync on
    both sides; returns (max over ranks, per-rank list) of the elapsed seconds."""
    grouped = torch.distributed.is_initialized()        # (a forced single-rank group takes the collective path too)

    def barrier():
        if grouped:
            torch.distributed.barrier()

    out = None
    for _ in range(warmup):
        out = step()
    sync()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank = [elapsed]
    if grouped:
        mine = torch.tensor([elapsed], dtype=torch.float64, device=reduce_device)
        every = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(every, mine)
        per_rank = [float(e.item()) for e in every]
    return max(per_rank), per_rank, out


def gather_floats(x, world, device):
    """One float per rank -> list over ranks (identity without a process group)."""
    if not torch.distributed.is_initialized():
        return [float(x)]
    mine = torch.tensor([float(x)], dtype=torch.float64, device=device)
    every = [torch.zeros_like(mine) for _ in range(world)]
    torch.distributed.all_gather(every, mine)
    return [float(e.item()) for e in every]


def launcher_selftest(args, rank, world):
    """`--launcher-selftest`: the launch / barrier / max-over-ranks / all-gather plumbing of this file on CPU
    ranks over gloo, with a stand-in step (NO forward, NO GPU).  Its line is labelled as such and is not a
    measurement; tests/test_bench_launcher_cpu.py runs it with --gpus 2."""
    B = args.batch or 4

    def step():
        return torch.full((B, 3), float(rank))

    elapsed, per_rank, rows = timed_steps(step, args.steps, args.warmup, world, lambda: None, torch.device("cpu"))
    idx = torch.arange(rank * B, (rank + 1) * B)
    all_rows, all_idx = mdist.gather_metric_rows(rows, idx)
    assert all_rows.shape[0] == B * world and all_idx.tolist() == list(range(B * world))
    # the per-rank quality fields travel the same way as in a real run (stand-in numbers: rank r reports frac 0.5 + r/10)
    fracs = gather_floats(0.5 + rank / 10.0, world, torch.device("cpu"))
    if rank == 0:
        skipped = {"skipped": "launcher self-test: no forward ran"}
        emit({"l1_vs_ref": skipped, "cpu_baseline": skipped, "chain_kernel": skipped,
                          "roofline": {"frac": min(fracs), "frac_per_rank": fracs, "stand_in": True},
                          "metric": "launcher self-test (no forward, not a measurement)", "value": 0.0,
                          "unit": "none", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "world_size": torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1,
                          "backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else "none",
                          "per_rank_ms_per_step": [e / args.steps * 1e3 for e in per_rank],
                          "rows_gathered": int(all_rows.shape[0]), "rank_sum": float(all_rows[:, 0].sum()),
                          "data": "none"})
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def batch_latency(net, batches=(1, 2, 4, 8), reps=20):
    """Single-stream latency at the batch sizes an evaluation loop uses (test.py:38 runs batch 1): ms per forward
    and depthmaps/s, inputs resident, with the whole forward replayed from a hipGraph (the default at small B)."""
    from multi_view_stereonet_amd.graphed import GraphedForward
    res = {}
    dev = next(net.parameters()).device
    for b in batches:
        _, inp = make_inputs(b, GOLDEN_SEED, dev)
        pack = (inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"], inp["right_image_pyr"])
        entry = {}
        for mode in ("eager", "graph"):
            fn = (lambda: run_forward(net, inp)) if mode == "eager" else None
            if mode == "graph":
                g = GraphedForward(net, *pack, D)
                fn = lambda: g(*pack)   # noqa: E731
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            blocks = []                 # median of five blocks (see other_configs)
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(max(1, reps // 2)):
                    fn()
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / max(1, reps // 2) * 1e3)
            ms = sorted(blocks)[2]
            entry[mode] = {"ms_per_forward": round(ms, 3), "depthmaps_per_s": round(b / ms * 1e3, 1)}
        res[f"B={b}"] = entry
    return res


def host_feed_rates(net, B, dev, steps=8):
    """PCIe-inclusive rate (never `value`): the batch dict lives in pinned host memory, as a DataLoader hands it
    over, and every step pays H2D copies + the device-side unpack (pyramids, K pyramid, pose normalisation) + the
    forward.  `serial`: multi_view_unpack_batch as is (blocking .to(device)).  `overlapped`: the copies of batch k+1
    run on a side stream while batch k computes (two sets of device buffers)."""
    host, _ = make_inputs(B, GOLDEN_SEED, torch.device("cpu"))
    pin = lambda t: t.pin_memory()   # noqa: E731
    host = {"left_image": pin(host["left_image"]), "right_image": [pin(r) for r in host["right_image"]],
            "K": pin(host["K"]), "T_right_in_left": [pin(t) for t in host["T_right_in_left"]]}
    nbytes = sum(t.numel() * 4 for t in [host["left_image"], host["K"]] + host["right_image"] + host["T_right_in_left"])

    def fwd(batch):
        inp = snu.multi_view_unpack_batch(batch, dev, 5)
        return run_forward(net, inp)

    for _ in range(2):
        fwd(host)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fwd(host)
    torch.cuda.synchronize()
    serial = B * steps / (time.perf_counter() - t0)

    side = torch.cuda.Stream()
    main = torch.cuda.current_stream()

    def stage():
        with torch.cuda.stream(side):
            b = {"left_image": host["left_image"].to(dev, non_blocking=True),
                 "right_image": [r.to(dev, non_blocking=True) for r in host["right_image"]],
                 "K": host["K"].to(dev, non_blocking=True),
                 "T_right_in_left": [t.to(dev, non_blocking=True) for t in host["T_right_in_left"]]}
            ev = torch.cuda.Event()
            ev.record(side)
        return b, ev

    nxt = stage()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        cur, ev = nxt
        nxt = stage()                 # copies of the next batch travel while this one computes
        main.wait_event(ev)
        for t in [cur["left_image"], cur["K"]] + cur["right_image"] + cur["T_right_in_left"]:
            t.record_stream(main)
        fwd(cur)
    torch.cuda.synchronize()
    overlapped = B * steps / (time.perf_counter() - t0)
    return {"bytes_per_depthmap": nbytes / B, "serial_depthmaps_per_s": round(serial, 1),
            "overlapped_depthmaps_per_s": round(overlapped, 1),
            "note": "host batch in pinned memory; includes H2D copies, device-side unpack (image / K pyramids, pose "
                    "normalisation) and the forward; NOT the headline value (inputs resident in HBM)"}


def evaluate_rate(net, B, dev, resident_value, steps=12):
    """The evaluation loop at throughput grade (never `value`): metrics.evaluate over `steps` batches of B images that
    live in pinned host memory with a ground-truth depth map each -- Prefetcher (copies of batch k+1 under batch k),
    device-side unpack, forward, mvsn_depth_metrics (nine doubles per image stay on the device), one synchronisation
    and one gather at the end.  Reported beside the resident-input rate it should approach."""
    from multi_view_stereonet_amd import metrics
    host, _ = make_inputs(B, GOLDEN_SEED, torch.device("cpu"))
    pin = lambda t: t.pin_memory()   # noqa: E731
    g = torch.Generator().manual_seed(5)
    depth = pin(2.0 + 6.0 * torch.rand(B, 1, ROWS, COLS, generator=g))
    batch = {"left_image": pin(host["left_image"]), "right_image": [pin(r) for r in host["right_image"]],
             "K": pin(host["K"]), "T_right_in_left": [pin(t) for t in host["T_right_in_left"]],
             "left_depthmap_true": depth, "right_depthmap_true": [depth] * S}
    params = {"num_idepth_samples": D, "cost_volume_filter": True, "refiners": [True] * 5}
    metrics.evaluate(net, [batch] * 2, params, "gta_sfm", dev)          # warm-up (allocator pools, pinned staging)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    avg = metrics.evaluate(net, [batch] * steps, params, "gta_sfm", dev)
    torch.cuda.synchronize()
    rate = B * steps / (time.perf_counter() - t0)
    return {"depthmaps_per_s": round(rate, 1), "fraction_of_resident_rate": round(rate / resident_value, 4),
            "batches": steps, "images_per_batch": B, "num_samples": avg["num_samples"], "abs_rel": avg.get("abs_rel"),
            "note": "host batches in pinned memory incl. a ground-truth depth map per image; H2D copies overlapped "
                    "(Prefetcher), metrics on the device (mvsn_depth_metrics), one sync + one gather at the end"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("MVSN_BENCH_BATCH", "0")),
                    help="reference images per GPU per step (default: the config's own, 256 for the headline)")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="headline",
                    help="which BASELINE.json configuration the timed region runs (default: the one the metric is "
                         "quoted on); config3 = 5 source views, one image per GPU")
    ap.add_argument("--lanes", type=int, default=int(os.environ.get("MVSN_BENCH_LANES", "1")),
                    help="batch slices run on separate HIP streams (images are independent)")
    ap.add_argument("--fold", action="store_true", help="fold residual blocks into the next conv's tile load")
    ap.add_argument("--precision", choices=["fp32", "bf16x3", "bf16"], default=os.environ.get("MVSN_BENCH_PRECISION", "fp32"),
                    help="arithmetic of the 32->32 3x3 layers: exact fp32 MFMA, or the 3 x bf16 split tier")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed to DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and check everything beyond the headline figure: "
                         "metric rows, parity against the reference fixture and the oracle, per-kernel rooflines, "
                         "the other precisions / batch sizes / configurations and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline and oracle checks")
    ap.add_argument("--no-tiers", action="store_true",
                    help="(--full) skip the bf16x3 / bf16 tier legs and the batch-latency leg")
    ap.add_argument("--sustain", type=float, default=0.0, metavar="SECONDS",
                    help="(--full) after the timed region: keep stepping for this long and report the rate per 2-second "
                         "window (clock settling under sustained MFMA load); writes nothing, adds a 'sustained' key")
    ap.add_argument("--single-device-selftest", action="store_true",
                    help="N > 1 ranks that ALL use cuda:0 and talk over gloo: exercises the multi-rank line (quality fields "
                         "at every world size) on a one-GPU box.  Its rate is NOT a scaling measurement and is labelled so.")
    ap.add_argument("--launcher-selftest", action="store_true",
                    help="CPU ranks over gloo with a stand-in step: checks the launch/timing/gather plumbing only")
    args = ap.parse_args()
    if args.sustain > 0 and not args.full:
        ap.error("--sustain is part of the --full record")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run on
        # the loopback address; rank 0 of the children prints the JSON line on the inherited stdout
        sys.exit(self_launch(args.gpus))
    # MVSN_BENCH_BACKEND=nccl|gloo: create the process group even for ONE rank, so that `--gpus 1` loads RCCL and sends
    # its barriers, timings and metric rows through the collectives an N-GPU run uses (no multi-GPU box needed)
    # stdout belongs to the JSON line: RCCL's debug output (the box sets NCCL_DEBUG=VERSION) goes to stderr
    os.environ.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")
    forced = os.environ.get("MVSN_BENCH_BACKEND") or None
    rank, world, local = mdist.init_from_env(backend="gloo" if (args.launcher_selftest or args.single_device_selftest)
                                             else forced, force=forced is not None)
    if args.single_device_selftest:
        local = 0
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag disagree")
    if args.launcher_selftest:
        return launcher_selftest(args, rank, world)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    cfg = CONFIGS[args.config]
    headline = args.config == "headline"
    net = MultiViewStereoNet()
    net.load_state_dict(load_weights(cfg["weights"]), strict=True)
    net = net.to(dev).eval()
    net.stream_lanes = args.lanes
    net.options.fold_residual_blocks = args.fold
    net.options.conv_precision = args.precision
    for item in filter(None, os.environ.get("MVSN_BENCH_OPTIONS", "").split(",")):   # A/B aid: engine switches, "name=value,..."
        key, val = item.split("=")
        cur = getattr(net.options, key)
        setattr(net.options, key, type(cur)(int(val)) if isinstance(cur, (bool, int)) else type(cur)(val))
    if args.single_device_selftest:
        net.options.chain_form = "winograd"    # (the banded chain form needs the device to itself: one process per GPU)
    B = args.batch if args.batch > 0 else cfg["batch"]
    Dn, Sn = cfg["D"], cfg["S"]
    _, inp, ref0 = config_inputs(cfg, B, rank, dev)
    step = lambda: run_forward(net, inp, Dn)   # noqa: E731

    # set-up, outside the warm-up / timed protocol and reported as "setup_forwards": the first forward packs the
    # weights, opts the kernels into their LDS sizes and grows the allocator pools (one-time work per process)
    step()
    torch.cuda.synchronize()
    coll_dev = torch.device("cpu") if args.single_device_selftest else dev     # (gloo ranks exchange host tensors)
    elapsed, per_rank, out = timed_steps(step, args.steps, args.warmup, world, torch.cuda.synchronize, coll_dev)
    if rank == 0 and args.dump_outputs:
        dump_outputs(out, args.dump_outputs)      # (before any other forward: a replayed plan reuses its buffers)

    if rank == 0:
        line = {"metric": "depthmaps/sec at 512x256, 64 hypotheses, 2 src views; L1 vs ref",
                "value": B * world * args.steps / elapsed, "unit": "depthmaps/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "setup_forwards": 1,
                "ms_per_step": elapsed / args.steps * 1e3,
                "per_rank_ms_per_step": [e / args.steps * 1e3 for e in per_rank],
                "world_size": torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1,
                "backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else "none",
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                "data": f"synthetic (seeded frames, pretrained {cfg['weights']} weights)",
                "config": {"workload": cfg["what"], "name": args.config, "images_per_gpu_per_step": B,
                           "global_batch": B * world, "parallelism": f"dp{world} (independent images, "
                                                                      "all-gather of metric rows)"}}
        if os.environ.get("MVSN_BENCH_OPTIONS"):
            line["engine_options_override"] = os.environ["MVSN_BENCH_OPTIONS"]       # (an A/B run, not the default line)
        if args.single_device_selftest:
            line["selftest"] = ("every rank ran on cuda:0 (gloo): the ranks time-share ONE GPU -- the multi-rank plumbing and "
                                "the per-N quality fields are what this line shows, its rate is not a scaling measurement")
        if not headline:
            line["metric"] = (f"depthmaps/sec at {cfg['cols']}x{cfg['rows']}, {Dn} hypotheses, {Sn} src views; L1 vs ref "
                              f"(--config {args.config}: NOT the headline configuration)")
    if args.full:
        # per-image metric rows, all-gathered (the path's only exchange step)
        idepth = out["left_idepthmap_pyr"][0]
        rows = torch.stack([idepth.mean(dim=(1, 2, 3)), (idepth > 0).float().mean(dim=(1, 2, 3)),
                            mask_mean(out["left_idepthmap_mask_pyr"][-1])], 1)     # (the COARSEST level's mask: see mask_mean)
        idx = torch.arange(rank * B, (rank + 1) * B, device=dev)
        all_rows, all_idx = mdist.gather_metric_rows(rows.to(coll_dev), idx.to(coll_dev))
        assert all_rows.shape[0] == B * world and bool(torch.isfinite(all_rows).all())

        # ---- quality fields, on EVERY rank (its own device), reduced to rank 0: the line of an N-GPU run carries the
        # same parity / roofline / chain-kernel / CPU-baseline fields as the 1-GPU line (roofline: min over ranks)
        agg = kernel_breakdown(net, inp, Dn)
        total_ms = sum(e["ms"] for e in agg.values())
        # the dominant kernel = the arithmetic kernel with the most device time (the bookkeeping launches carry no flops)
        name, dom = max(((k, v) for k, v in agg.items() if v["flops"] > 0), key=lambda kv: kv[1]["ms"])
        per_launch_ms = dom["ms"] / dom["launches"]
        # dom["flops"] counts the layer in its direct form (2 * cin * taps * cout per output).  The Winograd
        # kernels execute 16 multiplies per 2x2 outputs and tap plane instead of 36 (x 4/9): the roofline is
        # priced on the flops the matrix pipe actually executes, the direct-form figure is reported beside it.
        wino = " wino" in name
        direct_tfl = dom["flops"] / dom["launches"] / (per_launch_ms * 1e-3) / 1e12
        tfl = direct_tfl * (4.0 / 9.0 if wino else 1.0)
        fracs = gather_floats(tfl / PEAK_FP32_MFMA_TFLOPS, world, coll_dev)
        ch = agg.get("mvsn_incremental_cost_volume")
        chain_ms = gather_floats(ch["ms"] / ch["launches"] if ch else 0.0, world, coll_dev)

        if rank == 0:
            line["mean_idepth"] = float(mdist.average_rows(all_rows)[0])
            got0 = idepth[:1].cpu()
            line["l1_vs_ref"] = l1_against(ref0, got0, cfg["golden"])
            traffic, traffic_source = None, None
            # HBM bytes per launch from the committed PMC passes of THIS library (refused when the digest differs)
            pmc = load_profile_json(PMC_TRAFFIC_FILE)
            # (per-chain bytes depend on the configuration's geometry: the headline's entries are top-level -- configs 2 / 3 share
            # its coarse grid and depth --, the others come from passes of their own command under `configs`, or there is none)
            pmc_cfg = pmc if args.config in ("headline", "config2", "config3") else ((pmc or {}).get("configs", {}).get(args.config) or {})
            t = (pmc_cfg or {}).get(name)
            if t:
                traffic = (t["fetch_bytes_per_chain"] + t["write_bytes_per_chain"]) * B * Sn
                # (older files carry no flag: the raw / reported pair says whether the kernel's fetch figure was doubled)
                doubled = t.get("fetch_doubled", t["fetch_bytes_per_chain"] != t.get("fetch_bytes_per_chain_raw"))
                how = ("FETCH_SIZE x2 (gfx950 half-count of 16-byte streaming reads: this kernel's tiles arrive by 16-byte LDS-DMA)"
                       if doubled else "FETCH_SIZE as read (this kernel's 4- / 8-byte accesses are not half-counted)")
                traffic_source = (f"profiles/{pmc['_file']}: {how} + "
                                  f"WRITE_SIZE of separate rocprofv3 --pmc passes of the bench command with this library "
                                  f"(digest {pmc['_library_digest'][:12]}, {pmc.get('_chains_per_launch', '?')} chains per launch), "
                                  "per chain x this batch -- a committed pass, NOT a counter read during this run")
            elif pmc is not None:
                traffic_source = f"profiles/{pmc['_file']} holds no pass of this configuration's `{name}` kernel"
            else:
                traffic_source = (f"profiles/{PMC_TRAFFIC_FILE} is missing or was taken with another build of the library "
                                  "(digest mismatch): refused")
            line["roofline"] = {"kernel": name, "bound": "mfma", "achieved": tfl, "peak": PEAK_FP32_MFMA_TFLOPS,
                                "unit": "TFLOP/s", "frac": min(fracs), "frac_per_rank": fracs, "traffic": traffic,
                                "traffic_source": traffic_source,
                                "launches_per_step": dom["launches"], "avg_launch_ms": per_launch_ms,
                                "share_of_step": dom["ms"] / total_ms}
            if "+pass" in name:
                line["roofline"]["carried_pass"] = ("each of these launches also executes the in-place LeakyReLU(GroupNorm(.)) "
                                                    "pass of the other batch slice's previous layer (mvsn_conv_forward_carry): "
                                                    "its loads / stores are part of the launch time and of `traffic`, "
                                                    "`achieved` counts the convolution's flops only")
            if wino:
                line["roofline"]["form"] = ("Winograd F(2x2,3x3) per depth tap: 12 multiplies per output and "
                                            "(cin, cout) pair instead of 27; achieved = executed MFMA flops")
                line["roofline"]["direct_form_equivalent_TFLOPs"] = direct_tfl
            if ch:
                eng = net.engine()
                sec = max(chain_ms) * 1e-3 * ch["launches"]          # slowest rank
                form = {1: "direct", 2: "winograd", 3: "stepwise", 4: "banded"}.get(eng.last_chain_form, "?")
                wino_chain = form in ("winograd", "banded", "stepwise")
                direct_tfl_c = ch["flops"] / sec / 1e12
                exec_tfl = direct_tfl_c * (4.0 / 9.0 if wino_chain else 1.0)
                line["chain_kernel"] = {"kernel": "mvsn_incremental_cost_volume (warp + refine + cost volume, fused)",
                                        "form": form + (": Winograd F(2x2,3x3) for the three 3x3 convolutions of a step (16 "
                                                        "multiplies per 2x2 outputs instead of 36)" if wino_chain else ""),
                                        "avg_launch_ms": max(chain_ms), "avg_launch_ms_per_rank": chain_ms,
                                        "chains_per_launch": B * Sn,
                                        "algorithmic_GBps": ch["bytes"] / sec / 1e9,
                                        "frac_of_hbm_peak": ch["bytes"] / sec / 1e9 / PEAK_HBM_GBS,
                                        "direct_form_TFLOPs": direct_tfl_c,
                                        "direct_form_frac_of_fp32_mfma_peak": direct_tfl_c / PEAK_FP32_MFMA_TFLOPS,
                                        "executed_TFLOPs": exec_tfl,
                                        "executed_frac_of_fp32_mfma_peak": exec_tfl / PEAK_FP32_MFMA_TFLOPS,
                                        "share_of_step": ch["ms"] / total_ms}
                t = (pmc_cfg or {}).get("mvsn_incremental_cost_volume")
                if t and (form == "winograd" or args.config != "headline"):
                    line["chain_kernel"]["hbm_traffic_bytes_per_chain"] = {
                        "fetched": t["fetch_bytes_per_chain"], "written": t["write_bytes_per_chain"],
                        "algorithmic": t["algorithmic_bytes_per_chain"],
                        "ratio": (t["fetch_bytes_per_chain"] + t["write_bytes_per_chain"]) /
                        t["algorithmic_bytes_per_chain"], "source": f"profiles/{pmc['_file']} (separate PMC pass, this library)"}
            line["kernel_ms_per_step"] = {k: round(v["ms"], 3) for k, v in
                                          sorted(agg.items(), key=lambda kv: -kv[1]["ms"])[:16]}
            line["launches_per_forward"] = int(sum(v["launches"] for v in agg.values()))
            wino_chain_now = net.engine().last_chain_form in (2, 3, 4)      # every chain form but the direct one
            line["roofline_by_kernel"] = roofline_by_kernel(
                agg, total_ms, wino_names=("mvsn_incremental_cost_volume",) if wino_chain_now else ())
            if world == 1 and args.sustain > 0:
                windows, t_end = [], time.perf_counter() + args.sustain
                while time.perf_counter() < t_end:
                    n_steps, t1 = 0, time.perf_counter()
                    while time.perf_counter() - t1 < 2.0:
                        step()
                        n_steps += 1
                        if n_steps % 8 == 0:
                            torch.cuda.synchronize()
                    torch.cuda.synchronize()
                    windows.append(B * n_steps / (time.perf_counter() - t1))
                line["sustained"] = {"seconds": args.sustain, "window_s": 2.0,
                                     "depthmaps_per_s_per_window": [round(w, 1) for w in windows],
                                     "first": round(windows[0], 1), "last": round(windows[-1], 1),
                                     "min": round(min(windows), 1), "droop_last_vs_first": 1.0 - windows[-1] / windows[0],
                                     "timed_region_value": line["value"]}
            if world == 1 and headline and not args.no_tiers:
                # side legs: a failure in one of them must not cost the headline line
                for key, leg in (("pcie_inclusive", lambda: host_feed_rates(net, B, dev)),
                                 ("evaluate_rate", lambda: evaluate_rate(net, B, dev, line["value"])),
                                 ("batch_latency", lambda: batch_latency(net)),
                                 ("headline_by_batch", lambda: headline_by_batch(net, dev)),
                                 ("other_configs", lambda: other_configs(dev, skip=("headline",)))):
                    try:
                        line[key] = leg()
                    except Exception as exc:   # noqa: BLE001
                        line[key] = {"error": f"{type(exc).__name__}: {exc}"}
            if world == 1 and headline and args.precision == "fp32" and not args.no_tiers:
                # the two bf16-matrix-core tiers on the same resident inputs, reported beside the fp32 headline, never
                # as it: the 3 x bf16 split (fp32-equivalent arithmetic) and plain bf16 operands
                # (BASELINE config 5's speed tier -- outside the 1e-3 parity contract, its error is reported)
                eng = net.engine()
                for tier, key, dtype in (
                        ("bf16x3", "bf16x3_split_tier",
                         "3 x bf16 split (hi+lo operands, fp32 accumulate) on the 32->32 3x3 layers, f32 elsewhere"),
                        ("bf16", "bf16_operand_tier",
                         "bf16 operands, fp32 accumulate on the 32->32 3x3 layers (regulariser + refiner blocks), f32 "
                         "elsewhere; NOT within the 1e-3 parity contract"),
                        ("bf16s", "bf16_feature_tier",
                         "bf16 FEATURES (BASELINE config 5): the bf16-operand tier + the regulariser's intermediate volumes "
                         "STORED as bf16 (layer 0 fp32 -> bf16, layers 1-2 bf16 -> bf16, layer 3 bf16 -> fp32; fp32 "
                         "accumulation and GroupNorm statistics); NOT within the 1e-3 parity contract")):
                    eng.conv_precision = tier      # (= net.options.conv_precision: the engine's switches ARE the module's
                    #                                  options object, so the tier is part of every recorded plan's key)
                    for _ in range(max(1, args.warmup)):
                        out_t = step()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(args.steps):
                        out_t = step()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t1
                    got_t = out_t["left_idepthmap_pyr"][0][:1].cpu()
                    agg_t = kernel_breakdown(net, inp, Dn)
                    name_t, dom_t = max(agg_t.items(), key=lambda kv: kv[1]["ms"])
                    line[key] = {
                        "value": B * args.steps / dt, "unit": "depthmaps/s", "ms_per_step": dt / args.steps * 1e3,
                        "dtype": dtype,
                        "l1_vs_ref": {k: v for k, v in l1_against(ref0, got_t).items() if k != "rel_definitions"},
                        "dominant_kernel": name_t, "dominant_kernel_ms": round(dom_t["ms"], 3),
                        "kernel_ms_per_step": {k: round(v["ms"], 3) for k, v in
                                               sorted(agg_t.items(), key=lambda kv: -kv[1]["ms"])[:6]}}
                # the feature tier on the configuration BASELINE names it for: config 5's golden input at batch 1 (its error
                # against the reference's own depth map) and at 32 images (its rate), beside the fp32 figures of other_configs
                try:
                    c5 = CONFIGS["config5"]
                    eng.conv_precision = "bf16s"
                    _, inp5, ref5 = config_inputs(c5, 1, 0, dev)
                    out5 = run_forward(net, inp5, c5["D"])
                    entry = {"l1_vs_ref_config5": {k: v for k, v in l1_against(
                        ref5, out5["left_idepthmap_pyr"][0][:1].cpu(), c5["golden"]).items() if k != "rel_definitions"}}
                    del inp5, out5
                    _, inp5, _ = config_inputs(c5, 32, 0, dev)
                    for _ in range(2):
                        run_forward(net, inp5, c5["D"])
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(3):
                        run_forward(net, inp5, c5["D"])
                    torch.cuda.synchronize()
                    entry["config5_B=32_depthmaps_per_s"] = round(32 * 3 / (time.perf_counter() - t1), 1)
                    pmc5 = load_profile_json(FEATURE_TIER_PMC_FILE)
                    if pmc5:
                        entry["hbm_bytes_of_the_converted_launches"] = {k: v for k, v in pmc5.items() if not k.startswith("_l")}
                    line["bf16_feature_tier"].update(entry)
                    del inp5
                    torch.cuda.empty_cache()
                except Exception as exc:   # noqa: BLE001
                    line["bf16_feature_tier"]["config5"] = {"error": f"{type(exc).__name__}: {exc}"}
                eng.conv_precision = "fp32"
            if not args.no_cpu_baseline:
                # rank 0's host cores, once per job whatever N is (a bounded sample: shorter beside a multi-GPU run,
                # where the other ranks wait in the final barrier meanwhile)
                cb, ref_out = cpu_baseline(cfg, budget_s=15.0 if world == 1 else 6.0)
                line["cpu_baseline"] = cb
                o0 = ref_out["left_idepthmap_pyr"][0]
                line["l1_vs_oracle"] = float((got0 - o0).abs().mean())
                # image 0 sits in slice A of the two-slice towers and in the first round of every persistent kernel: the
                # first image of slice B and the LAST image of the step (last round, slice B) against the oracle as well
                for key, idx in (("l1_vs_oracle_slice_b", (B + 1) // 2), ("l1_vs_oracle_last", B - 1)):
                    if idx > 0:
                        line[key] = oracle_check(cfg, idx, idepth[idx:idx + 1].cpu())
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if rank == 0:
        emit(line)      # LAST: after the group is gone (nothing RCCL prints at tear-down can follow the line)


if __name__ == "__main__":
    main()
