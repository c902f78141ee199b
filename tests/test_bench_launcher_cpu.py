"""`python bench.py --gpus N` with no torchrun around it must launch its own ranks (the plain command
died on a WORLD_SIZE check).  Here: the launcher path with N=2 CPU ranks over gloo and a stand-in step
(--launcher-selftest: launch, barrier, max-over-ranks timing, all-gather of metric rows; no forward, no GPU)."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def _run(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout          # exactly ONE JSON line, from rank 0
    assert p.stdout.rstrip("\n").splitlines()[-1] == lines[0]        # ... and it is the LAST line printed
    assert len(lines[0]) < 4096
    return json.loads(lines[0])


def test_plain_command_self_launches_two_ranks():
    line = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4", "--launcher-selftest"])
    assert line["n_gpus"] == 2 and line["world_size"] == 2 and line["backend"] == "gloo"
    assert line["steps"] == 3 and line["warmup"] == 1
    assert len(line["per_rank_ms_per_step"]) == 2
    assert line["rows_gathered"] == 8 and line["rank_sum"] == 4.0       # 4 rows of rank 0 (0.0) + 4 of rank 1 (1.0)
    # the line of an N > 1 run carries the parity / roofline / chain-kernel / CPU-baseline fields too (stand-ins here),
    # the roofline fraction reduced as the minimum over the ranks' own measurements
    for key in ("l1_vs_ref", "roofline", "chain_kernel", "cpu_baseline"):
        assert key in line, key
    assert line["roofline"]["frac_per_rank"] == [0.5, 0.6] and line["roofline"]["frac"] == 0.5


def test_real_line_builds_quality_fields_for_every_world_size():
    """The measuring path itself (not the self-test): the quality fields are assembled outside any `world == 1`
    guard, and --config offers every BASELINE configuration with its own reference fixture."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")

    def guarded_by_world1(node, target, under=False):
        for child in ast.iter_child_nodes(node):
            here = under
            if isinstance(child, ast.If) and "world == 1" in ast.unparse(child.test):
                here = True
            if isinstance(child, ast.Assign) and any(target in ast.unparse(t) for t in child.targets) and here:
                return True
            if guarded_by_world1(child, target, here):
                return True
        return False

    for key in ('line["l1_vs_ref"]', 'line["roofline"]', 'line["chain_kernel"]', 'line["cpu_baseline"]'):
        assert key in src and not guarded_by_world1(main, key), key
    sys.path.insert(0, ROOT)
    import bench
    assert set(bench.CONFIGS) == {"headline", "config2", "config3", "config4", "config5"}
    assert bench.CONFIGS["config3"]["S"] == 5 and bench.CONFIGS["config3"]["batch"] == 1
    for cfg in bench.CONFIGS.values():
        assert os.path.exists(os.path.join(ROOT, "tests", "golden", cfg["golden"]))


def test_single_rank_needs_no_launcher():
    line = _run(["--gpus", "1", "--steps", "2", "--warmup", "0", "--batch", "3", "--launcher-selftest"])
    assert line["n_gpus"] == 1 and line["world_size"] == 1 and line["rows_gathered"] == 3


def test_final_line_is_small_last_and_carries_the_contract():
    """round 5's single 22 KB line outgrew the driver's stdout capture (`parsed: null`).  The full
    record of that very run (profiles/r05_final/bench_default.json), widened to 8 ranks, must come out as a DETAIL line
    + sidecar and ONE final JSON line < 4 KB holding the contract's keys, `roofline` and `cpu_baseline`."""
    import io
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_final", "bench_default.json")))
    assert len(json.dumps(full)) > 20000
    full["n_gpus"] = full["world_size"] = 8
    full["roofline"]["frac_per_rank"] = [0.66716 + i * 1e-3 for i in range(8)]
    full["chain_kernel"]["avg_launch_ms_per_rank"] = [5.6535 + i * 1e-2 for i in range(8)]
    full["per_rank_ms_per_step"] = [68.9 + i * 0.0123456789 for i in range(8)]
    buf = io.StringIO()
    saved, bench.DETAIL_FILE = bench.DETAIL_FILE, os.path.join(os.environ.get("TMPDIR", "/tmp"), "bench_detail_test.json")
    try:
        bench.emit(full, buf)
        assert json.load(open(bench.DETAIL_FILE)) == full
    finally:
        bench.DETAIL_FILE = saved
    out = buf.getvalue().rstrip("\n").splitlines()
    assert len(out) == 2 and out[0].startswith("DETAIL {") and json.loads(out[0][7:]) == full
    assert [ln for ln in out if ln.startswith("{")] == [out[-1]]
    assert len(out[-1]) < 4096
    line = json.loads(out[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "world_size", "backend",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "l1_vs_ref", "roofline",
                "chain_kernel", "cpu_baseline", "l1_vs_oracle"):
        assert key in line, key
    assert abs(line["value"] - full["value"]) < 1e-3 * full["value"]
    assert line["config"]["workload"] == full["config"]["workload"]
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "frac_per_rank", "traffic", "launches_per_step",
                "avg_launch_ms"):
        assert key in line["roofline"], key
    assert abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-3
    for key in ("value", "unit", "cores", "kind", "sample", "cpu_model", "one_thread", "all_physical_cores"):
        assert key in line["cpu_baseline"], key
    # no prose outside the contract's own strings: every other string leaf is short
    def strings(node, path=""):
        if isinstance(node, dict):
            for k, v in node.items():
                yield from strings(v, f"{path}.{k}")
        elif isinstance(node, str):
            yield path, node
    assert all(len(v) <= 160 for _, v in strings(line)), [p for p, v in strings(line) if len(v) > 160]
    # a pathological record (every optional group inflated) still yields a parsable line under the limit
    full["l1_vs_oracle_last"] = {f"k{i}": float(i) for i in range(300)}
    assert len(bench.final_line(full)) < 4096


def test_dump_outputs_writes_the_same_float_arrays_every_time(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: every tensor the forward returned becomes DIR/<key>_<level>.npy in float32 (bool masks as
    0 / 1); an output that fits its share of DUMP_LIMIT is written whole, a larger one as a seeded sample of its elements
    in increasing index order -- the same elements on every call, so that two builds compare output for output."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    assert bench.DUMP_LIMIT <= 64 * 10 ** 6 - 2 ** 16              # the files' headers fit beside it
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * 4 * 50000)        # 50 000 elements per array of three
    g = torch.Generator().manual_seed(3)
    big = torch.rand(2, 4, 100, 90, generator=g)
    small = torch.rand(2, 1, 25, 20, generator=g)
    out = {"left_idepthmap_pyr": [small, big], "left_idepthmap_mask_pyr": [big > 0.5, None]}
    shapes = bench.dump_outputs(out, str(tmp_path / "a"))
    assert shapes == {"left_idepthmap_pyr_0": [2, 1, 25, 20], "left_idepthmap_pyr_1": [50000],
                      "left_idepthmap_mask_pyr_0": [50000]}
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in shapes}
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["left_idepthmap_pyr_0"], small.numpy())
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(big.numel(), 50000, replace=False))
    assert np.array_equal(a["left_idepthmap_pyr_1"], big.numpy().reshape(-1)[idx])
    assert np.array_equal(a["left_idepthmap_mask_pyr_0"], (big.numpy().reshape(-1)[idx] > 0.5).astype(np.float32))
    bench.dump_outputs(out, str(tmp_path / "b"))
    for k in shapes:
        assert (tmp_path / "a" / f"{k}.npy").read_bytes() == (tmp_path / "b" / f"{k}.npy").read_bytes(), k
