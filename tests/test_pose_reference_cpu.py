"""The inputs of tests/test_setup_poses_gpu.py earn their names, without a GPU: every family of tests/pose_reference.py
reaches the branch it is listed for, no case that is compared numerically has a pixel on a predicate, the oracle alone
meets the tolerances the kernels are asked to meet against float64, and the numpy restatement of the reference's fp32
order (tests/test_reference_geometry_cpu.py -- what csrc/mvsn_setup.hip's namespace ref32 implements) equals the oracle
on these poses as it does on make_batch's."""
import functools

import numpy as np
import pytest
import torch

import pose_reference as pr
import test_reference_geometry_cpu as rg

LAUNCHES = pr.SETUP_CASES + pr.CLAMP_CASES + pr.NAN_CASES


@functools.lru_cache(maxsize=None)
def launch(name, shape, shear):
    """The chains of a launch: names, inputs, float64 facts and the oracle's outputs."""
    rows, cols, D = shape
    names = pr.mixed(name, 2, 2)
    Ts, K0, K4, r4, c4 = pr.chain_inputs(rows, cols, names, shear)
    flat = [names[s][b] for s in range(2) for b in range(2)]
    return flat, (Ts, K0, K4, r4, c4, D), pr.setup64_chains(Ts, K0, K4, r4, c4, D), pr.oracle_chains(Ts, K0, K4, r4, c4, D)


def chains():
    """Every distinct (family, shape, shear) chain of every launch, once."""
    seen = set()
    for name, shape, shear, path in LAUNCHES:
        flat, inputs, f64, ora = launch(name, shape, shear)
        for n, fam in enumerate(flat):
            if (fam, shape, shear) not in seen:
                seen.add((fam, shape, shear))
                yield fam, shape, shear, n, inputs, f64[n], [x[n] for x in ora]


def test_families_are_deterministic_rigid_poses_and_launches_mix_them():
    for name in pr.FAMILIES:
        T = pr.pose(name).double()
        assert torch.equal(pr.pose(name), pr.pose(name))
        assert float((T[:3, :3] @ T[:3, :3].T - torch.eye(3, dtype=torch.float64)).abs().max()) < 2e-7
        assert abs(float(torch.linalg.det(T[:3, :3])) - 1.0) < 2e-7 and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    names = pr.mixed("roll50", 2, 2)
    assert names == [["roll50", "yaw60"], ["diag", "vertical"]]
    assert pr.INTERCHANGES[names[0][0]] and not pr.INTERCHANGES[names[1][0]]       # pivoting and non-pivoting in one launch
    for name in pr.FINITE + ("backward", "pure_forward", "dive"):
        flat = sum(pr.mixed(name, 2, 3), [])
        assert flat[0] == name and len(set(flat)) == 6
    batch = pr.with_poses(pr.synthetic.make_batch(64, 128, 2, batch=2, seed=3), names)
    assert torch.equal(batch["T_right_in_left"][1][0, 0], pr.pose("diag")) and batch["T_right_in_left"][0].shape == (2, 1, 4, 4)


def test_every_family_reaches_the_interchanges_it_is_listed_for():
    """The LU of the transposed, normalised pose (MKL's, as lu_of_transpose restates it and torch confirms): the columns
    with a row interchange -- what ref32::inverse_pose mirrors with `ip[j] != j`."""
    for name, want in pr.INTERCHANGES.items():
        Tn = rg.own_baseline(pr.pose(name).numpy())
        LU, ip = rg.lu_of_transpose(Tn)
        assert [j for j in range(4) if ip[j] != j] == want, (name, ip)
        LU_t, piv_t = torch.linalg.lu_factor(torch.from_numpy(Tn).t().contiguous())
        assert [int(p) - 1 for p in piv_t] == ip and np.array_equal(LU.view(np.int32), LU_t.numpy().view(np.int32)), name
    assert sum(bool(v) for v in pr.INTERCHANGES.values()) >= 4


def test_partial_counts_cap_clamp_nan_and_the_degenerate_pixel_where_claimed():
    for name, shape, count, capped in pr.PARTIAL_CASES:
        f = launch(name, shape, 0.0)[2][0]
        P = (shape[0] // 16) * (shape[1] // 16)
        assert f["count"] == count and 0 < count < P and f["capped"] == capped and not f["nan"] and not f["clamped"], (name, shape, f["count"])
    f = launch("backward", (256, 512, 16), 0.0)[2][0]
    assert f["raw"] > 60.0 and f["samples"][-1] == 2.0
    for name, shape, shear, path in pr.NAN_CASES:
        flat, inputs, f64, ora = launch(name, shape, shear)
        f = f64[0]
        assert f["nan"] and np.isnan(f["samples"]).all() and np.isnan(f["H4"]).all() and np.isfinite(f["H0"]).all(), (name, shape)
        assert not any(g["nan"] for g in f64[1:])
        if name == "backward":
            assert f["count"] == 0 and np.isfinite(f["idepth"]).all() and (f["idepth"] < 0).all()
        else:                                                     # exactly one pixel, on the epipole: norm 0, idepth 0 / 0
            on = f["norm"] < 1e-6
            P = on.size
            assert int(on.sum()) == 1 and f["norm"][on][0] == 0.0 and np.isnan(f["idepth"][on]).all() and f["count"] == P - 1
            assert np.isfinite(f["idepth"][~on]).all() and (f["idepth"][~on] > 0).all()
    for name, shape, shear, path in pr.CLAMP_CASES:
        f = launch(name, shape, shear)[2][0]
        assert f["clamped"] and not f["capped"] and not f["nan"] and f["samples"][-1] == 1.0 / f["tz"], (name, shape)
    for name, shape, shear, path in pr.SETUP_CASES:                # ... and nowhere else
        for fam, f in zip(*launch(name, shape, shear)[:3:2]):
            assert not f["nan"] and not f["clamped"] and f["capped"] == (fam == "backward"), (name, shape, fam)
    f = launch("forward", (64, 128, 8), 0.0)[2][0]
    assert f["tz"] > 0.998 and abs(f["tz"]) < 1.0
    assert abs(pr.normalised_pose64(pr.pose("vertical").numpy())[1][1, 3]) > 0.99          # a baseline along y


def test_no_pixel_sits_on_a_predicate():
    """In float64, for every chain compared numerically: every per-pixel idepth is beyond +-1e-4 of the chain's mean, no
    `norm` within a factor 10 of 1e-6 (the one pixel of pure_forward is exactly 0), the raw mean and the capped one not
    within 1 % of 2.0 or of 1 / tz."""
    n = 0
    for fam, shape, shear, _, inputs, f, _ in chains():
        on = f["norm"] == 0.0
        assert int(on.sum()) == (1 if fam == "pure_forward" and f["nan"] else 0), (fam, shape)
        assert not ((f["norm"][~on] > 1e-7) & (f["norm"][~on] < 1e-5)).any() and (f["norm"][~on] > 1e-5).all(), (fam, shape, shear)
        if f["nan"]:
            continue
        assert (np.abs(f["idepth"]) > 1e-4 * abs(f["raw"])).all(), (fam, shape, shear, float(np.abs(f["idepth"]).min() / f["raw"]))
        assert abs(f["raw"] / 2.0 - 1.0) > 0.01, (fam, shape, shear, f["raw"])
        if f["tz"] > 0:
            assert abs(f["raw"] * f["tz"] - 1.0) > 0.01 and abs(min(f["raw"], 2.0) * f["tz"] - 1.0) > 0.01, (fam, shape, shear, f["raw"], f["tz"])
        n += 1
    assert n >= 60


def test_the_oracle_meets_the_tolerances_against_float64():
    """The reference's own fp32 pipeline stays inside what the kernel is asked to meet, and has float64's NaN pattern.
    The one exception is the H_inc line on the families of HINC_DROPPED, which the GPU test leaves out of that line for
    this reason: each of them is shown here to miss it."""
    worst = {k: 0.0 for k in pr.TOL}
    missed = set()
    for fam, shape, shear, n, inputs, f, (smp, H4, H0, inc, base) in chains():
        assert np.array_equal(np.isnan(smp.numpy()), np.isnan(f["samples"])), (fam, shape, shear)
        assert np.array_equal(np.isnan(H4.numpy()), np.isnan(f["H4"])), (fam, shape, shear)
        checks = [("baseline", base.numpy(), f["baseline"]), ("H0", H0.numpy(), f["H0"])]
        if not f["nan"]:
            H64 = H4.numpy().astype(np.float64)
            checks += [("samples", smp.numpy(), f["samples"]), ("H4", H4.numpy(), f["H4"]),
                       ("Hinc", inc.numpy(), np.linalg.inv(H64[:-1]) @ H64[1:])]
        for what, got, want in checks:
            ok, frac = pr.within(got, want, *pr.TOL[what])
            if what == "Hinc" and fam in pr.HINC_DROPPED:
                missed |= set() if ok else {fam}
                continue
            worst[what] = max(worst[what], frac)
            assert ok, (fam, shape, shear, what, frac)
    assert missed == set(pr.HINC_DROPPED)
    print("oracle against float64, worst error over tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_the_restatement_equals_the_oracle_on_these_poses():
    """inverse_pose, inverse3, restated_homography and idepth_samples_restated against torch on this host, bit for bit:
    every pose, every H0 / H4 / H_inc entry at the oracle's own samples.  The samples themselves: bit for bit except
    where torch's vectorised sqrt is an ulp off the correctly rounded root (the residue
    test_restated_idepth_samples_match_the_oracle_and_the_captured_reference documents; at least 0.9 of the chains)."""
    for name in pr.FAMILIES:
        Tn = rg.own_baseline(pr.pose(name).numpy())
        want = torch.linalg.inv(torch.from_numpy(Tn)[None])[0].numpy()
        assert np.array_equal(rg.inverse_pose(Tn).view(np.int32), want.view(np.int32)), name
    total = same = 0
    entries = {"H0": [0, 0], "H4": [0, 0], "Hinc": [0, 0]}
    for fam, shape, shear, n, (Ts, K0, K4, r4, c4, D), f, (smp, H4, H0, inc, base) in chains():
        if shear:
            continue                                               # (the restatement covers pin-hole intrinsics)
        T, b = Ts[n // 2][n % 2].numpy(), n % 2
        own, rH0, rH4, rinc = pr.restated_chain(T, K0[b].numpy(), K4[b].numpy(), r4, c4, D, samples=smp.numpy())
        total += 1
        same += int(pr.same_bits(own, smp.numpy()).all())
        assert np.array_equal(np.isnan(own), np.isnan(smp.numpy())), (fam, shape)
        if not f["nan"]:
            assert own[0] == 0 and pr.within(own[1:], smp.numpy()[1:], 2.0 ** -22, 0.0)[0], (fam, shape)
        for what, got, want in (("H0", rH0, H0.numpy()), ("H4", rH4, H4.numpy()), ("Hinc", rinc, inc.numpy())):
            eq = pr.same_bits(got, want)
            entries[what][0] += int(eq.sum())
            entries[what][1] += eq.size
            assert eq.all(), (fam, shape, what, int((~eq).sum()), eq.size)
    print(f"restated samples equal to the oracle's bit for bit: {same} of {total} chains; entries equal: "
          + ", ".join(f"{k} {a} of {b}" for k, (a, b) in entries.items()))
    assert same >= 0.9 * total and total >= 40


def test_the_restatement_keeps_the_error_ratio_of_the_kernel_it_describes():
    """What the GPU test asks of the kernel on the reference-order path, asked of the restatement: its error against
    float64 is at most RATIO_LIMIT times the oracle's (it is the oracle's, to the bit, wherever the test above holds)."""
    worst = [0.0, 0.0]
    for fam, shape, shear, n, (Ts, K0, K4, r4, c4, D), f, (smp, H4, H0, inc, base) in chains():
        if shear or f["nan"] or r4 * c4 < 8:
            continue
        own, _, rH4, _ = pr.restated_chain(Ts[n // 2][n % 2].numpy(), K0[n % 2].numpy(), K4[n % 2].numpy(), r4, c4, D)
        rs, rh = pr.error_ratios(own, rH4, smp.numpy(), H4.numpy(), f)
        worst = [max(worst[0], rs), max(worst[1], rh)]
        assert rs <= pr.RATIO_LIMIT and rh <= pr.RATIO_LIMIT, (fam, shape, rs, rh)
    print(f"restatement's error over the oracle's, against float64: samples {worst[0]:.2f}, H4 {worst[1]:.2f}")


@pytest.mark.parametrize("rows,cols", pr.PROJECTION_SIZES)
def test_projection_cases_keep_every_point_well_in_front_of_the_right_camera(rows, cols):
    """The condition of the reprojection test: float64 z' above 0.2 times the point's depth at every pixel."""
    from test_hip_parity import _project_f64
    for name, K, T, L, R in pr.projection_inputs(rows, cols):
        _, idp64, _ = _project_f64(K, T, L)
        z, depth = 1.0 / idp64 - 1e-6, 1.0 / (L.double() + 1e-6)
        assert float((z / depth).min()) > 0.2, (name, float((z / depth).min()))
