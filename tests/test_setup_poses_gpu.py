"""The kernels that turn a pose into what the forward consumes -- plane_sweep_setup_kernel (csrc/mvsn_setup.hip),
prepare_cameras_kernel (csrc/mvsn_prepare.hip), reproject_kernel (csrc/mvsn_consistency.hip) -- on source poses in
general position (tests/pose_reference.py): rolls and a yaw whose pivoted LU interchanges rows, baselines along y and z,
forward motion with the epipole inside the image, level-4 grids on which only some pixels or none have a positive
idepth, the cap, the clamp, and the pixel on the epipole whose idepth is 0 / 0.  tests/test_pose_reference_cpu.py shows on
the CPU that each input reaches the branch it is here for, that none sits on a predicate, and that the reference's own
fp32 pipeline meets every tolerance used below."""
import numpy as np
import pytest
import torch

import pose_reference as pr
from conftest import rel_err
from test_hip_parity import net_for, assert_contract, _project_f64
from multi_view_stereonet_amd import _native, synthetic
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
from multi_view_stereonet_amd.weights import load_weights
from oracle import mvsn_oracle as oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


def _bits(x):
    return x.contiguous().view(torch.int32)


def _setup_launch(names, shape, shear, path):
    """One launch through both entry points (identical bits required), on the path it means to test: the outputs as
    numpy arrays, with the inputs."""
    eng = net_for("gta_sfm_150epochs").engine()
    rows, cols, D = shape
    Ts, K0, K4, r4, c4 = pr.chain_inputs(rows, cols, names, shear)
    S, B = len(Ts), K0.shape[0]
    K0r, K4r = K0.repeat(S, 1, 1), K4.repeat(S, 1, 1)
    assert _native.plane_sweep_setup_path(K0r, K4r, r4, c4) == [path] * (S * B)
    out = eng.plane_sweep_setup(torch.cat(Ts, 0).to(DEV), K0r.to(DEV), K4r.to(DEV), r4, c4, D)
    src = eng.plane_sweep_setup_sources([t.to(DEV) for t in Ts], K0.to(DEV), K4.to(DEV), r4, c4, D)
    for a, b in zip(out, src):
        assert torch.equal(_bits(a), _bits(b))
    samples, H4, Hinc, H0, base = (x.cpu().numpy() for x in out)
    return {"samples": samples, "H4": H4, "Hinc": Hinc, "H0": H0[:, 0], "baseline": base}, (Ts, K0, K4, r4, c4, D)


def _check_launch(name, shape, shear, path):
    """Every line of the issue's item 3 on one launch of 2 x 2 chains (pose_reference.mixed)."""
    names = pr.mixed(name, 2, 2)
    flat = [names[s][b] for s in range(2) for b in range(2)]
    got, (Ts, K0, K4, r4, c4, D) = _setup_launch(names, shape, shear, path)
    f64 = pr.setup64_chains(Ts, K0, K4, r4, c4, D)
    o_s, o_H4, o_H0, o_inc, o_base = (x.numpy() for x in pr.oracle_chains(Ts, K0, K4, r4, c4, D))
    assert np.array_equal(got["Hinc"][:, 0], np.broadcast_to(np.eye(3, dtype=np.float32), (4, 3, 3)))
    # the oracle's NaN pattern exactly (float64 has the same one: tests/test_pose_reference_cpu.py)
    assert np.array_equal(np.isnan(got["samples"]), np.isnan(o_s)) and np.array_equal(np.isnan(got["H4"]), np.isnan(o_H4))
    report = []
    for n, (fam, f) in enumerate(zip(flat, f64)):
        what = f"{fam} {r4}x{c4} D {D} shear {shear:g} path {path}"
        assert np.isfinite(got["H0"][n]).all()
        lines = [("baseline", got["baseline"][n], f["baseline"]), ("H0", got["H0"][n], f["H0"])]
        if not f["nan"]:
            lines += [("samples", got["samples"][n], f["samples"]), ("H4", got["H4"][n], f["H4"])]
            if fam not in pr.HINC_DROPPED:
                H64 = got["H4"][n].astype(np.float64)
                lines.append(("Hinc", got["Hinc"][n, 1:], np.linalg.inv(H64[:-1]) @ H64[1:]))
        for key, a, want in lines:
            ok, frac = pr.within(a, want, *pr.TOL[key])
            assert ok, (what, key, frac)
        if not f["nan"]:
            rs, rh = pr.error_ratios(got["samples"][n], got["H4"][n], o_s[n], o_H4[n], f)
            report.append(f"{fam} {rs:.2f} / {rh:.2f}")
            assert rs <= pr.RATIO_LIMIT and rh <= pr.RATIO_LIMIT, (what, rs, rh)
        if path == 3:
            b = n % 2
            own, rH0, rH4, rinc = pr.restated_chain(Ts[n // 2][b].numpy(), K0[b].numpy(), K4[b].numpy(), r4, c4, D,
                                                    samples=got["samples"][n])
            for key, a, want in (("samples", got["samples"][n], own), ("H0", got["H0"][n], rH0), ("H4", got["H4"][n], rH4),
                                 ("Hinc", got["Hinc"][n, 1:], rinc)):
                eq = pr.same_bits(a, want)
                assert eq.all(), (what, key, "differs from the restated fp32 order in", int((~eq).sum()), "of", eq.size)
    print(f"{r4}x{c4} D {D} shear {shear:g} path {path}: error over the oracle's, samples / H4: " + ", ".join(report))
    return got, f64


@pytest.mark.parametrize("name,shape,shear,path", pr.SETUP_CASES + pr.CLAMP_CASES)
def test_plane_sweep_setup_on_general_poses(name, shape, shear, path):
    """Against float64 at the tolerances of test_plane_sweep_setup, on every path; the error against float64 over the
    oracle's at most 4 (printed); on the reference-order path, samples, H0, H4 and H_inc bit for bit the numpy
    restatement of that order evaluated at the kernel's own samples -- the line that fails if a row interchange of
    ref32::inverse_pose or ref32::inverse3 is mirrored wrongly.  The family `general` is left out of the H_inc line
    against float64 (not of the bit-for-bit one): the reference's own fp32 H_inc misses that tolerance on it (1.14 of it
    at 16x32, D 16).  CLAMP_CASES reach `1 / top < tz`."""
    got, f64 = _check_launch(name, shape, shear, path)
    if (name, shape, shear, path) in pr.CLAMP_CASES:
        assert f64[0]["clamped"] and pr.within(got["samples"][0, -1], 1.0 / f64[0]["tz"], *pr.TOL["samples"])[0]


@pytest.mark.parametrize("name,shape,count,capped", pr.PARTIAL_CASES)
def test_sample_top_with_a_partial_count_or_the_cap(name, shape, count, capped):
    """Only `count` of the level-4 pixels have a positive idepth: the sample top against float64 at the samples'
    tolerance.  A count off by one pixel moves it by 1 / 500 or more."""
    got, (Ts, K0, K4, r4, c4, D) = _setup_launch(pr.mixed(name, 2, 2), shape, 0.0, 3)
    f = pr.setup64(Ts[0][0].numpy(), K0[0].numpy(), K4[0].numpy(), r4, c4, D)
    assert f["count"] == count and f["capped"] == capped
    ok, frac = pr.within(got["samples"][0, -1], f["samples"][-1], *pr.TOL["samples"])
    print(f"{name} {r4}x{c4}: {count} of {r4 * c4} pixels positive, raw mean {f['raw']:.4g}, top {got['samples'][0, -1]:.7g} "
          f"({frac:.3f} of the tolerance)")
    assert ok, (name, shape, frac)
    if capped:
        assert got["samples"][0, -1] == 2.0


@pytest.mark.parametrize("name,shape,shear,path", pr.NAN_CASES)
def test_nan_chain_follows_the_reference_and_leaves_its_neighbours_alone(name, shape, shear, path):
    """No positive pixel (`backward`), or the pixel on the epipole whose idepth is 0 / 0 (`pure_forward`; on the fp64
    evaluation of the samples too -- under 8 pixels, a shear term --, which used to drop that pixel and return finite
    samples): samples and H4 have the oracle's NaN pattern exactly, H0 is finite and inside tolerance, and the other
    chains of the launch carry the bits they have in a launch without the NaN chain."""
    got, f64 = _check_launch(name, shape, shear, path)
    assert f64[0]["nan"] and np.isnan(got["samples"][0]).all() and np.isnan(got["H4"][0]).all()
    names = pr.mixed(name, 2, 2)
    names[0][0] = "diag"
    clean, _ = _setup_launch(names, shape, shear, path)
    for key in got:
        assert np.isfinite(clean[key]).all() and np.array_equal(got[key][1:].view(np.int32), clean[key][1:].view(np.int32)), key


UNPACK_NAMES = (pr.mixed("roll50", 2, 3), [["general", "backward", "pure_forward"], ["dive", "yaw60", "roll-120"]])


@pytest.mark.parametrize("names", UNPACK_NAMES)
def test_device_unpacker_on_general_poses(names):
    """mvsn_prepare_cameras, S = 2, B = 3 at 64x128: the rotation passes through untouched; the translation over the first
    source's baseline within 2 ulps of float64; the inverse -- an fp64 inverse rounded once, then one fp32 division: 1.5
    ulps at most -- within 2 ulps, entries that are zero in exact arithmetic within 2^-23 of the matrix's largest entry;
    the K pyramid the host unpacker's bits."""
    batch = pr.with_poses(synthetic.make_batch(64, 128, 2, batch=3, seed=9), names)
    dev = snu.multi_view_unpack_batch(batch, torch.device(DEV), 5)
    host = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    Tn64, Ti64, base64 = pr.unpacked64(batch)
    assert pr.within(dev["baseline"].cpu().numpy(), base64, 1e-6, 0.0)[0]
    for a, b in zip(dev["K_pyr"], host["K_pyr"]):
        assert torch.equal(_bits(a.cpu()), _bits(b))
    worst = [0.0, 0.0]
    for s in range(2):
        Tn, Ti = dev["T_right_in_left"][s].cpu().numpy(), dev["T_left_in_right"][s].cpu().numpy()
        raw = batch["T_right_in_left"][s][:, 0].numpy()
        assert np.array_equal(Tn[:, :, :3].view(np.int32), raw[:, :, :3].view(np.int32)) and np.array_equal(Tn[:, 3], raw[:, 3])
        e = np.abs(Tn[:, :3, 3] - Tn64[s][:, :3, 3]) / pr.ulp32(Tn64[s][:, :3, 3])
        assert (e <= 2.0).all(), (s, e)
        big = np.abs(Ti64[s]).reshape(3, -1).max(1)[:, None, None]
        zero = np.abs(Ti64[s]) < 1e-12 * big
        bound = np.where(zero, 2.0 ** -23 * big, 2.0 * pr.ulp32(Ti64[s]))
        ei = np.abs(Ti - Ti64[s]) / bound
        assert (ei <= 1.0).all(), (s, np.argwhere(ei > 1.0), ei.max())
        worst = [max(worst[0], float(e.max())), max(worst[1], float(ei.max()))]
    print(f"device unpacker: translation {worst[0]:.2f} ulps of float64 at most, inverse {worst[1]:.2f} of its bound")


@pytest.mark.parametrize("rows,cols", pr.PROJECTION_SIZES)
def test_projection_and_occlusion_on_general_poses(rows, cols):
    """mvsn_idepth_reproject / mvsn_occlusion_mask at level 0 through a roll, a general rotation, a vertical baseline and
    forward motion: test_two_view_projection_and_occlusion_through_changed_cameras's float64 reference and tolerances."""
    from multi_view_stereonet_amd import losses
    for name, K, T, L, R in pr.projection_inputs(rows, cols):
        uv, idp, inv = losses.idepthmap_projector(K.to(DEV), T.to(DEV), L.to(DEV))
        uv64, idp64, inv64 = _project_f64(K, T, L)
        e_uv = pr.within(uv.cpu().numpy(), uv64.numpy(), 1e-5, 2e-6)
        e_id = pr.within(idp.cpu().numpy(), idp64.numpy(), 1e-5, 1e-7)
        edge = torch.minimum((uv64[..., 0].abs() - 1.0).abs(), (uv64[..., 1].abs() - 1.0).abs()).unsqueeze(1)
        inv_diff = inv.cpu() != inv64
        occ = losses.get_occlusion_mask(K.to(DEV), T.to(DEV), L.to(DEV), None, R.to(DEV), None).cpu()
        ref = oracle.get_occlusion_mask(K, T, L, R)
        occ_diff = int((occ != ref).sum())
        print(f"{name} {rows}x{cols}: uv / idepth' error over tolerance {e_uv[1]:.3f} / {e_id[1]:.3f}; invalid flags differing "
              f"{int(inv_diff.sum())}, occlusion flags differing {occ_diff} of {ref.numel()} ({float(inv64.double().mean()):.3f} out of the image)")
        assert e_uv[0] and e_id[0], (name, e_uv, e_id)
        assert int(inv_diff.sum()) <= 1 and bool((edge[inv_diff] < 16 * 2.0 ** -23).all()), name
        assert occ.dtype == torch.bool and occ_diff <= max(2, ref.numel() // 2000), (name, occ_diff)


@pytest.mark.parametrize("name", pr.FINITE)
def test_forward_on_general_poses_vs_oracle(name):
    """End to end at 64x128, D 8, S 2, B 2 -- the only place the set-up's rolled H_inc meets the `auto` choice of chain
    form: every level at test_forward_ragged_sizes_vs_oracle's budgets, the final map under the contract."""
    wname, D = "gta_sfm_150epochs", 8
    batch = pr.with_poses(synthetic.make_batch(64, 128, 2, batch=2, seed=64 + 128, smooth=True), pr.mixed(name, 2, 2))
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    ref = oracle.forward(load_weights(wname), inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"],
                         inp["right_image_pyr"], D)
    net = net_for(wname)
    out = snu.multi_view_forward(net, snu.multi_view_unpack_batch(batch, torch.device(DEV), 5),
                                 {"num_idepth_samples": D, "cost_volume_filter": True, "refiners": [True] * 5})
    figures = [(lvl,) + tuple(rel_err(out["left_idepthmap_pyr"][lvl].cpu(), ref["left_idepthmap_pyr"][lvl])) for lvl in range(5)]
    print(f"{name} (with {pr.mixed(name, 2, 2)}), chain form {net.engine().last_chain_form}: "
          + "; ".join(f"level {l} mean-rel {m:.2e} max-rel {x:.2e}" for l, m, x in figures))
    for lvl, mean_rel, max_rel in figures:
        assert out["left_idepthmap_pyr"][lvl].shape == ref["left_idepthmap_pyr"][lvl].shape
        assert mean_rel < 2e-4 and max_rel < 1e-3, (name, lvl, mean_rel, max_rel)
    assert_contract(out["left_idepthmap_pyr"][0].cpu(), ref["left_idepthmap_pyr"][0], f"{name} 64x128")
