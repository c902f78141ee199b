"""What csrc/mvsn_setup.hip (namespace ref32) assumes about the reference's fp32 geometry, checked on the HOST against the torch
that generated the fixtures: the operation order of torch's CPU `inverse` of a pose, of the intrinsics and of a 3x3 homography, of
its small matrix products, of `matmul(KRKinv, xyz_pix)` and of `torch.sum` (stereo/image_predictor.py:120-209, 400-461,
multi_view_stereonet.py:131-194, 279-282).  A plain numpy restatement of those orders -- the same one the kernel implements --
reproduces torch bit for bit (random matrices, poses, homographies), the oracle's idepth samples and homographies, and the capture
of what the reference hands its warper (tests/golden/g11_incremental_homographies.npz; g12_camera_forms.npz: the same through
cameras with fx != fy, off-centre principal points and ragged pyramids).  If a future torch / MKL changes an order,
these tests say so (the kernel would then merely be one more correctly-behaved fp32 evaluation, a few ulps from the reference's, as
it was before round 6); the g11 / g12 comparisons are data against data and do not depend on the host."""
import numpy as np
import torch

from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
from multi_view_stereonet_amd import synthetic
from oracle import mvsn_oracle as oracle

f32 = np.float32


def fmaf(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def lu_of_transpose(T):
    """MKL's sgetrf as torch's `linalg_solve_ex` shortcut calls it (on A^T): right-looking, first-maximum partial pivoting, FMA
    updates, a column scaled by the reciprocal pivot -- except the last, one-element column, which is divided."""
    A = np.ascontiguousarray(T.T).astype(f32)
    n = 4
    ip = [0] * n
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        ip[j] = p
        if p != j:
            A[[j, p]] = A[[p, j]]
        r = f32(1) / A[j, j]
        for i in range(j + 1, n):
            A[i, j] = f32(A[i, j] / A[j, j]) if n - 1 - j <= 1 else f32(A[i, j] * r)
        for i in range(j + 1, n):
            for k in range(j + 1, n):
                A[i, k] = fmaf(-A[i, j], A[j, k], A[i, k])
    return A, ip


def inverse_pose(T):
    """... then sgetrs with trans = 'T' on the identity, element by element as MKL's small-matrix kernels order it (found by
    matching bits, element by element, on random matrices: 1200 of 1200 for every unknown).  U^T y = e_c: reciprocal diagonal,
    the products rounded and subtracted one by one, only the last term of the last unknown fused; L^T x = y: x3 = y3, x2 one fused
    multiply-subtract, x1 and x0 a DOT PRODUCT subtracted from y (the first product rounded, the others fused into it, in the
    order k = 3, 2 for x1 and k = 2, 1, 3 for x0); then the row interchanges in reverse."""
    A, ip = lu_of_transpose(T)
    r = [f32(1) / A[i, i] for i in range(4)]
    X = np.zeros((4, 4), f32)
    for c in range(4):
        b = np.zeros(4, f32)
        b[c] = 1
        y0 = f32(b[0] * r[0])
        y1 = f32(f32(b[1] - f32(A[0, 1] * y0)) * r[1])
        y2 = f32(f32(f32(b[2] - f32(A[1, 2] * y1)) - f32(A[0, 2] * y0)) * r[2])
        y3 = f32(fmaf(-A[2, 3], y2, f32(f32(b[3] - f32(A[1, 3] * y1)) - f32(A[0, 3] * y0))) * r[3])
        z3 = y3
        z2 = fmaf(-A[3, 2], z3, y2)
        z1 = f32(y1 - fmaf(A[2, 1], z2, f32(A[3, 1] * z3)))
        z0 = f32(y0 - fmaf(A[3, 0], z3, fmaf(A[1, 0], z1, f32(A[2, 0] * z2))))
        z = [z0, z1, z2, z3]
        for j in range(3, -1, -1):
            if ip[j] != j:
                z[j], z[ip[j]] = z[ip[j]], z[j]
        X[:, c] = z
    return X


def inverse3(M):
    """The same shortcut on a 3x3 (`torch.inverse(H[:, d-1].unsqueeze(1))`, multi_view_stereonet.py:281 -- the slice of the
    permuted (B,D,3,3) family is contiguous for every batch size): LU of the transpose as above, y without a fused operation,
    x2 = y2, x1 one fused multiply-subtract, x0 = y0 - fma(l10, x1, l20 * x2)."""
    A = np.ascontiguousarray(M.T).astype(f32)
    ip = [0] * 3
    for j in range(3):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        ip[j] = p
        if p != j:
            A[[j, p]] = A[[p, j]]
        rj = f32(1) / A[j, j]
        for i in range(j + 1, 3):
            A[i, j] = f32(A[i, j] / A[j, j]) if 2 - j <= 1 else f32(A[i, j] * rj)
        for i in range(j + 1, 3):
            for k in range(j + 1, 3):
                A[i, k] = fmaf(-A[i, j], A[j, k], A[i, k])
    r = [f32(1) / A[i, i] for i in range(3)]
    X = np.zeros((3, 3), f32)
    for c in range(3):
        b = np.zeros(3, f32)
        b[c] = 1
        y0 = f32(b[0] * r[0])
        y1 = f32(f32(b[1] - f32(A[0, 1] * y0)) * r[1])
        y2 = f32(f32(f32(b[2] - f32(A[1, 2] * y1)) - f32(A[0, 2] * y0)) * r[2])
        z2 = y2
        z1 = fmaf(-A[2, 1], z2, y1)
        z0 = f32(y0 - fmaf(A[1, 0], z1, f32(A[2, 0] * z2)))
        z = [z0, z1, z2]
        for j in (2, 1, 0):
            if ip[j] != j:
                z[j], z[ip[j]] = z[ip[j]], z[j]
        X[:, c] = z
    return X


def inverse_intrinsics(K):
    """`torch.inverse(K[:, :3, :3])` of [[fx,0,cx],[0,fy,cy],[0,0,1]] (stereo/image_predictor.py:456).  The 3x3 is a STRIDED slice
    of the (N,4,4) intrinsics, so ATen copies it column-major and factors K itself, not its transpose: K is upper triangular, the
    LU is L = I, U = K without an interchange whatever the values, and sgetrs 'N' is a back substitution that DIVIDES by the
    diagonal: 1 / f on it, (0 - c) / f above it (c = 0 gives +0).  Until g12 this read -(c * (1 / f)), which is the same number
    for every isotropic, centred camera the suite had (c = (n - 1) / 2, f = 0.8 cols) and another for a quarter of all others."""
    o = np.zeros((3, 3), f32)
    o[0, 0], o[1, 1], o[2, 2] = f32(1) / K[0, 0], f32(1) / K[1, 1], 1
    o[0, 2], o[1, 2] = f32(f32(0) - K[0, 2]) / K[0, 0], f32(f32(0) - K[1, 2]) / K[1, 1]
    return o


def mm3(a, b):
    """ATen's small-matrix bmm: acc = 0, acc += a[i][k] * b[k][j], every operation rounded (no FMA)."""
    o = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            acc = f32(0)
            for k in range(3):
                acc = f32(acc + f32(a[i, k] * b[k, j]))
            o[i, j] = acc
    return o


ANISO, OFFCENTRE = {"fy_scale": 1.137}, {"dcx": 13.25, "dcy": -7.6}
CAMERAS = (ANISO, OFFCENTRE, {**ANISO, **OFFCENTRE}, {"fy_scale": 0.83, "dcx": -21.5, "dcy": 9.125})
RAGGED = ((131, 277), (250, 500), (60, 90))       # pyramids whose level scales differ in x and y


def poses(jitter, cameras=False):
    """Normalised poses and K pyramids of the synthetic batches; `cameras`: the same through cameras with fx != fy and
    off-centre principal points (all three changes) at the headline size, and through all of them at the ragged sizes."""
    forms = [(256, 512, None)] * 24
    if cameras:
        forms = [(256, 512, CAMERAS[n % 4]) for n in range(12)] + [RAGGED[n % 3] + (CAMERAS[n % 4],) for n in range(12)]
        forms += [size + (None,) for size in RAGGED]
    for seed, (rows, cols, camera) in enumerate(forms):
        S = (1, 2, 4)[seed % 3]
        batch = synthetic.make_batch(rows, cols, S, batch=1, seed=300 + seed, pose_jitter=jitter)
        if camera:
            synthetic.with_camera(batch, **camera)
        inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
        for Tt in inp["T_right_in_left"]:
            T = Tt.clone()
            T[:, :3, 3] = T[:, :3, 3] / T[:, :3, 3].pow(2).sum(1).sqrt()[:, None]
            yield T, inp["K_pyr"]


def test_lu_of_the_transposed_pose_matches_torch_bit_for_bit():
    n = bad = 0
    for jitter in (0.0, 0.5):
        for T, _ in poses(jitter):
            LU_t, piv_t = torch.linalg.lu_factor(T[0].t().contiguous())
            LU, ip = lu_of_transpose(T[0].numpy())
            n += 1
            bad += int((LU.view(np.int32) != LU_t.numpy().view(np.int32)).any() or [int(p) - 1 for p in piv_t] != ip)
    assert n >= 100 and bad == 0, (n, bad)


def test_inverse_of_the_pose_matches_torch_bit_for_bit():
    total = wrong = 0
    for jitter in (0.0, 0.5):
        for T, _ in poses(jitter):
            want = torch.linalg.inv(T)[0].numpy()
            assert np.array_equal(want, torch.inverse(T)[0].numpy())
            got = inverse_pose(T[0].numpy())
            total += 16
            wrong += int((got.view(np.int32) != want.view(np.int32)).sum())
    rng = np.random.default_rng(33)
    for _ in range(60):                                 # ... and of matrices with no structure at all
        M = rng.standard_normal((4, 4)).astype(f32)
        total += 16
        wrong += int((inverse_pose(M).view(np.int32) != torch.linalg.inv(torch.from_numpy(M)[None])[0].numpy().view(np.int32)).sum())
    print(f"entries of the 4x4 inverse equal bit for bit: {total - wrong} of {total}")
    assert wrong == 0, (wrong, total)


def test_intrinsics_inverse_matches_torch_bit_for_bit_for_any_pinhole_camera():
    """`inverse_intrinsics` against `torch.linalg.inv(K[:, :3, :3])` (the strided slice the reference inverts): random fx != fy and
    principal points of either sign or zero, batches of 1, 2 and 96 (the reference inverts D * B copies at once), and every
    pyramid level of the ragged sizes through every changed camera."""
    rng = np.random.default_rng(12)
    total = same = 0
    for n in range(3000):
        B = (1, 2, 96)[n % 3]
        K = torch.eye(4).repeat(B, 1, 1)
        K[:, 0, 0] = float(rng.uniform(0.5, 5000.0))
        K[:, 1, 1] = K[:, 0, 0] * (float(rng.uniform(0.5, 2.0)) if n % 4 else 1.0)
        K[:, 0, 2] = 0.0 if n % 50 == 0 else float(rng.uniform(-3000.0, 3000.0))
        K[:, 1, 2] = 0.0 if n % 70 == 0 else float(rng.uniform(-3000.0, 3000.0))
        want = torch.linalg.inv(K[:, :3, :3])[B - 1].numpy()
        assert np.array_equal(oracle.inv_intrinsics(K[:, :3, :3])[B - 1].numpy().view(np.int32), want.view(np.int32))
        total += 1
        same += int(np.array_equal(inverse_intrinsics(K[B - 1, :3, :3].numpy()).view(np.int32), want.view(np.int32)))
    for rows, cols in RAGGED:
        for camera in CAMERAS:
            batch = synthetic.with_camera(synthetic.make_batch(rows, cols, 1, batch=2, seed=1), **camera)
            K_pyr = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)["K_pyr"]
            sizes = [tuple(im.shape[-2:]) for im in snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)["left_image_pyr"]]
            assert any(r * cols != c * rows for r, c in sizes), sizes      # some level is scaled differently in x and y
            for K in K_pyr:
                want = torch.linalg.inv(K[:, :3, :3])[1].numpy()
                total += 1
                same += int(np.array_equal(inverse_intrinsics(K[1, :3, :3].numpy()).view(np.int32), want.view(np.int32)))
    print(f"intrinsics inverses equal bit for bit: {same} of {total}")
    assert same == total and total >= 3060


def test_intrinsics_inverse_and_homographies_match_the_oracle():
    total = exact = 0
    for jitter, cameras in ((0.0, False), (0.5, False), (0.0, True), (0.3, True)):
        for T, K_pyr in poses(jitter, cameras):
            Tl = inverse_pose(T[0].numpy())
            for lvl in (0, 4):
                K = K_pyr[lvl]
                K3 = K[0, :3, :3].numpy()
                Ki = inverse_intrinsics(K3)
                assert np.array_equal(Ki.view(np.int32), torch.linalg.inv(K[:, :3, :3])[0].numpy().view(np.int32))
                idepths = torch.tensor([[0.0, 0.37, 1.9]])
                want = oracle.plane_sweep_homographies(T, K, idepths)[0].numpy()
                for d, idp in enumerate(idepths[0].numpy()):
                    H = restated_homography(K3, Ki, Tl, idp)
                    total += 9
                    exact += int((H.view(np.int32) == want[d].view(np.int32)).sum())
    print(f"homography entries equal bit for bit: {exact} of {total}")
    assert exact == total


def test_inverse_3x3_and_incremental_homographies_match_torch_bit_for_bit():
    """`H_inc = torch.inverse(H[:, d-1].unsqueeze(1)) @ H[:, d]` (multi_view_stereonet.py:279-282) as the kernel forms it."""
    rng = np.random.default_rng(3)
    for _ in range(150):
        M = rng.standard_normal((3, 3)).astype(f32)
        assert np.array_equal(inverse3(M).view(np.int32), torch.linalg.inv(torch.from_numpy(M)[None])[0].numpy().view(np.int32))
    total = 0
    for jitter in (0.0, 0.5):
        for n, (T, K_pyr) in enumerate(poses(jitter)):
            if n % 3:
                continue
            s = oracle.idepth_samples(T, K_pyr[-1], 16, 32, 64)
            H = oracle.plane_sweep_homographies(T, K_pyr[-1], s)
            for d in range(1, 64, 7):
                inv_t = torch.inverse(H[:, d - 1].unsqueeze(1))
                inc_t = torch.matmul(inv_t, H[:, d].unsqueeze(1))[0, 0].numpy()
                inv_m = inverse3(H[0, d - 1].numpy())
                assert np.array_equal(inv_m.view(np.int32), inv_t[0, 0].numpy().view(np.int32))
                assert np.array_equal(mm3(inv_m, H[0, d].numpy()).view(np.int32), inc_t.view(np.int32))
                total += 1
    assert total >= 100


def test_reference_layout_keeps_the_plane_slice_contiguous_for_any_batch():
    """The reference's H family is a permuted (D,B,3,3) tensor (multi_view_stereonet.py:192), so `H[:, d-1]` is contiguous and
    takes ATen's transposed-LU shortcut whatever the batch size; a plain (B,D,3,3) tensor's slice is strided for B > 1 and
    takes the other route, which rounds differently -- the oracle therefore makes its slice contiguous first."""
    g = torch.Generator().manual_seed(5)
    H = torch.eye(3).repeat(2, 8, 1, 1) + 0.1 * torch.rand(2, 8, 3, 3, generator=g)
    ref_layout = H.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert ref_layout[:, 3].is_contiguous() and not H[:, 3].is_contiguous()
    per_image = torch.stack([torch.inverse(H[i:i + 1, 3])[0] for i in range(2)])
    assert torch.equal(torch.inverse(ref_layout[:, 3].unsqueeze(1))[:, 0], per_image)
    assert torch.equal(oracle.inv3x3(H[:, 3]), per_image)


def captured_cases(files=("g11_incremental_homographies.npz", "g12_camera_forms.npz")):
    """The homographies the REFERENCE handed its warper (captured by a hook in make_golden.py), with the inputs regenerated
    from the recorded seeds: g11 through make_batch's own camera, g12 through the K stored with each case (fx != fy,
    off-centre and half-pixel principal points, a K per batch element, pyramids whose level scales differ)."""
    from conftest import load_golden
    for name in files:
        fix = load_golden(name)
        for key in sorted(k for k in fix if k.endswith("_meta")):
            tag = key[:-5]
            rows, cols, D, S, B, seed, jit = (int(v) for v in fix[key])
            batch = synthetic.make_batch(rows, cols, S, batch=B, seed=seed, pose_jitter=jit / 100.0)
            if f"{tag}_K" in fix:
                batch["K"] = torch.from_numpy(fix[f"{tag}_K"]).clone()
            inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
            yield tag, fix, inp, D, S, B


def test_both_captures_are_read_and_g12_holds_the_camera_forms():
    tags = {tag: inp for tag, fix, inp, D, S, B in captured_cases()}
    assert len(tags) >= 7 + 12 and "headline" in tags and "ragged_131x277_cam" in tags
    K = tags["ragged_131x277_cam"]["K_pyr"]
    assert K[0][0, 0, 0] != K[0][0, 1, 1] and K[4][0, 0, 0] / K[0][0, 0, 0] != K[4][0, 1, 1] / K[0][0, 1, 1]
    assert not torch.equal(tags["b2_fy_below_fx"]["K_pyr"][0][0], tags["b2_fy_below_fx"]["K_pyr"][0][1])


def test_host_intrinsics_pyramid_equals_the_captured_reference_bit_for_bit():
    """`multi_view_unpack_batch` on the CPU against the K pyramid the reference's unpacker made of the same K (g12): every
    level, every batch element -- the level scales sx = cols_l / cols_0 and sy = rows_l / rows_0 differ at the ragged sizes,
    and the principal points are off-centre, so an x / y mix-up in the pyramid shows here."""
    total = same = 0
    for tag, fix, inp, D, S, B in captured_cases(("g12_camera_forms.npz",)):
        want = fix[f"{tag}_Kpyr"]
        assert want.shape == (5, B, 4, 4)
        for lvl in range(5):
            eq = inp["K_pyr"][lvl].numpy().view(np.int32) == want[lvl].view(np.int32)
            total += eq.size
            same += int(eq.sum())
    print(f"K pyramid entries equal bit for bit: {same} of {total}")
    assert same == total and total >= 12 * 5 * 16


def test_oracle_geometry_equals_the_captured_reference_bit_for_bit():
    """Same torch, same host as the generator: idepth samples, both homography families and every incremental homography of the
    oracle ARE the reference's, for batches of one and of two (the permuted layout, `inv3x3`)."""
    for tag, fix, inp, D, S, B in captured_cases():
        r4, c4 = inp["left_image_pyr"][4].shape[-2:]
        for s in range(S):
            T = inp["T_right_in_left"][s].clone()
            T[:, :3, 3] = T[:, :3, 3] / T[:, :3, 3].pow(2).sum(1).sqrt()[:, None]
            smp = oracle.idepth_samples(T, inp["K_pyr"][-1], r4, c4, D)
            assert np.array_equal(smp.numpy(), fix[f"{tag}_samples_{s}"]), (tag, s)
            H4 = oracle.plane_sweep_homographies(T, inp["K_pyr"][-1], smp)
            H0 = oracle.plane_sweep_homographies(T, inp["K_pyr"][0], smp[:, :1])
            assert np.array_equal(H4.numpy().view(np.int32), fix[f"{tag}_H4_{s}"].view(np.int32)), (tag, s)
            assert np.array_equal(H0.numpy().view(np.int32), fix[f"{tag}_H0_{s}"].view(np.int32)), (tag, s)
            inc = torch.stack([oracle.inv3x3(H4[:, d - 1]) @ H4[:, d].contiguous() for d in range(1, D)], 1)
            assert np.array_equal(inc.numpy().view(np.int32), fix[f"{tag}_Hinc_{s}"].view(np.int32)), (tag, s)


def own_baseline(T):
    """A chain's pose over its own baseline (multi_view_stereonet.py:566-571), every operation rounded."""
    T = T.copy()
    tx, ty, tz = T[0, 3], T[1, 3], T[2, 3]
    base = np.sqrt(f32(f32(f32(tx * tx) + f32(ty * ty)) + f32(tz * tz)))
    T[:3, 3] = (T[:3, 3] / f32(base)).astype(f32)
    return T


def restated_homography(K3, Ki, Tl, idepth):
    core = Tl[:3, :3].copy()
    core[:, 2] = (core[:, 2] + (Tl[:3, 3] * f32(idepth)).astype(f32)).astype(f32)
    return mm3(K3, mm3(core, Ki))


def test_restated_orders_reproduce_the_captured_incremental_homographies():
    """The numpy restatement (= csrc/mvsn_setup.hip, ref32) on the reference's own H family: every H_inc entry, bit for bit --
    host-independent from here on (the fixture is data).  And the families themselves, H0 and H4, restated from the captured
    pose, the captured samples and the K pyramid: every entry of every case, g12's cameras included."""
    total = 0
    for tag, fix, inp, D, S, B in captured_cases():
        for s in range(S):
            H4, want = fix[f"{tag}_H4_{s}"], fix[f"{tag}_Hinc_{s}"]
            for b in range(B):
                for d in range(1, D, 5 if D > 16 else 1):
                    got = mm3(inverse3(H4[b, d - 1]), H4[b, d])
                    assert np.array_equal(got.view(np.int32), want[b, d - 1].view(np.int32)), (tag, s, b, d)
                    total += 1
    assert total >= 150
    entries = same = 0
    for tag, fix, inp, D, S, B in captured_cases():
        case = [0, 0]
        for s in range(S):
            for b in range(B):
                Tl = inverse_pose(own_baseline(fix[f"{tag}_T_{s}"][b]))
                K0, K4 = (inp["K_pyr"][lvl][b, :3, :3].numpy() for lvl in (0, 4))
                smp = fix[f"{tag}_samples_{s}"][b]
                H0 = restated_homography(K0, inverse_intrinsics(K0), Tl, smp[0])
                eq = [H0.view(np.int32) == fix[f"{tag}_H0_{s}"][b, 0].view(np.int32)]
                K4i = inverse_intrinsics(K4)
                for d in range(D):
                    eq.append(restated_homography(K4, K4i, Tl, smp[d]).view(np.int32) == fix[f"{tag}_H4_{s}"][b, d].view(np.int32))
                case[0] += int(np.sum(eq))
                case[1] += 9 * len(eq)
        print(f"{tag}: restated H0 / H4 entries equal to the capture bit for bit: {case[0]} of {case[1]}")
        same, entries = same + case[0], entries + case[1]
    assert same == entries, (same, entries)


# ---- the idepth samples (the maximum idepth is a mean over the level-4 pixels of an fp32 tensor program) ----------------------

def torch_sum_row(x, V=8):
    """torch.sum over a contiguous row of floats (ATen SumKernel.cpp: `vectorized_inner_sum` / `row_sum` / `multi_row_sum`): V-float
    vectors, four of them in flight, a four-level cascade that folds level j - 1 into level j every 16^j steps; then the vectors
    beyond the rounds of four, the four accumulators, the scalar tail, and the V partial sums one by one.  V = 8: the kernel is
    built for 8-float vectors also where torch reports AVX-512."""
    x = x.astype(f32)
    P = x.size
    nvec = P // V
    vecs = x[:nvec * V].reshape(nvec, V)
    rounds = nvec // 4
    acc = np.zeros((4, 4, V), f32)
    i = 0
    while i + 16 <= rounds:
        for _ in range(16):
            for k in range(4):
                acc[0, k] = (acc[0, k] + vecs[i * 4 + k]).astype(f32)
            i += 1
        for j in range(1, 4):
            acc[j] = (acc[j] + acc[j - 1]).astype(f32)
            acc[j - 1] = 0
            if i & (15 << (4 * j)):
                break
    while i < rounds:
        for k in range(4):
            acc[0, k] = (acc[0, k] + vecs[i * 4 + k]).astype(f32)
        i += 1
    for j in range(1, 4):
        acc[0] = (acc[0] + acc[j]).astype(f32)
    part = acc[0]
    for v in range(rounds * 4, nvec):
        part[0] = (part[0] + vecs[v]).astype(f32)
    for k in range(1, 4):
        part[0] = (part[0] + part[k]).astype(f32)
    total = f32(0)
    for p in range(nvec * V, P):
        total = f32(total + x[p])
    for k in range(V):
        total = f32(total + part[0][k])
    return total


def mm_naive(a, b):
    """ATen's small-matrix product for any shape: acc = 0, acc += a[i][k] * b[k][j], every operation rounded."""
    o = np.zeros((a.shape[0], b.shape[1]), f32)
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            acc = f32(0)
            for k in range(a.shape[1]):
                acc = f32(acc + f32(a[i, k] * b[k, j]))
            o[i, j] = acc
    return o


def vfma(a, b, c):
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def matmul_3xP(M, X):
    """`matmul(KRKinv, xyz_pix)`: MKL's sgemm -- a product and two fused multiply-adds in the order k = 0, 1, 2 -- unless
    3 * 3 * P < 400, where ATen's own loop runs (no fused operation)."""
    out = []
    for i in range(3):
        if 9 * X.shape[1] < 400:
            acc = ((M[i, 0] * X[0]).astype(f32) + (M[i, 1] * X[1]).astype(f32)).astype(f32)
            acc = (acc + (M[i, 2] * X[2]).astype(f32)).astype(f32)
        else:
            acc = vfma(M[i, 2], X[2], vfma(M[i, 1], X[1], (M[i, 0] * X[0]).astype(f32)))
        out.append(acc)
    return np.stack(out)


def idepth_samples_restated(T, K, rows, cols, D):
    """create_idepth_samples / disparity_to_idepth (multi_view_stereonet.py:131-165, stereo/image_predictor.py:120-209) operation
    by operation -- what csrc/mvsn_setup.hip (ref32::max_idepth_pixel and the sum after it) implements.  T: the pose already
    normalised by its own baseline."""
    P = rows * cols
    xs, ys = np.tile(np.arange(cols, dtype=f32), rows), np.repeat(np.arange(rows, dtype=f32), cols)
    grid = np.stack([xs, ys, np.ones(P, f32)])
    Kinv, Tlr = inverse_pose(K), inverse_pose(T)
    M = mm_naive(K[:3, :3], mm_naive(Tlr[:3, :3], Kinv[:3, :3]))
    Kt = mm_naive(K, Tlr)[:3, 3]
    inf = matmul_3xP(M, grid)
    infx, infy = (inf[0] / inf[2]).astype(f32), (inf[1] / inf[2]).astype(f32)
    far = (matmul_3xP(M, (grid * f32(1e2)).astype(f32)) + Kt[:, None]).astype(f32)
    farx, fary = (far[0] / far[2]).astype(f32), (far[1] / far[2]).astype(f32)
    dx, dy = (farx - infx).astype(f32), (fary - infy).astype(f32)
    norm = np.sqrt(((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)).astype(f32)
    den = (norm + f32(1e-6)).astype(f32)
    lx, ly = (dx / den).astype(f32), (dy / den).astype(f32)
    wz = (((M[2, 0] * grid[0]).astype(f32) + (M[2, 1] * grid[1]).astype(f32)).astype(f32) + M[2, 2]).astype(f32)
    disp = f32(D - 1)
    A0 = (Kt[0] - (Kt[2] * (infx + (disp * lx).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    A1 = (Kt[1] - (Kt[2] * (infy + (disp * ly).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    wd = (wz * disp).astype(f32)
    b0, b1 = (wd * lx).astype(f32), (wd * ly).astype(f32)
    num = ((A0 * b0).astype(f32) + (A1 * b1).astype(f32)).astype(f32)
    dd = ((A0 * A0).astype(f32) + (A1 * A1).astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        idp = (num / dd).astype(f32)
    idp = ((norm >= f32(1e-6)).astype(f32) * idp).astype(f32)
    m = ((idp > 0).astype(f32) * idp).astype(f32)
    top = f32(torch_sum_row(m) / f32((m > 0).sum()))
    top = f32(2.0) if top > f32(2.0) else top
    if f32(f32(1.0) / top) < T[2, 3]:
        top = f32(f32(1.0) / T[2, 3])
    return (np.arange(D, dtype=f32) * f32(top / f32(D - 1))).astype(f32)


def test_row_sum_order_matches_torch():
    rng = np.random.default_rng(0)
    for P in (8, 9, 30, 45, 300, 512, 1200, 2048, 8200):          # (rows shorter than one vector take another ATen path)
        for _ in range(12):
            x = rng.random(P).astype(f32) * f32(2.0)
            x[rng.random(P) < 0.3] = 0
            want = torch.sum(torch.from_numpy(x)[None], 1)[0].numpy()
            assert torch_sum_row(x).view(np.int32) == want.view(np.int32), P


def test_restated_idepth_samples_match_the_oracle_and_the_captured_reference():
    """Against the captured reference (g11, host-independent data): every chain.  Against the oracle on this host: torch's vectorised
    sqrt is an ulp off the correctly rounded root for ~0.7 % of its arguments, which the restatement does not follow -- the mean
    over the pixels absorbs it (204 of 204 chains when this was written); a chain or two may differ on another host."""
    for tag, fix, inp, D, S, B in captured_cases():
        r4, c4 = inp["left_image_pyr"][4].shape[-2:]
        for s in range(S):
            for b in range(B):
                T = own_baseline(fix[f"{tag}_T_{s}"][b])
                got = idepth_samples_restated(T, inp["K_pyr"][-1][b].numpy(), r4, c4, D)
                assert np.array_equal(got.view(np.int32), fix[f"{tag}_samples_{s}"][b].view(np.int32)), (tag, s, b)
    total = same = 0
    for rows, cols, D in ((256, 512, 64), (480, 640, 96), (80, 96, 8), (240, 320, 48)):
        for seed in range(4):
            batch = synthetic.make_batch(rows, cols, (1, 2, 4)[seed % 3], batch=1, seed=1200 + seed, pose_jitter=0.4 * (seed % 2))
            inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
            r4, c4 = inp["left_image_pyr"][4].shape[-2:]
            for Tt in inp["T_right_in_left"]:
                T = Tt.clone()
                T[:, :3, 3] = T[:, :3, 3] / T[:, :3, 3].pow(2).sum(1).sqrt()[:, None]
                want = oracle.idepth_samples(T, inp["K_pyr"][-1], r4, c4, D)[0].numpy()
                got = idepth_samples_restated(T[0].numpy(), inp["K_pyr"][-1][0].numpy(), r4, c4, D)
                total += 1
                same += int(np.array_equal(got.view(np.int32), want.view(np.int32)))
    print(f"idepth samples equal bit for bit: {same} of {total} chains")
    assert same >= 0.9 * total
