"""Source poses in general position, and a float64 evaluation from first principles of what the kernels that consume a
pose emit: mvsn_plane_sweep_setup (csrc/mvsn_setup.hip), mvsn_prepare_cameras (csrc/mvsn_prepare.hip) and, through
tests/test_hip_parity.py's `_project_f64`, mvsn_idepth_reproject (csrc/mvsn_consistency.hip).

Every other pose of the suite is synthetic.make_batch's: a rotation of 0.03 .. 0.15 rad about y and a baseline almost
along x.  With those the pivoted LU the kernels mirror (ref32::inverse_pose, ref32::inverse3, the Gauss-Jordan of the
unpacker, inverse4x4 of the reprojection) takes the diagonal as its pivot in almost every column, every level-4 pixel has
a positive idepth, and no epipole lies inside the image.  The families below reach the other branches; what each one
reaches is asserted on the CPU in tests/test_pose_reference_cpu.py, and the GPU tests of tests/test_setup_poses_gpu.py
run on the same inputs.

Written from the operations, not from the kernels, in float64.  The only float32 quantities are the inputs: a pose's
sixteen entries and the K pyramid, exactly as the kernels receive them.  The two masks of the idepth-sample reduction are
PRODUCTS, as in the reference (`(~degenerate).float() * idepth`, `(m > 0).float() * m`): a 0 / 0 stays a NaN.

The `1 / top < tz` clamp ("keep samples in front of the source camera") needs a mean above 1 / tz >= 1: motion that is
mostly forward AND enough disparity for the mean to grow.  None of the nine families of the first table reaches it at the
D of their shapes (under forward motion the raw mean stays below 1 / tz: 0.965 against 1.0018 at D 64).  A search in
float64 over those families with tz set to 0.3 .. 0.99 of the baseline, a yaw of +-0.3, the grids below and D up to 128
found it for the yaw of -0.3 with tz at 0.6 .. 0.8 of the baseline on the smaller grids from D 16 on (top * tz up to
1.39 at D 128; 125 of the 3465 combinations tried reach it, that yaw foremost).  The family `dive` is that
pose, and CLAMP_CASES its launches: top * tz = 1.09 .. 1.21 at D 32, neither within 1 % of the predicate nor capped.
"""
import math

import numpy as np
import torch

from multi_view_stereonet_amd import synthetic

# ---- the families ------------------------------------------------------------------------------------------------
# name: (rotations multiplied left to right, translation before normalisation).  rot(axis, a) is right-handed; about y it
# is what make_batch writes: T[0,2] = sin, T[2,0] = -sin.
FAMILIES = {
    "roll50": ((("z", 0.9),), (0.5, 0.05, 0.02)),
    "roll-120": ((("z", -2.1),), (0.4, -0.1, 0.03)),
    "yaw60": ((("y", 1.05),), (0.8, 0.0, 0.3)),
    "general": ((("x", 0.4), ("y", -0.7), ("z", 1.2)), (-0.2, 0.35, 0.3)),
    "diag": ((("x", 0.1), ("y", -0.2), ("z", 0.3)), (0.3, -0.3, 0.25)),
    "vertical": ((("x", 0.05),), (0.02, 0.5, 0.03)),
    "forward": ((("y", 0.02), ("x", 0.01)), (0.03, 0.02, 0.6)),
    "backward": ((("y", -0.02),), (0.03, -0.02, -0.6)),
    "pure_forward": ((), (0.0, 0.0, 0.5)),
    "dive": ((("y", -0.3),), (0.357, 0.0357, 0.35)),        # tz = 0.698: the clamp, from D 16 on the small grids
}
# the columns of the LU of the transposed, normalised pose in which a row interchange happens
INTERCHANGES = {"roll50": [0, 1], "roll-120": [0, 1], "yaw60": [0, 2], "general": [0], "diag": [], "vertical": [],
                "forward": [], "backward": [], "pure_forward": [], "dive": []}
# the families whose samples are finite at every shape used; in this order they are mixed into one launch
FINITE = ("roll50", "diag", "yaw60", "vertical", "roll-120", "forward", "general")

# ---- shapes of the set-up tests: (image rows, image cols, D); the level-4 grid is rows / 16 x cols / 16 ---------------
SETUP_SHAPES = ((64, 128, 8), (96, 160, 12), (256, 512, 16), (48, 80, 8))
SMALL_SHAPE = (16, 80, 8)             # a 1 x 5 level-4 grid, under 8 pixels: the samples from the fp64 evaluation
SHEAR = 0.3
SHEAR_SHAPES = ((64, 128, 8), (48, 80, 8))
# (family of chain (0, 0), shape, shear, path): a launch of S = 2 x B = 2 chains, the other three as `mixed` says
SETUP_CASES = tuple([(f, shape, 0.0, 3) for shape in SETUP_SHAPES for f in FINITE] + [("backward", (256, 512, 16), 0.0, 3)]
                    + [(f, SMALL_SHAPE, 0.0, 1) for f in FINITE] + [(f, shape, SHEAR, 0) for shape in SHEAR_SHAPES for f in FINITE])
# launches whose chain (0, 0) has NaN samples: no positive pixel / the pixel on the epipole is 0 / 0.  The last two take
# the fp64 evaluation for their samples (under 8 pixels; a shear term)
NAN_CASES = (("backward", (64, 128, 8), 0.0, 3), ("pure_forward", (48, 80, 8), 0.0, 3),
             ("pure_forward", SMALL_SHAPE, 0.0, 1), ("pure_forward", (48, 80, 8), SHEAR, 0))
# positive pixels strictly between 0 and P, and the cap: (family, shape, positive pixels, capped)
PARTIAL_CASES = (("yaw60", (256, 512, 16), 496, False), ("yaw60", (96, 160, 12), 54, False),
                 ("backward", (256, 512, 16), 58, True))
# launches whose chain (0, 0) reaches `1 / top < tz`, on each path
CLAMP_CASES = (("dive", (48, 80, 32), 0.0, 3), ("dive", (64, 128, 32), 0.0, 3), ("dive", SMALL_SHAPE[:2] + (32,), 0.0, 1),
               ("dive", (64, 128, 32), SHEAR, 0))


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64),
            "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)}[axis]


def pose(name):
    """T_right_in_left (4,4) float32 of a family: the rotation formed in float64 and rounded once."""
    rots, t = FAMILIES[name]
    R = np.eye(3)
    for axis, a in rots:
        R = R @ rot(axis, a)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return torch.from_numpy(T.astype(np.float32))


def mixed(name, S, B):
    """Family names [s][b] of a launch on `name`: chain (0, 0) is the family itself, every other chain (s, b) takes the
    family s + 2 b places further along FINITE -- with S = 2 the second source is another family, so one launch mixes
    pivoting and non-pivoting chains, and with B = 2 the second element takes two more.  A family whose samples can be NaN
    stands alone: its neighbours are counted from the start of FINITE."""
    at = FINITE.index(name) if name in FINITE else -1
    return [[name if s == 0 and b == 0 else FINITE[(at + s + 2 * b) % len(FINITE)] for b in range(B)] for s in range(S)]


def with_poses(batch, names):
    """Replace T_right_in_left of a make_batch batch IN PLACE (and return the batch): source s of element b takes the
    pose of family names[s][b]."""
    for s, Tb in enumerate(batch["T_right_in_left"]):
        for b in range(Tb.shape[0]):
            Tb[b, 0] = pose(names[s][b])
    return batch


def chain_inputs(rows, cols, names, shear=0.0):
    """What a set-up launch takes for the chains n = s * B + b of `names`: the raw poses (N,4,4) -- the kernel divides
    each by its own baseline --, the level-0 and level-4 intrinsics of make_batch's camera (B,4,4) with `shear` written
    into K[0,1] of both, and the level-4 grid."""
    from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
    S, B = len(names), len(names[0])
    batch = with_poses(synthetic.make_batch(rows, cols, S, batch=B, seed=3), names)
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    r4, c4 = inp["left_image_pyr"][4].shape[-2:]
    K0, K4 = inp["K_pyr"][0].clone(), inp["K_pyr"][4].clone()
    K0[:, 0, 1] = shear
    K4[:, 0, 1] = shear
    Ts = [Tb[:, 0].clone() for Tb in batch["T_right_in_left"]]
    return Ts, K0, K4, int(r4), int(c4)


# ---- float64 from first principles -------------------------------------------------------------------------------
def normalised_pose64(T, baseline=None):
    """The pose over a baseline (its own when none is given) and the inverse of that, float64."""
    T = np.asarray(T, np.float64)
    base = float(np.sqrt((T[:3, 3] ** 2).sum())) if baseline is None else float(baseline)
    Tn = T.copy()
    Tn[:3, 3] = T[:3, 3] / base
    return base, Tn, np.linalg.inv(Tn)


def homography64(K, Tl, idepth):
    """K (R + t idepth e3^T) K^-1 with (R, t) of the inverted pose."""
    K3 = np.asarray(K, np.float64)[:3, :3]
    core = Tl[:3, :3].copy()
    core[:, 2] = core[:, 2] + Tl[:3, 3] * idepth
    return K3 @ core @ np.linalg.inv(K3)


def max_idepth64(K4, Tl, rows4, cols4, D):
    """Per level-4 pixel, the idepth that moves it D - 1 px along its epipolar line (the operation of
    stereo/image_predictor.py:120-209): `idepth` before either mask, `norm` of the epipolar direction, and `m`, the
    value that enters the mean."""
    K = np.asarray(K4, np.float64)
    xs, ys = np.tile(np.arange(cols4, dtype=np.float64), rows4), np.repeat(np.arange(rows4, dtype=np.float64), cols4)
    grid = np.stack([xs, ys, np.ones_like(xs)])
    M = K[:3, :3] @ Tl[:3, :3] @ np.linalg.inv(K)[:3, :3]
    Kt = (K @ Tl)[:3, 3]
    disp = float(D - 1)
    with np.errstate(all="ignore"):
        inf = M @ grid
        inf_xy = inf[:2] / inf[2]
        far = M @ (grid * 1e2) + Kt[:, None]
        diff = far[:2] / far[2] - inf_xy
        norm = np.sqrt((diff ** 2).sum(0))
        line = diff / (norm + 1e-6)
        A = Kt[:2, None] - Kt[2] * (inf_xy + disp * line)
        b = inf[2] * disp * line
        idepth = (A * b).sum(0) / (A * A).sum(0)
        masked = (norm >= 1e-6).astype(np.float64) * idepth
        m = (masked > 0).astype(np.float64) * masked
    return idepth, norm, m


def setup64(T, K0, K4, rows4, cols4, D):
    """Everything mvsn_plane_sweep_setup emits for one chain, and what decides it: `baseline`, `samples` (D), `H0` (3,3),
    `H4` (D,3,3); `idepth`, `norm`, `m` per pixel; `count` of positive pixels, the `raw` mean before cap and clamp,
    `tz` of the normalised pose, and which of `capped`, `clamped`, `nan` applied."""
    base, Tn, Tl = normalised_pose64(T)
    idepth, norm, m = max_idepth64(K4, Tl, rows4, cols4, D)
    count = int((m > 0).sum())
    with np.errstate(all="ignore"):
        raw = float(m.sum() / np.float64(count))
        top = raw
        capped = bool(top > 2.0)
        top = 2.0 if capped else top
        tz = float(Tn[2, 3])
        clamped = bool(1.0 / top < tz)
        top = 1.0 / tz if clamped else top
        samples = np.arange(D, dtype=np.float64) * (top / (D - 1))
    return {"baseline": base, "Tn": Tn, "Tl": Tl, "samples": samples, "H0": homography64(K0, Tl, 0.0),
            "H4": np.stack([homography64(K4, Tl, s) for s in samples]), "idepth": idepth, "norm": norm, "m": m,
            "count": count, "raw": raw, "tz": tz, "capped": capped, "clamped": clamped, "nan": bool(np.isnan(raw))}


def setup64_chains(Ts, K0, K4, rows4, cols4, D):
    """setup64 of the chains n = s * B + b of per-source poses Ts [S x (B,4,4)] and the batch's intrinsics (B,4,4)."""
    B = K0.shape[0]
    return [setup64(Ts[s][b].numpy(), K0[b].numpy(), K4[b].numpy(), rows4, cols4, D) for s in range(len(Ts)) for b in range(B)]


def unpacked64(batch):
    """What multi_view_unpack_batch makes of a batch's poses, float64: per source (B,4,4) the pose and its inverse with
    both translations over the baseline to the FIRST source, and that baseline (B)."""
    Ts = [Tb[:, 0].numpy().astype(np.float64) for Tb in batch["T_right_in_left"]]
    base = np.sqrt((Ts[0][:, :3, 3] ** 2).sum(1))
    Tn, Ti = [], []
    for T in Ts:
        a, b = T.copy(), np.linalg.inv(T)
        a[:, :3, 3] /= base[:, None]
        b[:, :3, 3] /= base[:, None]
        Tn.append(a)
        Ti.append(b)
    return Tn, Ti, base


def ulp32(x):
    """The spacing of float32 at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- reprojection ------------------------------------------------------------------------------------------------
PROJECTION_FAMILIES = ("roll50", "diag", "vertical", "forward")
PROJECTION_SIZES = ((37, 53), (96, 160))


def projection_inputs(rows, cols):
    """K, the unpacked pose of each PROJECTION_FAMILIES member and the idepth maps of
    test_two_view_projection_and_occlusion_through_changed_cameras at level 0, batch of two: element 0 takes the family,
    element 1 the next one."""
    from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
    out = []
    for i, name in enumerate(PROJECTION_FAMILIES):
        names = [[name, PROJECTION_FAMILIES[(i + 1) % len(PROJECTION_FAMILIES)]]]
        batch = with_poses(synthetic.make_batch(rows, cols, 1, batch=2, seed=13), names)
        inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
        gen = torch.Generator().manual_seed(99)
        L = 0.06 + 0.04 * synthetic._smooth_image(gen, 2, rows, cols)[:, :1]
        R = 0.06 + 0.04 * synthetic._smooth_image(gen, 2, rows, cols)[:, :1]
        R[:, :, : rows // 3] += 0.05                                          # a nearer band: real occlusions
        out.append((name, inp["K_pyr"][0], inp["T_right_in_left"][0], L, R))
    return out


# ---- the oracle and the numpy restatement of the reference's fp32 order, per chain ------------------------------------
def oracle_chains(Ts, K0, K4, rows4, cols4, D):
    """The oracle (torch on the CPU, the reference's own fp32 ops) on the chains n = s * B + b: samples (N,D), H4
    (N,D,3,3), H0 (N,3,3), H_inc (N,D-1,3,3), baseline (N), all float32 tensors."""
    from oracle import mvsn_oracle as oracle
    S = len(Ts)
    Tn = torch.cat(Ts, 0).clone()
    base = Tn[:, :3, 3].pow(2).sum(1).sqrt()
    Tn[:, :3, 3] /= base[:, None]
    K0r, K4r = K0.repeat(S, 1, 1), K4.repeat(S, 1, 1)
    smp = oracle.idepth_samples(Tn, K4r, rows4, cols4, D)
    H4 = oracle.plane_sweep_homographies(Tn, K4r, smp)
    H0 = oracle.plane_sweep_homographies(Tn, K0r, torch.zeros_like(smp[:, :1]))[:, 0]       # plane 0: idepth 0
    inc = torch.stack([oracle.inv3x3(H4[:, d - 1]) @ H4[:, d].contiguous() for d in range(1, D)], 1)
    return smp, H4, H0, inc, base


def restated_chain(T, K0, K4, rows4, cols4, D, samples=None):
    """tests/test_reference_geometry_cpu.py's numpy restatement of the reference's fp32 order -- what the kernel's
    namespace ref32 implements -- for one chain: samples (idepth_samples_restated), and H0, H4 and H_inc
    (restated_homography; inverse3 followed by mm3) evaluated at `samples` (the restated ones when none are given)."""
    import test_reference_geometry_cpu as rg
    T, K0, K4 = (np.ascontiguousarray(np.asarray(x, np.float32)) for x in (T, K0, K4))
    with np.errstate(all="ignore"):
        Tn = rg.own_baseline(T)
        own = rg.idepth_samples_restated(Tn, K4, rows4, cols4, D)
        smp = own if samples is None else np.asarray(samples, np.float32)
        Tl = rg.inverse_pose(Tn)
        K03, K43 = K0[:3, :3].copy(), K4[:3, :3].copy()
        H0 = rg.restated_homography(K03, rg.inverse_intrinsics(K03), Tl, np.float32(0))
        K4i = rg.inverse_intrinsics(K43)
        H4 = np.stack([rg.restated_homography(K43, K4i, Tl, s) for s in smp])
        inc = np.stack([rg.mm3(rg.inverse3(H4[d - 1]), H4[d]) for d in range(1, D)])
    return own, H0, H4, inc


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN whatever its payload."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def within(got, want, rtol, atol):
    """|got - want| <= atol + rtol |want| in every entry (float64), as torch.allclose; and the worst entry over it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    frac = np.abs(got - want) / (atol + rtol * np.abs(want))
    return bool((frac <= 1.0).all()), float(frac.max())


# the tolerances of test_hip_parity.py's _plane_sweep_setup_case: (rtol, atol)
TOL = {"baseline": (1e-6, 0.0), "samples": (2e-5, 1e-7), "H4": (1e-4, 2e-5), "H0": (1e-4, 1e-4), "Hinc": (1e-5, 1e-6)}
# families left out of the H_inc line against float64 (and of no other): the reference's own fp32 `inverse(H[d-1]) @ H[d]`
# misses that line's tolerance on them -- general at 16x32, D 16: 1.14 of it (tests/test_pose_reference_cpu.py)
HINC_DROPPED = ("general",)
RATIO_LIMIT = 4.0       # a kernel's error over the oracle's, both against float64: fp32 chains of the same length


def error_ratios(got_s, got_H4, ora_s, ora_H4, f64):
    """(samples, H4): the error of `got` against float64 over the oracle's, per chain.  Samples relative to the largest
    sample, H4 per matrix relative to its largest entry and then the worst matrix of the chain; under the oracle's error
    a floor of one float32 ulp of that largest entry, so that an oracle that happens to be exact divides by something."""
    s64, H64 = f64["samples"], f64["H4"]
    top = np.abs(s64).max()
    floor_s = float(ulp32(top)) / top
    rs = (np.abs(np.asarray(got_s, np.float64) - s64).max() / top) / max(np.abs(np.asarray(ora_s, np.float64) - s64).max() / top, floor_s)
    big = np.abs(H64).reshape(len(H64), -1).max(1)
    err = lambda H: (np.abs(np.asarray(H, np.float64) - H64).reshape(len(H64), -1).max(1) / big).max()      # noqa: E731
    rh = err(got_H4) / max(err(ora_H4), float((ulp32(big) / big).max()))
    return float(rs), float(rh)
