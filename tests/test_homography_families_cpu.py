"""CPU side of the general-homography tests of tests/test_hip_parity.py: the INPUTS those GPU tests use are what their
docstrings say they are, so that a failure on the GPU cannot be blamed on them.  Families, case tables, the float64
restatement of the warp and the mask rule are the GPU tests' own (imported, not copied)."""
import pytest
import torch

import test_hip_parity as hp
from oracle import mvsn_oracle as oracle

torch.set_grad_enabled(False)
CHAIN_CASES = hp.GENERAL_CHAIN_CASES
GRIDS = ((16, 32), (30, 40), (32, 64))


def _u2(H, rows, cols):
    """u2 at every pixel centre, in float64 and as an fp32 evaluation (either association)."""
    u64 = hp._coords_f64(H, rows, cols)[0]
    ys, xs = torch.meshgrid(torch.arange(rows, dtype=torch.float32), torch.arange(cols, dtype=torch.float32), indexing="ij")
    e = lambda j: H[..., 2, j, None, None]
    return u64, (e(0) * xs + e(1) * ys) + e(2), e(0) * xs + (e(1) * ys + e(2))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind", hp.GENERAL_KINDS)
def test_families_are_what_they_claim(kind, grid):
    rows, cols = grid
    N, D = 2, 8
    H, Hinc = hp._motion_family(N, D, kind, 3, grid)
    assert H.dtype == torch.float32 and Hinc.dtype == torch.float32
    H2, Hinc2 = hp._motion_family(N, D, kind, 3, grid)
    assert torch.equal(H, H2) and torch.equal(Hinc, Hinc2)                       # seeded
    assert torch.equal(Hinc[:, 0], torch.eye(3).expand(N, 3, 3)) and torch.equal(H[:, 0], Hinc[:, 0])
    prod = H[:, :-1].double() @ Hinc[:, 1:].double()                              # H is the running product (rounded once)
    assert float(((prod - H[:, 1:].double()).abs() / H[:, 1:].double().abs().amax((2, 3), keepdim=True)).max()) < 1e-5
    for fam in (H, Hinc):                                                          # u2 is never 0: no NaN coordinate
        for u in _u2(fam, rows, cols):
            assert float(u.abs().min()) > 0
        _, nx, ny, _ = hp._coords_f64(fam, rows, cols)
        assert bool(torch.isfinite(nx).all() and torch.isfinite(ny).all())
    u2H, u2I = hp._coords_f64(H, rows, cols)[0], hp._coords_f64(Hinc, rows, cols)[0]
    outside = hp._coords_f64(H, rows, cols)[3].float().mean((2, 3))               # (N, D)
    ys = torch.arange(rows, dtype=torch.float64)[:, None]
    iy = ((hp._coords_f64(Hinc, rows, cols)[2] + 1.0) * rows - 1.0) / 2.0        # source row of the incremental gather
    if kind == "roll":       # ~4 rows at the edges (opposite signs), sub-row in the middle, on the planes d % 3 == 1
        dy = (iy - ys)[:, 1]
        assert float(dy[:, :, 0].abs().mean()) > 3.3 and float(dy[:, :, -1].abs().mean()) > 3.3
        assert bool((dy[:, :, 0].mean(1) * dy[:, :, -1].mean(1) < 0).all())
        assert float(dy[:, :, cols // 2 - 1:cols // 2 + 1].abs().max()) < 1.0
    if kind == "zoom":       # the cumulative scale reaches ~0.3x on even chains and ~3x on odd ones
        s = H[:, -1, 0, 0] / H[:, -1, 2, 2]
        assert 0.15 < float(s[0]) < 0.45 and 2.0 < float(s[1]) < 5.0
    if kind == "tilt":       # u2 > 0 everywhere; every Hinc and every other H spans 0.4 .. 2.5 (relative to its centre)
        assert float(u2H.min()) > 0 and float(u2I.min()) > 0
        span = u2I[:, 1:].amax((2, 3)) / u2I[:, 1:].amin((2, 3))
        assert float(span.min()) > 6.0
        assert float((u2H[:, 1::2].amax((2, 3)) / u2H[:, 1::2].amin((2, 3))).min()) > 4.0
        assert float(u2I[:, 1:].amin((2, 3)).max()) < 0.41 and float(u2I[:, 1:].amax((2, 3)).min()) > 2.49
    if kind in ("behind", "general"):   # u2 changes sign inside the image on some planes; some voxels behind stay unmasked
        flips = (u2H.amin((2, 3)) < 0) & (u2H.amax((2, 3)) > 0)
        assert bool(flips.any())
        unmasked_behind = (u2H < 0) & ~hp._coords_f64(H, rows, cols)[3]
        assert kind == "general" or bool(unmasked_behind.any())
    if kind == "gone":       # a whole plane outside, its neighbours partly inside
        gone = (outside == 1.0).nonzero().tolist()
        assert gone
        for n, d in gone:
            assert 0.0 < float(outside[n, d - 1]) < 1.0 and 0.0 < float(outside[n, d + 1]) < 1.0
    if kind == "general":
        assert bool(((outside > 0.0) & (outside < 1.0)).any())


@pytest.mark.parametrize("kind,N,D,grid,seed", CHAIN_CASES)
def test_chain_case_masks_leave_the_fp32_oracle_within_the_cap(kind, N, D, grid, seed):
    """The condition test_chain_forms_on_general_homographies puts on its inputs: the fp32 oracle's mask against the
    float64 predicate, on exactly the GPU test's homographies, obeys the near-predicate rule and the cap -- for H (the
    mask the chain stores) and for Hinc (the mask inside the feature gather)."""
    _, H, Hinc, _, _ = hp._general_chain_inputs(kind, N, D, grid, seed)
    rows, cols = grid
    for name, fam in (("H", H), ("Hinc", Hinc)):
        _, _, m32 = oracle.warp_coordinates(fam.reshape(-1, 3, 3), rows, cols)
        m64 = hp._coords_f64(fam, rows, cols)[3]
        hp._mask_rule(m32.reshape(m64.shape), m64, fam, f"oracle {kind} {rows}x{cols} N={N} D={D} {name}")


@pytest.mark.parametrize("B,C,n,rows,cols", hp.WARP_GENERAL_SHAPES)
@pytest.mark.parametrize("kind", hp.GENERAL_KINDS)
def test_warp_case_masks_leave_the_fp32_oracle_within_the_cap(kind, B, C, n, rows, cols):
    """Likewise for test_homography_warp_on_general_homographies' inputs (masks only: the big frames stay cheap)."""
    H = hp._family_H(kind, B, n, rows, cols)
    _, _, m32 = oracle.warp_coordinates(H.reshape(-1, 3, 3), rows, cols)
    m64 = hp._coords_f64(H, rows, cols)[3]
    hp._mask_rule(m32.reshape(m64.shape), m64, H, f"oracle {kind} {B}x{n}x{rows}x{cols}")
    assert bool(torch.isfinite(hp._coords_f64(H, rows, cols)[1]).all())


@pytest.mark.parametrize("kind,N,D,grid,seed", [c for c in CHAIN_CASES if c[0] in hp.BOTH_PATHS_KINDS])
def test_roll_and_general_put_bands_of_one_plane_on_both_gather_paths(kind, N, D, grid, seed):
    """The GPU test's own assertion on its own inputs: any split for roll, a split between INTERIOR bands for general."""
    _, _, Hinc, _, _ = hp._general_chain_inputs(kind, N, D, grid, seed)
    hp._assert_both_paths(kind, Hinc, grid)


@pytest.mark.parametrize("grid", [(16, 32), (30, 40)])
def test_both_paths_assertion_has_teeth(grid):
    """Swapping "roll" for the older tests' "small" makes the both-paths assertion fail: a near-translation of under a row
    keeps EVERY band of a +-3-row window on the window path.  (On 32x64's +-1-row window the image border alone splits
    the bands of such a plane, the first band having no row above it to reach for -- there only the INTERIOR form of the
    assertion, which "general" is held to, has teeth: see the second test below.)"""
    _, Hinc = hp._motion_family(2, 8, "small", 3)
    assert all(not planes for planes in hp._planes_on_both_paths(Hinc, grid))
    with pytest.raises(AssertionError):
        hp._assert_both_paths("roll", Hinc, grid)
    for BR, W in hp.BAND_PLANS[grid]:
        assert bool(hp._band_paths(Hinc, grid, BR, W).all())


@pytest.mark.parametrize("grid", GRIDS)
def test_interior_both_paths_assertion_has_teeth_on_every_grid(grid):
    """What "general" is held to fails for "small" on all three grids, 32x64 included: no plane of a sub-row translation
    splits its interior bands."""
    _, Hinc = hp._motion_family(2, 8, "small", 3)
    with pytest.raises(AssertionError):
        hp._assert_both_paths("general", Hinc, grid)


@pytest.mark.parametrize("B,C,n,rows,cols", [(2, 3, 1, 64, 128), (1, 3, 16, 4, 8), (2, 32, 3, 16, 32), (1, 5, 4, 7, 9)])
def test_float64_restatement_agrees_with_the_oracle_on_near_identity_homographies(B, C, n, rows, cols):
    """_warp_f64 against oracle.homography_warp on test_homography_warp's own near-identity family, within that test's
    tolerance: a wrong restatement would show here."""
    g = torch.Generator().manual_seed(rows * cols + n)
    img = torch.rand(B, C, rows, cols, generator=g) * 2 - 1
    H = torch.eye(3).repeat(B, n, 1, 1) + 0.04 * (torch.rand(B, n, 3, 3, generator=g) - 0.5)
    H[..., 0, 2] += (torch.rand(B, n, generator=g) - 0.5) * cols * 0.5
    H[..., 1, 2] += (torch.rand(B, n, generator=g) - 0.5) * rows * 0.5
    H[..., 2, :2] *= 0.02
    vref, mref = oracle.homography_warp(img, H)
    v64, m64 = hp._warp_f64(img, H)
    hp._mask_rule(mref, m64, H, f"oracle near-identity {B}x{C}x{n}x{rows}x{cols}")
    agree = (mref == m64)[:, None].expand_as(vref)
    assert torch.allclose(vref.double()[agree], v64[agree], rtol=1e-4, atol=cols * 2.0 ** -23 * 8)
    for kind in ("small", "mixed"):            # and on the chain tests' near-translations
        Hk = hp._motion_family(B, n + 1, kind, 3)[0][:, 1:].contiguous()
        vref, mref = oracle.homography_warp(img, Hk)
        v64, m64 = hp._warp_f64(img, Hk)
        agree = (mref == m64)[:, None].expand_as(vref)
        assert int((mref != m64).sum()) <= max(1, mref.numel() // 20000)
        assert torch.allclose(vref.double()[agree], v64[agree], rtol=1e-4, atol=cols * 2.0 ** -23 * 8)


def test_float64_restatement_reproduces_the_reference_on_zero_denominators():
    """tests/golden/g13_zero_denominator.npz, the reference's own warper where u2 == 0 on a column of pixel centres: no
    NaN in its volume (grid_sample's border clamp sends a NaN coordinate to 0), and _warp_f64 follows it bit for bit in
    the mask and to rounding in the values."""
    from conftest import load_golden, t
    fix = load_golden("g13_zero_denominator.npz")
    img, H, vref, mref = t(fix["zd_image"]), t(fix["zd_H"]), t(fix["zd_volume"]), t(fix["zd_mask"])[:, 0]
    u64 = hp._coords_f64(H, 8, 12)[0]
    assert bool((u64[0, :, :, 5] == 0).all()) and int((u64 == 0).sum()) == 3 * 8
    assert not bool(torch.isnan(vref).any())
    v64, m64 = hp._warp_f64(img, H)
    assert torch.equal(m64, mref)
    assert torch.allclose(v64, vref.double(), rtol=1e-5, atol=2e-6)
