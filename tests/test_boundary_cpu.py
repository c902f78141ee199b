"""CPU-side checks of the drop-in boundary: checkpoint layout, the C-ABI library and its header,
host plumbing.  No compute calls into the library here (no GPU)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from multi_view_stereonet_amd import MultiViewStereoNet, _native, synthetic
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
from multi_view_stereonet_amd.params import parameter_shapes
from multi_view_stereonet_amd.weights import load_weights, PRETRAINED


def test_state_dict_layout_matches_reference_checkpoints():
    net = MultiViewStereoNet()
    assert net.num_levels == 5
    sd = net.state_dict()
    assert len(sd) == 226
    assert sum(v.numel() for v in sd.values()) == 752742
    for name in PRETRAINED:
        w = load_weights(name)
        assert set(w) == set(sd)
        missing, unexpected = net.load_state_dict(w, strict=True)
        assert not missing and not unexpected
    # the source extractor shares the left extractor's storage
    a = net.left_feature_extractor.conv0.weight
    b = net.right_feature_extractor.feature_extractor.conv0.weight
    assert a.data_ptr() == b.data_ptr()
    assert len(list(net.parameters())) == 202


def test_parameter_shapes_examples():
    ps = parameter_shapes()
    assert ps["right_feature_extractor.refiner.conv0.weight"] == (32, 35, 3, 3)
    assert ps["volume_filter4.conv4.weight"] == (1, 32, 3, 3, 3)
    assert ps["refiner0.conv0.weight"] == (32, 4, 3, 3)
    assert ps["refiner3.conv0.weight"] == (32, 36, 3, 3)
    assert "left_feature_extractor.conv0.bias" not in ps and "left_feature_extractor.conv_final.bias" in ps


def test_plane_sweep_setup_path_reports_the_kernels_own_predicate():
    """mvsn_plane_sweep_setup_path (host only): 3 = homographies and idepth samples in the reference's fp32 order for every
    pin-hole K -- fx != fy, principal point anywhere -- on a level-4 grid of 8 .. 8192 pixels; 1 outside that range (the
    samples from the fp64 evaluation); 0 for a K off the form [[fx,0,cx],[0,fy,cy],[0,0,1]] at either level."""
    import torch
    from multi_view_stereonet_amd import synthetic
    from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
    batch = synthetic.with_camera(synthetic.make_batch(131, 277, 1, batch=2, seed=1), fy_scale=(1.137, 0.83), dcx=13.25, dcy=-7.6)
    K = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)["K_pyr"]
    K0, K4 = K[0], K[4]
    path = _native.plane_sweep_setup_path
    assert path(K0, K4, 9, 18) == [3, 3]
    assert path(K0, K4, 2, 4) == [3, 3] and path(K0, K4, 64, 128) == [3, 3]                    # 8 and 8192 pixels
    assert path(K0, K4, 1, 7) == [1, 1] and path(K0, K4, 1, 8193) == [1, 1] and path(K0, K4, 96, 100) == [1, 1]
    assert path(K0, K4, 0, 18) == [0, 0]
    for lvl in (0, 4):
        for (i, j), v in (((0, 1), 0.3), ((1, 0), 1e-6), ((2, 0), 1e-3), ((2, 1), -1e-3), ((2, 2), 0.5), ((0, 0), 0.0),
                          ((1, 1), 0.0), ((0, 1), float("nan"))):
            Ks = [K0.clone(), K4.clone()]
            Ks[lvl // 4][1, i, j] = v
            assert path(Ks[0], Ks[1], 9, 18) == [3, 0], (lvl, i, j, v)
    zero_centre = K0.clone()
    zero_centre[:, 0, 2] = 0.0
    zero_centre[:, 1, 2] = -4.5
    assert path(zero_centre, K4, 9, 18) == [3, 3]
    assert _native.load().mvsn_plane_sweep_setup_path(None, None, 9, 18) == 0


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "mvsn_hip.h")).read()
    declared = set(re.findall(r"\b(mvsn_[a-z0-9_]+)\s*\(", header))
    declared -= {"mvsn_stream_t"}
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(_native.library_path())
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/mvsn_hip.h but not exported"
    assert declared == set(_native.SIGNATURES), (declared ^ set(_native.SIGNATURES))
    typed = _native.load()
    assert typed.mvsn_abi_version() == _native.ABI_VERSION == 7
    # direct form + the chain's Winograd U + the same three layers in the convolution kernels' layout (stepwise form)
    assert typed.mvsn_feature_refiner_packed_floats() == (9 * 9 * 128 + 2 * 9 * 8 * 128 + 7 * 32) + 25 * 2048 + 25 * 2048
    assert typed.mvsn_incremental_cost_volume_form(16, 32) == _native.CHAIN_WINOGRAD
    assert typed.mvsn_incremental_cost_volume_form(4, 8) == _native.CHAIN_WINOGRAD
    assert typed.mvsn_incremental_cost_volume_form(30, 40) == _native.CHAIN_DIRECT      # planes + U exceed 160 KB
    assert typed.mvsn_incremental_cost_volume_form(5, 6) == _native.CHAIN_DIRECT        # odd rows
    # the stepwise form: workspace grows with the planes (image volume) and is 0 for the plane-resident Winograd form
    ws = typed.mvsn_incremental_cost_volume_workspace_bytes_for
    assert ws(2, 64, 16, 32, _native.CHAIN_WINOGRAD) == 0
    assert ws(1, 96, 30, 40, _native.CHAIN_STEPWISE) > ws(1, 48, 30, 40, _native.CHAIN_STEPWISE) > 0
    assert ws(1, 96, 30, 42, _native.CHAIN_STEPWISE) == 0                               # cols % 4 != 0: no such form
    assert ws(4, 96, 30, 40, _native.CHAIN_DIRECT) == typed.mvsn_incremental_cost_volume_workspace_bytes(4, 30, 40)


def test_conv_planning_is_host_side_and_validates():
    lib = _native.load()
    d = _native.ConvDesc(2, 32, 32, 64, 16, 32, 3, 3, 3, 1, 1)
    assert lib.mvsn_conv_num_tiles(ctypes.byref(d)) == 32 * 2 * 1 * 16     # partial records: tiles x 4 waves x 4 lane rows
    dw = _native.ConvDesc(2, 32, 32, 64, 16, 32, 3, 3, 3, 1, 1, _native.CONV_FP32_WINO)
    assert lib.mvsn_conv_winograd_supported(ctypes.byref(dw)) == 1          # volume form: planes x tiles x 8 waves x 4 rows
    assert lib.mvsn_conv_num_tiles(ctypes.byref(dw)) == 64 * 1 * 32
    assert lib.mvsn_conv_packed_floats(ctypes.byref(dw)) == 3 * 8 * 16 * 128
    assert lib.mvsn_conv_packed_floats(ctypes.byref(d)) == 4 * 27 * 256
    bad = _native.ConvDesc(2, 32, 33, 1, 16, 32, 1, 3, 3, 1, 1)      # c_out > 32
    assert lib.mvsn_conv_packed_floats(ctypes.byref(bad)) == 0
    even = _native.ConvDesc(2, 32, 32, 1, 16, 32, 1, 4, 4, 1, 1)     # even kernels unsupported
    assert lib.mvsn_conv_num_tiles(ctypes.byref(even)) == 0
    # argument validation happens before any device work
    rc = lib.mvsn_soft_argmin(None, None, 1, 4, 16, None, None)
    assert rc == -1 and b"null" in lib.mvsn_last_error()
    # direct form: the step's moved features always travel through the workspace (32 x P floats per chain, ABI 3) ...
    assert lib.mvsn_incremental_cost_volume_workspace_bytes(4, 16, 32) == 4 * 32 * 512 * 4      # ... alone (planes in LDS)
    assert lib.mvsn_incremental_cost_volume_workspace_bytes(4, 30, 40) > 4 * 32 * 1200 * 4      # ... + global planes
    assert lib.mvsn_incremental_cost_volume_repair_workspace_bytes(4, 16, 32) == 0   # the repair form there is Winograd
    assert lib.mvsn_incremental_cost_volume_repair_workspace_bytes(4, 30, 40) == \
        lib.mvsn_incremental_cost_volume_workspace_bytes(4, 30, 40)
    assert lib.mvsn_incremental_cost_volume_workspace_bytes(1, 32, 64) > 0        # config 5 grid


def test_winograd_form_selection_is_pinned_host_side():
    """Which kernel form every Winograd layer runs on -- (k-steps, ring stages, carried units, tile form, full-width
    transform) -- its LDS bytes, work items per sample and steps per item, through mvsn_debug_wino_plan (host only).  The
    expected rows are the plans and launch branches of the code before the forms became one table."""
    lib = _native.load()
    RP = 3

    def plan(cin, rows, cols, dil=1, depth=1, kd=1, carrying=0, k=3, stride=1):
        d = _native.ConvDesc(1, cin, 32, depth, rows, cols, kd, k, k, stride, dil, _native.CONV_FP32_WINO)
        out = (ctypes.c_int * 8)()
        return list(out) if lib.mvsn_debug_wino_plan(ctypes.byref(d), carrying, ctypes.byref(out)) else None

    def forms(*a, **kw):
        return tuple(p and tuple(p[:5]) for p in (plan(*a, **kw), plan(*a, carrying=1, **kw)))

    old = lib.mvsn_debug_set_wino_rowphase(0)
    try:
        # 2-D layers on 256 x 512
        assert forms(32, 256, 512) == ((2, 4, 0, 0, 0), (2, 3, 2, 0, 0))
        assert plan(32, 256, 512)[5:] == [4 * 2 * 4 * 736 * 4 + 8 * 2048 * 4 + 128, 16 * 16, 4] and 159872 == 4 * 2 * 4 * 736 * 4 + 8 * 2048 * 4 + 128
        assert plan(32, 256, 512, carrying=1)[5:] == [3 * 2 * 4 * 736 * 4 + 8 * 2048 * 4 + 128 + 8 * 2 * 1024, 16 * 16, 4]
        assert forms(36, 256, 512) == ((2, 3, 0, 0, 0), None)            # 36 -> 32 channels: nothing carries
        assert plan(36, 256, 512)[5:] == [3 * 2 * 4 * 736 * 4 + 10 * 2048 * 4 + 128, 16 * 16, 5]   # (a zero tenth chunk)
        assert forms(4, 256, 512) == ((1, 6, 0, 0, 0), None)             # the head
        for dil in (2, 4):                                               # row-phase items
            assert forms(32, 256, 512, dil) == ((2, 4, 0, RP, 0), (2, 3, 2, RP, 0)), dil
        assert forms(36, 256, 512, 2) == ((2, 3, 0, RP, 0), None)
        assert forms(32, 256, 512, 8) == ((2, 3, 0, RP, 0), (1, 3, 1, RP, 0))
        assert plan(32, 256, 512, 8, carrying=1)[5:] == [3 * 4 * 880 * 4 + 65536 + 128 + 8192, 8 * 2 * 16, 8]
        assert 3 * 4 * 880 * 4 + 65536 + 128 + 8192 == 116096
        assert forms(32, 40, 512, 8) == ((1, 3, 0, 0, 0), (1, 3, 1, 0, 0))   # 8 phases x 1 item row > 3 tile rows: square
        assert forms(4, 256, 512, 2) == (None, None) and forms(36, 256, 512, 4) == (None, None)   # not instantiated
        assert plan(32, 256, 512, k=5, stride=2, carrying=1) is None     # the stride-2 layer carries nothing
        lib.mvsn_debug_set_wino_rowphase(2)                              # square tiles only
        assert forms(32, 256, 512, 2) == ((2, 3, 0, 0, 0), (2, 3, 2, 0, 0))
        assert forms(32, 256, 512, 4) == ((2, 3, 0, 0, 0), (1, 3, 1, 0, 0))
        assert forms(32, 256, 512, 8) == ((1, 3, 0, 0, 0), (1, 3, 1, 0, 0))
        assert plan(32, 256, 512, 4)[5:] == [3 * 2 * 4 * (24 * 40 + 16) * 4 + 65536 + 128, 16 * 16, 4]
        lib.mvsn_debug_set_wino_rowphase(0)
        # volume form
        assert forms(32, 16, 32, depth=64, kd=3) == ((2, 3, 0, 0, 1), (2, 3, 1, 0, 1))
        assert forms(32, 64, 128, depth=64, kd=3)[0] == (2, 3, 0, 0, 0)
        assert forms(32, 10, 40, depth=64, kd=3)[0] == (2, 3, 0, 1, 0)
        assert forms(32, 30, 40, depth=96, kd=3) == ((2, 4, 0, 2, 0), (2, 3, 1, 2, 0))
        # rolling strips: 15 raw rows x 48 columns; U streams through 4 (3 when carrying) stages of two chunks
        assert plan(32, 30, 40, depth=96, kd=3)[5:] == [4 * 2 * 4 * (15 * 48 + 16) * 4 + 4 * 2 * 2048 * 4 + 128, 240, 12]
        assert plan(32, 30, 40, depth=96, kd=3, carrying=1)[5:] == [3 * 2 * 4 * 736 * 4 + 3 * 2 * 2048 * 4 + 128, 240, 12]
    finally:
        lib.mvsn_debug_set_wino_rowphase(old)


def test_direct_form_selection_is_pinned_host_side():
    """Which kernel form every direct fp32 layer runs on -- row of the table, kind, pixel tiles per wave, staged elements
    or DMA pieces, 16-byte staging, cout tiles -- its LDS bytes and tiles per sample, through mvsn_debug_conv_plan (host
    only).  The expected plans (conv_form_cases.py) are the geometry and launch ladder of the code before the forms became
    one table; together the cases name every row, so a new row cannot arrive unpinned."""
    import conv_form_cases as cf
    lib = _native.load()
    hit, nrows = set(), set()
    for c in cf.CASES + [cf.PADDED_CHUNK]:
        got, n = cf.plan(lib, _native, c)
        assert got == c.plan, (cf.case_id(c), got, c.plan)
        if got is not None:
            hit.add(got[0])
            nrows.add(n)
            # partial records per sample: tiles x 4 waves x 4 lane rows; the batch changes nothing
            d = _native.ConvDesc(1, c.cin, c.cout, c.depth, c.rows, c.cols, c.kd, c.k, c.k, c.stride, c.dil)
            assert lib.mvsn_conv_num_tiles(ctypes.byref(d)) == got[7] * 16
            assert cf.plan(lib, _native, c, n=5)[0] == got
        else:
            assert n == 0
    assert nrows == {12} and hit == set(range(12)), (nrows, sorted(hit))
    # written out once: the 16-row LDS-DMA tile at dilation 8 with a residual tile, and the register-staged 3x3x3 tile
    big, = [c for c in cf.CASES if (c.rows, c.cols, c.dil, c.mode, c.cout) == (17, 36, 8, 2, 8)]
    assert big.plan[6] == (2 * (2 * 4 * (6 * 256 + 16) + 1280) + 80) * 4 == 109888
    assert cf._staged_lds(25, 27) == (4 * 1616 + 3456 + 128) * 4 == 40192
    # the head needs cols % 8 == 0 and a plain call; a Winograd or bf16 descriptor has no direct plan
    out = (ctypes.c_int * 8)()
    head = _native.ConvDesc(1, 3, 32, 1, 17, 72, 1, 5, 5, 2, 1)
    assert lib.mvsn_debug_conv_plan(ctypes.byref(head), 1, ctypes.byref(out)) == 12 and out[0] == cf.S2_V4
    for prec in (_native.CONV_FP32_WINO, _native.CONV_BF16X3):
        d = _native.ConvDesc(1, 32, 32, 1, 17, 36, 1, 3, 3, 1, 1, prec)
        assert lib.mvsn_debug_conv_plan(ctypes.byref(d), 0, ctypes.byref(out)) == 0
    assert lib.mvsn_debug_conv_plan(None, 0, ctypes.byref(out)) == 0


def test_banded_plan_selection_host_logic():
    """Which plan a banded call runs, and what it needs, from the host side alone (no device: the library assumes 256
    CUs): thin bands while the chains fit one of their passes, slabs beyond (mvsn_chain_slab.hip); passes of equal size, or
    full slab passes + one thin pass for a small remainder;
    the status word behind the granules of the largest pass."""
    lib = _native.load()
    groups = lib.mvsn_incremental_cost_volume_banded_groups
    assert [groups(n, 30, 40) for n in (1, 17, 18, 128, 1000)] == [15, 15, 3, 3, 3]
    assert [groups(n, 32, 64) for n in (1, 16, 17, 64, 300)] == [16, 16, 4, 4, 4]
    assert [groups(n, 16, 32) for n in (1, 32, 33, 64, 512)] == [8, 8, 4, 4, 4]       # 16x32: thin bands only
    assert groups(4, 24, 40) == 0 and groups(0, 30, 40) == 0
    form_for = lib.mvsn_incremental_cost_volume_form_for
    assert all(form_for(n, r, c) == _native.CHAIN_BANDED for n in (1, 20, 128, 1000) for r, c in ((30, 40), (32, 64)))
    assert form_for(64, 16, 32) == _native.CHAIN_BANDED and form_for(65, 16, 32) == _native.CHAIN_WINOGRAD
    ws = lib.mvsn_incremental_cost_volume_workspace_bytes_for
    off = lib.mvsn_incremental_cost_volume_status_offset
    for (rows, cols) in ((30, 40), (32, 64)):
        cap = 256 // groups(1000, rows, cols)
        # one pass: the workspace grows with the chains; several passes: it is the largest pass's (equal sizes)
        b18, b19 = ws(18, 96, rows, cols, _native.CHAIN_BANDED), ws(19, 96, rows, cols, _native.CHAIN_BANDED)
        assert 0 < b18 < b19 and off(18, rows, cols) + 64 == b18
        n = 2 * cap + 40                      # three passes of (n + 2) // 3 chains
        per = -(-n // 3)
        assert ws(n, 96, rows, cols, _native.CHAIN_BANDED) == ws(per, 96, rows, cols, _native.CHAIN_BANDED)
        assert off(n, rows, cols) == off(per, rows, cols)
        # a remainder that fits ONE thin-band pass: full slab passes + that thin pass, its granules inside the slab
        # passes' workspace (status block where a full pass has it)
        n = 2 * cap + 2
        assert ws(n, 96, rows, cols, _native.CHAIN_BANDED) == ws(cap, 96, rows, cols, _native.CHAIN_BANDED)
        assert off(n, rows, cols) == off(cap, rows, cols) and groups(n, rows, cols) == groups(1000, rows, cols)


def test_forward_refuses_cpu_tensors():
    net = MultiViewStereoNet()
    batch = synthetic.make_batch(64, 128, 1)
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        net(inp["left_image_pyr"], inp["K_pyr"], inp["T_right_in_left"], inp["right_image_pyr"], 8, True, [True] * 5)


def test_unpack_batch_semantics():
    batch = synthetic.make_batch(60, 90, 3, batch=2, seed=4, pose_jitter=0.2)
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    sizes = [tuple(p.shape[-2:]) for p in inp["left_image_pyr"]]
    assert sizes == [(60, 90), (30, 45), (15, 23), (8, 12), (4, 6)]
    # first source has unit baseline after normalisation, every pose shares that scale
    t0 = inp["T_right_in_left"][0][:, :3, 3].norm(dim=1)
    assert torch.allclose(t0, torch.ones(2), atol=1e-6)
    raw1 = batch["T_right_in_left"][1].squeeze(1)[:, :3, 3]
    assert torch.allclose(inp["T_right_in_left"][1][:, :3, 3], raw1 / inp["baseline"][:, None], atol=1e-6)
    for T, Tinv in zip(inp["T_right_in_left"], inp["T_left_in_right"]):
        assert torch.allclose(T @ Tinv, torch.eye(4).expand(2, 4, 4), atol=1e-5)
    K4 = inp["K_pyr"][4]
    sx = 6.0 / 90.0
    assert torch.allclose(K4[:, 0, 0], inp["K_pyr"][0][:, 0, 0] * sx)
    assert torch.allclose(K4[:, 0, 2], sx * (inp["K_pyr"][0][:, 0, 2] + 0.5) - 0.5)
    # the caller's batch is not modified
    assert batch["T_right_in_left"][0].shape == (2, 1, 4, 4)


def test_multi_view_forward_wrapper_passes_params():
    seen = {}

    def fake(lp, kp, ts, rp, D, flt, refs):
        seen.update(D=D, flt=flt, refs=refs)
        z = [torch.zeros(1)] * 5
        return {"left_idepthmap_pyr": z, "left_idepthmap_raw_pyr": z, "left_idepthmap_mask_pyr": z}

    batch = synthetic.make_batch(32, 64, 1)
    inp = snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5)
    out = snu.multi_view_forward(fake, inp, {"num_idepth_samples": 12})        # DeMoN yaml lacks the flags
    assert seen == {"D": 12, "flt": True, "refs": [True] * 5} and out["stereo_time_ms"] >= 0.0
    snu.multi_view_forward(fake, inp, {"num_idepth_samples": 7, "cost_volume_filter": False,
                                       "refiners": [False, True, True, True, False]})
    assert seen == {"D": 7, "flt": False, "refs": [False, True, True, True, False]}


def test_module_copies_and_pickles_with_a_live_engine():
    """The cached engine holds ctypes function pointers (not picklable); copies drop it and keep the options."""
    import copy
    import io
    import pickle
    net = MultiViewStereoNet()
    net.load_state_dict(load_weights("gta_sfm_150epochs"), strict=True)
    net.options.conv_precision = "bf16x3"

    class FakeEngine:                     # stands in for PlaneSweepEngine (which needs a device to pack weights)
        def __init__(self):
            self.lib = _native.load()
            self.fn = self.lib.mvsn_abi_version

    net._engine, net._engine_key = FakeEngine(), ("stale",)
    with pytest.raises(Exception):
        pickle.dumps(net._engine)
    for dup in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert dup._engine is None and dup._engine_key is None
        assert dup.options.conv_precision == "bf16x3" and dup.options is not net.options
        assert torch.equal(dup.refiner0.conv0.weight, net.refiner0.conv0.weight)
        assert dup.left_feature_extractor.conv0.weight.data_ptr() == \
            dup.right_feature_extractor.feature_extractor.conv0.weight.data_ptr()      # sharing survives the copy
    buf = io.BytesIO()
    torch.save(net, buf)
    assert net._engine is not None        # the original keeps its engine


def test_library_is_the_build_of_the_sources_beside_it():
    """__graft_entry__.build() rebuilds on a content mismatch (sha256 of the .hip / .h files in libmvsn_hip.so.sources),
    so a binary that travelled with a snapshot is known to correspond to the snapshot's sources."""
    from multi_view_stereonet_amd import build
    assert build.built_from_current_sources(), "libmvsn_hip.so does not match csrc/: run __graft_entry__.build()"
    assert len(build.source_digest()) == 64
