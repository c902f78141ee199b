"""The per-pixel confidence on the device: the kernels of csrc/mvsn_misc.hip against the float64
restatement of tests/confidence_reference.py under its ambiguity rule, the option through the three forward routes
(eager, recorded plans with their hipGraph replay, stream lanes), and the gated fusion against its own composition."""
import numpy as np
import pytest
import torch

import confidence_reference as cr
from fusion_reference import nearest_neighbours
from test_hip_parity import net_for, to_dev
from multi_view_stereonet_amd import metrics, synthetic
from multi_view_stereonet_amd import multi_view_stereonet_utils as snu
from multi_view_stereonet_amd.fusion import frame_pair_poses, fuse_depthmaps, point_values, reconstruct

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
WEIGHTS = "gta_sfm_150epochs"


def engine():
    return net_for(WEIGHTS).engine()


def same_bits(a, b):
    """torch.equal with NaNs in the same places counting as equal."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ---- the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows,cols", cr.CONF_SHAPES)
@pytest.mark.parametrize("D", cr.CONF_D)
def test_soft_argmin_confidence(D, n, rows, cols):
    eng = engine()
    for scale in cr.CONF_SCALES:
        cost, samples = cr.conf_inputs(n, D, rows, cols, scale)
        idepth, conf = eng.soft_argmin_confidence(cost.to(DEV), samples.to(DEV))
        assert torch.equal(idepth, eng.soft_argmin(cost.to(DEV), samples.to(DEV)))
        conf = conf.cpu()
        assert conf.shape == (n, 1, rows, cols)
        frac, share = cr.compare(conf, cost)
        print(f"confidence D={D} {n}x{rows}x{cols} scale {scale:g}: {frac:.4f} of conf_bound, ambiguous {share:.3%}")
        assert frac <= 1.0, (D, n, rows, cols, scale, frac)
        assert float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0 + cr.conf_bound(D)
    flat = torch.full((n, D, rows, cols), 3.0)
    conf = eng.soft_argmin_confidence(flat.to(DEV), samples.to(DEV))[1].cpu()
    assert cr.compare(conf, flat)[0] <= 1.0
    assert float((conf.double() - min(D, 4) / D).abs().max()) <= cr.conf_bound(D)


@pytest.mark.parametrize("D", (3, 17, 33, 64))
def test_soft_argmin_confidence_nan_stays_in_its_pixel(D):
    eng = engine()
    cost, samples = cr.conf_inputs(3, D, 7, 37, 50.0)
    clean_i, clean_c = (t.cpu() for t in eng.soft_argmin_confidence(cost.to(DEV), samples.to(DEV)))
    for d_nan in (0, D // 2, D - 1):
        bad = cost.clone()
        bad[1, d_nan, 2, 5] = float("nan")
        idepth, conf = (t.cpu() for t in eng.soft_argmin_confidence(bad.to(DEV), samples.to(DEV)))
        assert bool(conf[1, 0, 2, 5].isnan()) and int(conf.isnan().sum()) == 1
        assert bool(idepth[1, 0, 2, 5].isnan()) and int(idepth.isnan().sum()) == 1
        keep = torch.ones_like(conf, dtype=torch.bool)
        keep[1, 0, 2, 5] = False
        assert torch.equal(conf[keep], clean_c[keep]) and torch.equal(idepth[keep], clean_i[keep])


@pytest.mark.parametrize("rows,cols", cr.FUSE_GRIDS)
@pytest.mark.parametrize("B", cr.FUSE_B)
@pytest.mark.parametrize("S", cr.FUSE_S)
def test_confidence_fuse_sources(S, B, rows, cols):
    eng = engine()
    conf = cr.fuse_min_inputs(S, B, rows, cols)
    got = eng.confidence_fuse_sources(conf.to(DEV), S, B).cpu()
    assert torch.equal(got, cr.fuse_min_ref(conf, S, B))
    if S > 1 and B > 1 and rows * cols > 1:
        assert not torch.equal(got, cr.fuse_min_ref(conf, S, B, chain=cr.chain_bs))     # chain n = s*B + b, not b*S + s
    # a NaN in one source (the last chain: s = S-1, b = B-1) and in the first
    conf[S * B - 1, 0, rows // 2, cols // 2] = float("nan")
    conf[0, 0, 0, 0] = float("nan")
    got = eng.confidence_fuse_sources(conf.to(DEV), S, B).cpu()
    ref = cr.fuse_min_ref(conf, S, B)
    assert bool(got[B - 1, 0, rows // 2, cols // 2].isnan()) and bool(got[0, 0, 0, 0].isnan())
    assert torch.equal(got.isnan(), ref.isnan()) and same_bits(got, ref)


# ---- the forward -----------------------------------------------------------------------------------------------------
def _inputs(B, S, seed):
    batch = synthetic.make_batch(64, 128, S, batch=B, seed=seed)
    return to_dev(snu.multi_view_unpack_batch(batch, torch.device("cpu"), 5))


def _run(net, x, D, confidence, capture=None):
    keep = net.options.confidence
    net.options.confidence = confidence
    try:
        return net(*x, D, True, [True] * 5, capture=capture)
    finally:
        net.options.confidence = keep


def _same_pyramids(a, b, keys):
    for k in keys:
        assert len(a[k]) == len(b[k]) == 5
        for x, y in zip(a[k], b[k]):
            assert x.dtype == y.dtype and torch.equal(x, y), k


IDEPTH_KEYS = ("left_idepthmap_pyr", "left_idepthmap_raw_pyr", "left_idepthmap_mask_pyr")


@pytest.mark.parametrize("B,S,D", [(1, 2, 16), (6, 3, 16), (1, 2, 3)])    # a recorded plan; 18 chains: eager; a cut window
def test_forward_confidence(B, S, D):
    net = net_for(WEIGHTS)
    eng = net.engine()
    x = _inputs(B, S, seed=5)
    off = _run(net, x, D, False)
    assert set(off) == set(IDEPTH_KEYS)
    on = _run(net, x, D, True)
    assert set(on) == set(IDEPTH_KEYS) | {"left_confidence_pyr"}
    _same_pyramids(on, off, IDEPTH_KEYS)
    cap = {}
    captured = _run(net, x, D, True, capture=cap)
    _same_pyramids(captured, on, IDEPTH_KEYS + ("left_confidence_pyr",))
    raw, chain = eng.soft_argmin_confidence(cap["filtered_cost"], cap["idepth_samples"])
    assert torch.equal(chain, cap["confidence_per_chain"]) and torch.equal(raw, cap["raw_per_chain"])
    assert chain.shape == (S * B, 1, 4, 8)
    conf = on["left_confidence_pyr"]
    want = eng.confidence_fuse_sources(chain, S, B)
    assert torch.equal(conf[4], want)
    frac, _ = cr.compare(chain.cpu(), cap["filtered_cost"].cpu())
    assert frac <= 1.0
    assert torch.equal(conf[4].cpu(), cr.fuse_min_ref(chain.cpu(), S, B))
    for lvl in (3, 2, 1, 0):
        size = x[0][lvl].shape[-2:]
        assert conf[lvl].shape == (B, 1) + tuple(size) and conf[lvl].dtype == torch.float32
        assert torch.equal(conf[lvl], eng.upsample(conf[lvl + 1], size))
    assert float(conf[0].min()) >= 0.0 and float(conf[0].max()) <= 1.0 + cr.conf_bound(D)
    cap_off = {}
    _run(net, x, D, False, capture=cap_off)
    assert "confidence_per_chain" not in cap_off and "raw_per_chain" in cap_off


def test_planned_and_graph_replayed_forwards_match_eager():
    net = net_for(WEIGHTS)
    D, keys = 16, IDEPTH_KEYS + ("left_confidence_pyr",)
    sets = [_inputs(1, 2, seed=20 + k) for k in range(4)]
    keep = (net.options.plan_max_chains, net.options.confidence)
    try:
        net.options.confidence = True
        net.options.plan_max_chains = 0
        eager = [net(*x, D, True, [True] * 5) for x in sets]
        assert not torch.equal(eager[0]["left_confidence_pyr"][0], eager[1]["left_confidence_pyr"][0])
        net.options.plan_max_chains = 16
        before = net.engine().replays
        for x, ref in zip(sets, eager):               # records, replays the list, captures the graph, replays the graph
            _same_pyramids(net(*x, D, True, [True] * 5), ref, keys)
        assert net.engine().replays - before >= 3
        # a plan recorded with the option off is not replayed with it on, and the other way round
        net.options.confidence = False
        off = net(*sets[0], D, True, [True] * 5)
        assert set(off) == set(IDEPTH_KEYS)
        _same_pyramids(off, eager[0], IDEPTH_KEYS)
    finally:
        net.options.plan_max_chains, net.options.confidence = keep


def test_stream_lanes_give_the_same_confidence():
    net = net_for(WEIGHTS)
    x = _inputs(4, 2, seed=9)
    keep = (net.options.plan_max_chains, net.stream_lanes)
    try:
        net.options.plan_max_chains = 0
        one = _run(net, x, 16, True)
        net.stream_lanes = 2
        two = _run(net, x, 16, True)
        torch.cuda.synchronize()
    finally:
        net.options.plan_max_chains, net.stream_lanes = keep
    assert set(two) == set(one)
    _same_pyramids(two, one, IDEPTH_KEYS + ("left_confidence_pyr",))


def test_wrappers_pass_the_confidence_through():
    net = net_for(WEIGHTS)
    batch = synthetic.make_batch(64, 128, 2, batch=1, seed=3)
    inputs = snu.multi_view_unpack_batch(batch, torch.device(DEV), 5)
    params = {"num_idepth_samples": 16}
    keep = net.options.confidence
    try:
        assert "left_confidence_pyr" not in snu.multi_view_forward(net, inputs, params)
        net.options.confidence = True
        a = snu.multi_view_forward(net, inputs, params)
        b = snu.multi_view_forward(net, inputs, params, sync_timer=False)
        torch.cuda.synchronize()
    finally:
        net.options.confidence = keep
    for x, y in zip(a["left_confidence_pyr"], b["left_confidence_pyr"]):
        assert torch.equal(x, y)
    assert a["left_confidence_pyr"][0].shape == (1, 1, 64, 128)


# ---- fusion ----------------------------------------------------------------------------------------------------------
THR = 0.375


def _confidence_maps(V, H, W, seed=11):
    g = torch.Generator().manual_seed(seed)
    conf = torch.rand(V, 1, H, W, generator=g)
    conf[torch.rand(V, 1, H, W, generator=g) < 0.02] = float("nan")
    conf[torch.rand(V, 1, H, W, generator=g) < 0.05] = THR          # exactly at the threshold: kept
    return conf


def test_gated_fusion_is_fusion_with_the_combined_mask():
    V, H, W = 6, 96, 128
    sc = synthetic.fusion_scene(V, H, W, device=DEV)
    nb = nearest_neighbours(V, 4)
    conf = _confidence_maps(V, H, W)
    assert int(conf.isnan().sum()) > 0 and int((conf == THR).sum()) > 0
    host_mask = conf >= THR                                             # NaN compares false
    assert bool(host_mask[conf == THR].all()) and not bool(host_mask[conf.isnan()].any())
    args = (sc["depth"], sc["K"], sc["T_cam_in_world"], nb)
    got = fuse_depthmaps(*args, images=sc["images"], confidence=conf.to(DEV), min_confidence=THR)
    want = fuse_depthmaps(*args, images=sc["images"], valid=host_mask.to(DEV))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    plain = fuse_depthmaps(*args, images=sc["images"])
    assert 0 < got.points.shape[0] < plain.points.shape[0]
    # confidence without a threshold gates nothing
    for a, b in zip(fuse_depthmaps(*args, images=sc["images"], confidence=conf.to(DEV)), plain):
        assert torch.equal(a, b)
    # an existing valid is combined, not replaced (bool and uint8 alike)
    g = torch.Generator().manual_seed(7)
    valid = torch.rand(V, 1, H, W, generator=g) > 0.1
    want = fuse_depthmaps(*args, images=sc["images"], valid=(valid & host_mask).to(DEV))
    for v in (valid, valid.to(torch.uint8)):
        got2 = fuse_depthmaps(*args, images=sc["images"], valid=v.to(DEV), confidence=conf.to(DEV), min_confidence=THR)
        for a, b in zip(got2, want):
            assert torch.equal(a, b)
    assert want.points.shape[0] < got.points.shape[0]
    # point_values: the maps at every point's view and pixel
    vals = point_values(got, conf.to(DEV))
    idx = got.view.long() * (H * W) + got.pixel.long()
    assert vals.shape == (got.points.shape[0],) and vals.dtype == torch.float32
    assert torch.equal(vals, conf.to(DEV).reshape(-1)[idx])
    assert float(vals.min()) >= THR
    # a subset of reference views: maps that hold those views only
    refs = [4, 1, 3]
    sub = fuse_depthmaps(sc["depth"], sc["K"], sc["T_cam_in_world"], np.array([[3, 5, 2], [0, 2, 3], [2, 4, 1]]),
                         ref_views=refs, confidence=conf.to(DEV), min_confidence=THR)
    assert sub.points.shape[0] > 0
    assert torch.equal(point_values(sub, conf.to(DEV)), conf.to(DEV).reshape(-1)[sub.view.long() * (H * W) + sub.pixel.long()])
    assert torch.equal(point_values(sub, conf[refs].to(DEV), ref_views=refs), point_values(sub, conf.to(DEV)))
    # no points: an empty result, no launch
    none = fuse_depthmaps(*args, confidence=conf.to(DEV), min_confidence=2.0)
    assert none.points.shape == (0, 3) and point_values(none, conf.to(DEV)).shape == (0,)


@pytest.mark.parametrize("batch", [2, 6])     # 2 x 3 sources: recorded plans; 6 x 3 = 18 chains: eager forward
def test_reconstruct_with_confidence_is_its_composition(batch):
    net = net_for(WEIGHTS)
    V, S, D = 6, 3, 16
    sc = synthetic.fusion_scene(V, 64, 128, device=DEV)
    nb = nearest_neighbours(V, S)
    assert net.options.confidence is False
    res, depth, conf = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, num_idepth_samples=D,
                                   batch=batch, max_rel_depth=0.05, min_consistent=1, with_confidence=True,
                                   min_confidence=0.5)
    assert net.options.confidence is False
    plain = reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, num_idepth_samples=D, batch=batch,
                        max_rel_depth=0.05, min_consistent=1)
    assert len(plain) == 2 and torch.equal(plain[1], depth)
    depths, confs = [], []
    net.options.confidence = True
    try:
        for lo in range(0, V, batch):
            ref = list(range(lo, min(lo + batch, V)))
            frames = {"left_image": sc["images"][ref], "right_image": [sc["images"][nb[ref, s].tolist()] for s in range(S)],
                      "K": sc["K"].cpu()[ref].unsqueeze(1).contiguous(),
                      "T_right_in_left": [frame_pair_poses(sc["T_cam_in_world"], ref, nb[ref, s]) for s in range(S)]}
            inputs = snu.multi_view_unpack_batch(frames, torch.device(DEV), net.num_levels)
            out = net(inputs["left_image_pyr"], inputs["K_pyr"], inputs["T_right_in_left"], inputs["right_image_pyr"], D,
                      True, [True] * 5)
            depths.append(metrics.idepth_to_depth(out["left_idepthmap_pyr"][0], inputs["baseline"]))
            confs.append(out["left_confidence_pyr"][0])
    finally:
        net.options.confidence = False
    assert torch.equal(depth, torch.cat(depths, 0)) and torch.equal(conf, torch.cat(confs, 0))
    assert conf.shape == (V, 1, 64, 128)
    want = fuse_depthmaps(depth, sc["K"], sc["T_cam_in_world"], nb, images=sc["images"], max_rel_depth=0.05,
                          min_consistent=1, valid=conf >= 0.5)
    for x, y in zip(res, want):
        assert torch.equal(x, y)
    # the option is restored when a forward raises, too
    with pytest.raises(AssertionError):
        reconstruct(net, sc["images"], sc["K"], sc["T_cam_in_world"], nb, num_idepth_samples=D, batch=batch,
                    refiners=(True,) * 4, with_confidence=True)
    assert net.options.confidence is False
