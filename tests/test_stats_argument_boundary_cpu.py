"""CPU-side checks of the two consumers of GroupNorm statistics, mvsn_groupnorm_lrelu_apply (csrc/mvsn_groupnorm.hip) and
mvsn_conv_to1_block (csrc/mvsn_conv_to1.hip): each takes `stats, stat_tiles` (0: finalised, > 0: the producer's records)
and refuses a bad argument before any device work, with a message that names the entry.  No GPU."""
import ctypes
import os
import re

from multi_view_stereonet_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 0x1000          # a non-null address that is never dereferenced: every call below fails its checks first
BADARG, TOOLARGE = -1, -2


def _fails(rc, lib, entry, word=b"", code=BADARG):
    msg = lib.mvsn_last_error()
    assert rc == code and msg.startswith(entry + b":") and word in msg, (rc, msg)


def test_groupnorm_lrelu_apply_refuses_bad_arguments_before_any_device_work():
    lib = _native.load()
    name = b"mvsn_groupnorm_lrelu_apply"

    def call(x=ONE, stats=ONE, tiles=0, gamma=ONE, beta=ONE, residual=None, r_stats=None, r_gamma=None, r_beta=None, n=2,
             spatial=96, out=ONE):
        return lib.mvsn_groupnorm_lrelu_apply(x, stats, tiles, gamma, beta, residual, r_stats, r_gamma, r_beta, n, spatial,
                                              out, None)

    for null in ("x", "stats", "gamma", "beta", "out"):
        for tiles in (0, 3):                                   # (either form of `stats`)
            _fails(call(tiles=tiles, **{null: None}), lib, name, b"bad argument")
    for bad in (dict(n=0), dict(n=-1), dict(spatial=0), dict(spatial=-4), dict(tiles=-1)):
        _fails(call(**bad), lib, name, b"bad argument")
    # a raw residual: its statistics need the residual itself, gamma and beta
    full = dict(residual=ONE, r_stats=ONE, r_gamma=ONE, r_beta=ONE)
    for missing in ("residual", "r_gamma", "r_beta"):
        for tiles in (0, 3):
            _fails(call(tiles=tiles, **dict(full, **{missing: None})), lib, name, b"raw residual")


def test_conv_to1_block_refuses_bad_arguments_before_any_device_work():
    lib = _native.load()
    name = b"mvsn_conv_to1_block"

    def call(in_raw=ONE, in_stats=ONE, tiles=0, in_gamma=ONE, in_beta=ONE, in_residual=None, weight=ONE, bias=None,
             prior=None, fx=None, n=2, rows=8, cols=12, out=ONE):
        return lib.mvsn_conv_to1_block(in_raw, in_stats, tiles, in_gamma, in_beta, in_residual, weight, bias, prior, fx, n,
                                       rows, cols, out, None)

    for null in ("in_raw", "in_stats", "in_gamma", "in_beta", "weight", "out"):
        for tiles in (0, 3):
            _fails(call(tiles=tiles, **{null: None}), lib, name, b"null pointer")
    _fails(call(tiles=-1), lib, name, b"stat_tiles")
    for bad in (dict(n=0), dict(rows=0), dict(cols=0), dict(n=-1)):
        _fails(call(**bad), lib, name, b"bad sizes")
    _fails(call(cols=10), lib, name, b"multiple of 4")
    _fails(call(prior=ONE), lib, name, b"needs fx")
    _fails(call(n=65536), lib, name, b"grid", code=TOOLARGE)


def test_one_entry_per_consumer_in_header_binding_and_binary():
    with open(os.path.join(ROOT, "include", "mvsn_hip.h")) as f:
        declared = set(re.findall(r"^(?:int|size_t)\s+(mvsn_[a-z0-9_]+)\s*\(", f.read(), flags=re.M))
    lib = ctypes.CDLL(_native.library_path())
    for gone in ("mvsn_groupnorm_lrelu_add2", "mvsn_groupnorm_lrelu_apply_records", "mvsn_conv_to1_block_records"):
        assert gone not in declared and gone not in _native.SIGNATURES and not hasattr(lib, gone), gone
    from ctypes import c_int, c_long, c_void_p
    assert _native.SIGNATURES["mvsn_groupnorm_lrelu_apply"] == (
        c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 6 + [c_int, c_long, c_void_p, c_void_p])
    assert _native.SIGNATURES["mvsn_conv_to1_block"] == (
        c_int, [c_void_p, c_void_p, c_int] + [c_void_p] * 7 + [c_int] * 3 + [c_void_p, c_void_p])
