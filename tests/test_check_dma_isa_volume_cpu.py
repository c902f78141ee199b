"""tools/check_dma_isa.py on the volume carriers (conv_wino_kernel<.., VOL, RIDE = 1>): their carried loads are inline
assembly the compiler's waitcnt pass does not see, so besides the DMA-block / M0 / no-spill properties of every carrier the
checker asserts that nothing names a hidden load's registers before a hand-placed counted wait and that no wait of the
compiler's own on the vector-memory queue sits inside a loop.  First the checker itself on hand-written bodies (it must
report what it is there to catch), then a gfx950 build of the file (hipcc cross-compiles on the CPU box)."""
import importlib.util
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("check_dma_isa", os.path.join(ROOT, "tools", "check_dma_isa.py"))
chk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(chk)

VOL = dict(mode=0, ks=2, nstage=3, dil=1, vol=1, ride=1, tile=0, fullw=1)
PIECE = [";;#ASMSTART", "s_mov_b32 m0, s56", "s_nop 0", "buffer_load_dwordx4 v184, s[56:59], 0 offen lds", ";;#ASMEND"]
LOAD = [";;#ASMSTART", "buffer_load_dwordx4 v[0:3], v180, s[60:63], 0 offen offset:0 nt", ";;#ASMEND"]
WAIT = [";;#ASMSTART", "s_waitcnt vmcnt(1)", ";;#ASMEND"]


def body(between, tail=(), load=LOAD):
    """A step loop: wait, use, load, piece, back edge -- `between` sits between the load and the next wait."""
    return ([".LBB0_1:"] + WAIT + ["v_fma_f32 v4, v8, v0, v9", "buffer_store_dwordx4 v[4:7], v180, s[60:63], 0 offen nt"] + list(load) +
            PIECE + list(between) + ["s_cmp_lg_u32 s4, 0", "s_cbranch_scc1 .LBB0_1", "; %bb.2:"] + list(tail) + ["s_endpgm"])


def errors(lines):
    return chk.check("k", VOL, lines)[0]


def test_checker_accepts_the_intended_shape():
    errs, ndma, nwait, (_, _, hidden) = chk.check("k", VOL, body([]))
    assert errs == [] and ndma == 1 and nwait == 1 and hidden == 1


@pytest.mark.parametrize("insn", ["v_mov_b32_e32 v10, v2", "v_mov_b64_e32 v[10:11], v[0:1]", "v_add_f32_e32 v3, v3, v3",
                                  "scratch_store_dwordx4 off, v[0:3], off"])
def test_checker_reports_a_touch_of_the_hidden_registers(insn):
    errs = errors(body([insn]))
    assert any("names its registers before a counted wait" in e for e in errs), errs


def test_checker_follows_the_exit_path_to_the_last_wait():
    # behind the loop the last unit is used without a wait: reported; with the drain in front of it: accepted
    use = ["v_fma_f32 v4, v8, v0, v9"]
    assert any("names its registers" in e for e in errors(body([], tail=use)))
    assert errors(body([], tail=[";;#ASMSTART", "s_waitcnt vmcnt(0)", ";;#ASMEND"] + use)) == []


def test_checker_reports_a_compiler_wait_inside_the_loop():
    errs = errors(body(["s_waitcnt vmcnt(0)"]))
    assert any("compiler-placed" in e for e in errs), errs
    assert errors(body([], tail=["s_waitcnt vmcnt(0)"])) == []          # (outside the loops it is harmless)
    assert errors(body(["s_waitcnt lgkmcnt(0)"])) == []                 # (the LDS / scalar queue is the compiler's)


def test_checker_reports_a_stale_volume_check():
    builtin = body([], load=["buffer_load_dwordx4 v[0:3], v180, s[60:63], 0 offen nt"])     # (not in an assembly block)
    assert any("the check is stale" in e for e in errors(builtin))


def test_volume_carriers_of_the_gfx950_build_pass():
    text = chk.assemble()
    seen = {}
    for name, p, lines in chk.kernels(text):
        if not (p["vol"] and p["ride"] > 0):
            continue
        errs, ndma, nwait, (_, _, hidden) = chk.check(name, p, lines)
        assert errs == [], (p, errs[:5])
        assert ndma > 0 and nwait > 0 and hidden >= 2, (p, ndma, nwait, hidden)      # (the set-up's load and the loop's)
        seen[(p["mode"], p["tile"], p["fullw"])] = hidden
    # plain 16 x 32 tiles, full-width planes, 10 x 40 tiles, rolling strips: each with and without the input transform
    assert set(seen) == {(m, t, f) for m in (0, 1) for t, f in ((0, 0), (0, 1), (1, 0), (2, 0))}, sorted(seen)
