"""The layers that pin the direct fp32 convolution forms (csrc/mvsn_conv.hip: CV_FORMS, conv_select), shared by the
host-side selection test (test_boundary_cpu.py) and the GPU parity test (test_hip_parity.py).

The expected plans are written by hand from make_geom and the launch ladder of the code before the forms became one
table.  A 2-D 3x3 stride-1 layer gets 16-row tiles (NPT 8) when it has more than 8 rows and its dilation is at most 8 on
the LDS-DMA kernel (cols % 4 == 0, dilation <= 8) or at most 2 on the register-staged one, 8-row tiles (NPT 4)
otherwise; the staged rows are TY + 2 dil, the staged columns 32 + 2 dil.
  LDS-DMA: rows of dq = (32 + 2 * roundup4(dil)) / 4 16-byte pieces, ceil(rows * dq / 64) pieces per channel (IPC 4 up
    to four, 6 beyond), channel stride dCST = pieces * 256 + 16; LDS = two stages of [4 * dCST (twice with a residual
    tile)][1280 weight floats] + 80 floats.
  register-staged: elements = staged rows * columns per channel, SE 3 up to 768 of them, 6 beyond; channel stride
    CST = ceil(elements / 64) * 64 + 16; LDS = 4 * CST + taps * 128 weight floats + 128 floats.  The 3x3x3 (2 x 8 x 32
    tiles: 4 x 10 staged rows) and 5x5 stride-2 (19 staged rows) layers with cols % 4 == 0 stage rows of 40 / 72 floats
    as 16-byte groups (V4, SE 2), rows of 34 / 67 elements otherwise (SE 6).
  The 3 -> 32 5x5 stride-2 layer with cols % 8 == 0 has the head kernel: a static ring of 2 x 3 x (19 * 72 + 4) floats."""
from collections import namedtuple

# row indices of CV_FORMS
DMA8_4, DMA8_6, DMA4_4, DMA4_6, ST8_3, ST4_3, ST4_6, VOL_V4, VOL, S2_V4, S2, HEAD = range(12)
STAGED, DMA, HEAD_KIND = 0, 1, 2

Case = namedtuple("Case", "cin cout kd k stride dil depth rows cols mode plan")
# plan: (row, kind, NPT, SE or IPC, V4, CT, LDS bytes, tiles per sample), None: no direct form


def _dma_lds(pieces, mode):
    return (2 * (4 * (pieces * 256 + 16) * (2 if mode == 2 else 1) + 1280) + 80) * 4


def _staged_lds(runs, taps):
    return (4 * (runs * 64 + 16) + taps * 128 + 128) * 4


def _cases():
    out = []
    # 2-D 3x3 stride 1 on cols 36: the four LDS-DMA rows.  (rows, dil) -> row, NPT, IPC, pieces per channel, tiles
    for rows, dil, row, npt, ipc, pieces, tiles in ((8, 1, DMA4_4, 4, 4, 2, 1 * 2),      # 10 rows x 10 pieces = 100
                                                   (17, 1, DMA8_4, 8, 4, 3, 2 * 2),     # 18 x 10 = 180
                                                   (8, 8, DMA4_6, 4, 6, 5, 1 * 2),      # 24 x 12 = 288
                                                   (17, 8, DMA8_6, 8, 6, 6, 2 * 2)):    # 32 x 12 = 384
        for mode in (0, 1, 2):
            for cout in (32, 8):
                out.append(Case(32, cout, 1, 3, 1, dil, 1, rows, 36, mode,
                                (row, DMA, npt, ipc, 0, 2 if cout == 32 else 1, _dma_lds(pieces, mode), tiles)))
    # the same layers on cols 35: register-staged.  -> row, NPT, SE, 64-element runs per channel, tiles
    for rows, dil, row, npt, se, runs, tiles in ((8, 1, ST4_3, 4, 3, 6, 1 * 2),          # 10 x 34 = 340 elements
                                                 (17, 2, ST8_3, 8, 3, 12, 2 * 2),        # 20 x 36 = 720
                                                 (17, 4, ST4_3, 4, 3, 10, 3 * 2),        # 16 x 40 = 640
                                                 (17, 8, ST4_6, 4, 6, 18, 3 * 2)):       # 24 x 48 = 1152
        for mode in (0, 1, 2):
            for cout in (32, 8):
                out.append(Case(32, cout, 1, 3, 1, dil, 1, rows, 35, mode,
                                (row, STAGED, npt, se, 0, 2 if cout == 32 else 1, _staged_lds(runs, 9), tiles)))
    for mode in (0, 1, 2):   # dilation above the LDS-DMA limit: 8-row tiles, 26 x 50 = 1300 elements
        out.append(Case(32, 32, 1, 3, 1, 9, 1, 17, 36, mode, (ST4_6, STAGED, 4, 6, 0, 2, _staged_lds(21, 9), 3 * 2)))
    out.append(Case(32, 32, 1, 3, 1, 11, 1, 17, 36, 0, None))      # 30 x 54 = 1620 elements: more than 6 per thread
    out.append(Case(32, 32, 1, 7, 1, 1, 1, 17, 36, 0, None))
    for mode in (0, 1):      # 3x3x3 on 3 x 9 planes: 2 x 2 x 2 tiles; 40 x 40 floats / 40 x 34 elements per channel
        out.append(Case(32, 32, 3, 3, 1, 1, 3, 9, 36, mode, (VOL_V4, STAGED, 8, 2, 1, 2, _staged_lds(25, 27), 8)))
        out.append(Case(32, 32, 3, 3, 1, 1, 3, 9, 35, mode, (VOL, STAGED, 8, 6, 0, 2, _staged_lds(22, 27), 8)))
    # 5x5 stride 2 on 17 rows: 9 x 18 outputs, 2 x 1 tiles; 19 x 72 floats / 19 x 67 elements per channel
    out.append(Case(32, 32, 1, 5, 2, 1, 1, 17, 36, 0, (S2_V4, STAGED, 4, 2, 1, 2, _staged_lds(22, 25), 2)))
    out.append(Case(32, 32, 1, 5, 2, 1, 1, 17, 35, 0, (S2, STAGED, 4, 6, 0, 2, _staged_lds(20, 25), 2)))
    out.append(Case(3, 32, 1, 5, 2, 1, 1, 17, 72, 0, (HEAD, HEAD_KIND, 4, 0, 0, 2, 2 * 3 * (19 * 72 + 4) * 4, 2 * 2)))
    out.append(Case(3, 32, 1, 5, 2, 1, 1, 17, 36, 0, (S2_V4, STAGED, 4, 2, 1, 2, _staged_lds(22, 25), 2)))
    return out


CASES = _cases()
# a zero-padded last chunk of input channels, on the GPU only
PADDED_CHUNK = Case(35, 32, 1, 3, 1, 1, 1, 17, 36, 0, (DMA8_4, DMA, 8, 4, 0, 2, _dma_lds(3, 0), 2 * 2))


def case_id(c):
    return "%dto%d-k%d%s-s%d-d%d-%s%dx%d-m%d" % (c.cin, c.cout, c.k, "x3" if c.kd == 3 else "", c.stride, c.dil,
                                                 "%dx" % c.depth if c.kd == 3 else "", c.rows, c.cols, c.mode)


def plan(lib, native, c, n=1):
    """mvsn_debug_conv_plan's report for the case: (row, kind, NPT, SE / IPC, V4, CT, LDS bytes, tiles) and the number
    of rows in the table; (None, 0) where no direct form runs the layer."""
    import ctypes
    d = native.ConvDesc(n, c.cin, c.cout, c.depth, c.rows, c.cols, c.kd, c.k, c.k, c.stride, c.dil, native.CONV_FP32)
    out = (ctypes.c_int * 8)()
    nrows = lib.mvsn_debug_conv_plan(ctypes.byref(d), c.mode, ctypes.byref(out))
    return (tuple(out) if nrows else None), nrows
