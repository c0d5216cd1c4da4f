"""The instantiations of the fused restoration kernel (jxlatte_amd/csrc/restore_fused_body.h) and the cases that run each of them.

Per output sink kind (restore_sink.h, enum SinkKind) the kernel template is compiled 22 times: single launch on raster planes
(Gaborish on / off x 0..3 EPF iterations), single launch on cell-tiled pooled planes (x 0..2), batch launch (x 0..3); the float sink
has ITERS = 4 besides, the first half of a split three-iteration run. This module holds the geometry of those instantiations
restated as plain numbers, the table of (transfer, out_format) rows that lead into a sink, the launch forms, and the runner both
tests/test_restore_variants_gpu.py and its child process (tests/switch_cases.py, JXL_EPF3_SPLIT=0) go through. It holds no test;
importing it needs neither the device library nor a GPU. tests/test_restore_variants_cpu.py keeps table and geometry honest."""
import collections

# ---- geometry: Geo<GAB, ITERS> of restore_fused_body.h ----------------------------------------------------------------------------
# ITERS -> (output tile width, height, halo without Gaborish); Gaborish adds RG = 1 to the halo. 4 = the 13-tap iteration alone.
_GEO = {0: (64, 32, 0), 1: (64, 32, 2), 2: (62, 30, 3), 3: (58, 26, 6), 4: (64, 64, 3)}


def geo(gab, iters):
    """-> (OW, OH, RT): output tile and input halo"""
    ow, oh, re = _GEO[iters]
    return ow, oh, re + (1 if gab else 0)


def tile_grid(w, h, gab, iters):
    ow, oh, _ = geo(gab, iters)
    return (w + ow - 1) // ow, (h + oh - 1) // oh


def is_interior(w, h, gab, iters, i, j):
    """the rule of restore_fused_body.h (tc.edge): the input tile of output tile (i, j) lies inside the frame"""
    ow, oh, rt = geo(gab, iters)
    return i * ow - rt >= 0 and j * oh - rt >= 0 and (i + 1) * ow + rt <= w and (j + 1) * oh + rt <= h


def interior_tiles(w, h, gab, iters):
    tx, ty = tile_grid(w, h, gab, iters)
    return [(i, j) for j in range(ty) for i in range(tx) if is_interior(w, h, gab, iters, i, j)]


def ragged(w, h, gab, iters):
    """the last tile column and the last tile row are both cut by the frame edge"""
    ow, oh, _ = geo(gab, iters)
    return w % ow != 0 and h % oh != 0


def launched_workgroups(n_tiles):
    return (n_tiles + 7) // 8 * 8  # launch_tph / launch_batch_t round the grid up for the XCD remap


# ---- what jxl_debug_last_restore_launches reports ---------------------------------------------------------------------------------
SINK_KINDS = {"SK_PLAIN": 0, "SK_GENERIC": 1, "SK_PQ_U16": 2, "SK_PQ_RGB16": 3, "SK_SRGB_RGB8": 4, "SK_SRGB_RGB16": 5}
COMPILE_TIME_KINDS = ("SK_PQ_U16", "SK_PQ_RGB16", "SK_SRGB_RGB8", "SK_SRGB_RGB16")
TILED_BIT, BATCH_BIT = 128, 256


def code(kind, gab, iters, tiled=False, batch=False):
    """restore_fused_variant() | the hook's two bits"""
    return (64 if gab else 0) | (iters & 7) << 3 | SINK_KINDS[kind] | (TILED_BIT if tiled else 0) | (BATCH_BIT if batch else 0)


def describe(c):
    kind = [k for k, v in SINK_KINDS.items() if v == (c & 7)]
    return "%s gab %d iters %d%s%s" % (kind[0] if kind else "kind %d" % (c & 7), c >> 6 & 1, c >> 3 & 7, " tiled" if c & TILED_BIT else "",
                                      " batch" if c & BATCH_BIT else "")


# ---- the rows: one per way into a sink ---------------------------------------------------------------------------------------------
TRANSFERS = {"NONE": 0, "PQ": 1, "SRGB": 2, "PQ_EXACT": 3}           # JXL_TRANSFER_* of include/jxlatte_amd.h
OUT_FORMATS = {"F32": 0, "U16": 1, "U8": 2, "RGB8": 3, "RGB16": 4}    # JXL_OUT_*
MAX_VALUE = {"F32": 0, "U16": 65535, "U8": 255, "RGB8": 255, "RGB16": 65535}
ELEM = {"F32": 4, "U16": 2, "U8": 1, "RGB8": 1, "RGB16": 2}
INTERLEAVED = ("RGB8", "RGB16")


def sink_kind(transfer, fmt):
    """sink_kind_of (restore_sink.h) restated from its four conditions, for a default build and context (every table there).
    JXL_TRANSFER_PQ_EXACT reaches the kernel as PQ without the PQ table (fill_restore_params), so it stays generic."""
    mx, el, il = MAX_VALUE[fmt], ELEM[fmt], fmt in INTERLEAVED
    if transfer == "NONE" and mx == 0:
        return "SK_PLAIN"
    if transfer == "PQ" and mx == 65535 and el == 2:
        return "SK_PQ_RGB16" if il else "SK_PQ_U16"
    if transfer == "SRGB" and mx == 255 and el == 1 and il:
        return "SK_SRGB_RGB8"
    if transfer == "SRGB" and mx == 65535 and el == 2 and il:
        return "SK_SRGB_RGB16"
    return "SK_GENERIC"


Row = collections.namedtuple("Row", "transfer fmt kind full")
# (transfer, out_format, the kind sink_kind_of must select, full = every launch form; else the basic form and one batch)
ROWS = (
    # the four kinds fixed at compile time (k_restore_fused_q.hip)
    Row("PQ", "U16", "SK_PQ_U16", True),
    Row("PQ", "RGB16", "SK_PQ_RGB16", True),
    Row("SRGB", "RGB8", "SK_SRGB_RGB8", True),
    Row("SRGB", "RGB16", "SK_SRGB_RGB16", True),
    # the run-time-generic sink, integer output
    Row("PQ", "U8", "SK_GENERIC", False),      # fp_pq8
    Row("PQ", "RGB8", "SK_GENERIC", False),    # fp_pq8, interleaved bytes
    Row("SRGB", "U8", "SK_GENERIC", False),    # fp_srgb8, planar
    Row("SRGB", "U16", "SK_GENERIC", True),    # fp_srgb16, planar
    Row("NONE", "U8", "SK_GENERIC", False),    # the cast alone
    Row("NONE", "U16", "SK_GENERIC", False),
    Row("NONE", "RGB8", "SK_GENERIC", False),
    Row("NONE", "RGB16", "SK_GENERIC", True),
    Row("PQ_EXACT", "U16", "SK_GENERIC", False),  # the double-precision PQ + the cast
    Row("PQ_EXACT", "U8", "SK_GENERIC", False),
    Row("PQ_EXACT", "RGB8", "SK_GENERIC", False),
    Row("PQ_EXACT", "RGB16", "SK_GENERIC", False),
    # the run-time-generic sink, float output behind a transfer function (the tail of sink_store_k)
    Row("PQ", "F32", "SK_GENERIC", True),
    Row("SRGB", "F32", "SK_GENERIC", False),
    Row("PQ_EXACT", "F32", "SK_GENERIC", False),
    # float planes: covered in depth elsewhere (test_restore_tiles_gpu.py, *_ref64_gpu.py, test_tiled_plane_a_gpu.py); here for the hook
    Row("NONE", "F32", "SK_PLAIN", False),
)


def row_id(row):
    return "%s-%s" % (row.transfer, row.fmt)


# ---- sizes and launch forms ---------------------------------------------------------------------------------------------------------
MAIN = (264, 112)       # interior tile, ragged last tiles, tile count no multiple of 8: ITERS 0, 1, 2 and the single-launch ITERS 3
SPLIT = (264, 136)      # the same for both launches of the split three-iteration form (64x64 first, 62x30 second)
ALL_EDGE = (72, 40)     # no interior tile at any variant that has a halo
BATCH = (MAIN, (136, 72), ALL_EDGE)  # one batch launch: the grid is sized by the first, the others' surplus workgroups leave
SEEDS = {MAIN: 811, SPLIT: 812, (136, 72): 813, ALL_EDGE: 814}

# form -> needs the child process (JXL_EPF3_SPLIT=0 is read once per process)
FORMS = {"raster": False, "tiled": False, "split3": False, "batch": False, "single3": True, "batch3": True}

Case = collections.namedtuple("Case", "row form gab iters sizes")


def case_id(c):
    return "%s %s gab %d epf %d %s" % (row_id(c.row), c.form, c.gab, c.iters, "+".join("%dx%d" % s for s in c.sizes))


def cases_of(row, form):
    """the cases of one row in one launch form, in a fixed order"""
    out = []
    if form == "raster":
        if row.full:
            out = [Case(row, form, g, it, (s,)) for s in (MAIN, ALL_EDGE) for g in (1, 0) for it in (0, 1, 2)]
        else:
            out = [Case(row, form, 1, 2, (MAIN,))]
    elif form == "tiled" and row.full:
        out = [Case(row, form, g, it, (MAIN,)) for g in (1, 0) for it in (0, 1, 2)]
    elif form == "split3" and row.full:
        out = [Case(row, form, g, 3, (SPLIT,)) for g in (1, 0)]
    elif form == "batch":
        out = [Case(row, form, g, it, BATCH) for g in (1, 0) for it in (0, 1, 2)] if row.full else [Case(row, form, 1, 2, BATCH)]
    elif form == "single3" and row.full:
        out = [Case(row, form, g, 3, (MAIN,)) for g in (1, 0)]
    elif form == "batch3" and row.full:
        out = [Case(row, form, g, 3, BATCH) for g in (1, 0)]
    return out


def all_cases(child=None):
    """every case; child = True / False: those that need / do not need the child process"""
    return [c for row in ROWS for form, in_child in FORMS.items() if child is None or in_child == child for c in cases_of(row, form)]


def expected_launches(c):
    """the codes jxl_debug_last_restore_launches must report on every context of the case"""
    k = c.row.kind
    if c.form == "split3":  # Gaborish + the 13-tap iteration into float planes, then two iterations without Gaborish into the sink
        return [code("SK_PLAIN", c.gab, 4), code(k, 0, 2)]
    return [code(k, c.gab, c.iters, tiled=c.form == "tiled", batch=c.form in ("batch", "batch3"))]


def promised(child=None):
    """the set of instantiations the table runs"""
    return {x for c in all_cases(child) for x in expected_launches(c)}


def inventory(kind):
    """the 22 instantiations of one sink kind, as hook codes"""
    return ({code(kind, g, it) for g in (1, 0) for it in (0, 1, 2, 3)} | {code(kind, g, it, tiled=True) for g in (1, 0) for it in (0, 1, 2)} |
            {code(kind, g, it, batch=True) for g in (1, 0) for it in (0, 1, 2, 3)})


# ---- the runner (device and oracle; imported lazily) ----------------------------------------------------------------------------------
_frames = {}
_oracle = {}


def base_frame(size):
    """the synthetic frame of a size: default mix (DCT64 and smaller: the 256-thread IDCT launch alone, so that pooled planes are
    cell-tiled), seeded, unaligned tiling. Header fields are set per case (switch_cases.with_params)."""
    from jxlatte_amd import synth
    if size not in _frames:
        _frames[size] = synth.make_vardct_frame(size[0], size[1], seed=SEEDS[size], mix="default", aligned=False)
    return _frames[size]


def frame_of(c, size, transfer=None, fmt=None):
    import switch_cases as sc
    transfer = c.row.transfer if transfer is None else transfer
    fmt = c.row.fmt if fmt is None else fmt
    stages = 15 if (transfer, fmt) == ("NONE", "F32") else 31
    return sc.with_params(base_frame(size), stages, gab=c.gab, epf_iters=c.iters, transfer=TRANSFERS[transfer], out_format=OUT_FORMATS[fmt])


def oracle_of(c, size):
    """the oracle's decode of the case's frame at `size`: orc.vardct_frame of the frame itself, [3][H][W], int32 for the integer
    formats (the interleaved formats hold the same samples). The oracle has no form of its own for JXL_TRANSFER_PQ_EXACT -- the
    reference knows one PQ, of which _EXACT is the device's double-precision evaluation --: those rows are held to the frame with
    JXL_TRANSFER_PQ. Made once per (size, Gaborish, iterations, transfer, max value) and never written to."""
    from oracle import pyoracle as orc
    tf = "PQ" if c.row.transfer == "PQ_EXACT" else c.row.transfer
    key = (size, c.gab, c.iters, tf, MAX_VALUE[c.row.fmt])
    if key not in _oracle:
        fmt = {0: "F32", 255: "U8", 65535: "U16"}[MAX_VALUE[c.row.fmt]]
        exp = orc.vardct_frame(frame_of(c, size, tf, fmt))
        exp.setflags(write=False)
        _oracle[key] = exp
    return _oracle[key]


def last_launches(ctx):
    """jxl_debug_last_restore_launches: the codes of the fused restoration launches of the context's last run"""
    from jxlatte_amd import host
    return host.lastRestoreLaunches(ctx)


def last_tiled(ctx):
    import ctypes as C
    fn = ctx.lib.jxl_debug_last_plane_a_tiled
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return fn(ctx.h)


class Contexts:
    """the contexts the launch forms need: three with streams of their own (raster planes; the batch), and two on the stream of a
    third that runs nothing, whose IDCT output goes to the stream's pooled, cell-tiled planes (as tests/test_tiled_plane_a_gpu.py)"""

    def __init__(self):
        from jxlatte_amd import _lib
        self.own = [_lib.Context(0) for _ in range(3)]
        self.holder = _lib.Context(0)
        self.pooled = [_lib.Context(0) for _ in range(2)]
        for c in self.pooled:
            c.call("jxl_ctx_set_stream", self.holder.stream)

    def close(self):
        for c in self.pooled + [self.holder] + self.own:
            c.close()


def run_case(c, ctxs):
    """decode the case's frames in its launch form -> [(what, context, frame, device result)], one per context that ran"""
    from jxlatte_amd import host
    if c.form in ("batch", "batch3"):
        frs = [host.Frame.from_synth(cx, frame_of(c, s)) for cx, s in zip(ctxs.own, c.sizes)]
        host.Frame.runBatch(frs)
        return [("%s frame %d" % (case_id(c), i), cx, s, fr.readOutput()) for i, (cx, s, fr) in enumerate(zip(ctxs.own, c.sizes, frs))]
    if c.form == "tiled":
        frs = [host.Frame.from_synth(cx, frame_of(c, c.sizes[0])) for cx in ctxs.pooled]
        for fr in frs:
            fr.run()
        return [("%s context %d" % (case_id(c), i), cx, c.sizes[0], fr.readOutput()) for i, (cx, fr) in enumerate(zip(ctxs.pooled, frs))]
    fr = host.Frame.from_synth(ctxs.own[0], frame_of(c, c.sizes[0]))
    return [(case_id(c), ctxs.own[0], c.sizes[0], fr.decodeFrame())]


def check_case(c, ctxs, check, seen=None):
    """run the case, hold every result to the oracle through check(got, expected, what), and the hook's report to the table's;
    -> the problems found with the launches (a case that fell to another path is one), as strings"""
    import switch_cases as sc
    problems = []
    want = expected_launches(c)
    for what, cx, size, got in run_case(c, ctxs):
        launches = last_launches(cx)
        if seen is not None:
            seen.update(launches)
        if launches != want:
            problems.append("%s: ran [%s], the table promises [%s]" % (what, "; ".join(describe(x) for x in launches) or "no fused launch",
                                                                       "; ".join(describe(x) for x in want)))
        if last_tiled(cx) != (1 if c.form == "tiled" else 0):
            problems.append("%s: jxl_debug_last_plane_a_tiled = %d" % (what, last_tiled(cx)))
        if c.row.fmt == "F32" and c.row.transfer != "NONE":
            check_float_transfer(c, cx, size, got, what, check)
        else:
            check(sc.planar(got), oracle_of(c, size), what + ": against the oracle")
    return problems


# share of the floats that may differ from the oracle's by one ulp (none by more): the bars of tests/test_stages_gpu.py --
# test_transfer_within_one_ulp for the tabulated PQ and for sRGB, test_transfer_pq_exact_form for the double-precision PQ
FLOAT_BAR = {"PQ": 0.05, "SRGB": 1e-3, "PQ_EXACT": 1e-4}


def ulp_diff(a, b):
    import numpy as np
    a = a.view(np.int32).astype(np.int64)
    b = b.view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def check_float_transfer(c, cx, size, got, what, check):
    """float output behind a transfer function: bit-identical to jxl_stage_transfer applied to the same context's float-plane decode
    of the frame (both evaluate sample_ops.h's curve); against the oracle NaNs where it has NaNs (out-of-gamut samples through PQ),
    elsewhere within one ulp, and no more than FLOAT_BAR of the samples differing"""
    import numpy as np
    from jxlatte_amd import host
    planes = host.Frame.from_synth(cx, frame_of(c, size, "NONE", "F32")).decodeFrame()
    check(got, host.transfer(cx, planes, TRANSFERS[c.row.transfer]), what + ": against jxl_stage_transfer of the float-plane decode")
    exp = oracle_of(c, size)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs elsewhere than the oracle's"
    d = ulp_diff(got[~nan], exp[~nan])
    share = float((d != 0).mean())
    print("%s: against the oracle max %d ulp, share %.3e" % (what, int(d.max()), share))
    assert d.max() <= 1 and share < FLOAT_BAR[c.row.transfer], (what, int(d.max()), share)
