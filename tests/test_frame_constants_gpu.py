"""Frame constants built once per frame on the host: the EPF's inverse-sigma plane, which the fused restoration kernel now loads, and
the persistent IDCT launch's dequantisation tables (tests/test_frame_constants_cpu.py holds the host builders to the formulas).

Here: the plane as it lies in device memory against the float32 formula; every launch form that reads it -- private raster planes,
pooled cell-tiled planes of contexts that share a stream, the batch launch, the split three-iteration pair, a quantising sink, the
form that keeps the plain divisions, jxl_stage_restore_fused on caller planes -- bit for bit against the oracle, with
jxl_debug_last_restore_launches naming the promised instantiation; a context that runs frame A, then a frame B in which every input
of the constants differs, then A again (a stale plane or table would show); and the IDCT tables' fall-backs (coefficients beyond
+-64, multipliers beyond 255) on 64x64 frames of one transform type each, single launch and batch launch."""
import ctypes as C

import numpy as np
import pytest

import restore_variants as rv
import switch_cases as sc
from conftest import assert_bits_equal
from jxlatte_amd import abi, host, synth
from test_frame_constants_cpu import inv_sigma_np, planted_maps

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN_BIT = 512
PLAIN_ROW = rv.Row("NONE", "F32", "SK_PLAIN", False)
RGB8_ROW = rv.Row("SRGB", "RGB8", "SK_SRGB_RGB8", True)
SIZES = [rv.MAIN, (136, 72), rv.ALL_EDGE]  # 264x112: 5x4 tiles, interior and ragged last ones; 72x40: edge tiles only


@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


def _read_plane(ctx, bh, bw):
    fn = ctx.lib.jxl_debug_read_inv_sigma
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]
    out = np.full((bh, bw), np.nan, np.float32)
    assert fn(ctx.h, out.ctypes.data, out.size) == out.size
    return out


def _with_maps(frame, hf_mul=None, sharpness=None):
    """a copy of a one-LF-group synth frame with other cell maps"""
    assert len(frame["lfgroups"]) == 1
    g = dict(frame["lfgroups"][0])
    f2 = dict(frame)
    if hf_mul is not None:
        g["hf_mul"] = np.ascontiguousarray(hf_mul, np.int32)
        f2["hf_mul"] = g["hf_mul"]
    if sharpness is not None:
        g["sharpness"] = np.ascontiguousarray(sharpness, np.int32)
        f2["sharpness"] = g["sharpness"]
    f2["lfgroups"] = [g]
    return f2


# ---- the plane in device memory ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [F(65536.0) / F(2500), F(3e-38)], ids=["default", "denormal-sigma"])
def test_inverse_sigma_plane_on_the_device(ctx, gs):
    w, h = 136, 72
    hf, sh = planted_maps(h // 8, w // 8, seed=21)
    frame = _with_maps(sc.with_params(rv.base_frame((w, h)), 15, global_scale_f=gs), hf, sh)
    fr = host.Frame.from_synth(ctx, frame)
    got = _read_plane(ctx, h // 8, w // 8)
    exp = inv_sigma_np(hf, sh, gs, list(fr.params.epf_sharp_lut))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.isinf(got).any() and (got < 0).any()


# ---- every launch form, against the oracle ----------------------------------------------------------------------------------------------
FORM_CASES = ([rv.Case(PLAIN_ROW, "raster", g, it, (s,)) for s in SIZES for g in (1, 0) for it in (0, 1, 2)] +   # private raster planes
              [rv.Case(PLAIN_ROW, "split3", 1, 3, (rv.SPLIT,)),
               rv.Case(RGB8_ROW, "raster", 1, 2, (rv.MAIN,)),
               rv.Case(PLAIN_ROW, "tiled", 1, 2, (rv.MAIN,)),      # contexts that share a stream: pooled cell-tiled planes
               rv.Case(PLAIN_ROW, "batch", 1, 2, rv.BATCH)])       # jxl_vardct_run_batch


@pytest.mark.parametrize("case", FORM_CASES, ids=rv.case_id)
def test_frame_parity(ctxs, case):
    problems = rv.check_case(case, ctxs, assert_bits_equal)
    assert not problems, "\n".join(problems)


def test_frame_parity_plain_divisions(ctxs, orc):
    """a negative border_sad_mul: the instantiation that keeps the plain divisions (and max alone for the weight) reads the plane too"""
    frame = sc.with_params(rv.base_frame(rv.MAIN), 15, gab=1, epf_iters=2, epf_border_sad_mul=F(-2.0) / F(3.0))
    cx = ctxs.own[0]
    got = host.Frame.from_synth(cx, frame).decodeFrame()
    assert host.lastRestoreLaunches(cx) == [rv.code("SK_PLAIN", 1, 2) | PLAIN_BIT]
    assert_bits_equal(got, orc.vardct_frame(frame), "negative border_sad_mul, frame path", any_nan=True)


def _stage_oracle(orc, planes, hf, sh, p):
    x = planes
    if p.gab:
        x = orc.gab(x, list(p.gab_w1), list(p.gab_w2))
    if p.epf_iters:
        sig = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        x = orc.epf(x, p.epf_iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale,
                    p.epf_border_sad_mul)
    return orc.xyb(x, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), p.intensity_target)


@pytest.mark.parametrize("w,h,iters", [(w, h, it) for (w, h) in SIZES for it in (1, 2)] + [rv.SPLIT + (3,)])
def test_stage_entry_point_on_caller_planes(ctx, orc, w, h, iters):
    """jxl_stage_restore_fused has no frame behind it: its plane comes from k_epf_sigma. Maps with sharpness 0 and multipliers 255,
    256 and 4096 among cells on both sides of the skip rule; three iterations run as the split pair, at its own size"""
    rng = np.random.default_rng(300 + w + h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    amp = np.array([0.004, 0.05, 0.03], np.float32)[:, None, None]
    planes = (amp * (np.stack([np.sin(xx / 17 + c) * np.cos(yy / 11 - c) for c in range(3)]) + 0.2 * rng.standard_normal((3, h, w)))).astype(np.float32)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    hf, sh = planted_maps(bh, bw, seed=w)
    hf = np.abs(hf)  # (a negative multiplier selects the other instantiation: the frame path's case above, and the diet tests)
    cy, cx = np.mgrid[0:bh, 0:bw]
    sh = np.where((cy + cx) % 2 == 0, np.maximum(sh, 4), sh).astype(np.int32)
    hf = np.where((cy + cx) % 2 == 0, np.minimum(hf, 3), hf).astype(np.int32)
    hf[2, :4], sh[2, :4] = [1, 255, 256, 4096], [7, 6, 5, 4]
    p = synth.default_params(bw * 8, bh * 8, epf_iters=iters, gab=True)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    want = [rv.code("SK_PLAIN", 1, 4), rv.code("SK_PLAIN", 0, 2)] if iters == 3 else [rv.code("SK_PLAIN", 1, iters)]
    assert host.lastRestoreLaunches(ctx) == want
    assert_bits_equal(got, _stage_oracle(orc, planes, hf, sh, p), "restoreFused %dx%d it%d" % (w, h, iters))


# ---- stale constants -----------------------------------------------------------------------------------------------------------------
def _f8(vals):
    return (C.c_float * 8)(*vals)


def _f3(vals):
    return (C.c_float * 3)(*vals)


def test_a_context_that_changes_every_input_of_the_constants(orc):
    """frame A, frame B (another epf_sharp_lut, global_scale_f, multiplier map, quant_bias, quant_bias_numerator and scale_factor), A
    again: each equals the oracle's decode, and A's three outputs -- two clean runs and the one after B -- are the same bytes"""
    from jxlatte_amd import _lib
    size = (136, 72)
    fa = sc.with_params(rv.base_frame(size), 15, gab=1, epf_iters=2)
    base_b = synth.make_vardct_frame(size[0], size[1], seed=4242, mix="default", aligned=False)  # other maps, other blocks
    lut_b = [F(0.05) + F(0.07) * F(i) for i in range(8)]
    fb = sc.with_params(base_b, 15, gab=1, epf_iters=2, epf_sharp_lut=_f8(lut_b), global_scale_f=F(19.5),
                        quant_bias=_f3([0.91, 0.88, 0.97]), quant_bias_numerator=F(0.21), scale_factor=_f3([17.25, 24.0, 30.5]))
    fb = _with_maps(fb, hf_mul=np.where(base_b["hf_mul"] % 3 == 0, base_b["hf_mul"] + 300, base_b["hf_mul"]))
    ea, eb = orc.vardct_frame(fa), orc.vardct_frame(fb)
    assert not np.array_equal(ea, eb)
    cx = _lib.Context(0)
    try:
        fr = host.Frame.from_synth(cx, fa)
        a1 = fr.decodeFrame()
        a2 = fr.decodeFrame()  # a clean re-run: nothing is rebuilt
        b1 = host.Frame.from_synth(cx, fb).decodeFrame()
        a3 = host.Frame.from_synth(cx, fa).decodeFrame()
    finally:
        cx.close()
    assert_bits_equal(a1, ea, "frame A")
    assert_bits_equal(b1, eb, "frame B behind A on the same context")
    assert a1.tobytes() == a2.tobytes(), "A run twice"
    assert a1.tobytes() == a3.tobytes(), "A again behind B"


# ---- the IDCT tables' fall-backs ------------------------------------------------------------------------------------------------------
KINDS = ["DCT8", "DCT16", "DCT32", "DCT32_16", "AFV1", "DCT64", "DCT64_32"]  # (the last: the 512-thread class, same prologue)
_idct = {}


def _idct_frame(kind):
    """64x64, one transform type, coefficients far beyond +-64 (|q| >= 64 leaves the table) and multipliers 1 .. 8 and 301 .. 308
    (beyond 255 the scale factor is divided in place)"""
    if kind not in _idct:
        f = synth.make_vardct_frame(64, 64, seed=700 + len(kind) + abi.TT_BY_NAME[kind], mix={kind: 1.0}, aligned=True, nonzero_p=0.3,
                                    coeff_scale=400.0)
        assert set(np.unique(f["block_types"])) == {abi.TT_BY_NAME[kind]}
        hf = f["hf_mul"].copy()
        if kind != "DCT64":  # (one block: its multiplier goes beyond 255 in every frame)
            hf = np.where(hf % 2 == 0, hf + 300, hf)
        else:
            hf = hf + 300
        f = _with_maps(sc.with_params(f, 15), hf_mul=hf)
        assert np.abs(f["coeff"]).max() > 64 and (np.abs(f["coeff"]) < 64).any() and hf.max() > 255
        from oracle import pyoracle
        exp = pyoracle.vardct_frame(f)
        exp.setflags(write=False)
        _idct[kind] = (f, exp)
    return _idct[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_idct_tables_single_launch(ctxs, kind):
    f, exp = _idct_frame(kind)
    assert_bits_equal(host.Frame.from_synth(ctxs.own[0], f).decodeFrame(), exp, kind)


@pytest.mark.parametrize("kinds", [("DCT8", "DCT16", "DCT32"), ("DCT32_16", "AFV1", "DCT64"), ("DCT64_32", "DCT64_32", "DCT8")], ids="+".join)
def test_idct_tables_batch_launch(ctxs, kinds):
    frs = [host.Frame.from_synth(cx, _idct_frame(k)[0]) for cx, k in zip(ctxs.own, kinds)]
    host.Frame.runBatch(frs)
    for fr, k in zip(frs, kinds):
        assert_bits_equal(fr.readOutput(), _idct_frame(k)[1], "batch: " + k)
