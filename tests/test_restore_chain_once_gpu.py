"""EPF pair chains formed once per tile (restore_fused_body.h, epf_stage): in the 5-tap iterations a thread forms only the chains of
its 4 x 1 patch to the east and to the south; the west and north chains come from the threads that formed them -- by DPP inside a
4 x 4 block of patches, through the handoff area in LDS across blocks and waves, and from the one-wave edge pass for the window's top
row and left column. Every result here is held bit for bit to the oracle.

What produces and what consumes a chain depends on where a patch lies in the 64 x 32 window, and what the chains are formed from
depends on the frame edge (mirrored rows and columns of the LDS image), so the sizes put every kind on both:

  planes of any size through host.restoreFused (raster planes, float planes out; the oracle's stage functions as in
  tests/test_restore_tiles_gpu.py):
    8x8, 16x24, 62x30   one tile alone, the window mostly / partly outside the frame
    126x62              two tile rows and two tile columns (62 x 30 output tiles)
    63x31, 64x33, 65x35 1 / 2 / 3 columns and 1 / 3 / 5 rows in the last tile of two iterations
    65x33, 66x35, 67x37 the same remnants behind the 64 x 32 tiles of one iteration
    190x95              interior tiles (the path without coordinate clamps), all their neighbours edge tiles
  frames (synth.make_vardct_frame: multiples of 8, so remnants are even) against oracle.pyoracle.vardct_frame, on the three entries
  -- one frame on pooled, cell-tiled planes; one frame on a context's private raster planes; jxl_vardct_run_batch of two frames --
  into the three sinks float planes, RGB8 (sRGB) and u16 (PQ):
    8x8, 16x24, 56x24   one tile alone
    120x56              2 x 2 tiles
    64x32, 128x64       2 / 4 columns and rows in the last tiles
    192x96              with interior tiles

EPF iterations 1 and 2, Gaborish on and off, and two cell maps: one with skipped cells (sharpness 0: inverse sigma +inf, besides
finite ones above 1 / 0.3f) and one in which the filter runs on every cell.
"""
import numpy as np
import pytest

import restore_variants as rv
import switch_cases as sc
from conftest import assert_bits_equal
from jxlatte_amd import host, synth

pytestmark = pytest.mark.gpu

PLANE_SIZES = [(8, 8), (16, 24), (62, 30), (126, 62), (63, 31), (64, 33), (65, 35), (65, 33), (66, 35), (67, 37), (190, 95)]
FRAME_SIZES = [(8, 8), (16, 24), (56, 24), (120, 56), (64, 32), (128, 64), (192, 96)]
BATCH_SIZES = ((120, 56), (64, 32))
MAPS = ["skipped", "none"]
SINKS = [("NONE", "F32"), ("SRGB", "RGB8"), ("PQ", "U16")]
LIMIT = np.float32(1.0 / 0.3)


def _maps(kind, hf, sh):
    """(hf_mul, sharpness) of a map kind from random maps: hf_mul stays a function of the given one (constant inside a varblock)"""
    if kind == "skipped":
        return hf.copy(), sh.copy()
    return (1 + hf % 3).astype(np.int32), (4 + sh % 4).astype(np.int32)


def _check_maps(orc, kind, hf, sh, p):
    s = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
    skip = np.isnan(s) | (s > LIMIT)
    if kind == "none":
        assert not skip.any()
    elif s.size >= 12:
        assert skip.any() and not skip.all()


# ---- caller planes of any size (raster) -------------------------------------------------------------------------------------------------
def _case(w, h):
    """smooth planes with a little noise in the range of XYB samples (weights neither all 0 nor all 1), a different cell value per cell"""
    rng = np.random.default_rng(9100 + 7 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    amp = np.array([0.004, 0.05, 0.03], np.float32)[:, None, None]
    base = np.stack([np.sin(x / 23 + c) * np.cos(y / 17 - c) for c in range(3)])
    planes = (amp * (base + 0.15 * rng.standard_normal((3, h, w)))).astype(np.float32)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    return planes, rng.integers(1, 16, (bh, bw)).astype(np.int32), rng.integers(0, 8, (bh, bw)).astype(np.int32)


def _oracle_planes(orc, planes, hf, sh, p):
    x = planes
    if p.gab:
        x = orc.gab(x, list(p.gab_w1), list(p.gab_w2))
    sig = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
    x = orc.epf(x, p.epf_iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    return orc.xyb(x, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), p.intensity_target)


def test_the_filter_is_at_work_on_these_planes(orc):
    planes, hf, sh = _case(190, 95)
    p = synth.default_params(192, 96, epf_iters=2, gab=False, xyb=False)
    for kind in MAPS:
        h2, s2 = _maps(kind, hf, sh)
        _check_maps(orc, kind, h2, s2, p)
        sig = orc.epf_sigma(h2, s2, p.global_scale_f, list(p.epf_sharp_lut))
        e = orc.epf(planes, 2, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
        assert (e != planes).mean() > 1.0 / 3, kind
    assert p.epf_border_sad_mul != 1.0


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("w,h", PLANE_SIZES)
def test_planes(ctx, orc, w, h, iters, gab, kind):
    planes, hf, sh = _case(w, h)
    hf, sh = _maps(kind, hf, sh)
    p = synth.default_params((w + 7) // 8 * 8, (h + 7) // 8 * 8, epf_iters=iters, gab=gab)
    _check_maps(orc, kind, hf, sh, p)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    assert host.lastRestoreLaunches(ctx) == [rv.code("SK_PLAIN", gab, iters)]
    assert_bits_equal(got, _oracle_planes(orc, planes, hf, sh, p), "planes %dx%d it%d gab%d %s" % (w, h, iters, gab, kind))


# ---- frames: three entries x three sinks ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


_base, _expected = {}, {}


def _frame(size, kind, iters, gab, sink):
    if (size, kind) not in _base:
        base = synth.make_vardct_frame(size[0], size[1], seed=4300 + size[0] + 3 * size[1], mix="default", aligned=False)
        groups = []
        for g in base["lfgroups"]:
            hf, sh = _maps(kind, g["hf_mul"], g["sharpness"])
            groups.append(dict(g, hf_mul=np.ascontiguousarray(hf), sharpness=np.ascontiguousarray(sh)))
        _base[(size, kind)] = dict(base, lfgroups=groups)
    transfer, fmt = sink
    return sc.with_params(_base[(size, kind)], 15 if sink == SINKS[0] else 31, gab=1 if gab else 0, epf_iters=iters,
                          transfer=rv.TRANSFERS[transfer], out_format=rv.OUT_FORMATS[fmt])


def _frame_oracle(orc, size, kind, iters, gab, sink):
    """once per case, shared by the entries, never written to"""
    key = (size, kind, iters, gab, sink)
    if key not in _expected:
        exp = orc.vardct_frame(_frame(size, kind, iters, gab, sink))
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def _kind(sink):
    return rv.sink_kind(*sink)


@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("size", FRAME_SIZES)
def test_frames_pooled_and_private(ctxs, orc, size, iters, gab):
    for kind in MAPS:
        for sink in SINKS:
            f = _frame(size, kind, iters, gab, sink)
            for g in f["lfgroups"]:
                _check_maps(orc, kind, g["hf_mul"], g["sharpness"], f["params"])
            exp = _frame_oracle(orc, size, kind, iters, gab, sink)
            what = "%dx%d it%d gab%d %s %s" % (size + (iters, gab, kind, "-".join(sink)))
            # one frame on pooled planes (cell-tiled from one window upwards; below that whichever layout the frame path picks)
            cx = ctxs.pooled[0]
            fr = host.Frame.from_synth(cx, f)
            fr.run()
            got = fr.readOutput()
            ran = host.lastRestoreLaunches(cx)
            tiled = rv.last_tiled(cx) == 1
            assert ran == [rv.code(_kind(sink), gab, iters, tiled=tiled)], (what, [rv.describe(c) for c in ran])
            assert tiled or size[0] * size[1] < 64 * 32, what + ": pooled planes not cell-tiled"
            assert_bits_equal(sc.planar(got), exp, what + " pooled")
            # the same frame on a context with planes of its own (raster)
            cx = ctxs.own[0]
            got = host.Frame.from_synth(cx, f).decodeFrame()
            ran = host.lastRestoreLaunches(cx)
            assert ran == [rv.code(_kind(sink), gab, iters)], (what, [rv.describe(c) for c in ran])
            assert_bits_equal(sc.planar(got), exp, what + " private")


@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [1, 2])
def test_batch_of_two_frames(ctxs, orc, iters, gab):
    for kind in MAPS:
        for sink in SINKS:
            frs = [host.Frame.from_synth(cx, _frame(s, kind, iters, gab, sink)) for cx, s in zip(ctxs.own, BATCH_SIZES)]
            host.Frame.runBatch(frs)
            for cx, s, fr in zip(ctxs.own, BATCH_SIZES, frs):
                what = "batch %dx%d it%d gab%d %s %s" % (s + (iters, gab, kind, "-".join(sink)))
                got = fr.readOutput()
                ran = host.lastRestoreLaunches(cx)
                assert ran == [rv.code(_kind(sink), gab, iters, batch=True)], (what, [rv.describe(c) for c in ran])
                assert_bits_equal(sc.planar(got), _frame_oracle(orc, s, kind, iters, gab, sink), what)
