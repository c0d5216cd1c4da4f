"""Skipped EPF cells as zero weights, and the whole-piece tile load, of the fused restoration kernel (restore_fused_body.h).

The kernel's window load turns the inverse sigma of every cell the reference skips (Frame.java:608-612: NaN, or above 1 / 0.3f) into
+inf; on the fast-division path the weights of such a pixel are then exactly 0 and its quotient is its centre sample, without a
select. The select stays on the plain-division branch, where +-0, denormal, huge and non-finite samples send a whole wave. Every
case here is held bit for bit to the oracle, the way tests/test_restore_tiles_gpu.py compares, on two routes:

  * host.restoreFused on caller planes (raster input);
  * a synthetic frame on a context that shares its stream (pooled, cell-tiled planes: the whole-piece loader). The hook must report
    a cell-tiled launch (| 128) without the plain-division form (| 512) for one and two iterations; three iterations run as the split
    pair, which takes raster planes (restore_fused_takes_tiled), and must report exactly that pair.

Shapes: 264 x 112 -- interior tiles at origins 58, 120, 182 (both residues mod 4 of the straddling 16-byte piece) and ragged last
tiles -- and the all-edge 72 x 40. EPF iterations 1, 2, 3; Gaborish on and off. Cell maps:

  inf           every cell skipped through sigma = 0 (sharpness 0: inverse sigma +inf)
  finite        every cell skipped through a finite inverse sigma above 1 / 0.3f (sharpness 1, hf_mul 6..8 at global_scale 2500): the
                case that needs the +inf of the window load
  checkerboard  skipped and kept cells alternate, so that 4-pixel patches straddle both in both EPF stages

Samples can be planted on the raster route only (a frame's samples come out of its inverse transforms): one skipped cell of +0, -0,
a denormal, 2^95 and 2^-110 inside an ordinary frame, and frames of skipped cells with infinities and NaNs, Gaborish and XYB off, whose
output must be the input's bits.
"""
import numpy as np
import pytest

import restore_variants as rv
import switch_cases as sc
from conftest import assert_bits_equal
from jxlatte_amd import _lib, host, synth

pytestmark = pytest.mark.gpu

SHAPES = [(264, 112), (72, 40)]
MAPS = ["inf", "finite", "checkerboard"]
TILED_BIT, PLAIN_BIT = 128, 512
LIMIT = np.float32(1.0 / 0.3)


def _maps(kind, base_hf, rng_sh):
    """(hf_mul, sharpness) of a case from a per-block hf_mul map in 1..8 (kept constant inside a varblock) and a random sharpness map"""
    bh, bw = base_hf.shape
    cy, cx = np.mgrid[0:bh, 0:bw]
    if kind == "inf":
        return base_hf.copy(), np.zeros((bh, bw), np.int32)
    if kind == "finite":
        return (6 + base_hf % 3).astype(np.int32), np.ones((bh, bw), np.int32)
    assert kind == "checkerboard"
    return (1 + base_hf % 3).astype(np.int32), np.where((cy + cx) % 2 == 0, 0, 4 + rng_sh % 4).astype(np.int32)


def _planes(w, h):
    """smooth planes with a little noise in the range of XYB samples (as tests/test_restore_tiles_gpu.py): weights neither all 0 nor all 1"""
    rng = np.random.default_rng(4100 + 5 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    amp = np.array([0.004, 0.05, 0.03], np.float32)[:, None, None]
    base = np.stack([np.sin(x / 23 + c) * np.cos(y / 17 - c) for c in range(3)])
    planes = (amp * (base + 0.15 * rng.standard_normal((3, h, w)))).astype(np.float32)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    return planes, rng.integers(1, 9, (bh, bw)).astype(np.int32), rng.integers(0, 8, (bh, bw)).astype(np.int32)


def _params(w, h, iters, gab, xyb=True, border=None):
    p = synth.default_params((w + 7) // 8 * 8, (h + 7) // 8 * 8, epf_iters=iters, gab=gab, xyb=xyb)
    if border is not None:
        p.epf_border_sad_mul = border
    return p


def _inv_sigma(orc, hf, sh, p):
    return orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))


def _oracle_planes(orc, planes, hf, sh, p):
    x = planes
    if p.gab:
        x = orc.gab(x, list(p.gab_w1), list(p.gab_w2))
    if p.epf_iters:
        x = orc.epf(x, p.epf_iters, _inv_sigma(orc, hf, sh, p), 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale,
                    p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    if p.xyb:
        x = orc.xyb(x, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), p.intensity_target)
    return x


def _check_maps(orc, kind, hf, sh, p):
    """the maps are what the docstring says (printed by a failing case, asserted for every case)"""
    s = _inv_sigma(orc, hf, sh, p)
    if kind == "inf":
        assert np.isposinf(s).all()
    elif kind == "finite":
        assert np.isfinite(s).all() and (s > LIMIT).all()
    else:
        skip = (s > LIMIT) | np.isnan(s)
        assert (skip[:, :-1] != skip[:, 1:]).all() and (skip[:-1] != skip[1:]).all()


def test_the_maps_are_what_the_docstring_says(orc):
    for w, h in SHAPES:
        _, base_hf, rsh = _planes(w, h)
        for kind in MAPS:
            hf, sh = _maps(kind, base_hf, rsh)
            _check_maps(orc, kind, hf, sh, _params(w, h, 2, True))
    # the filter is at work on the kept cells of the checkerboard
    planes, base_hf, rsh = _planes(264, 112)
    hf, sh = _maps("checkerboard", base_hf, rsh)
    p = _params(264, 112, 2, False, xyb=False)
    assert (_oracle_planes(orc, planes, hf, sh, p) != planes).mean() > 0.2


# ---- caller planes (raster) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_planes(ctx, orc, w, h, iters, gab, kind):
    planes, base_hf, rsh = _planes(w, h)
    hf, sh = _maps(kind, base_hf, rsh)
    p = _params(w, h, iters, gab)
    _check_maps(orc, kind, hf, sh, p)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    ran = host.lastRestoreLaunches(ctx)
    assert ran and all(not (c & (TILED_BIT | PLAIN_BIT)) for c in ran), [rv.describe(c) for c in ran]
    assert_bits_equal(got, _oracle_planes(orc, planes, hf, sh, p), "planes %dx%d it%d gab%d %s" % (w, h, iters, gab, kind))


SPECIAL = np.array([0.0, -0.0, 3e-41, 2.0 ** 95, 2.0 ** -110], np.float32)


@pytest.mark.parametrize("gab,xyb", [(False, False), (True, True)])
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_one_skipped_cell_of_special_samples(ctx, orc, iters, gab, xyb):
    """cell (6, 12) -- pixels 96..103 x 48..55, inside the interior tile at (62, 30) -- is skipped and holds +0, -0, a denormal, 2^95 and
    2^-110 in all three channels; its neighbours are ordinary kept cells. The window test must send these waves to the plain
    divisions, whose select keeps the centre: without Gaborish and XYB the cell's output is the input's bits."""
    w, h = 264, 112
    planes, base_hf, rsh = _planes(w, h)
    hf, sh = (1 + base_hf % 3).astype(np.int32), (4 + rsh % 4).astype(np.int32)
    sh[6, 12] = 0
    planes[:, 48:56, 96:104] = SPECIAL[(np.arange(8)[:, None] * 3 + np.arange(8)[None, :]) % 5]
    p = _params(w, h, iters, gab, xyb=xyb)
    s = _inv_sigma(orc, hf, sh, p)
    assert np.isposinf(s[6, 12]) and (s <= LIMIT).sum() == s.size - 1
    got = host.restoreFused(ctx, planes, p, hf, sh)
    assert all(not (c & PLAIN_BIT) for c in host.lastRestoreLaunches(ctx))
    if not gab and not xyb:
        assert_bits_equal(got[:, 48:56, 96:104], planes[:, 48:56, 96:104], "the skipped cell, it%d" % iters)
    # (2^95 overflows in the XYB stage, and an invalid operation's NaN has another sign bit on the oracle's host)
    assert_bits_equal(got, _oracle_planes(orc, planes, hf, sh, p), "special cell it%d gab%d" % (iters, gab), any_nan=xyb)


@pytest.mark.parametrize("kind", ["inf", "finite"])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_skipped_frames_with_infinities_and_nans_come_out_as_they_went_in(ctx, w, h, iters, kind):
    """Gaborish and XYB off, every cell skipped: the output is the input bit for bit, NaN payloads included (so no oracle: Java leaves
    NaN patterns open)"""
    planes, base_hf, rsh = _planes(w, h)
    rng = np.random.default_rng(77 + w)
    bits = planes.view(np.uint32)
    for v in (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC12345, 0x7F800001):
        c, y, x = rng.integers(0, 3, 40), rng.integers(0, h, 40), rng.integers(0, w, 40)
        bits[c, y, x] = v
    bits[:, 0, 0] = 0x7FC00BAD      # a frame corner (mirrored taps), a tile's last column and the ragged patch column
    bits[:, h - 1, w - 1] = 0xFF800000
    bits[:, h // 2, 61:63] = 0x7FC00001
    hf, sh = _maps(kind, base_hf, rsh)
    p = _params(w, h, iters, False, xyb=False)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    assert_bits_equal(got, planes, "skipped %dx%d it%d %s" % (w, h, iters, kind))


def test_planes_negative_border_factor_keeps_the_plain_form(ctx, orc):
    w, h = 264, 112
    planes, base_hf, rsh = _planes(w, h)
    hf, sh = _maps("checkerboard", base_hf, rsh)
    p = _params(w, h, 2, True, border=-2.0 / 3.0)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    ran = host.lastRestoreLaunches(ctx)
    assert ran and all(c & PLAIN_BIT for c in ran), [rv.describe(c) for c in ran]
    assert_bits_equal(got, _oracle_planes(orc, planes, hf, sh, p), "negative border factor", any_nan=True)


def test_planes_repeat_byte_for_byte(ctx):
    """twice on one context, once on a fresh one: the pad columns of the LDS tile now receive data, and a result that depended on
    what they held would differ from run to run"""
    w, h = 264, 112
    planes, base_hf, rsh = _planes(w, h)
    hf, sh = _maps("checkerboard", base_hf, rsh)
    p = _params(w, h, 2, True)
    first = host.restoreFused(ctx, planes, p, hf, sh).tobytes()
    assert host.restoreFused(ctx, planes, p, hf, sh).tobytes() == first
    fresh = _lib.Context(0)
    try:
        assert host.restoreFused(fresh, planes, p, hf, sh).tobytes() == first
    finally:
        fresh.close()


# ---- frames on pooled, cell-tiled planes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


_frames, _expected = {}, {}


def _frame(size, kind, iters, gab, border=None):
    """the frame of tests/restore_variants.py at `size` with the case's cell maps (hf_mul stays constant inside a varblock) and header"""
    if (size, kind) not in _frames:
        base = rv.base_frame(size)
        groups = []
        for g in base["lfgroups"]:
            hf, sh = _maps(kind, g["hf_mul"], g["sharpness"])
            groups.append(dict(g, hf_mul=np.ascontiguousarray(hf), sharpness=np.ascontiguousarray(sh)))
        _frames[(size, kind)] = dict(base, lfgroups=groups)
    fields = dict(gab=1 if gab else 0, epf_iters=iters)
    if border is not None:
        fields["epf_border_sad_mul"] = border
    return sc.with_params(_frames[(size, kind)], 15, **fields)


def _frame_oracle(orc, size, kind, iters, gab, border=None):
    key = (size, kind, iters, gab, border)
    if key not in _expected:
        exp = orc.vardct_frame(_frame(size, kind, iters, gab, border))
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def _promised(ran, iters, gab, plain=False):
    bit = PLAIN_BIT if plain else 0
    if iters == 3:  # the split pair on raster planes
        return ran == [rv.code("SK_PLAIN", gab, 4) | bit, rv.code("SK_PLAIN", 0, 2) | bit]
    return ran == [rv.code("SK_PLAIN", gab, iters, tiled=True) | bit] and bool(ran[0] & TILED_BIT) and bool(ran[0] & PLAIN_BIT) == plain


def _run_frame(cx, f):
    fr = host.Frame.from_synth(cx, f)
    fr.run()
    return fr.readOutput()


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("size", SHAPES)
def test_frames(ctxs, orc, size, iters, gab, kind):
    f = _frame(size, kind, iters, gab)
    p = f["params"]
    for g in f["lfgroups"]:
        _check_maps(orc, kind, g["hf_mul"], g["sharpness"], p)
    cx = ctxs.pooled[0]
    got = _run_frame(cx, f)
    ran = host.lastRestoreLaunches(cx)
    assert _promised(ran, iters, gab), [rv.describe(c) for c in ran]
    assert_bits_equal(got, _frame_oracle(orc, size, kind, iters, gab), "frame %dx%d it%d gab%d %s" % (size + (iters, gab, kind)))


def test_frame_negative_border_factor_keeps_the_plain_form(ctxs, orc):
    size = (264, 112)
    cx = ctxs.pooled[0]
    got = _run_frame(cx, _frame(size, "checkerboard", 2, True, border=-2.0 / 3.0))
    ran = host.lastRestoreLaunches(cx)
    assert _promised(ran, 2, True, plain=True), [rv.describe(c) for c in ran]
    assert_bits_equal(got, _frame_oracle(orc, size, "checkerboard", 2, True, -2.0 / 3.0), "negative border factor", any_nan=True)


def test_frames_repeat_byte_for_byte(ctxs):
    size = (264, 112)
    f = _frame(size, "checkerboard", 2, True)
    cx = ctxs.pooled[0]
    first = _run_frame(cx, f).tobytes()
    assert _promised(host.lastRestoreLaunches(cx), 2, True)
    assert _run_frame(cx, f).tobytes() == first
    fresh = rv.Contexts()
    try:
        assert _run_frame(fresh.pooled[0], f).tobytes() == first
        assert _promised(host.lastRestoreLaunches(fresh.pooled[0]), 2, True)
    finally:
        fresh.close()
