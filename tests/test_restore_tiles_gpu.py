"""The fused restoration kernel's tile geometry against the oracle. Interior and edge tiles take two code paths (one
workgroup-uniform branch after Gaborish), so every layout of the 62 x 30 output tile and of the 8 x 8 sigma cells is held bit
for bit to the reference here.

Planes of any size reach the frame path's own launch through host.restoreFused (jxl_stage_restore_fused); the kernel itself takes
planes of at least 8 x 8, so the 1 x 1 and 7 x 9 cases check that the entry declines them and are restored by the stage kernels.
Plane sizes (W x H) around the tile and the cells:
  61x29, 62x30, 63x31: one tile, exactly one tile, one tile plus a one-pixel second tile;  124x60, 125x61: 2 x 2 tiles, exact and
  ragged;  190x95: the smallest size with interior tiles, all their neighbours edge tiles;  200x33: interior columns with both
  edge rows in adjacent tiles.
Every case: a different hf_mul / sharpness per 8 x 8 cell, with cells on both sides of the skip rule (inverse sigma above 1 / 0.3,
infinite ones included), border_sad_mul = 2 / 3.
"""
import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth

pytestmark = pytest.mark.gpu

SIZES = [(61, 29), (62, 30), (63, 31), (124, 60), (125, 61), (190, 95), (200, 33)]


def _case(w, h, seed=None):
    """smooth planes with a little noise, in the range of XYB samples -- neighbouring samples close enough for the EPF weights to
    be neither all 0 nor all 1 -- and cell maps with a different value per cell"""
    rng = np.random.default_rng(5000 + 7 * w + h if seed is None else seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    amp = np.array([0.004, 0.05, 0.03], np.float32)[:, None, None]
    base = np.stack([np.sin(x / 23 + c) * np.cos(y / 17 - c) for c in range(3)])
    planes = (amp * (base + 0.15 * rng.standard_normal((3, h, w)))).astype(np.float32)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    hf = rng.integers(1, 16, (bh, bw)).astype(np.int32)
    sh = rng.integers(0, 8, (bh, bw)).astype(np.int32)
    return planes, hf, sh


def _params(w, h, iters, gab):
    return synth.default_params((w + 7) // 8 * 8, (h + 7) // 8 * 8, epf_iters=iters, gab=gab)


_expected = {}


def _reference(orc, key, planes, hf, sh, p):
    """Gab -> EPF -> XYB by the oracle's stage functions, computed once per case"""
    if key not in _expected:
        x = planes
        if p.gab:
            x = orc.gab(x, list(p.gab_w1), list(p.gab_w2))
        if p.epf_iters:
            sig = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
            x = orc.epf(x, p.epf_iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale,
                        p.epf_border_sad_mul)
        _expected[key] = orc.xyb(x, list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias), p.intensity_target)
    return _expected[key]


def test_cases_have_skip_cells_and_a_border_factor(orc):
    """what the cases below rely on: cells on both sides of the skip rule in every size, a border factor != 1"""
    for w, h in SIZES:
        _, hf, sh = _case(w, h)
        p = _params(w, h, 2, True)
        s = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        assert (s > 1.0 / 0.3).any() and (s <= 1.0 / 0.3).any(), (w, h)
        assert len(np.unique(s)) >= min(8, s.size // 2), (w, h)
        assert p.epf_border_sad_mul != 1.0
    # the filter is at work on these planes: it changes a good part of the samples outside the skipped cells
    planes, hf, sh = _case(190, 95)
    s = orc.epf_sigma(hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
    e = orc.epf(planes, 2, s, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    assert (e != planes).mean() > 1.0 / 3


@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_restore_planes_f32(ctx, orc, w, h, iters, gab):
    """float planes out: exact"""
    planes, hf, sh = _case(w, h)
    p = _params(w, h, iters, gab)
    got = host.restoreFused(ctx, planes, p, hf, sh)
    assert_bits_equal(got, _reference(orc, (w, h, iters, gab), planes, hf, sh, p), "restore %dx%d it%d gab%d" % (w, h, iters, gab))


@pytest.mark.parametrize("gab", [True, False])
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 9)])
def test_planes_below_one_cell(ctx, orc, w, h, iters, gab):
    """the fused kernel takes no plane under 8 x 8 (its mirror fix-up assumes one reflection): the entry says so, and the stage
    kernels that the frame path falls back to restore such planes exactly"""
    planes, hf, sh = _case(w, h)
    p = _params(w, h, iters, gab)
    with pytest.raises(_lib.IllegalArgumentException):
        host.restoreFused(ctx, planes, p, hf, sh)
    x = planes
    if gab:
        x = host.performGabConvolution(ctx, x, list(p.gab_w1), list(p.gab_w2))
    if iters:
        sig = host.epfInverseSigma(ctx, hf, sh, p.global_scale_f, list(p.epf_sharp_lut))
        x = host.performEdgePreservingFilter(ctx, x, iters, sig, 0.0, list(p.epf_channel_scale), p.epf_pass0_sigma_scale,
                                             p.epf_pass2_sigma_scale, p.epf_border_sad_mul)
    m = host.OpsinInverseMatrix(list(p.opsin_matrix), list(p.opsin_bias), list(p.cbrt_opsin_bias))
    got = m.invertXYB(ctx, x, p.intensity_target)
    assert_bits_equal(got, _reference(orc, (w, h, iters, gab), planes, hf, sh, p), "stages %dx%d it%d gab%d" % (w, h, iters, gab))


@pytest.mark.parametrize("iters", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", [(64, 32), (128, 64), (192, 96), (248, 120)])
def test_restore_frames_u16_pq(ctx, orc, w, h, iters):
    """a quantised sink (PQ, 16 bits) through the frame path, by the rule of test_u16_pq_output_path: exact. Frame sizes are
    multiples of 8: a two-pixel second tile, ragged 3 x 3 tiles, interior tiles, and 248 x 120 = 4 x 4 exact tiles"""
    f = synth.make_vardct_frame(w, h, seed=700 + w + 3 * h, mix="default", epf_iters=iters, gab=True, transfer=abi.TRANSFER_PQ,
                                out_format=abi.OUT_U16, intensity_target=10000.0)
    got = host.Frame.from_synth(ctx, f).decodeFrame()
    assert got.dtype == np.uint16
    assert np.array_equal(got, orc.vardct_frame(f))


@pytest.mark.parametrize("iters,gab", [(2, True), (1, True), (3, True), (2, False)])
def test_interior_tiles_do_not_depend_on_what_lies_outside(ctx, iters, gab):
    """The 190 x 95 planes restored as a whole, and as the crop at (248, 120) -- a multiple of both the tile and the cell -- of
    500 x 240 planes whose other pixels and cells differ. Every output pixel at least 6 pixels (Gab 1 + EPF 2 + 1, + margin; 9 with three
    iterations, whose reach is 7) from the crop's edge is bit-identical in both; that region holds the interior tiles of the small planes (columns 62..185, rows
    30..89) but for their outermost pixels. An interior path that read mirrored or stale halo data would differ here."""
    w, h, ox, oy = 190, 95, 248, 120
    small, hf, sh = _case(w, h)
    big, bhf, bsh = _case(500, 240, seed=99)
    big[:, oy:oy + h, ox:ox + w] = small
    bhf[oy // 8:oy // 8 + hf.shape[0], ox // 8:ox // 8 + hf.shape[1]] = hf
    bsh[oy // 8:oy // 8 + sh.shape[0], ox // 8:ox // 8 + sh.shape[1]] = sh
    a = host.restoreFused(ctx, small, _params(w, h, iters, gab), hf, sh)
    b = host.restoreFused(ctx, big, _params(500, 240, iters, gab), bhf, bsh)
    # a pixel's reach: Gab 1 + the EPF radii (iteration 0: 3, iteration 1: 2, iteration 2: 1), + 2 of margin: 6 with two iterations
    k = (1 if gab else 0) + {1: 2, 2: 3, 3: 6}[iters] + 2
    k = max(k, 6)
    assert_bits_equal(a[:, k:h - k, k:w - k], b[:, oy + k:oy + h - k, ox + k:ox + w - k], "crop it%d gab%d" % (iters, gab))
    assert not np.array_equal(a, b[:, oy:oy + h, ox:ox + w])  # the surroundings do reach the crop's rim


def test_repeatable_on_one_context_and_on_a_shared_stream(ctx, orc):
    """the 125 x 61 case twice on one context; and a frame run on two contexts that share one stream (jxl_ctx_set_stream)"""
    planes, hf, sh = _case(125, 61)
    p = _params(125, 61, 2, True)
    first = host.restoreFused(ctx, planes, p, hf, sh)
    second = host.restoreFused(ctx, planes, p, hf, sh)
    assert_bits_equal(first, second, "same context, run twice")
    assert_bits_equal(first, _reference(orc, (125, 61, 2, True), planes, hf, sh, p), "against the oracle")
    f = synth.make_vardct_frame(128, 64, seed=77, mix="default", epf_iters=2, gab=True)
    exp = orc.vardct_frame(f)
    c1, c2 = _lib.Context(0), _lib.Context(0)
    try:
        c2.call("jxl_ctx_set_stream", c1.stream)
        f1, f2 = host.Frame.from_synth(c1, f), host.Frame.from_synth(c2, f)
        f1.run()
        f2.run()
        f1.run()
        o2 = f2.decodeFrame().copy()
        o1 = f1.decodeFrame().copy()
        assert_bits_equal(o1, exp, "context 1 on the shared stream")
        assert_bits_equal(o2, exp, "context 2 on the shared stream")
        assert_bits_equal(host.restoreFused(c2, planes, p, hf, sh), first, "planes on the second context")
    finally:
        c2.close()
        c1.close()
