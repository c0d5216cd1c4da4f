"""The device spline stage on the GPU: jxl_stage_splines / jxl_planes_splines against the bracket of tests/spline_ref.py
(lo <= device <= hi at every pixel, NaN where mid is NaN, untouched pixels bit-identical, at most 1 in 10^4 touched samples
different from mid), determinism, resident == stage, the decoder switch and the chained tail's plane crossings."""
import ctypes as C
import os

import numpy as np
import pytest

import spline_ref as R
from jxlatte_amd import _lib, abi, decoder, host

F = np.float32
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sp(control, sigma_row, color=(90, 60, -40)):
    coeff = np.zeros((4, 32), np.int64)
    coeff[:3, 0] = color
    coeff[3, :len(sigma_row)] = sigma_row
    return dict(quant_adjust=0, control=control, coeff=coeff.tolist())


# The inputs that carry non-finite values into the stage. An arc whose sigma is NaN or infinite has a non-finite maxDist and is
# left out of the table, so these are the ways in:
def _sigma_zero():
    """coeffSigma all zero: sigma == 0 exactly, maxDist 0 (a one-pixel box), inv_sigma = +inf, mul = +-0. The erf arguments
    are +-inf: t = 1 / inf = 0, exp(-inf) = 0, erf = +-1"""
    return [_sp([(5, 5), (40, 70)], [0])] + R.random_splines(28, 2, 64, 96)  # (every spline takes spline 0's coefficients)


def _repeated_points():
    """repeated control points give NaN knots; each such spline keeps two samples, the last with a NaN arc length: NaN values
    and NaN mul at a finite position in a finite box. Those arcs draw NaN over their boxes"""
    return [_sp([(10, 10), (10, 10), (30, 50)], [6]), _sp([(8, 9), (30, 40), (30, 40), (50, 20)], [6]), _sp([(50, 10), (20, 80)], [6])]


@pytest.fixture(scope="module")
def device_backend():
    be = decoder.DeviceBackend(0)
    yield be
    be.close()


CASES = {  # height, width, splines, base_corr_x
    "1x1": (1, 1, lambda: R.random_splines(21, 2, 1, 1, sigma=(3, 6), margin=3), -0.125),
    "7x300_thin": (7, 300, lambda: R.random_splines(22, 6, 7, 300, sigma=(2, 4), margin=4), -0.125),
    "257x255_thick_crossing": (257, 255, lambda: R.random_splines(23, 8, 257, 255, sigma=(15, 40)), -0.125),
    "257x255_edges": (257, 255, lambda: R.random_splines(24, 10, 257, 255, sigma=(3, 9), margin=60), -0.125),
    # sigma changes sign along the spline (never exactly 0): arcs with a negative sigma, inv_sigma and maxDist as they come
    "96x128_sigma_changes_sign": (96, 128, lambda: [_sp([(5, 5), (40, 70), (10, 90)], (1, 4, -3, 2))] + R.random_splines(25, 2, 96, 128),
                                  -0.125),
    "64x96_sigma_zero_inf_inv_sigma": (64, 96, _sigma_zero, -0.125),
    "64x96_repeated_points_nan_mul": (64, 96, _repeated_points, -0.125),
    # base_corr_x = NaN: coeffX, values[0] and mul[0] of every arc are NaN while maxDist stays finite (MathHelper.max skips NaN)
    "64x96_nan_base_corr_x": (64, 96, lambda: R.random_splines(29, 3, 64, 96, sigma=(3, 9)), float("nan")),
    "32x32_small_z": (32, 32, lambda: [dict(quant_adjust=0, control=[(16, 10), (16, 11)],  # sigma ~ 2066: z = 7.1e-5 at distance 1,
                                            coeff=[[120, 60, -40] + [0] * 29, [80, 40, -27] + [0] * 29,   # the small branch of erf
                                                   [-60, -30, 20] + [0] * 29, [6200] + [0] * 31])], -0.125),
    "1080p": (1080, 1920, lambda: R.random_splines(26, 12, 1080, 1920, sigma=(3, 20), margin=40), -0.125),
    "4k_1e4_arcs": (2160, 3840, lambda: R.random_splines(27, 1200, 2160, 3840, points=(2, 3), sigma=(2, 5), step=60, margin=20), -0.125),
}


def _check(dev, planes, splines, bcx, bcb, what):
    br = R.render_bracket(planes, splines, bcx, bcb)
    outside, nan_bad, untouched_bad, touched, differ = R.check_device(dev, planes, br)
    print("%s: %d arcs, %d touched samples, %d differ from mid (%.3g %%), %d outside the bracket" %
          (what, len(br["arcs"]), touched, differ, 100.0 * differ / max(touched, 1), outside))
    assert outside == 0 and nan_bad == 0 and untouched_bad == 0
    assert differ * 10000 <= touched, (differ, touched)
    return br


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_splines_lies_in_the_bracket(ctx, name):
    h, w, make, bcx = CASES[name]
    splines, planes = make(), R.random_planes(31, h, w)
    dev = host.renderSplines(ctx, planes, splines, bcx, 0.875)
    br = _check(dev, planes, splines, bcx, 0.875, name)
    mid, arcs = br["mid"], br["arcs"]
    if name == "4k_1e4_arcs":
        assert len(arcs) >= 10000
    # the non-finite cases are value tests: each must really carry what its name says, in the model and on the device
    if name == "96x128_sigma_changes_sign":
        assert sum(1 for a in arcs if a[2] < 0) > 50 and sum(1 for a in arcs if a[2] > 0) > 50
    if name == "64x96_sigma_zero_inf_inv_sigma":
        assert len(arcs) > 50 and all(np.isinf(a[3]) and a[2] == 0 for a in arcs)
        assert not np.isnan(mid).any()  # (0.5f * distance - SQRT_F is never exactly 0 here: no 0 * inf)
    if name == "64x96_repeated_points_nan_mul":
        assert sum(1 for a in arcs if np.isnan(a[4]).all()) == 2
        assert np.isnan(mid).all(axis=0).sum() > 100 and np.isnan(dev).sum() == np.isnan(mid).sum()
    if name == "64x96_nan_base_corr_x":
        assert len(arcs) > 50 and all(np.isnan(a[4][0]) and np.isfinite(a[4][1]) and np.isfinite(a[4][2]) for a in arcs)
        assert np.isnan(mid[0]).sum() > 1000 and not np.isnan(mid[1:]).any()
        assert np.array_equal(np.isnan(dev), np.isnan(mid))
    again = host.renderSplines(ctx, planes, splines, bcx, 0.875)  # determinism: the same call, the same bits
    assert np.array_equal(dev.view(np.uint32), again.view(np.uint32))


def test_no_splines_leaves_the_planes_alone(ctx):
    planes = R.random_planes(32, 40, 50)
    out = host.renderSplines(ctx, planes, [], 0.0, 1.0)
    assert np.array_equal(out.view(np.uint32), planes.view(np.uint32))


def test_resident_planes_equal_the_stage(ctx):
    h, w = 90, 130
    splines, planes = R.random_splines(41, 5, h, w, sigma=(3, 15), margin=10), R.random_planes(42, h, w)
    exp = host.renderSplines(ctx, planes, splines, 0.0, 1.0)
    rp = host.ResidentPlanes.upload(ctx, planes)
    rp.splines(splines, 0.0, 1.0)
    assert np.array_equal(rp.download().view(np.uint32), exp.view(np.uint32))
    # after upsample(2), before noise: against the staged sequence
    from jxlatte_amd.upweights import DEFAULT_UP
    wts = host.getUpWeights(2, DEFAULT_UP[2])
    lut = np.linspace(0.01, 0.08, 8).astype(F)
    up = np.stack([host.performUpsampling(ctx, planes[c], 2, wts) for c in range(3)])
    big = R.random_splines(43, 5, 2 * h, 2 * w, sigma=(3, 15))
    st = host.renderSplines(ctx, up, big, 0.0, 1.0)
    noise = host.initializeNoise(ctx, 2 * h, 2 * w, (1 << 32) | 0, 256, 3)
    st = host.synthesizeNoise(ctx, st, noise, lut, 0.0, 1.0)
    rp = host.ResidentPlanes.upload(ctx, planes)
    rp.upsample(2, wts)
    rp.splines(big, 0.0, 1.0)
    rp.noise(256, (1 << 32) | 0, lut, 0.0, 1.0)
    assert np.array_equal(rp.download().view(np.uint32), np.asarray(st, F).view(np.uint32))


def test_error_statuses(ctx):
    lib = _lib.load()
    d, keep = abi.make_spline_desc(R.random_splines(1, 1, 8, 8), 0.0, 1.0)
    planes = R.random_planes(1, 8, 8)
    p3 = (C.POINTER(C.c_float) * 3)(*[abi.fptr(planes[c]) for c in range(3)])
    assert lib.jxl_stage_splines(ctx.h, None, 8, 8, C.byref(d)) == abi.JXL_ERR_INVALID_ARGUMENT
    assert lib.jxl_stage_splines(ctx.h, p3, 8, -1, C.byref(d)) == abi.JXL_ERR_INVALID_ARGUMENT
    assert lib.jxl_stage_splines(ctx.h, p3, 8, 8, None) == abi.JXL_ERR_INVALID_ARGUMENT
    d.n_splines = -2
    assert lib.jxl_stage_splines(ctx.h, p3, 8, 8, C.byref(d)) == abi.JXL_ERR_INVALID_ARGUMENT
    d.n_splines = 1
    with _lib.Context(0) as fresh:
        assert lib.jxl_planes_splines(fresh.h, C.byref(d)) == abi.JXL_ERR_STATE
    assert lib.jxl_stage_splines(ctx.h, p3, 8, 8, C.byref(d)) == 0  # and the context still works


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _stage_in_place_of_the_host_render(ctx, seen):
    """a stand-in for decoder.render_splines that calls the stage entry (the same kernel, host planes) and records what went
    in and what came out: the decoder's default path with it is the STAGED sequence of the device path"""
    def staged(buffers, splines, bcx, bcb, width, height):
        before = np.stack([np.asarray(buffers[c], F) for c in range(3)])
        assert before.shape[1:] == (height, width)
        after = host.renderSplines(ctx, before, splines, bcx, bcb)
        seen.append((before, splines, bcx, bcb, after))
        for c in range(3):
            buffers[c][...] = after[c]
    return staged


def test_wb_rainbow_with_device_splines(ctx, device_backend, monkeypatch):
    """device_splines=True against (a) the default decode whose host render is replaced by the stage entry: the same bits, with
    no tolerance; (b) the bracket of the default decode where it applies, at the spline stage: the stage entry's output on the
    very planes the default decode hands to render_splines lies in [lo, hi] of the host render of those planes. Identity with
    the default decode is reported, the PNG samples are equal"""
    p = os.path.join(ROOT, "tests", "golden", "samples", "wb-rainbow.jxl")
    ref = decoder.JXLDecoder(p, backend=device_backend).decode()
    dev = decoder.JXLDecoder(p, backend=device_backend, device_splines=True).decode()
    seen = []
    monkeypatch.setattr(decoder, "render_splines", _stage_in_place_of_the_host_render(ctx, seen))
    staged = decoder.JXLDecoder(p, backend=device_backend).decode()
    monkeypatch.undo()
    assert len(seen) == 2  # two frames of this image carry a spline each
    for before, splines, bcx, bcb, after in seen:
        _check(after, before, splines, bcx, bcb, "wb-rainbow at the spline stage")
    assert len(dev.buffer) == len(staged.buffer) and _same_bits(dev.buffer, staged.buffer)
    print("wb-rainbow device_splines: identical to the default decode: %s" % _same_bits(ref.buffer, dev.buffer))
    assert np.array_equal(decoder.PNGWriter(ref).samples, decoder.PNGWriter(dev).samples)


class _Rec:
    """a frame record for _chained_tail: upsampling 2, splines, noise, XYB"""
    upsampling, num_patches, has_splines, has_noise, save_before_ct, save_as_reference, do_ycbcr = 2, 0, 1, 1, 0, 0, 0
    group_dim, base_corr_x, base_corr_b = 256, 0.0, 1.0
    noise = [0.01 * (i + 1) for i in range(8)]


def _tail(device_backend, device_splines, start_resident):
    h, w = 48, 64
    planes = R.random_planes(51, h, w)
    splines = R.random_splines(52, 4, 2 * h, 2 * w, sigma=(3, 10))
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.backend, dec.device_splines = device_backend, device_splines
    dec.visibleFrames, dec.invisibleFrames, dec.stats, dec.reference = 1, 0, [{}], [None] * 4

    class Info:
        bits_per_sample, xyb_encoded, intensity_target = 8, 1, 255.0
        prim_xy, white_xy = list(decoder.PRI_SRGB), list(decoder.WP_D65)
        opsin_matrix = [11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                        -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863]
        opsin_bias = [-0.0037930732552754493] * 3
        custom_up = [0, 0, 0]

    class Fe:
        def splines(self):
            return splines
    dec.info, dec.fe = Info, Fe()
    buffers = [planes[c].copy() for c in range(3)]
    rp = device_backend.keep_planes(planes) if start_resident else None
    dec._chained_tail(_Rec, decoder.FramePlanes(device_backend, Info, buffers, 3, rp=rp), False, False)
    return np.stack(buffers[:3]), dec.stats[-1]["plane_moves"], planes, splines


@pytest.mark.parametrize("start_resident", [False, True])
def test_chained_tail_keeps_the_planes_on_the_device(ctx, device_backend, start_resident, monkeypatch):
    """upsampling 2 + splines + noise + XYB. Noise and the inverse XYB follow the splines, so the spline bracket is applied
    where it holds, at the spline stage, and the samples after it are compared without a tolerance: the device tail equals,
    bit for bit, the staged sequence upsample -> (down) stage entry (up) -> noise -> XYB, i.e. the switch-off tail with the host
    render replaced by jxl_stage_splines; and that stage's output lies in the bracket of the host render of the same planes"""
    on, moves_on, planes, splines = _tail(device_backend, True, start_resident)
    off, moves_off, _, _ = _tail(device_backend, False, start_resident)
    first = [] if start_resident else ["h2d"]
    assert moves_on == first + ["d2h"]
    assert moves_off == first + ["d2h", "h2d", "d2h"]  # down for the host splines, up again for the noise
    seen = []
    monkeypatch.setattr(decoder, "render_splines", _stage_in_place_of_the_host_render(ctx, seen))
    staged, moves_staged, _, staged_splines = _tail(device_backend, False, start_resident)
    monkeypatch.undo()
    assert moves_staged == moves_off and len(seen) == 1
    before, sp, bcx, bcb, after = seen[0]
    assert before.shape == (3, 96, 128) and sp is staged_splines and sp == splines
    _check(after, before, sp, bcx, bcb, "chained tail at the spline stage")
    assert np.array_equal(on.view(np.uint32), staged.view(np.uint32))
    print("chained tail, device vs host splines: identical %s" % np.array_equal(on.view(np.uint32), off.view(np.uint32)))
