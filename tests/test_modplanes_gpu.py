"""GPU, C ABI: jxl_canvas_from_modular -- the Modular context's result channels cropped into the planes of a plane set as one
launch -- bit for bit against a numpy restatement (int64 add -> wrap to int32 -> float32 -> ONE float32 multiply) and against
jxl_stage_modular_to_float, which existed before it. No tolerance anywhere: every comparison is equality of bits.

Shapes: the bounds (1,1) (2,3) (5,7) (9,64) (33,130) -- widths below 4 (the scalar tail alone), widths that are no multiple of 4
and one that is, and a plane of more than one workgroup (33 rows of 33 lane groups: 1089 lanes) -- inside channels that are
larger (40 x 140, and 131-wide ones whose rows start at odd offsets) and inside channels of exactly that size."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth

pytestmark = pytest.mark.gpu

BOUNDS = [(1, 1), (2, 3), (5, 7), (9, 64), (33, 130)]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _samples(rng, shape):
    """full-range int32 with the extremes, values above 2^24 (where (float)v rounds) and small ones"""
    a = rng.integers(INT_MIN, INT_MAX, size=shape, endpoint=True).astype(np.int64)
    pool = np.array([INT_MIN, INT_MAX, INT_MIN + 1, INT_MAX - 1, 0, -1, 1, 2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 24 + 3, 2 ** 30 + 65, 255, 65535], np.int64)
    pick = rng.random(shape) < 0.4
    a[pick] = rng.choice(pool, size=int(pick.sum()))
    return a.astype(np.int32)


def _identity(ctx, chans):
    """an identity plan (no squeeze step, no RCT): the result list is the uploaded channels"""
    ms = host.ModularStream(ctx, chans, [])
    ms.run()
    return ms


def _expect(chans, h, w, planes):
    out = []
    for ch, add, t, scale in planes:
        v = chans[ch][:h, :w].astype(np.int64)
        if add >= 0:
            v = v + chans[add][:h, :w].astype(np.int64)
        v = ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)  # Java int add
        out.append(np.ascontiguousarray(v) if np.dtype(t) == np.int32 else np.float32(scale) * v.astype(np.float32))
    return out


def _check(cv, want, what):
    assert len(cv) == len(want) and cv.dtypes == [a.dtype for a in want]
    for i, a in enumerate(want):
        assert_bits_equal(cv.download(i), a, "%s plane %d" % (what, i))


@pytest.fixture(scope="module")
def big(ctx):
    """five result channels: three of 40 x 140, a 40 x 131 one (odd row starts) and a second 40 x 131 one to add to it"""
    rng = np.random.default_rng(2024)
    chans = [_samples(rng, (40, 140)) for _ in range(3)] + [_samples(rng, (40, 131)) for _ in range(2)]
    # pairs whose sum wraps, in both channels pairs
    chans[0][0, :8] = [INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, 1, -1, 2 ** 30]
    chans[2][0, :8] = [1, -1, INT_MAX, INT_MIN, INT_MIN, INT_MAX, INT_MIN, 2 ** 30]
    for c in chans:
        c.setflags(write=False)
    return chans


@pytest.mark.parametrize("h,w", BOUNDS)
def test_int32_copies_and_float_casts_of_larger_channels(ctx, big, h, w):
    _identity(ctx, big)
    planes = [(0, -1, np.int32, 1.0), (3, -1, np.int32, 0.0), (1, -1, np.float32, 1.0), (3, 4, np.float32, 1.0 / 255),
              (0, 2, np.float32, 3.0)]
    cv = host.DeviceCanvas.fromModular(ctx, h, w, planes)
    try:
        assert cv.shape == (h, w)
        want = _expect(big, h, w, planes)
        _check(cv, want, "%dx%d" % (h, w))
        # the float planes once more, against the stage entry that held this arithmetic before
        for i, (ch, add, t, scale) in enumerate(planes):
            if np.dtype(t) == np.float32:
                a = np.ascontiguousarray(big[ch][:h, :w])
                b = np.ascontiguousarray(big[add][:h, :w]) if add >= 0 else None
                assert_bits_equal(cv.download(i), host.modularToFloat(ctx, a, b, scale), "stage entry, plane %d" % i)
    finally:
        cv.release()


@pytest.mark.parametrize("h,w", BOUNDS)
def test_bounds_equal_to_the_channels(ctx, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    chans = [_samples(rng, (h, w)) for _ in range(3)]
    _identity(ctx, chans)
    planes = [(2, -1, np.int32, 1.0), (1, 0, np.float32, 0.5), (0, -1, np.int32, 1.0)]
    cv = host.DeviceCanvas.fromModular(ctx, h, w, planes)
    try:
        _check(cv, _expect(chans, h, w, planes), "exact %dx%d" % (h, w))
    finally:
        cv.release()


@pytest.mark.parametrize("n", [1, 3, 4, 16])
def test_plane_counts(ctx, big, n):
    _identity(ctx, big)
    rng = np.random.default_rng(n)
    planes = []
    for i in range(n):
        ch = int(rng.integers(0, 3))
        if i % 2:
            planes.append((ch, int(rng.integers(-1, 3)), np.float32, float(np.float32(1.0) / np.float32(1 + i))))
        else:
            planes.append((ch, -1, np.int32, 1.0))
    cv = host.DeviceCanvas.fromModular(ctx, 33, 130, planes)
    try:
        _check(cv, _expect(big, 33, 130, planes), "%d planes" % n)
    finally:
        cv.release()


def test_xyb_mapping_with_three_scales(ctx, big):
    """Frame.java:437-448 for an XYB frame: the channels are Y, X, B - Y; the planes X, Y, B = scale_c * (float)(...) with B = (B - Y) + Y"""
    _identity(ctx, big)
    s = [float(np.float32(1.0 / 4096)), float(np.float32(1.0 / 512)), float(np.float32(1.0 / 256))]
    planes = [(1, -1, np.float32, s[0]), (0, -1, np.float32, s[1]), (2, 0, np.float32, s[2])]
    cv = host.DeviceCanvas.fromModular(ctx, 40, 140, planes)
    try:
        want = _expect(big, 40, 140, planes)
        _check(cv, want, "xyb")
        assert_bits_equal(want[2], host.modularToFloat(ctx, big[2], big[0], s[2]), "restatement against the stage entry")
        # the row of wrapping pairs is in plane 2: INT_MAX + 1 wraps to INT_MIN before the conversion
        assert want[2][0, 0] == np.float32(s[2]) * np.float32(INT_MIN)
    finally:
        cv.release()


def test_real_squeeze_and_rct_plan(ctx):
    """a plan with work in it: the default squeeze of a 100 x 60 image and an RCT, left on the device; the set equals the channels the
    same plan hands the host (jxl_modular_read_channel)"""
    mod = synth.make_modular_frame(100, 60, channels=3, seed=11)
    down = host.ModularStream(ctx, mod["chans"], mod["sp"], rctType=10, rctBegin=0).applyTransforms()
    assert [c.shape for c in down] == [(60, 100)] * 3
    ms = host.ModularStream(ctx, mod["chans"], mod["sp"], rctType=10, rctBegin=0)
    ms.run()
    planes = [(0, -1, np.int32, 1.0), (1, -1, np.int32, 1.0), (2, -1, np.int32, 1.0), (1, 2, np.float32, 1.0 / 255)]
    cv = host.DeviceCanvas.fromModular(ctx, 60, 100, planes)
    crop = host.DeviceCanvas.fromModular(ctx, 33, 97, planes)
    try:
        _check(cv, _expect(down, 60, 100, planes), "squeeze + rct")
        _check(crop, _expect(down, 33, 97, planes), "squeeze + rct, cropped")
    finally:
        cv.release()
        crop.release()


def test_the_set_owns_a_copy(ctx, big):
    _identity(ctx, big)
    planes = [(0, -1, np.int32, 1.0), (3, -1, np.int32, 1.0)]
    cv = host.DeviceCanvas.fromModular(ctx, 40, 131, planes)
    try:
        _identity(ctx, [np.zeros((50, 150), np.int32)] * 5)  # the next plan takes the result channels
        _check(cv, _expect(big, 40, 131, planes), "after the next plan")
    finally:
        cv.release()


def _next_free_id(ctx):
    cv = host.DeviceCanvas.create(ctx, [np.int32], 1, 1)
    i = cv.id
    cv.release()
    return i


def _refused(ctx, desc, status):
    """the call is refused with `status`; *id and the set store are as they were"""
    free = _next_free_id(ctx)
    id_ = C.c_int32(-77)
    with pytest.raises(_lib.JxlError) as e:
        ctx.call("jxl_canvas_from_modular", C.byref(desc) if desc is not None else None, C.byref(id_))
    assert e.value.status == status, e.value
    assert id_.value == -77
    assert _next_free_id(ctx) == free


def test_refusals_leave_id_and_the_store_untouched(ctx, big):
    chans = list(big[:3]) + [np.zeros((9, 131), np.int32), np.zeros((40, 139), np.int32)]
    ms = host.ModularStream(ctx, chans, [])
    ms.begin()
    good = [(0, -1, np.int32, 1.0), (1, -1, np.float32, 1.0), (2, 0, np.float32, 1.0)]
    _refused(ctx, host.modularPlanesDesc(33, 130, good), abi.JXL_ERR_STATE)  # begun, not run
    ms.run()
    INV = abi.JXL_ERR_INVALID_ARGUMENT
    _refused(ctx, None, INV)
    d = host.modularPlanesDesc(33, 130, good)
    d.n_planes = 0
    _refused(ctx, d, INV)
    d.n_planes = 17
    _refused(ctx, d, abi.JXL_ERR_UNSUPPORTED)
    _refused(ctx, host.modularPlanesDesc(0, 130, good), INV)
    _refused(ctx, host.modularPlanesDesc(33, 0, good), INV)
    _refused(ctx, host.modularPlanesDesc(-1, -1, good), INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, good[:2] + [(5, -1, np.int32, 1.0)]), INV)      # channel index past the list
    _refused(ctx, host.modularPlanesDesc(33, 130, [(-1, -1, np.int32, 1.0)]), INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, good + [(3, -1, np.int32, 1.0)]), INV)          # 9 rows < 33
    _refused(ctx, host.modularPlanesDesc(40, 140, good + [(4, -1, np.int32, 1.0)]), INV)          # 139 columns < 140
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, 1, np.int32, 1.0)]), INV)                  # add on an int32 plane
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, 4, np.float32, 1.0)]), INV)                # add of another size
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, 7, np.float32, 1.0)]), INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, -2, np.float32, 1.0)]), INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, -1, 2, 1.0)]), INV)                        # a type other than the two
    # and the same descriptor family still works afterwards
    cv = host.DeviceCanvas.fromModular(ctx, 33, 130, good)
    try:
        _check(cv, _expect(chans, 33, 130, good), "after the refusals")
    finally:
        cv.release()
