"""GPU, C ABI: jxl_canvas_from_modular_up -- the Modular context's result channels cast and upsampled into the planes of a plane
set as one launch (k_modplanes_up) -- and jxl_canvas_take_planes, the way back from the resident planes into a set.

Two witnesses for the upsampled planes. (1) Bit for bit: the numpy cast (int64 add -> wrap to int32 -> float32 -> ONE float32
multiply, as tests/test_modplanes_gpu.py restates it) followed by the stage entry that held the upsampling before,
host.performUpsampling, plane by plane. (2) The float64 upsampling model of tests/pixel_ref64.py on the cast planes, under its
bound K = 25 (tests/test_pixel_ref64_cpu.py: |result - model| <= 25 u (A + |model|)).

Shapes: bounds 1 x 1, 2 x 3 and 3 x 2 (the mirror loop iterates: a coordinate is reflected more than once) in channels of exactly
that size; 5 x 7 and 33 x 65 inside larger channels (the pitch is not the width, the width no multiple of 4, 131-wide channels whose
rows start at odd offsets); 70 x 130 for several workgroups (9100 input pixels: 72 workgroups at k = 2); k = 2, 4, 8."""
import ctypes as C

import numpy as np
import pytest

import pixel_ref64 as M
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth
from jxlatte_amd.upweights import DEFAULT_UP

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
F = np.float32
K_UPSAMPLE = 25  # the model's bound for the upsampling (tests/test_pixel_ref64_cpu.py)
S8, S12 = float(F(1) / F(255)), float(F(1) / F(4095))


def _samples(rng, shape):
    """full-range int32 with the extremes, values above 2^24 (where (float)v rounds) and small ones"""
    a = rng.integers(INT_MIN, INT_MAX, size=shape, endpoint=True).astype(np.int64)
    pool = np.array([INT_MIN, INT_MAX, INT_MIN + 1, INT_MAX - 1, 0, -1, 1, 2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 24 + 3, 2 ** 30 + 65, 255, 65535], np.int64)
    pick = rng.random(shape) < 0.4
    a[pick] = rng.choice(pool, size=int(pick.sum()))
    return a.astype(np.int32)


def _pixels(rng, shape, depth):
    """samples of a `depth`-bit image, a few below zero and above the maximum"""
    return rng.integers(-3, (1 << depth) + 3, size=shape).astype(np.int32)


def _identity(ctx, chans):
    ms = host.ModularStream(ctx, chans, [])
    ms.run()
    return ms


def _cast(chans, h, w, plane):
    ch, add, _, scale = plane
    v = chans[ch][:h, :w].astype(np.int64)
    if add >= 0:
        v = v + chans[add][:h, :w].astype(np.int64)
    v = ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)  # Java int add
    return np.ascontiguousarray(F(scale) * v.astype(F))


def _weights(k):
    return host.getUpWeights(k, DEFAULT_UP[k])


_weights_model = {}


def _check(ctx, cv, chans, h, w, planes, k, what):
    """both witnesses, plane by plane"""
    assert cv.shape == (h * k, w * k) and cv.types == [abi.PLANE_FLOAT] * len(planes)
    wts = _weights(k)
    if k not in _weights_model:
        _weights_model[k] = M.up_weights(k, DEFAULT_UP[k])
        assert np.array_equal(_weights_model[k].astype(F), wts)
    worst = 0.0
    for i, p in enumerate(planes):
        cast = _cast(chans, h, w, p)
        got = cv.download(i)
        assert_bits_equal(got, host.performUpsampling(ctx, cast, k, wts), "%s k %d plane %d: cast + stage entry" % (what, k, i))
        x, a, _ = M.upsample(cast, k, _weights_model[k])
        r = M.error_ratio(got, x, a)
        worst = max(worst, r)
        assert r <= K_UPSAMPLE, "%s k %d plane %d: error ratio %.2f above %d" % (what, k, i, r, K_UPSAMPLE)
    print("%s k %d: largest error ratio %.2f (bound %d)" % (what, k, worst, K_UPSAMPLE))


@pytest.fixture(scope="module")
def big(ctx):
    """six result channels: three of 72 x 140 (pixel-like 8-bit, pixel-like 12-bit, full range), two 72 x 131 ones of full range
    (odd row starts; the second to add to the first) and a third 72 x 140 one whose sum with channel 2 wraps"""
    rng = np.random.default_rng(950)
    chans = [_pixels(rng, (72, 140), 8), _pixels(rng, (72, 140), 12), _samples(rng, (72, 140)),
             _samples(rng, (72, 131)), _samples(rng, (72, 131)), _samples(rng, (72, 140))]
    chans[2][0, :8] = [INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, 1, -1, 2 ** 30]
    chans[5][0, :8] = [1, -1, INT_MAX, INT_MIN, INT_MIN, INT_MAX, INT_MIN, 2 ** 30]
    for c in chans:
        c.setflags(write=False)
    return chans


PLANES = [(0, -1, F, S8), (1, -1, F, S12), (2, -1, F, S8), (3, 4, F, 1.0), (2, 5, F, S12), (3, -1, F, 0.5)]


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("h,w", [(5, 7), (33, 65)])
def test_bounds_inside_larger_channels(ctx, big, h, w, k):
    _identity(ctx, big)
    cv = host.DeviceCanvas.fromModularUp(ctx, h, w, PLANES, k, _weights(k))
    try:
        _check(ctx, cv, big, h, w, PLANES, k, "%dx%d" % (h, w))
    finally:
        cv.release()


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (3, 2)])
def test_bounds_where_the_mirror_loop_iterates(ctx, h, w, k):
    rng = np.random.default_rng(h * 100 + w * 10 + k)
    chans = [_pixels(rng, (h, w), 8), _samples(rng, (h, w)), _samples(rng, (h, w))]
    _identity(ctx, chans)
    planes = [(0, -1, F, S8), (1, -1, F, S12), (1, 2, F, 1.0)]
    cv = host.DeviceCanvas.fromModularUp(ctx, h, w, planes, k, _weights(k))
    try:
        _check(ctx, cv, chans, h, w, planes, k, "exact %dx%d" % (h, w))
    finally:
        cv.release()


@pytest.mark.parametrize("k", [2, 4, 8])
def test_several_workgroups(ctx, big, k):
    _identity(ctx, big)
    planes = [(0, -1, F, S8), (2, 5, F, S12)]
    cv = host.DeviceCanvas.fromModularUp(ctx, 70, 130, planes, k, _weights(k))
    try:
        _check(ctx, cv, big, 70, 130, planes, k, "70x130")
    finally:
        cv.release()


@pytest.mark.parametrize("n", [1, 4, 16])
def test_plane_counts(ctx, big, n):
    _identity(ctx, big)
    planes = [PLANES[i % len(PLANES)][:3] + (float(F(1) / F(1 + i)),) for i in range(n)]
    cv = host.DeviceCanvas.fromModularUp(ctx, 9, 13, planes, 2, _weights(2))
    try:
        assert len(cv) == n
        _check(ctx, cv, big, 9, 13, planes, 2, "%d planes" % n)
    finally:
        cv.release()


def test_a_wrapping_add_channel(ctx, big):
    """the row of wrapping pairs is in channels 2 and 5: INT_MAX + 1 wraps to INT_MIN before the conversion"""
    _identity(ctx, big)
    planes = [(2, 5, F, 1.0)]
    assert _cast(big, 1, 8, planes[0])[0, 0] == F(INT_MIN) and _cast(big, 1, 8, planes[0])[0, 1] == F(INT_MAX)
    cv = host.DeviceCanvas.fromModularUp(ctx, 1, 8, planes, 4, _weights(4))
    try:
        _check(ctx, cv, big, 1, 8, planes, 4, "wrapping add")
    finally:
        cv.release()


def test_real_rct_and_squeeze_plan(ctx):
    """a plan with work in it: the default squeeze of a 100 x 60 image and an RCT, left on the device; the set equals the cast and
    the upsampling of the channels the same plan hands the host (jxl_modular_read_channel), whole and cropped"""
    mod = synth.make_modular_frame(100, 60, channels=3, seed=11)
    down = host.ModularStream(ctx, mod["chans"], mod["sp"], rctType=10, rctBegin=0).applyTransforms()
    assert [c.shape for c in down] == [(60, 100)] * 3
    ms = host.ModularStream(ctx, mod["chans"], mod["sp"], rctType=10, rctBegin=0)
    ms.run()
    planes = [(0, -1, F, S8), (1, -1, F, S8), (2, -1, F, S8), (1, 2, F, S12)]
    cv = host.DeviceCanvas.fromModularUp(ctx, 60, 100, planes, 2, _weights(2))
    crop = host.DeviceCanvas.fromModularUp(ctx, 33, 97, planes, 4, _weights(4))
    try:
        _check(ctx, cv, down, 60, 100, planes, 2, "rct + squeeze")
        _check(ctx, crop, down, 33, 97, planes, 4, "rct + squeeze, cropped")
    finally:
        cv.release()
        crop.release()


def _next_free_id(ctx):
    cv = host.DeviceCanvas.create(ctx, [np.int32], 1, 1)
    i = cv.id
    cv.release()
    return i


def _refused(ctx, desc, k, weights, status):
    """the call is refused with `status`; *id and the set store are as they were"""
    free = _next_free_id(ctx)
    id_ = C.c_int32(-77)
    with pytest.raises(_lib.JxlError) as e:
        ctx.call("jxl_canvas_from_modular_up", C.byref(desc) if desc is not None else None, k,
                 abi.fptr(weights) if weights is not None else None, C.byref(id_))
    assert e.value.status == status, e.value
    assert id_.value == -77
    assert _next_free_id(ctx) == free


def test_refusals_leave_id_and_the_store_untouched(ctx, big):
    chans = list(big[:3]) + [np.zeros((9, 131), np.int32), np.zeros((72, 139), np.int32)]
    ms = host.ModularStream(ctx, chans, [])
    ms.begin()
    good = [(0, -1, F, S8), (1, -1, F, S12), (2, 0, F, 1.0)]
    w2 = np.ascontiguousarray(_weights(2), F)
    INV = abi.JXL_ERR_INVALID_ARGUMENT
    _refused(ctx, host.modularPlanesDesc(33, 130, good), 2, w2, abi.JXL_ERR_STATE)  # begun, not run
    ms.run()
    _refused(ctx, None, 2, w2, INV)
    for k in (0, 1, 3, 16, -2):
        _refused(ctx, host.modularPlanesDesc(33, 130, good), k, w2, INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, good), 2, None, INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, good[:2] + [(2, -1, np.int32, 1.0)]), 2, w2, INV)  # the reference casts first
    d = host.modularPlanesDesc(33, 130, good)
    d.n_planes = 17
    _refused(ctx, d, 2, w2, abi.JXL_ERR_UNSUPPORTED)
    _refused(ctx, host.modularPlanesDesc(0, 130, good), 2, w2, INV)
    _refused(ctx, host.modularPlanesDesc(33, 130, good + [(5, -1, F, 1.0)]), 2, w2, INV)   # channel index past the list
    _refused(ctx, host.modularPlanesDesc(33, 130, good + [(3, -1, F, 1.0)]), 2, w2, INV)   # 9 rows < 33
    _refused(ctx, host.modularPlanesDesc(72, 140, good + [(4, -1, F, 1.0)]), 2, w2, INV)   # 139 columns < 140
    _refused(ctx, host.modularPlanesDesc(33, 130, [(0, 4, F, 1.0)]), 2, w2, INV)           # add of another size
    cv = host.DeviceCanvas.fromModularUp(ctx, 33, 130, good, 2, w2)  # and the same descriptor works afterwards
    try:
        _check(ctx, cv, chans, 33, 130, good, 2, "after the refusals")
    finally:
        cv.release()


# ---- jxl_canvas_take_planes ----------------------------------------------------------------------------------------------------
def test_take_planes_after_to_planes_and_a_resident_stage(ctx, big):
    """the way of a frame with a tail stage: the set's float colour planes become the resident planes, noise is added there, and the
    set takes them back -- its colour planes equal the downloaded resident planes, its other planes are what they were"""
    _identity(ctx, big)
    planes = [(0, -1, F, S8), (1, -1, F, S12), (0, -1, F, S8), (2, -1, np.int32, 1.0), (3, 4, F, 1.0)]
    fs = host.DeviceCanvas.fromModular(ctx, 33, 65, planes)
    ints = host.DeviceCanvas.fromModular(ctx, 33, 65, [(c, -1, np.int32, 1.0) for c in range(4)])
    try:
        before = [fs.download(c) for c in range(5)]
        rp = fs.toPlanes()
        rp.noise(256, (3 << 32) | 1, np.linspace(0.05, 0.6, 8).astype(F), 0.0, 1.0)
        exp = rp.download()
        assert not any(np.array_equal(exp[c].view(np.uint32), before[c].view(np.uint32)) for c in range(3))  # (the stage did something)
        fs.takePlanes()
        for c in range(3):
            assert_bits_equal(fs.download(c), exp[c], "colour plane %d" % c)
        for c in (3, 4):
            assert_bits_equal(fs.download(c), before[c], "plane %d is left alone" % c)
        assert fs.types == [0, 0, 0, 1, 0] and rp.live()
        assert_bits_equal(rp.download(), exp, "the resident planes stay")
        # int32 colour planes are replaced and tagged float; the fourth plane keeps its samples and its tag
        fourth = ints.download(3)
        ints.takePlanes()
        assert ints.types == [0, 0, 0, 1]
        for c in range(3):
            assert_bits_equal(ints.download(c), exp[c], "int32 set, colour plane %d" % c)
        assert_bits_equal(ints.download(3), fourth, "int32 set, plane 3")
    finally:
        fs.release()
        ints.release()


def test_a_refused_take_leaves_the_sets_bytes_untouched(ctx, big):
    _identity(ctx, big)
    fs = host.DeviceCanvas.fromModular(ctx, 33, 65, [(0, -1, np.int32, 1.0), (1, -1, F, S12), (2, -1, np.int32, 1.0)])
    two = host.DeviceCanvas.fromModular(ctx, 20, 30, [(0, -1, np.int32, 1.0), (1, -1, F, S12)])
    other = _lib.Context(0)  # a context that never had resident planes
    try:
        before, before2 = [fs.download(c) for c in range(3)], [two.download(c) for c in range(2)]
        host.ResidentPlanes.upload(ctx, np.full((3, 20, 30), 0.5, F))
        with pytest.raises(_lib.JxlError) as e:
            fs.takePlanes()  # resident planes of another size
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
        with pytest.raises(_lib.JxlError) as e:
            two.takePlanes()  # the size fits, the set has two planes
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
        with pytest.raises(_lib.JxlError) as e:
            ctx.call("jxl_canvas_take_planes", 9999)
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
        assert fs.types == [1, 0, 1] and two.types == [1, 0]
        for c in range(3):
            assert_bits_equal(fs.download(c), before[c], "refused take, plane %d" % c)
        for c in range(2):
            assert_bits_equal(two.download(c), before2[c], "refused take, two planes, plane %d" % c)
        lone = host.DeviceCanvas.create(other, [F] * 3, 4, 4)
        with pytest.raises(_lib.JxlError) as e:
            lone.takePlanes()
        assert e.value.status == abi.JXL_ERR_STATE
        assert lone.types == [0, 0, 0] and not any(lone.download(c).any() for c in range(3))
        lone.release()
    finally:
        fs.release()
        two.release()
        other.close()
