"""k_pfm_samples through its two entries (jxl_stage_pfm_samples, jxl_planes_pfm_samples) against the numpy model of
tests/pfm_ref.py, byte for byte: the shapes where the kernel takes another path (a row shorter than one lane's group of 4, the
sample-by-sample tail, row pitches that leave every wide load and store 4-byte aligned only, one row, several workgroups), the
values a byte swap or a division would get wrong (NaNs of every kind, -0, subnormals; integers that round in the conversion),
planes of mixed kind, what the entries refuse, and the resident planes' ownership."""
import ctypes as C

import numpy as np
import pytest

import pfm_ref
from jxlatte_amd import _lib, abi, host

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 33)
HEIGHTS = (1, 2, 3, 9)
LARGER = (67, 130)  # (height, width): 33 groups a row, 2211 groups: 9 workgroups, rows that begin in the middle of a wave
DEPTHS = (1, 8, 12, 16, 24, 31)
# quiet and signalling NaNs with payloads and both signs, +-0, +-inf, the smallest and the largest subnormal, FLT_MAX, 1.0
SPECIAL_F = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0xffffffff, 0x7f800001, 0x7fbfffff, 0xffa5a5a5, 0xff800001,
                      0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7f7fffff, 0xff7fffff,
                      0x3f800000], np.uint32)


def _float_plane(rng, shape, shift):
    """random bit patterns (every class of float among them), the special values laid over the front, rotated by `shift` so that
    the small shapes see all of them between them"""
    a = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    n = min(flat.size, SPECIAL_F.size)
    flat[:n] = np.roll(SPECIAL_F, -shift)[:n]
    return a.view(np.float32)


def _int_plane(rng, shape, depth, shift):
    """0, max, max + 1, negative values, INT32_MIN and INT32_MAX, values that are no float (they round in the conversion)"""
    mx = (1 << depth) - 1
    special = np.array([0, mx, mx + 1, -1, -mx, -(1 << 31), (1 << 31) - 1, (1 << 24) + 1, -(1 << 25) - 3, 1, mx - 1, 0x7fffffbf], np.int64)
    a = rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64)
    flat = a.reshape(-1)
    n = min(flat.size, special.size)
    flat[:n] = np.roll(special, -shift)[:n]
    return (a & 0xffffffff).astype(np.uint32).view(np.int32)


def _planes(rng, shape, kinds, depths, shift=0):
    return [_float_plane(rng, shape, shift + 5 * c) if k == "f" else _int_plane(rng, shape, depths[c], shift + c)
            for c, k in enumerate(kinds)]


def _check(got, planes, depths, what):
    exp = np.frombuffer(pfm_ref.payload(planes, depths), np.uint8)
    got = got.reshape(-1)
    assert got.size == exp.size, what
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (what, bad.size, bad[0])


SMALL = [(h, w) for h in HEIGHTS for w in WIDTHS]


@pytest.mark.parametrize("kinds", ["f", "i", "fff", "iii", "fif", "iff", "ifi"])
def test_small_shapes_equal_the_model(ctx, kinds):
    rng = np.random.default_rng(len(kinds) * 100 + sum(map(ord, kinds)))
    for n, shape in enumerate(SMALL):
        depths = [DEPTHS[(n + c) % len(DEPTHS)] for c in range(len(kinds))]
        planes = _planes(rng, shape, kinds, depths, shift=n)
        _check(host.pfmSamples(ctx, planes, depths), planes, depths, "%s %s depths %s" % (kinds, shape, depths))


@pytest.mark.parametrize("kinds", ["f", "i", "fff", "iii", "fii"])
def test_several_workgroups_equal_the_model(ctx, kinds):
    rng = np.random.default_rng(7 + len(kinds))
    depths = [31, 8, 12][:len(kinds)]
    planes = _planes(rng, LARGER, kinds, depths)
    out = host.pfmSamples(ctx, planes, depths)
    assert out.shape == LARGER + (len(kinds), 4) and out.dtype == np.uint8
    _check(out, planes, depths, kinds)


@pytest.mark.parametrize("depth", DEPTHS)
def test_every_depth_rounds_before_the_multiply(ctx, depth):
    """(float)v * (1.0f / max): a quotient v / max, or a multiply in double, differs on these planes"""
    rng = np.random.default_rng(depth)
    for kinds in ("i", "iii"):
        planes = _planes(rng, (5, 13), kinds, [depth] * 3)
        _check(host.pfmSamples(ctx, planes, [depth] * len(kinds)), planes, [depth] * len(kinds), "depth %d %s" % (depth, kinds))
    mx = (1 << depth) - 1
    one = host.pfmSamples(ctx, [np.full((1, 1), mx, np.int32)], [depth])
    # max * (1.0f / max) is 1.0f at every depth here (at 31 the conversion of max itself rounds up to 2^31)
    assert bytes(one.reshape(-1)) == bytes([0x3f, 0x80, 0, 0])


def np_orient(a, o):
    return {1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1, :], 5: a.T, 6: a.T[:, ::-1], 7: a[::-1, ::-1].T, 8: a.T[::-1, :]}[o]


@pytest.fixture(scope="module")
def resident_src():
    rng = np.random.default_rng(99)
    return _planes(rng, (37, 53), "fff", [0] * 3)


@pytest.mark.parametrize("o", [1, 2, 5, 8])
def test_resident_entry_equals_the_stage_entry_and_the_model(ctx, resident_src, o):
    rp = host.ResidentPlanes.upload(ctx, resident_src)
    rp.orient(o)
    got = rp.pfmSamples()
    oriented = [np.ascontiguousarray(np_orient(a, o)) for a in resident_src]
    assert got.shape == oriented[0].shape + (3, 4) and rp.shape == ((53, 37) if o > 4 else (37, 53))
    _check(got, oriented, None, "resident, orientation %d" % o)
    assert np.array_equal(got, host.pfmSamples(ctx, oriented))


def test_resident_entry_on_odd_small_planes(ctx):
    rng = np.random.default_rng(3)
    for shape in [(1, 1), (2, 3), (3, 7), (9, 33)]:
        planes = _planes(rng, shape, "fff", [0] * 3)
        _check(host.ResidentPlanes.upload(ctx, planes).pfmSamples(), planes, None, "resident %s" % (shape,))


# ---- refusals: the status, nothing written ----
def _stage(ctx, planes, out, h, w, n_planes, is_int=(0, 0, 0), depth=(8, 8, 8)):
    p = abi.PfmParams()
    p.height, p.width, p.n_planes = h, w, n_planes
    for c in range(3):
        p.is_int[c], p.tagged_depth[c] = is_int[c], depth[c]
    arr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
    return ctx.lib.jxl_stage_pfm_samples(ctx.h, arr, C.byref(p), out.ctypes.data_as(C.c_void_p))


def _resident(ctx, out, h, w, n_planes=3, is_int=(0, 0, 0), depth=(8, 8, 8)):
    p = abi.PfmParams()
    p.height, p.width, p.n_planes = h, w, n_planes
    for c in range(3):
        p.is_int[c], p.tagged_depth[c] = is_int[c], depth[c]
    return ctx.lib.jxl_planes_pfm_samples(ctx.h, C.byref(p), out.ctypes.data_as(C.c_void_p))


def test_refusals_leave_the_output_untouched(ctx):
    h, w = 4, 6
    planes = [np.zeros((h, w), np.float32) for _ in range(3)]
    ints = [np.zeros((h, w), np.int32) for _ in range(3)]
    out = np.full(4 * 3 * h * w, 0xA5, np.uint8)
    INV, STATE = abi.JXL_ERR_INVALID_ARGUMENT, abi.JXL_ERR_STATE
    assert _stage(ctx, planes, out, 0, w, 3) == INV
    assert _stage(ctx, planes, out, h, 0, 3) == INV
    assert _stage(ctx, planes, out, -1, w, 3) == INV
    for n in (0, 2, 4):
        assert _stage(ctx, planes, out, h, w, n) == INV
    for bad in (0, 32):  # max = ~(~0 << depth) < 1
        assert _stage(ctx, ints, out, h, w, 3, (1, 1, 1), (8, bad, 8)) == INV
        assert _stage(ctx, ints, out, h, w, 1, (1, 0, 0), (bad, 8, 8)) == INV
    # a depth that only a float plane carries is not looked at, nor is one behind the last plane
    assert _stage(ctx, planes, out, h, w, 3, (0, 0, 0), (0, 0, 0)) == 0
    out[:] = 0xA5
    assert _stage(ctx, ints, out, h, w, 1, (1, 1, 1), (8, 0, 32)) == 0
    out[:] = 0xA5
    # the resident entry: no planes yet on a fresh context; then the layouts it has no planes for
    fresh = _lib.Context(0)
    try:
        assert _resident(fresh, out, h, w) == STATE
    finally:
        fresh.close()
    rp = host.ResidentPlanes.upload(ctx, planes)
    assert _resident(ctx, out, h, w, n_planes=1) == INV
    assert _resident(ctx, out, h, w, n_planes=2) == INV
    assert _resident(ctx, out, h, w, is_int=(0, 1, 0)) == INV
    assert _resident(ctx, out, h, w, is_int=(0, 1, 0), depth=(8, 0, 8)) == INV
    assert _resident(ctx, out, 0, w) == INV and _resident(ctx, out, h, -3) == INV
    assert _resident(ctx, out, w, h) == INV  # the geometry is the planes'
    assert np.all(out == 0xA5)
    with pytest.raises(_lib.IllegalArgumentException):
        host.pfmSamples(ctx, ints, [8, 32, 8])
    assert rp.live() and _resident(ctx, out, h, w) == 0 and not np.any(out == 0xA5)  # 0.0f everywhere


def test_planes_taken_by_a_later_upload_raise(ctx, resident_src):
    first = host.ResidentPlanes.upload(ctx, resident_src)
    second = host.ResidentPlanes.upload(ctx, [a[:5, :9] for a in resident_src])
    with pytest.raises(_lib.IllegalStateException):
        first.pfmSamples()
    assert second.pfmSamples().shape == (5, 9, 3, 4)
