"""k_varblocks through both C-ABI entries (jxl_stage_varblocks on host planes, jxl_planes_varblocks on the resident planes)
against the numpy model of tests/varblocks_ref.py, bit for bit with any NaN equal to any NaN, on the shapes of
tests/varblocks_cases.py: one block; a mix of block sizes with interior cells; a ragged, 4-byte-aligned plane cut by its edge;
all 27 types with unowned cells; an upsampled frame's smaller block list; a plane smaller than its one block.

Bit equality across two cbrt implementations (numpy's on the host, the device library's) needs a condition, which the module
asserts for its own inputs: every finite non-zero float64 cube root the model takes lies at least 4 double-ulps from the nearest
midpoint between two floats, so any cbrt good to an ulp or two casts to the same float. (A root that is itself a float, like the
-0.5 of the planted -0.125 pixel, sits half a float-ulp from the midpoints: far inside the condition.)"""
import ctypes as C

import numpy as np
import pytest

import varblocks_cases
import varblocks_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host

pytestmark = pytest.mark.gpu
NAMES = sorted(varblocks_cases.CASES)


@pytest.fixture(scope="module")
def cases():
    """per case: the seeded planes and the model's result, computed once and never written"""
    out = {}
    for name in NAMES:
        h, w, cells, blocks = varblocks_cases.CASES[name]
        planes = varblocks_cases.samples(name)
        with np.errstate(all="ignore"):
            exp = ref.draw(planes, blocks)
        for a in planes + exp:
            a.setflags(write=False)
        out[name] = (planes, blocks, cells, exp)
    return out


def _midpoint_distance_ulps(root):
    """for finite non-zero float64 values: the distance to the nearest midpoint between two neighbouring floats, in double ulps"""
    f = root.astype(np.float32)
    fd = f.astype(np.float64)
    lo = np.where(fd <= root, f, np.nextafter(f, np.float32(-np.inf)))
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) * 0.5  # exact: two floats 1 ulp apart
    return np.abs(root - mid) / np.spacing(np.abs(root))


def test_seeded_cube_roots_keep_clear_of_the_float_midpoints(cases):
    smallest = np.inf
    for name in NAMES:
        planes = cases[name][0]
        root = ref.light_root(*planes).reshape(-1)
        root = root[np.isfinite(root) & (root != 0)]
        d = _midpoint_distance_ulps(root)
        smallest = min(smallest, d.min())
        assert d.min() >= 4, (name, d.min())
    print("smallest distance to a float midpoint: %.1f double ulps" % smallest)


def test_planted_values_are_where_they_matter(cases):
    planes, blocks, cells, exp = cases["b_24x40_mix"]
    assert np.isnan(planes[0][2, 1]) and np.isinf(planes[1][3, 4]) and planes[2][6, 3] == np.float32(-0.125)
    assert np.isneginf(exp[0][6, 3])                      # light == 0: a division by zero
    assert np.isnan(exp[1][2, 1]) and np.isnan(exp[2][2, 1])  # a NaN in R reaches every channel through light
    unowned = cases["d_512x512_all_types"]
    assert np.array_equal(unowned[3][0][400:, 400:].view(np.uint32), unowned[0][0][400:, 400:].view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_stage_entry_equals_the_model(ctx, cases, name):
    planes, blocks, cells, exp = cases[name]
    got = host.varblocks(ctx, np.stack(planes), blocks, cells)
    for c in range(3):
        assert_bits_equal(got[c], exp[c], "%s plane %d" % (name, c), any_nan=True)


@pytest.mark.parametrize("name", NAMES)
def test_resident_entry_equals_the_model(ctx, cases, name):
    planes, blocks, cells, exp = cases[name]
    rp = host.ResidentPlanes.upload(ctx, np.stack(planes))
    rp.varblocks(blocks, cells)
    got = rp.download()
    for c in range(3):
        assert_bits_equal(got[c], exp[c], "%s plane %d" % (name, c), any_nan=True)


def test_an_empty_block_list_changes_nothing(ctx, cases):
    planes = cases["c_21x37_ragged"][0]
    got = host.varblocks(ctx, np.stack(planes), np.zeros((0, 3), np.int32), (3, 5))
    for c in range(3):
        assert_bits_equal(got[c], planes[c], "plane %d" % c)


# ---- refusals: the status, nothing queued, nothing written ----
def _stage(ctx, planes, out, h, w, blocks, cells, n=None):
    d, keep = abi.make_varblock_desc(blocks, cells)
    if n is not None:
        d.n_blocks = n
    p3 = C.POINTER(C.c_float) * 3
    i = p3(*[abi.ptr(a, C.c_float) for a in planes]) if planes is not None else None
    o = p3(*[abi.ptr(a, C.c_float) for a in out]) if out is not None else None
    return ctx.lib.jxl_stage_varblocks(ctx.h, i, h, w, C.byref(d), o)


def _resident(ctx, blocks, cells):
    d, keep = abi.make_varblock_desc(blocks, cells)
    return ctx.lib.jxl_planes_varblocks(ctx.h, C.byref(d))


BAD_LISTS = [
    ([(0, 0, 27)], (4, 4)),                # a type above 26
    ([(0, 0, -1)], (4, 4)),
    ([(0, 0, 0), (0, 0, 1)], (4, 4)),      # one cell claimed twice
    ([(0, 0, 4), (1, 1, 0)], (4, 4)),      # ... by a block inside another
    ([(0, 3, 4)], (4, 4)),                 # a 16x16 over the right edge of the grid
    ([(3, 0, 4)], (4, 4)),                 # ... over the bottom edge
    ([(0, 4, 0)], (4, 4)),
    ([(-1, 0, 0)], (4, 4)),
    ([(0, 0, 24)], (31, 32)),              # a 256x256 on a grid one row short
    ([(0, 0, 0)], (0, 4)),
    ([(0, 0, 0)], (4, -1)),
]


def test_refusals_leave_the_output_untouched(ctx):
    h, w = 12, 20
    rng = np.random.default_rng(5)
    planes = [rng.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(3)]
    out = [np.full((h, w), np.float32(-77.5)) for _ in range(3)]
    INV, STATE = abi.JXL_ERR_INVALID_ARGUMENT, abi.JXL_ERR_STATE
    for blocks, cells in BAD_LISTS:
        assert _stage(ctx, planes, out, h, w, blocks, cells) == INV, (blocks, cells)
    good = [(0, 0, 0)]
    assert _stage(ctx, planes, out, 0, w, good, (4, 4)) == INV
    assert _stage(ctx, planes, out, h, -2, good, (4, 4)) == INV
    assert _stage(ctx, planes, out, h, w, good, (4, 4), n=-1) == INV
    assert _stage(ctx, None, out, h, w, good, (4, 4)) == INV
    assert _stage(ctx, planes, None, h, w, good, (4, 4)) == INV
    assert ctx.lib.jxl_stage_varblocks(ctx.h, (C.POINTER(C.c_float) * 3)(*[abi.ptr(a, C.c_float) for a in planes]), h, w, None,
                                       (C.POINTER(C.c_float) * 3)(*[abi.ptr(a, C.c_float) for a in out])) == INV
    assert all((a == np.float32(-77.5)).all() for a in out)
    with pytest.raises(_lib.IllegalArgumentException):
        host.varblocks(ctx, np.stack(planes), [(0, 0, 27)], (4, 4))
    # the resident entry: no planes on a fresh context; with planes the same refusals, and the planes stay as they were
    fresh = _lib.Context(0)
    try:
        assert _resident(fresh, good, (4, 4)) == STATE
    finally:
        fresh.close()
    rp = host.ResidentPlanes.upload(ctx, np.stack(planes))
    for blocks, cells in BAD_LISTS:
        assert _resident(ctx, blocks, cells) == INV, (blocks, cells)
    with pytest.raises(_lib.IllegalArgumentException):
        rp.varblocks([(0, 0, 0), (0, 0, 0)], (4, 4))
    got = rp.download()
    for c in range(3):
        assert_bits_equal(got[c], planes[c], "resident plane %d after the refusals" % c)
    # and the good call goes through on both
    assert _stage(ctx, planes, out, h, w, good, (4, 4)) == 0 and _resident(ctx, good, (4, 4)) == 0
    exp = ref.draw(planes, good)
    got = rp.download()
    for c in range(3):
        assert_bits_equal(out[c], exp[c], "stage plane %d" % c)
        assert_bits_equal(got[c], exp[c], "resident plane %d" % c)


def test_planes_taken_by_a_later_upload_raise(ctx, cases):
    planes = np.stack(cases["b_24x40_mix"][0])
    first = host.ResidentPlanes.upload(ctx, planes)
    second = host.ResidentPlanes.upload(ctx, planes[:, :8, :8])
    with pytest.raises(_lib.IllegalStateException):
        first.varblocks([(0, 0, 0)], (1, 1))
    second.varblocks([(0, 0, 0)], (1, 1))
    assert not second.download()[:, 0, :].any()
