"""jxl_modular_begin_chain on the device against the Python model of tests/modchain_ref.py (ModularStream.java:224-380), exactly,
on every case of tests/modchain_cases.py: as the plan runs by default -- every fusable Palette run as one k_palette_run launch --
and with the hook forcing the step form (k_palette_lookup / k_palette_chain on the plan's device channels). The form that ran and
the redo come from jxl_debug_last_palette_run, the forcing from jxl_debug_set_palette_fuse: hooks outside the C ABI."""
import ctypes as C

import numpy as np
import pytest

import modchain_cases as cases
import modchain_ref as ref
from jxlatte_amd import _lib, abi, host

pytestmark = pytest.mark.gpu
NAMES = sorted(cases.CASES)


@pytest.fixture
def fuse(ctx, request):
    before = host.setPaletteFuse(ctx, request.param)
    yield request.param
    host.setPaletteFuse(ctx, before)


def _stream(ctx, name):
    c = cases.CASES[name]
    return host.ModularStream(ctx, c["chans"], transforms=c["transforms"], bitDepth=c["bit_depth"])


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "steps"], indirect=True)
@pytest.mark.parametrize("name", NAMES)
def test_plan_equals_the_model_in_the_form_it_must_take(ctx, name, fuse):
    c = cases.CASES[name]
    inputs = [a.copy() for a in c["chans"]]
    redos = ctx.lib.jxl_modular_redo_count(ctx.h)
    ms = _stream(ctx, name)
    got = ms.applyTransforms()
    want = cases.expected(name)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (name, k)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s: channel %d: %d samples differ, the first at %s: %d, expected %d" % (
            name, k, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
    want_stats = cases.stats(name, fuse)
    assert host.lastPaletteRun(ctx) == want_stats, name
    assert ctx.lib.jxl_modular_redo_count(ctx.h) - redos == want_stats[2]
    assert all(np.array_equal(a, b) for a, b in zip(inputs, c["chans"]))  # the inputs are not written
    if want_stats[2]:
        # the plan remembers: a second run takes the exact step form at once and is not redone
        ms.run()
        again = ms.getDecodedBuffer()
        assert ref.same(again, want)
        stages = sum(n for n, _ in c["runs"])
        assert host.lastPaletteRun(ctx) == (0, stages + sum(cases.chained(name)), 0)
    else:
        ms.run()  # a plan runs again from its inputs: an RCT works on copies of them
        assert ref.same(ms.getDecodedBuffer(), want)


@pytest.mark.parametrize("name", cases.PLAIN)
def test_plain_chain_is_jxl_modular_begins_plan(ctx, name):
    """[RCT, Squeeze] through jxl_modular_begin_chain and through jxl_modular_begin: the same channels, the same launch count"""
    c = cases.CASES[name]
    steps, rct_type, rct_begin = [], -1, 0
    for t in c["transforms"]:
        if t["kind"] == ref.SQUEEZE:
            steps = t["steps"]
        else:
            rct_type, rct_begin = t["rct_type"], t["begin_c"]
    old = host.ModularStream(ctx, c["chans"], steps, rctType=rct_type, rctBegin=rct_begin)
    a = old.applyTransforms()
    launches = ctx.lib.jxl_modular_last_launch_count(ctx.h)
    b = _stream(ctx, name).applyTransforms()
    assert ref.same(a, b) and ref.same(b, cases.expected(name))
    assert ctx.lib.jxl_modular_last_launch_count(ctx.h) == launches > 0
    assert host.lastPaletteRun(ctx) == (0, 0, 0)


def test_jxl_modular_begin_after_a_chain_plan_is_as_before(ctx):
    """a chain plan's Palette runs do not outlive it: jxl_modular_begin on the same context gives what it gave before"""
    c = cases.CASES["rct_squeeze"]
    args = (c["chans"], c["transforms"][1]["steps"])
    first = host.ModularStream(ctx, *args, rctType=6, rctBegin=0).applyTransforms()
    launches = ctx.lib.jxl_modular_last_launch_count(ctx.h)
    _stream(ctx, "sample_shape_33x70").applyTransforms()
    second = host.ModularStream(ctx, *args, rctType=6, rctBegin=0).applyTransforms()
    assert ref.same(first, second) and ctx.lib.jxl_modular_last_launch_count(ctx.h) == launches
    assert host.lastPaletteRun(ctx) == (0, 0, 0)


def _refusals():
    """(name, status, transforms, changes to the channel list): one of each family of tests/test_modchain_cpu.py's REFUSALS, on the
    channels of sample_shape_5x7"""
    p, r, s = cases.pal, cases.rct, cases.squeeze
    return [("unknown_kind", -1, [dict(p(0, 1, 2), kind=3)]), ("palette_num_c_0", -1, [p(3, 0, 29)]),
            ("palette_pal_h_below_num_c", -1, [p(3, 5, 29)]), ("palette_pal_w_below_nb_colors", -1, [p(3, 4, 30)]),
            ("palette_d_pred_14", -1, [p(3, 4, 29, 0, 14)]), ("palette_weighted_deltas", -3, [p(3, 4, 29, 1, 6)]),
            ("palette_index_past_the_list", -1, [p(4, 4, 29)]), ("palette_begin_c_negative", -1, [p(-1, 4, 29)]),
            ("palette_sizes_at_that_point", -1, [p(0, 1, 19), p(2, 1, 23), p(4, 1, 18), p(3, 4, 29)]),
            ("rct_past_the_list", -1, [r(3, 0)]), ("rct_unequal_sizes", -2, [r(0, 0)]), ("rct_type_42", -1, [r(1, 42)]),
            ("squeeze_residual_past_the_list", -2, [s([(1, 1, 4, 1)])]), ("squeeze_horizontal_mismatch", -1, [s([(1, 1, 0, 1)])])]


@pytest.mark.parametrize("what,status,transforms", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_queue_nothing_and_leave_the_context_usable(ctx, what, status, transforms):
    c = cases.CASES["sample_shape_5x7"]
    good = _stream(ctx, "sample_shape_5x7")
    good.run()
    tr, keep = abi.make_transforms(transforms)
    ca = abi.make_channels(c["chans"])
    st = ctx.lib.jxl_modular_begin_chain(ctx.h, ca, len(c["chans"]), tr, len(transforms), c["bit_depth"])
    assert st == status, what
    # the plan before the refused call is still there, and a new one runs
    assert ref.same(good.getDecodedBuffer(), cases.expected("sample_shape_5x7"))
    assert ref.same(_stream(ctx, "depth2_5x7").applyTransforms(), cases.expected("depth2_5x7"))


def test_bit_depth_is_checked_where_a_palette_needs_it(ctx):
    c = cases.CASES["sample_shape_5x7"]
    tr, keep = abi.make_transforms(c["transforms"])
    ca = abi.make_channels(c["chans"])
    assert ctx.lib.jxl_modular_begin_chain(ctx.h, ca, len(c["chans"]), tr, len(c["transforms"]), 0) == -1
    assert ctx.lib.jxl_modular_begin_chain(ctx.h, ca, len(c["chans"]), tr, len(c["transforms"]), 33) == -1
    assert ref.same(_stream(ctx, "sample_shape_5x7").applyTransforms(), cases.expected("sample_shape_5x7"))
