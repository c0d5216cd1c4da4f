"""Patches on device plane sets, on the GPU: jxl_canvas_patches and jxl_canvas_cast_planes against the stage entries
(jxl_stage_patches / jxl_planes_patches, jxl_canvas_cast), JXLDecoder's patch stage on sets (device_patch_sets: _patches_sets,
_chained_tail) against the same run on host lists, and the patches-lossless sample against the recorded plane CRCs of
tests/golden/decode_routes.json. Every comparison is bit equality."""
import io
import json
import os
import zlib

import numpy as np
import pytest

import patch_ref as R
from jxlatte_amd import _lib, abi, decoder, host
from test_patches_gpu import _Rec, _case, _device

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl")
RECORD = os.path.join(ROOT, "tests", "golden", "decode_routes.json")


@pytest.fixture(scope="module")
def be():
    b = decoder.DeviceBackend()
    yield b
    b.close()


def _zero_filled(lst, like):
    """a slot's list with its absent planes as zero planes of the slot's own kind"""
    return [np.zeros(lst[0].shape, like) if a is None else a for a in lst]


def _on_sets(be, info, patches, frame, reference, resident=False, alias=None):
    """the patch stage of JXLDecoder on plane sets: the frame's planes go up with fromArrays (FramePlanes.adopt_set) -- or, with
    `resident`, the colours as the context's resident planes and the extras in the set --, every slot is a DeviceCanvas made with
    fromArrays (absent planes as zero planes; alias = (k, j): slot k is slot j's set). Returns (frame planes, per slot the planes
    downloaded or None, the stats row, the frame set's dtypes)"""
    ctx = be.ctx
    kind = frame[0].dtype
    sets = [None if r is None else host.DeviceCanvas.fromArrays(ctx, _zero_filled(r, kind)) for r in reference]
    if alias is not None:
        sets[alias[0]] = sets[alias[1]]
    dec = R.shell(info, patches, list(sets), be)
    dec._dead_sets = []
    fb = [b.copy() for b in frame]
    rp = be.keep_planes(np.stack(fb[:3])) if resident else None
    planes = decoder.FramePlanes(be, info, [None] * 3 + fb[3:] if resident else fb, 3, rp=rp)
    try:
        why = dec._patches_sets(R.frame_rec(patches), planes)
        assert why is None, why
        if planes.set is None:  # (no application: nothing was made)
            out = fb
        elif resident:
            out = [np.ascontiguousarray(a) for a in rp.download()] + [planes.set.download(c) for c in range(3, len(planes.set))]
        else:
            out = [planes.set.download(c) for c in range(len(planes.set))]
        refs = [None if s is None else [s.download(c) for c in range(len(s))] for s in sets]
        return out, refs, dec.stats[-1]["patches"], None if planes.set is None else planes.set.dtypes
    finally:
        dec._release_dead()
        for s in {id(s): s for s in sets if s is not None}.values():
            s.release()
        if planes.set is not None:
            planes.set.release()


def _assert_slots(got, exp, before, what):
    """the slots' planes after the stage: those of the host path, where it has them; a plane it never made is still zero"""
    for k in range(4):
        assert (got[k] is None) == (before[k] is None), (what, k)
        for n, a in enumerate(got[k] or []):
            b = exp[k][n]
            if b is None or b.shape != a.shape:
                assert not a.view(np.uint32).any(), "%s: slot %d plane %d" % (what, k, n)
            else:
                assert R.same_bits(a, b), "%s: slot %d plane %d (%s / %s)" % (what, k, n, a.dtype, b.dtype)
            if before[k][n] is not None and before[k][n].dtype == a.dtype:  # nothing writes a reference plane
                assert R.same_bits(a, before[k][n]), "%s: slot %d plane %d was written" % (what, k, n)


@pytest.mark.parametrize("is_int", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("n_extra", [0, 1, 2])
def test_set_entry_equals_the_stage_entry(ctx, be, n_extra, is_int):
    """the cases of tests/test_patches_gpu.py (frame 37 x 75, slot 0 of 23 x 41), 6 lists each and on until every mode was drawn: every frame plane equals
    jxl_stage_patches' result bit for bit, the slots' planes are those the host path leaves, a second run gives the same bits;
    modes 0..7 and both clamp values are reached"""
    seen, ran, seed = set(), 0, 1000 * n_extra + (500 if is_int else 0)
    want = set([0, 2] if is_int and n_extra else range(8)) - {1}  # (mode 1 is refused: tests/test_patches_gpu.py)

    def reached():
        return {s[0] for s in seen} == want and {s[1] for s in seen} == {0, 1}
    while (ran < 6 or not reached()) and seed % 500 < 200:  # (six lists at least, and on until every mode has been drawn)
        seed += 1
        info, patches, frame, reference = _case(seed, n_extra, is_int)
        try:
            exp = _device(ctx, info, patches, frame, reference)
        except (RuntimeError, ValueError, _lib.JxlError):  # (a list the stage entry refuses: the next seed)
            continue
        got = _on_sets(be, info, patches, frame, reference)
        for n, (a, b) in enumerate(zip(got[0], exp[0])):
            assert R.same_bits(a, b), "seed %d: frame plane %d (%s / %s)" % (seed, n, a.dtype, b.dtype)
        _assert_slots(got[1], exp[1], reference, "seed %d" % seed)
        assert got[2]["path"] == "plane sets" and got[2]["applications"] == exp[2]["applications"]
        again = _on_sets(be, info, patches, frame, reference)
        assert all(R.same_bits(a, b) for a, b in zip(again[0], got[0])), "seed %d, second run" % seed
        ran += 1
        for p in patches:
            if reference[p["ref"]] is not None:
                seen.update((int(m), int(cl)) for m, _, cl in p["blend"][0])
    assert 6 <= ran <= 12 and reached(), (ran, sorted(seen))


def test_two_slots_naming_one_set(ctx, be):
    info = R.make_info(1)
    rng = np.random.default_rng(19)
    frame = [rng.uniform(-0.5, 1.5, (37, 75)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (37, 75)).astype(F)]
    slot = [rng.uniform(-0.5, 1.5, (23, 41)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (23, 41)).astype(F)]
    row = [[2, 0, 0], [2, 0, 0]]
    patches = [R.patch(0, 0, 0, 9, 40, [(0, 0), (28, 35), (10, 20)], [row] * 3), R.patch(2, 1, 2, 7, 9, [(3, 4), (20, 60), (12, 22)], [row] * 3)]
    reference = [slot, None, None, None]
    aliased = [slot, None, slot, None]  # (float planes: no cast, so the host path's separate copies of the one list stay equal)
    exp = _device(ctx, info, patches, frame, aliased)
    got = _on_sets(be, info, patches, frame, aliased, alias=(2, 0))
    assert all(R.same_bits(a, b) for a, b in zip(got[0], exp[0]))
    assert not all(R.same_bits(a, b) for a, b in zip(got[0], _device(ctx, info, patches, frame, reference)[0]))  # (slot 2 was read)


def test_resident_colours_equal_the_resident_entry(ctx, be):
    """colors_resident = 1 against jxl_planes_patches: the colours never leave the resident planes, the extras sit in the set"""
    for base, n_extra in ((1000, 1), (2000, 2), (0, 0)):
        for seed in range(base + 1, base + 200):
            info, patches, frame, reference = _case(seed, n_extra, False)
            try:
                staged = _device(ctx, info, patches, frame, reference)
            except (RuntimeError, ValueError, _lib.JxlError):  # (a list the stage entry refuses: the next seed)
                continue
            plan = decoder.patch_type_plan(info, patches, frame, reference, 3)
            if len(plan.segments) == 1:
                break
        else:
            pytest.fail("no case")
        rp = host.ResidentPlanes.upload(ctx, np.stack(frame[:3]))
        extras = [b.copy() for b in frame[3:]]
        is_alpha, assoc = [t == 0 for t in info.ec_type], [bool(v) for v in info.ec_alpha_associated]
        rp.patches(extras, [None if r is None else list(r) for r in reference], plan.pos, plan.blend, is_alpha, assoc)
        exp = [np.ascontiguousarray(a) for a in rp.download()] + extras
        got = _on_sets(be, info, patches, frame, reference, resident=True)
        for n in range(3 + n_extra):
            assert R.same_bits(got[0][n], exp[n]) and R.same_bits(exp[n], staged[0][n]), (seed, n)
    # the refusals that need a context: no resident planes, resident planes of another size, an unknown set, frame == slot
    fresh = _lib.Context(0)
    try:
        fs = host.DeviceCanvas.create(fresh, [F] * 3, 8, 8)
        pos = np.array([(0, 0, 4, 4, 0, 0, 0, 0)], abi.PATCH_POS_DTYPE)
        row = np.array([[[2, 0, 0]] * 3], np.int32)
        with pytest.raises(_lib.IllegalStateException):
            host.canvas_patches(fs, [None] * 4, pos, row, 3, [], [], colorsResident=True)
        host.ResidentPlanes.upload(fresh, np.zeros((3, 8, 9), F))
        with pytest.raises(_lib.IllegalArgumentException, match="another size"):
            host.canvas_patches(fs, [None] * 4, pos, row, 3, [], [], colorsResident=True)
        with pytest.raises(_lib.IllegalArgumentException, match="reference set"):
            host.canvas_patches(fs, [fs, None, None, None], pos, row, 3, [], [])
        gone = host.DeviceCanvas.create(fresh, [F] * 3, 8, 8)
        stale = host.DeviceCanvas(fresh, gone.id, gone.types, gone.shape)
        gone.release()
        with pytest.raises(_lib.IllegalArgumentException, match="unknown set"):
            host.canvas_patches(fs, [stale, None, None, None], pos, row, 3, [], [])
        with pytest.raises(_lib.InvalidBitstreamException, match="Patch too large"):
            host.canvas_patches(fs, [host.DeviceCanvas.create(fresh, [F] * 3, 3, 3), None, None, None], pos, row, 3, [], [])
        assert not fs.download(0).any()  # nothing was queued
    finally:
        fresh.close()


def test_order_and_edge_cases(ctx, be):
    # the order witness: two overlapping float ADD positions whose result changes under a reversal of the list
    info, patches, frame, reference = R.order_witness()
    exp = _device(ctx, info, patches, frame, reference)
    got = _on_sets(be, info, patches, frame, reference)
    assert all(R.same_bits(a, b) for a, b in zip(got[0], exp[0])) and got[0][0][8, 12] == 0.0
    # non-finite samples
    rng = np.random.default_rng(11)
    frame = [rng.uniform(-1, 1, (24, 40)).astype(F) for _ in range(3)]
    specials = np.frombuffer(np.array([0x7FC00001, 0xFFC54321, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32).tobytes(), F)
    for c in range(3):
        frame[c].reshape(-1)[rng.choice(24 * 40, 300, replace=False)] = specials[rng.integers(0, 6, 300)]
    ref = [rng.uniform(-1, 1, (16, 32)).astype(F) for _ in range(3)]
    ref[0][:4, :8] = F(-0.0)
    patches = [R.patch(0, 0, 0, 10, 20, [(3, 5), (8, 11), (14, 20)], [[[2, 0, 0]]] * 3), R.patch(0, 0, 0, 4, 8, [(0, 0), (20, 32)], [[[2, 0, 0]]] * 2)]
    exp = _device(ctx, info, patches, frame, [ref, None, None, None])
    got = _on_sets(be, info, patches, frame, [ref, None, None, None])
    assert np.isnan(exp[0][0]).any() and np.isinf(exp[0][0]).any() and (exp[0][0].view(np.uint32) == 0x80000000).any()
    assert all(R.same_bits(a, b) for a, b in zip(got[0], exp[0]))
    # deep overlap on 64 x 96: untouched pixels keep their bits, NaN payloads included
    info = R.make_info(1)
    rng = np.random.default_rng(7)
    h, w = 64, 96
    frame = [rng.uniform(-0.5, 1.5, (h, w)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (h, w)).astype(F)]
    frame[0][::3, ::5] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), F)[0]
    frame[1][1::3, ::5] = F(-0.0)
    ref = [rng.uniform(-0.5, 1.5, (20, 30)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (20, 30)).astype(F)]
    rows = [[[3, 0, 1], [3, 0, 0]], [[2, 0, 0], [0, 0, 0]], [[4, 0, 1], [2, 0, 0]], [[6, 0, 0], [3, 0, 1]]]
    frame[0][20:40, 30:60] = rng.uniform(0, 1, (20, 30)).astype(F)
    patches = [R.patch(0, 0, 0, 12, 20, [(20 + k, 30 + k) for k in range(5)], [rows[(i + k) % 4] for k in range(5)]) for i in range(3)]
    depth = np.zeros((h, w), int)
    for p in patches:
        for y0, x0 in p["positions"]:
            depth[y0:y0 + 12, x0:x0 + 20] += 1
    assert depth.max() >= 8
    exp = _device(ctx, info, patches, frame, [ref, None, None, None])
    got = _on_sets(be, info, patches, frame, [ref, None, None, None])
    assert all(R.same_bits(a, b) for a, b in zip(got[0], exp[0]))
    for n in range(4):
        assert got[0][n][depth == 0].tobytes() == frame[n][depth == 0].tobytes()


def test_casts_in_the_middle_run_as_two_segments(ctx, be):
    """int planes added as ints, then a mode that casts planes already used: two cast + patch rounds; the sets' tags and bits
    afterwards are the host path's frame and reference[...]"""
    info = R.make_info(1)
    rng = np.random.default_rng(5)
    frame = [rng.integers(0, 255, (30, 50)).astype(np.int32) for _ in range(4)]
    ref = [rng.integers(0, 255, (30, 50)).astype(np.int32) for _ in range(4)]
    cast_all = R.patch(0, 0, 0, 10, 10, [(3, 3), (12, 30)], [[[2, 0, 0], [2, 0, 0]]] * 2)
    # mode 1 meets the switch of blendBuffers, which has no case for it: refused before a set is made
    refused = [R.patch(0, 2, 3, 8, 9, [(1, 1), (5, 6)], [[[1, 0, 0], [0, 0, 0]]] * 2), cast_all]
    with pytest.raises(decoder.InvalidBitstreamException, match="Illegal blend mode"):
        _on_sets(be, info, refused, frame, [ref, None, None, None])
    patches = [R.patch(0, 2, 3, 8, 9, [(1, 1), (5, 6)], [[[0, 0, 0], [6, 0, 0]]] * 2),  # mode 6 on the int alpha channel: a copy, no cast
               R.patch(0, 2, 3, 8, 9, [(4, 4)], [[[0, 0, 0], [6, 0, 1]]]), cast_all]
    exp = _device(ctx, info, patches, frame, [ref, None, None, None])
    got = _on_sets(be, info, patches, frame, [ref, None, None, None])
    assert got[2]["segments"] >= 2 and exp[2]["segments"] == got[2]["segments"]
    assert got[3] == [b.dtype for b in exp[0]] and got[0][0].dtype == F
    assert all(R.same_bits(a, b) for a, b in zip(got[0], exp[0]))
    assert all(R.same_bits(a, b) for a, b in zip(got[1][0], exp[1][0]))  # (dtypes included: the slot's casts persist in its set)


# ---- jxl_canvas_cast_planes ----------------------------------------------------------------------------------------------------
def test_cast_planes_equals_the_per_plane_cast(ctx):
    """sizes 1 x 1, 5 x 7, 37 x 75 and 64 x 96 (one workgroup with a head only, odd sample counts, more than one run of 4096 samples)
    in ONE call across three sets, depths 1, 8, 12, 16, 24, the extreme integers, float planes mixed in with NaN payloads"""
    rng = np.random.default_rng(3)
    depths = [1, 8, 12, 16, 24]

    def ints(shape, depth):
        a = rng.integers(-(1 << 20), 1 << 24, shape).astype(np.int32)
        flat = a.reshape(-1)
        vals = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, -1, (1 << depth) - 1], np.int32)
        flat[:min(flat.size, 5)] = vals[:min(flat.size, 5)]
        if flat.size > 5:
            flat[-5:] = vals[::-1]
        return a

    def floats(shape):
        a = rng.uniform(-2, 2, shape).astype(F)
        a.reshape(-1)[0] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), F)[0]
        a.reshape(-1)[-1] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), F)[0]
        return a
    layout = [((1, 1), [1, 8, None]), ((5, 7), [12, None, 16, 24]), ((37, 75), [8, 16, None, 1, 24]), ((64, 96), [None, 12, 8])]
    made, items = [], []
    for shape, plan in layout:
        arrays = [floats(shape) if d is None else ints(shape, d) for d in plan]
        s = host.DeviceCanvas.fromArrays(ctx, arrays)
        made.append((s, s.clone(), plan, arrays))
    try:
        sets = made[:1] + made[2:]  # three sets in the one call ...
        for s, _, plan, _ in sets:
            items += [(s, n, d if d is not None else 0) for n, d in enumerate(plan)]  # (a float plane's depth is never looked at)
        host.canvas_cast_planes(ctx, items)
        host.canvas_cast_planes(ctx, [(made[1][0], n, d if d is not None else 8) for n, d in enumerate(made[1][2])])  # ... the fourth by itself
        assert {d for _, _, plan, _ in made for d in plan if d is not None} == set(depths)
        for s, clone, plan, arrays in made:
            for n, d in enumerate(plan):
                clone.cast(n, d if d is not None else 8)
                got, exp = s.download(n), clone.download(n)
                assert got.dtype == F and R.same_bits(got, exp), (s.shape, n, d)
                if d is None:
                    assert R.same_bits(got, arrays[n])
                else:
                    assert R.same_bits(got, (arrays[n].astype(F) * F(F(1) / F((1 << d) - 1))).astype(F))
            assert s.types == [abi.PLANE_FLOAT] * len(plan)
            shape = abi.CanvasShape()
            ctx.call("jxl_canvas_describe", s.id, shape)
            assert [shape.types[n] for n in range(shape.n)] == s.types
        # refused with nothing queued and no tag changed
        a = host.DeviceCanvas.fromArrays(ctx, [ints((5, 7), 8), ints((5, 7), 8)])
        made.append((a, a.clone(), [], []))
        before = [a.download(n) for n in range(2)]
        for bad, msg in (([(a, 0, 8), (a, 0, 8)], "twice"), ([(a, 0, 8), (a, 1, 0)], "invalid Max Value"), ([(a, 0, 8), (a, 2, 8)], "bad plane"),
                         ([(a, n % 2, 8) for n in range(81)], "more than 80")):
            with pytest.raises(_lib.IllegalArgumentException, match=msg):
                host.canvas_cast_planes(ctx, bad)
            assert a.types == [abi.PLANE_INT32] * 2  # (download checks them against the library's)
            assert all(R.same_bits(a.download(n), before[n]) for n in range(2))
    finally:
        for s, clone, _, _ in made:
            s.release()
            clone.release()


# ---- the decoder's tail --------------------------------------------------------------------------------------------------------
def _tail(be, sets, is_int, start_resident):
    """_chained_tail on a shell decoder: patches from slot 0 (a host list) and slot 1 (the canvas itself), then noise and the
    inverse XYB. sets: device_patch_sets acts, with slot 1 and the canvas one DeviceCanvas; else everything is a host list.
    Returns (the frame's planes, the slots as lists of arrays, the canvas' dtypes, the stats row)"""
    h, w = 40, 56
    rng = np.random.default_rng(61)
    n_chan = 4

    def plane(shape, alpha, ints):
        if ints:
            return rng.integers(0, 256, shape).astype(np.int32)
        return rng.uniform(0.1, 0.9, shape).astype(F) if alpha else rng.uniform(-0.2, 0.8, shape).astype(F)
    frame = [plane((h, w), c == 3, is_int and not start_resident) for c in range(n_chan)]
    if start_resident:
        frame[3] = plane((h, w), True, is_int)
    slot0 = [plane((20, 30), c == 3, is_int) for c in range(n_chan)]
    canvas = [plane((h, w), c == 3, is_int) for c in range(n_chan)]
    mix = [[2, 0, 0], [2, 0, 0]]  # patch mode 2 with an alpha channel casts everything it touches (:446-465)
    patches = [R.patch(0, 1, 2, 12, 20, [(0, 0), (5, 9), (28, 36)], [mix] * 3), R.patch(1, 4, 4, 9, 33, [(20, 10), (31, 23)], [mix] * 2)]
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.backend, dec.device_splines, dec.device_patches, dec.device_canvas = be, True, True, sets
    dec.device_patch_sets = dec._patch_sets = sets
    dec._dead_sets, dec._landed = [], None
    dec.visibleFrames, dec.invisibleFrames, dec.stats = 1, 0, [{}]

    class Info:
        bits_per_sample, xyb_encoded, intensity_target = 8, 1, 255.0
        prim_xy, white_xy = list(decoder.PRI_SRGB), list(decoder.WP_D65)
        opsin_matrix = [11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                        -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863]
        opsin_bias = [-0.0037930732552754493] * 3
        custom_up = [0, 0, 0]
        colour_space, num_extra, ec_type, ec_alpha_associated, ec_bits = decoder.CE_RGB, 1, [0], [0], [8]

    class Rec(_Rec):
        upsampling, has_splines, ec_upsampling = 1, 0, [1]
    dec.info, dec.fe = Info, R.Fe(patches)
    cv = host.DeviceCanvas.fromArrays(be.ctx, canvas) if sets else [b.copy() for b in canvas]
    dec.canvas = cv
    dec.reference = [[b.copy() for b in slot0], cv, None, None]
    buffers = [b.copy() for b in frame]
    rp = be.keep_planes(np.stack(buffers[:3])) if start_resident else None
    planes = decoder.FramePlanes(be, Info, buffers, 3, rp=rp)
    try:
        dec._chained_tail(Rec, planes, False, False, keep=True)
        out = planes.land() if planes.set is not None else [np.ascontiguousarray(a) for a in planes.to_host()]
        slots = [dec.reference[0], [cv.download(c) for c in range(n_chan)] if sets else dec.reference[1]]
        return out, slots, list(cv.dtypes) if sets else [b.dtype for b in dec.reference[1]], dec.stats[-1], planes
    finally:
        dec._release_dead()
        if sets:
            cv.release()
        if planes.set is not None:
            planes.set.release()


@pytest.mark.parametrize("start_resident", [False, True], ids=["host planes", "resident planes"])
@pytest.mark.parametrize("is_int", [False, True], ids=["float", "int"])
def test_chained_tail_on_sets_equals_the_tail_on_host_lists(be, is_int, start_resident):
    """slot 1 is a DeviceCanvas that is also the canvas, slot 0 a host list: the planes, the slot contents and dtypes afterwards
    and the canvas' tags equal the same run on host lists without the switch; the frame's planes go up once"""
    bus0 = list(getattr(be.ctx, "blend_bus", (0, 0)))
    on, slots_on, tags_on, st_on, planes = _tail(be, True, is_int, start_resident)
    bus1 = list(be.ctx.blend_bus)
    off, slots_off, tags_off, st_off, _ = _tail(be, False, is_int, start_resident)
    assert st_on["patches"]["path"] == "plane sets" and "canvas" not in st_on
    assert st_on["patches"]["applications"] == st_off["patches"]["applications"] > 0
    assert len(on) == len(off) == 4
    for n, (a, b) in enumerate(zip(on, off)):
        assert R.same_bits(a, np.ascontiguousarray(b)), "frame plane %d (%s / %s)" % (n, a.dtype, b.dtype)
    for k in range(2):
        for n, (a, b) in enumerate(zip(slots_on[k], slots_off[k])):
            assert R.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b)), "slot %d plane %d (%s / %s)" % (k, n, a.dtype, b.dtype)
    assert tags_on == tags_off
    if is_int:
        assert np.dtype(F) in tags_on  # (the aliased canvas took the casts of its slot)
    # up: the frame's planes once (the extras alone from resident colours) and slot 0's list; down: what the test itself read
    plane, small = 40 * 56 * 4, 20 * 30 * 4
    assert bus1[0] - bus0[0] == (1 if start_resident else 4) * plane + 4 * small + 4 * plane  # (+ the canvas the test made)
    assert planes.moves.count("d2h") == 0


# ---- the sample ----------------------------------------------------------------------------------------------------------------
ALL = dict(sparse_coeffs=True, device_splines=True, device_patches=True, device_output=True, device_canvas=True, device_palette=True,
           device_image=True, device_frames=True)


def _crc(plane):
    a = bits = np.ascontiguousarray(plane)
    if a.dtype == np.float32:
        bits = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    return [a.dtype.str, list(a.shape), zlib.crc32(bits.tobytes())]


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        r = json.load(f)
    return {sec: r[sec]["samples"]["patches-lossless"] for sec in ("oracle", "device")}


@pytest.fixture(scope="module")
def default_png(be):
    dec = decoder.JXLDecoder(SAMPLE, backend=be)
    out = io.BytesIO()
    decoder.PNGWriter(dec.decode()).write(out)
    dec.close()
    return out.getvalue()


def _slot_bytes(dec):
    """the planes of the reference slots that are host lists (the sample's one reference frame, saved before the colour transform)"""
    lists = {id(r): r for r in dec.reference if isinstance(r, list)}
    return sum(b.nbytes for r in lists.values() for b in r if b is not None)


def _check_rows(dec, record):
    for st in dec.stats:
        assert st["canvas"] == "device", st["canvas"]
    st = dec.stats[1]
    assert st["patches"]["path"] == "plane sets" and st["patches"]["positions"] == 650 and st["patches"]["applications"] == 1950
    assert st["blend_bus"][1] == 0
    assert st["blend_bus"][0] == 4 * 1600 * 1096 * 4 + _slot_bytes(dec), st["blend_bus"]


def test_sample_with_the_switch(be, record):
    dec = decoder.JXLDecoder(SAMPLE, backend=be, device_canvas=True, device_patches=True, device_patch_sets=True)
    try:
        im = dec.decode()
        _check_rows(dec, record)
        crcs = [_crc(p) for p in im.getBuffer(False)]
        assert crcs == record["oracle"]["default"]["images"][0] == record["device"]["default"]["images"][0]
    finally:
        dec.close()


def test_sample_with_the_switch_to_the_png_samples(be, record, default_png):
    """... and with device_image + device_output: the image is the canvas set, PNGWriter(deviceSamples=True) reads it, and the
    whole decode brings down the PNG's samples and nothing else"""
    bus0 = list(getattr(be.ctx, "blend_bus", (0, 0)))
    dec = decoder.JXLDecoder(SAMPLE, backend=be, device_canvas=True, device_patches=True, device_patch_sets=True, device_image=True,
                             device_output=True)
    try:
        im = dec.decode()
        _check_rows(dec, record)
        assert dec.stats[-1]["image"] == "device set (canvas)" and im.planeSet is not None
        w = decoder.PNGWriter(im, deviceSamples=True)
        out = io.BytesIO()
        w.write(out)
        assert out.getvalue() == default_png
        bus1 = list(be.ctx.blend_bus)
        assert bus1[1] - bus0[1] == w.samples.nbytes
        crcs = [_crc(p) for p in im.getBuffer(False)]  # (now the planes come down: the recorded CRCs)
        assert crcs == record["device"]["default"]["images"][0]
        im.close()
    finally:
        dec.close()


def test_switch_off_leaves_the_recorded_row(be, record):
    dec = decoder.JXLDecoder(SAMPLE, backend=be, **ALL)
    try:
        im = dec.decode()
        im.close()
        got = json.loads(json.dumps(dec.stats[1], default=lambda v: v.item() if isinstance(v, np.generic) else list(v)))
        assert got == record["device"]["all"]["stats"][1]
    finally:
        dec.close()
