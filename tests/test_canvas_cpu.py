"""CPU-only checks of the resident canvas: blend_type_plan (jxlatte_amd/decoder.py) executed with numpy equals the restatement of
blendFrame + blendBuffers in tests/blend_ref.py bit for bit wherever it answers "device", and answers "land" for the hand-built
cases one launch cannot replay; jxl_canvas_blend_check (through ctypes, no device) refuses every malformed descriptor; the
plan run over the frame headers of the two blending samples never lands."""
import itertools
import os
import types

import numpy as np
import pytest

import blend_ref as R
from conftest import assert_bits_equal
from jxlatte_amd import abi, host
from jxlatte_amd import decoder as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.dtype(np.float32), np.dtype(np.int32)
H, W = 9, 11  # the image


def make_info(num_extra, ec_type=None, assoc=None, bits=8, ec_bits=None):
    return types.SimpleNamespace(colour_space=D.CE_RGB, num_extra=num_extra, ec_type=list(ec_type or [0] * num_extra),
                                 ec_alpha_associated=list(assoc or [0] * num_extra), ec_bits=list(ec_bits or [8] * num_extra),
                                 bits_per_sample=bits, height=H, width=W)


def make_frame(num_extra, mode, ec_modes, origin=(0, 0), size=(H, W), alpha=0, ec_alpha=None, clamp=0, ec_clamp=None, source=0,
               ec_source=None):
    return types.SimpleNamespace(y0=origin[0], x0=origin[1], height=size[0], width=size[1], upsampling=1, blend_mode=mode,
                                 blend_alpha=alpha, blend_clamp=clamp, blend_source=source, ec_blend_mode=list(ec_modes),
                                 ec_blend_alpha=list(ec_alpha or [0] * num_extra), ec_blend_clamp=list(ec_clamp or [0] * num_extra),
                                 ec_blend_source=list(ec_source if ec_source is not None else [source] * num_extra))


def plane(rng, dt, shape):
    if dt == I:
        return rng.integers(-40, 300, shape).astype(np.int32)
    a = rng.normal(0.4, 0.8, shape).astype(np.float32)
    flat = a.reshape(-1)
    flat[::7] = np.float32(np.nan)
    flat[1::11] = np.float32(-0.0)
    flat[2::13] = np.float32(0.0)
    flat[3::17] = np.float32(1.5)
    return a


def ref_types_of(reference, canvas):
    return [None if r is None else "canvas" if r is canvas else [None if b is None else b.a.dtype for b in r] for r in reference]


def run_plan(plan, info, canvas, frame, reference):
    """the plan with numpy: every hoisted cast first, then the channels in order with the function the descriptor names (the
    sample arithmetic is blend_ref's; which function runs on which planes, and when a plane is cast, is the plan's)"""
    assert plan.verdict == "device"
    if plan.rect is None:
        return
    bh, bw, py, px, fy, fx, ry, rx = plan.rect
    ref = None
    if plan.source is not None:
        if plan.ref_zero:
            ref = [R.Buf(np.zeros((H, W), t)) for t in plan.ref_types]
        else:
            ref = reference[plan.source]
            assert (ref is canvas) == plan.aliased
    for which, p, depth in plan.casts:
        {"c": canvas, "f": frame, "r": ref}[which][p].cast_to_float(depth)
    assert [b.a.dtype for b in canvas] == plan.canvas_types and [b.a.dtype for b in frame] == plan.frame_types
    for c, (fp, mode, flags, fa, ra) in enumerate(plan.chans):
        is_alpha, has_extra = bool(flags & abi.BLEND_FLAG_IS_ALPHA), bool(flags & abi.BLEND_FLAG_HAS_EXTRA)
        clamp, premult = bool(flags & abi.BLEND_FLAG_CLAMP), bool(flags & abi.BLEND_FLAG_PREMULT)
        args = ((py, px), (fy, fx), (ry, rx), (bh, bw))
        if mode == abi.BLEND_REPLACE:
            R.copy_to_canvas(canvas[c], (py, px), (fy, fx), (bh, bw), frame[fp])
        elif mode == abi.BLEND_ADD:
            R.blend_add(canvas[c], frame[fp], ref[c], *args)
        elif mode == abi.BLEND_MULT:
            R.blend_mult(canvas[c], frame[fp], ref[c], *args, clamp)
        elif mode == abi.BLEND_BLEND:
            R.blend_blend(canvas[c], frame[fp], ref[c], frame[fa] if has_extra else None, ref[ra] if has_extra else None, *args, is_alpha,
                          has_extra, clamp, premult)
        else:
            R.blend_muladd(canvas[c], frame[fp], ref[c], frame[fa] if has_extra else None, *args, is_alpha, has_extra, clamp)


def one_case(rng, num_extra, mode, ec_modes, arrangement, ctypes_, ftypes, rtypes, origin, size, clamp, assoc, ec_type, ec_alpha, alpha):
    info = make_info(num_extra, ec_type=ec_type, assoc=assoc, bits=8, ec_bits=[8, 12, 5][:num_extra])
    fr = make_frame(num_extra, mode, ec_modes, origin=origin, size=size, alpha=alpha, ec_alpha=ec_alpha, clamp=clamp,
                    ec_clamp=[clamp] * num_extra, source=1)
    n = 3 + num_extra

    def build():
        r2 = np.random.default_rng(int(rng_seed))
        canvas = [R.Buf(plane(r2, ctypes_[c], (H, W))) for c in range(n)]
        frame = [R.Buf(plane(r2, ftypes[c], size)) for c in range(n)]
        reference = [None] * 4
        if arrangement == "alias":
            reference[1] = canvas
        elif arrangement == "other":
            reference[1] = [R.Buf(plane(r2, rtypes[c], (H, W))) for c in range(n)]
        return canvas, frame, reference

    rng_seed = rng.integers(1 << 30)
    canvas_a, frame_a, ref_a = build()
    canvas_b, frame_b, ref_b = build()
    plan = D.blend_type_plan(info, fr, [b.a.dtype for b in canvas_b], [b.a.dtype for b in frame_b], ref_types_of(ref_b, canvas_b))
    try:
        R.blend_frame(info, fr, canvas_a, frame_a, ref_a)
    except (R.NotModelled, R.TypeClash):  # the model's own limit, or types the reference itself would throw on: never "device"
        assert plan.verdict.startswith("land: "), plan.verdict
        return "land"
    if plan.verdict != "device":
        return "land"
    run_plan(plan, info, canvas_b, frame_b, ref_b)
    what = "extra %d mode %d ec %s %s c %s f %s r %s origin %s" % (num_extra, mode, ec_modes, arrangement, ctypes_, ftypes, rtypes, origin)
    for c in range(n):
        assert_bits_equal(canvas_b[c].a, canvas_a[c].a, what + " canvas %d" % c, any_nan=True)
    if arrangement == "other":  # the casts of the reference persist in the slot
        for c in range(n):
            assert ref_b[1][c].a.dtype == ref_a[1][c].a.dtype
            assert_bits_equal(ref_b[1][c].a, ref_a[1][c].a, what + " ref %d" % c, any_nan=True)
    return "device"


def test_plan_executed_with_numpy_equals_the_reference_model():
    rng = np.random.default_rng(2024)
    seen = {"device": 0, "land": 0}
    per_mode = {m: 0 for m in range(5)}
    for num_extra, mode, arrangement in itertools.product((0, 1, 2, 3), range(5), ("null", "alias", "other")):
        n = 3 + num_extra
        for rep in range(24):
            ec_modes = [int(v) for v in rng.integers(0, 5, num_extra)]
            ctypes_ = [I if rng.random() < 0.4 else F] * 3 if rep % 2 else [I if rng.random() < 0.4 else F for _ in range(3)]
            ctypes_ = list(ctypes_) + [I if rng.random() < 0.5 else F for _ in range(num_extra)]
            ftypes = [I if rng.random() < 0.4 else F for _ in range(n)]
            rtypes = [I if rng.random() < 0.4 else F for _ in range(n)]
            if rep % 3 == 0:  # everything float: the common case of a VarDCT animation
                ctypes_, ftypes, rtypes = [F] * n, [F] * n, [F] * n
            if rep % 6 == 1:  # everything int: lossless frames
                ctypes_, ftypes, rtypes = [I] * n, [I] * n, [I] * n
            origin, size = [((0, 0), (H, W)), ((2, 3), (5, 6)), ((-2, -1), (6, 7)), ((4, 5), (9, 9))][rep % 4]
            ec_type = [0, 0, 1][:num_extra] if rep % 2 else [0, 1, 0][:num_extra]
            # two alpha channels, and channels that point at the LATER one
            ec_alpha = [int(v) for v in rng.integers(0, max(1, num_extra), num_extra)]
            alpha = int(rng.integers(0, max(1, num_extra)))
            got = one_case(rng, num_extra, mode, ec_modes, arrangement, ctypes_, ftypes, rtypes, origin, size, rep % 2,
                           [int(v) for v in rng.integers(0, 2, num_extra)], ec_type, ec_alpha, alpha)
            seen[got] += 1
            if got == "device":
                per_mode[mode] += 1
    assert seen["device"] > 3 * seen["land"] and all(v > 20 for v in per_mode.values()), (seen, per_mode)


def test_int_read_then_cast_later_lands():
    """hand-built: the alpha plane is ADDed as int32 by its own channel's turn ... after a colour channel has cast it; and the
    other way round, where the hoisted cast would turn the earlier int sum into a float sum"""
    # 1. canvas aliases the reference. Channel 3 (extra 0, not the alpha the colours use) is int and ADDed as int; channel 4
    #    (extra 1) BLENDs with alphaChannel 0 -> casts reference plane 3 == canvas plane 3 to float AFTER channel 3 summed ints
    info = make_info(2, ec_type=[0, 1], ec_bits=[8, 8])
    fr = make_frame(2, abi.BLEND_REPLACE, [abi.BLEND_ADD, abi.BLEND_BLEND], ec_alpha=[0, 0], source=1)
    ct, ft = [F, F, F, I, F], [F, F, F, I, F]
    plan = D.blend_type_plan(info, fr, ct, ft, [None, "canvas", None, None])
    assert plan.verdict.startswith("land: ") and "int32" in plan.verdict
    # the same with a separate reference object: the FRAME's alpha plane is read as int by channel 3, cast by channel 4
    plan = D.blend_type_plan(info, fr, ct, ft, [None, [F, F, F, I, F], None, None])
    assert plan.verdict.startswith("land: ") and "int32" in plan.verdict
    # 2. the other order is fine: the colours BLEND first (cast of plane 3 hoisted in front of every read), then plane 3 blends as float
    fr = make_frame(1, abi.BLEND_BLEND, [abi.BLEND_BLEND], source=1)
    plan = D.blend_type_plan(make_info(1), fr, [F, F, F, I], [F, F, F, I], [None, "canvas", None, None])
    assert plan.verdict == "device" and ("c", 3, 8) in plan.casts and ("f", 3, 8) in plan.casts
    # 3. a copied int plane that a later channel casts as the frame's alpha
    fr = make_frame(2, abi.BLEND_REPLACE, [abi.BLEND_REPLACE, abi.BLEND_MULADD], ec_alpha=[0, 0], source=1)
    plan = D.blend_type_plan(make_info(2, ec_type=[0, 1]), fr, [F, F, F, I, F], [F, F, F, I, F], [None, [F] * 5, None, None])
    assert plan.verdict.startswith("land: ")


def test_other_landings():
    info = make_info(1)
    fr = make_frame(1, abi.BLEND_ADD, [abi.BLEND_ADD], source=1)
    assert D.blend_type_plan(info, fr, [F] * 17, [F] * 17, [None] * 4).verdict == "land: more than 16 planes"
    grey = make_info(0)
    grey.colour_space = D.CE_GRAY
    assert D.blend_type_plan(grey, make_frame(0, 0, []), [F], [F], [None] * 4).verdict == "land: one-colour image"
    assert D.blend_type_plan(info, fr, [F] * 4, [F] * 2, [None] * 4).verdict.startswith("land: the frame's colour count")
    two = make_frame(1, abi.BLEND_ADD, [abi.BLEND_ADD], source=1, ec_source=[2])
    assert D.blend_type_plan(info, two, [F] * 4, [F] * 4, [None, [F] * 4, [F] * 4, None]).verdict.startswith("land: channels blend from different")
    # ... but a REPLACE channel names no slot that matters
    one = make_frame(1, abi.BLEND_ADD, [abi.BLEND_REPLACE], source=1, ec_source=[2])
    assert D.blend_type_plan(info, one, [F] * 4, [F] * 4, [None, [F] * 4, [F] * 4, None]).verdict == "device"
    assert D.blend_type_plan(info, fr, [F] * 4, [F] * 4, [None, [F, None, F, F], None, None]).verdict.startswith("land: the reference slot lacks")
    # blendMulAdd copies the alpha channel from the reference at frameOffset: aliased and shifted, the canvas would copy itself
    mul = make_frame(1, abi.BLEND_MULADD, [abi.BLEND_MULADD], origin=(2, 2), size=(4, 4), source=1)
    assert D.blend_type_plan(info, mul, [F] * 4, [F] * 4, [None, "canvas", None, None]).verdict.startswith("land: the alpha channel is copied")
    assert D.blend_type_plan(info, mul, [F] * 4, [F] * 4, [None, [F] * 4, None, None]).verdict == "device"
    # an empty rectangle: nothing to do, on the device
    off = make_frame(1, abi.BLEND_BLEND, [abi.BLEND_BLEND], origin=(H, 0), source=1)
    plan = D.blend_type_plan(info, off, [F] * 4, [I] * 4, [None] * 4)
    assert plan.verdict == "device" and plan.rect is None and not plan.casts


# ---- jxl_canvas_blend_check: host only ---------------------------------------------------------------------------------------
def shape(n, h, w, types_):
    s = abi.CanvasShape()
    s.n, s.h, s.w = n, h, w
    for i, t in enumerate(types_):
        s.types[i] = t
    return s


def check(desc_args, canvas, frame, ref):
    host.canvas_blend_check(host.canvasBlendDesc(*desc_args), canvas, frame, ref)


def test_blend_check_refuses_malformed_descriptors():
    from jxlatte_amd import _lib
    FL, IN = abi.PLANE_FLOAT, abi.PLANE_INT32
    cv, fr_, rf = shape(4, 20, 30, [FL] * 4), shape(4, 10, 12, [FL] * 4), shape(4, 20, 30, [FL] * 4)
    rect = (10, 12, 5, 6, 0, 0, 5, 6)
    he = abi.BLEND_FLAG_HAS_EXTRA
    good = [(c, abi.BLEND_BLEND, he | (abi.BLEND_FLAG_IS_ALPHA if c == 3 else 0), 3, 3) for c in range(4)]
    check((0, 1, 2, rect, good), cv, fr_, rf)            # a separate reference
    check((0, 1, 0, rect, good), cv, fr_, cv)            # the canvas itself
    check((0, 1, -1, rect, [(c, abi.BLEND_REPLACE, he, 3, 3) for c in range(4)]), cv, fr_, None)

    def refused(exc, needle, desc_args, canvas=cv, frame=fr_, ref=rf):
        with pytest.raises(exc) as e:
            check(desc_args, canvas, frame, ref)
        assert needle in str(e.value), str(e.value)

    bad_mode = [good[0], (1, 5, he, 3, 3)] + good[2:]
    refused(_lib.InvalidBitstreamException, "Illegal blend mode", (0, 1, 2, rect, bad_mode))
    refused(_lib.InvalidBitstreamException, "Illegal blend mode", (0, 1, 2, rect, [good[0], (1, -1, he, 3, 3)] + good[2:]))
    ints = shape(4, 10, 12, [IN, FL, FL, FL])
    refused(_lib.IllegalArgumentException, "float samples", (0, 1, 2, rect, good), canvas=shape(4, 20, 30, [IN, FL, FL, FL]), frame=ints,
            ref=shape(4, 20, 30, [IN, FL, FL, FL]))
    add = [(c, abi.BLEND_ADD, he, 3, 3) for c in range(4)]
    refused(_lib.IllegalArgumentException, "canvas and frame plane differ", (0, 1, 2, rect, add), frame=shape(4, 10, 12, [FL, IN, FL, FL]))
    refused(_lib.IllegalArgumentException, "reference and frame plane differ", (0, 1, 2, rect, add), ref=shape(4, 20, 30, [FL, IN, FL, FL]))
    refused(_lib.IllegalArgumentException, "frame's alpha plane", (0, 1, 2, rect, [(0, abi.BLEND_BLEND, he, 3, 3)] + add[1:]),
            canvas=shape(4, 20, 30, [FL, FL, FL, IN]), frame=shape(4, 10, 12, [FL, FL, FL, IN]), ref=shape(4, 20, 30, [FL, FL, FL, IN]))
    refused(_lib.IllegalArgumentException, "reference's alpha plane", (0, 1, 2, rect, [(0, abi.BLEND_BLEND, he, 3, 7)] + add[1:]))
    refused(_lib.IllegalArgumentException, "frame plane out of range", (0, 1, 2, rect, [(4, abi.BLEND_ADD, he, 3, 3)] + add[1:]))
    refused(_lib.IllegalArgumentException, "a plane this mode reads is NULL", (0, 1, -1, rect, add), ref=None)
    refused(_lib.IllegalArgumentException, "one entry per canvas channel", (0, 1, 2, rect, good[:3]))
    refused(_lib.IllegalArgumentException, "bad set ids", (0, 0, 2, rect, good))
    refused(_lib.IllegalArgumentException, "bad set ids", (0, 1, 1, rect, good))
    refused(_lib.IllegalArgumentException, "disagree", (0, 1, -1, rect, good))
    refused(_lib.IllegalArgumentException, "bad plane set", (0, 1, 2, rect, good), frame=shape(4, 0, 12, [FL] * 4))
    refused(_lib.IllegalArgumentException, "bad plane set", (0, 1, 2, rect, good), frame=shape(4, 10, 12, [FL, 2, FL, FL]))
    refused(_lib.UnsupportedOperationException, "more than 16 planes", (0, 1, 2, rect, good), frame=shape(17, 10, 12, [FL] * 16))
    # rectangles outside a plane that is read or written
    for r in ((10, 12, 11, 6, 0, 0, 11, 6), (10, 12, 5, 19, 0, 0, 5, 6), (10, 12, 5, 6, 1, 0, 5, 6), (10, 12, 5, 6, 0, 1, 5, 6),
              (10, 12, 5, 6, 0, 0, 11, 6), (10, 12, -1, 6, 0, 0, 5, 6), (-1, 12, 5, 6, 0, 0, 5, 6)):
        refused(_lib.IllegalArgumentException, "rectangle outside a plane", (0, 1, 2, r, good))
    # ... a copy reads no reference: its offset is free
    check((0, 1, 2, (10, 12, 5, 6, 0, 0, 15, 26), [(c, abi.BLEND_REPLACE, he, 3, 3) for c in range(4)]), cv, fr_, rf)
    # blendMulAdd's alpha copy reads the reference at frameOffset
    mul = [(c, abi.BLEND_MULADD, he | (abi.BLEND_FLAG_IS_ALPHA if c == 3 else 0), 3, 3) for c in range(4)]
    check((0, 1, 2, rect, mul), cv, fr_, rf)
    refused(_lib.IllegalArgumentException, "rectangle outside a plane", (0, 1, 2, rect, mul), ref=shape(4, 9, 30, [FL] * 4))
    # what one in-place launch cannot replay
    refused(_lib.UnsupportedOperationException, "away from the pixel", (0, 1, 0, (10, 12, 5, 6, 0, 0, 4, 6), good), ref=cv)
    refused(_lib.UnsupportedOperationException, "away from the pixel", (0, 1, 0, rect, mul), ref=cv)
    check((0, 1, 0, (10, 12, 0, 0, 0, 0, 0, 0), mul), cv, fr_, cv)
    refused(_lib.IllegalArgumentException, "its shape is not", (0, 1, 0, rect, good), ref=shape(4, 20, 31, [FL] * 4))


# ---- the committed samples never land ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames", [("blendmodes_5", 5), ("wb-rainbow", 5)])
def test_no_landing_on_the_samples(name, frames):
    """front-end only: the plan over the frame headers of the two blending samples says "device" for every frame. The canvas
    bookkeeping of JXLDecoder.decode is replayed on types: the frame's planes are float after VarDCT, XYB, a float bit depth or
    an upsampling, else int32; a slot saved after the colour transform is the canvas object"""
    from jxlatte_amd import frontend
    from oracle.pybackend import OracleBackend
    be = OracleBackend()
    fe = frontend.Frontend(open(os.path.join(ROOT, "tests", "golden", "samples", name + ".jxl"), "rb").read())
    info = fe.image
    n = 3 + info.num_extra
    canvas, token, reference, verdicts = None, 0, [None] * 4, []
    while True:
        fr = fe.next_frame(be.squeeze, be.rct)
        if fr is None:
            break
        assert fr.type == D.REGULAR_FRAME and not fr.save_before_ct and not fr.num_patches
        ftypes = [F if (info.xyb_encoded or fr.encoding == D.VARDCT or info.exp_bits != 0 or fr.upsampling > 1) else I] * 3
        ftypes += [F if (info.ec_exp_bits[e] != 0 or fr.ec_upsampling[e] > 1) else I for e in range(info.num_extra)]
        if canvas is None:
            canvas = dict(types=[ftypes[0]] * n, token=token)
        if any(r is canvas and i != fr.save_as_reference for i, r in enumerate(reference)):
            token += 1
            canvas = dict(types=list(canvas["types"]), token=token)  # the copy-on-write of :645-653
        rts = [None if r is None else "canvas" if r is canvas else list(r["types"]) for r in reference]
        plan = D.blend_type_plan(info, fr, canvas["types"], ftypes, rts)
        verdicts.append(plan.verdict)
        if plan.verdict == "device":
            canvas["types"] = list(plan.canvas_types)
            if plan.source is not None and not plan.aliased and not plan.ref_zero:
                reference[plan.source]["types"] = list(plan.ref_types)
        save = (fr.save_as_reference != 0 or fr.duration == 0) and not fr.is_last
        if save:
            reference[fr.save_as_reference] = canvas
        if fr.is_last:
            break
    assert verdicts == ["device"] * frames, verdicts


def test_cli_parses_device_canvas_and_the_default_is_off():
    import inspect
    from jxlatte_amd import __main__ as cli
    a = cli.parser().parse_args(["in.jxl", "out.png", "--device-canvas"])
    assert a.device_canvas and not a.device_png
    assert not cli.parser().parse_args(["in.jxl"]).device_canvas
    assert inspect.signature(D.JXLDecoder.__init__).parameters["device_canvas"].default is False
