"""A third witness, on the CPU: bitstreams made by tests/jxl_writer.py from known arrays, decoded by the front-end and JXLDecoder on
the oracle backend, against expectations computed from the SOURCE arrays (tests/jxl_writer_cases.py) -- never against another
decode of the same bytes. A lossless single frame must come back as its source, re-oriented, bit for bit; a multi-frame image as
tests/blend_ref.py makes it from the source frames and the header fields the writer was given; an upsampled frame within
K["upsample"] of tests/pixel_ref64.upsample (test_pixel_ref64_cpu.py's bound, no new constant).

Arbitration. Where the writer (or its expectation) and the front-end or decoder disagreed, the reference's Java decided:
  * [RCT, Squeeze] on 1x1, 1x7 and 7x1 ("unexpected end of codestream section"): the WRITER was wrong. An empty channel is allocated,
    not decoded (ModularStream.java:198-199), so Pass.java:33-41 still hands it to the pass group, whose stream then has a channel
    list and reads its four header bits (ModularStream.java:78-83). The writer now writes them (jxl_writer.write_frame).
  * float samples: the EXPECTATION was wrong. Frame.java:443-448 multiplies the decoded integer by a float scale of 1: the samples
    are the integers converted, not their bit patterns reinterpreted. The decoder does as the Java does (jxl_writer_cases.typed_planes).
  * draw 54, MULADD on an integer alpha channel that names itself as its alpha: the DECODER was wrong. JXLCodestreamDecoder.java:455
    casts the frame's alpha plane in place, which is the plane :420 has in hand, so :461 sees a float frame plane and casts the canvas
    and the reference too; _blend_buffers compared its stale integer array and left the canvas int32. Fixed; the case is kept as
    MULTI_FIXED["muladd_on_its_own_integer_alpha"]. (In draw 54 the source slot was empty as well, where the reference itself throws,
    :441; such draws are drawn again, jxl_writer_cases.ReferenceThrows.)
  * an image of more than 16 planes under device_canvas ended in UnsupportedOperationException ("canvas: more than 16 planes") from
    jxl_canvas_create, although blend_type_plan's answer for it is to land: the DECODER was wrong, no reference line is involved.
    _canvas_route now lands such an image before a set is made; ROUTED["fourteen_extra"] is the case.

A grey frame in an RGB image does not exist in the format as the reference reads it: Frame.getColorChannelCount (Frame.java:874-877)
gives a Modular frame of an image that is not XYB-encoded the IMAGE's colour count, and LFGlobal.java:88-96 sizes the stream from the
image header too. A frame of another colour count is a three-colour frame (XYB, do_ycbcr or VarDCT) in a grey image; the writer makes
one (jxl_writer_lossy_cases: grey_tagged_xyb_9x11_gab1_epf2), but patch_sets_rule never says "a frame of another colour count" of it:
it looks at the image's colour count first (jxl_writer_cases.UNREACHABLE)."""
import io
import os
import re
import time

import numpy as np
import pytest

import jxl_writer as W
import jxl_writer_cases as C
from conftest import assert_bits_equal
from jxlatte_amd.decoder import JXLDecoder, PFMWriter, PNGWriter
from test_decoder import read_png
from test_pixel_ref64_cpu import K, ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def backend(orc):
    from oracle.pybackend import OracleBackend
    return OracleBackend()


def decode(im, backend, **kw):
    dec = JXLDecoder(W.encode(im), backend=backend, **kw)
    return dec, dec.decode()


def png_of(writer):
    """the writer's samples as [H][W][channels] integers"""
    ch = {0: 1, 2: 3, 4: 2, 6: 4}[writer.colorMode]
    raw = np.ascontiguousarray(writer.samples).tobytes()
    return np.frombuffer(raw, ">u2" if writer.bitDepth == 16 else "u1").reshape(writer.height, writer.width, ch)


def check_outputs(im, got_image, exp_planes, what, png_kw=None, pfm_kw=None):
    """PNG samples, PNG file and PFM bytes against numpy packing of the expected planes; the writers first (while the planes are the
    image's), then the planes: dtype, shape, bits"""
    bit_depth, exp_png = C.png_samples(im, exp_planes)
    w = PNGWriter(got_image, **(png_kw or {}))
    assert w.bitDepth == bit_depth and (w.height, w.width) == exp_png.shape[:2], what
    got_png = png_of(w)
    assert got_png.shape == exp_png.shape and np.array_equal(got_png, exp_png), "%s: %d PNG samples differ" % (what, int((got_png != exp_png).sum()))
    buf = io.BytesIO()
    w.write(buf)  # and the file itself: its IDAT rows, inflated, are those samples
    px, bd = read_png(buf.getvalue())
    assert bd == bit_depth and np.array_equal(px.reshape(exp_png.shape), exp_png), what + ": PNG file"
    buf = io.BytesIO()
    PFMWriter(got_image, **(pfm_kw or {})).write(buf)
    assert buf.getvalue() == C.pfm_bytes(im, exp_planes), what + ": PFM bytes"
    got = got_image.getBuffer()
    assert len(got) == len(exp_planes), what
    for c, (a, b) in enumerate(zip(got, exp_planes)):
        assert_bits_equal(a, b, "%s plane %d" % (what, c), any_nan=True)


# ---- the cases themselves ---------------------------------------------------------------------------------------------------
def _plane_can_betray(a, bits, what):
    h, w = a.shape
    room = min(16, a.size, 1 << bits)
    assert len(np.unique(a)) >= room or len(np.unique(a)) >= a.size // 3, (what, len(np.unique(a)))
    if a.size >= 2:
        assert a.min() == 0 and a.max() == (1 << bits) - 1, what
    if h > 1 and w > 1:
        for o in range(2, 9):
            b = C.orient(a, o)
            assert b.shape != a.shape or not np.array_equal(a, b), (what, o)
    elif a.size > 1:
        assert not np.array_equal(a.reshape(-1), a.reshape(-1)[::-1]), what


def test_the_cases_themselves():
    """every source plane can betray an error (jxl_writer_cases' docstring); a blended frame differs from the canvas under it; the
    float blends meet alpha exactly 0, exactly 1 and strictly between"""
    for table in list(C.SINGLE.values()) + [C.UPSAMPLED, C.MULTI, C.MULTI_FIXED]:
        for name, im in table.items():
            depths = C.depths_of(im)
            for k, fr in enumerate(im["frames"]):
                assert len(fr["planes"]) == len(depths), name
                for c, a in enumerate(fr["planes"]):
                    if "palette" in name and a.size < 256:
                        assert len(np.unique(a)) >= 16, name  # few colours on purpose, still 16 values
                    _plane_can_betray(a, depths[c], "%s frame %d plane %d" % (name, k, c))
    overlaps = 0
    for table in (C.MULTI, C.MULTI_FIXED):
        for name, im in table.items():
            trace = []
            C.decode_model(im, trace)
            n_col = 1 if im.get("grey") else 3
            ai = C.alpha_index(im)
            for k, (canvas, planes, hdr) in enumerate(trace):
                py, px = min(max(hdr.y0, 0), im["height"]), min(max(hdr.x0, 0), im["width"])
                bh, bw = min(hdr.y0 + hdr.height, im["height"]) - py, min(hdr.x0 + hdr.width, im["width"]) - px
                if bh <= 0 or bw <= 0:
                    continue
                overlaps += 1
                fy, fx = py - hdr.y0, px - hdr.x0
                for c in range(len(planes)):
                    over = C.cast_to_float(canvas[c][py:py + bh, px:px + bw], C.depths_of(im)[c])
                    new = C.cast_to_float(planes[c][fy:fy + bh, fx:fx + bw], C.depths_of(im)[c])
                    assert bh * bw < 4 or not np.array_equal(over, new), (name, k, c)
                if bh * bw >= 200:
                    a = planes[n_col + ai][fy:fy + bh, fx:fx + bw]
                    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any(), (name, k)
    assert overlaps > 100


# ---- single frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(C.SINGLE))
def test_single_frames_come_back_as_their_source(backend, group):
    t0 = time.time()
    for name, im in C.SINGLE[group].items():
        dec, got = decode(im, backend)
        exp = C.expected_planes(im)
        h, w = exp[0].shape
        assert (got.getHeight(), got.getWidth()) == (h, w), name
        check_outputs(im, got, exp, name)
        dec.close()
    print("%s: %d images in %.2f s" % (group, len(C.SINGLE[group]), time.time() - t0))


def test_a_wrong_sample_is_seen(backend):
    """the comparison discriminates: one source sample changed by one after the encode"""
    im = C.SINGLE["predictors"]["predictor_5"]
    dec, got = decode(im, backend)
    exp = [p.copy() for p in im["frames"][0]["planes"]]
    exp[1][16, 32] ^= 1
    with pytest.raises(AssertionError):
        check_outputs(im, got, exp, "mutated")


# ---- multi-frame images ------------------------------------------------------------------------------------------------------
def test_at_most_one_draw_in_twenty_is_left_out():
    """blend_ref raises NotModelled where an operand that is the canvas is read away from the pixel written; such a draw is left out"""
    print("left out: %d of %d draws %s" % (len(C.LEFT_OUT), C.MULTI_DRAWS, C.LEFT_OUT))
    assert len(C.LEFT_OUT) <= 0.05 * C.MULTI_DRAWS and len(C.MULTI) + len(C.LEFT_OUT) == C.MULTI_DRAWS


def test_the_draws_cover_what_they_are_for():
    seen = dict(modes=set(), ec_modes=set(), slots=set(), saves=set(), sbct=0, outside=0, straddle=0, inside=0, canvas_ref=0, grey=0, negative=0)
    for im in list(C.MULTI.values()) + list(C.MULTI_FIXED.values()):
        seen["grey"] += bool(im.get("grey"))
        for fr in im["frames"][1:]:
            seen["modes"].add(fr["blend"]["mode"])
            seen["ec_modes"].update(b["mode"] for b in fr["ec_blend"])
            seen["slots"].add(fr["blend"]["source"])
            x0, y0 = fr.get("crop") or (0, 0)
            h, w = fr["planes"][0].shape
            seen["negative"] += x0 < 0 or y0 < 0
            if x0 >= im["width"] or y0 >= im["height"] or x0 + w <= 0 or y0 + h <= 0:
                seen["outside"] += 1
            elif x0 < 0 or y0 < 0 or x0 + w > im["width"] or y0 + h > im["height"]:
                seen["straddle"] += 1
            else:
                seen["inside"] += 1
        for fr in im["frames"][:-1]:
            seen["saves"].add(fr.get("save_as_reference", 0))
            seen["sbct"] += bool(fr.get("save_before_ct"))
    assert seen["modes"] == seen["ec_modes"] == set(C.MODES) and seen["slots"] == seen["saves"] == {0, 1, 2, 3}
    assert min(seen["sbct"], seen["outside"], seen["straddle"], seen["inside"], seen["grey"], seen["negative"]) >= 3, seen


@pytest.mark.parametrize("part", range(4))
def test_multi_frame_images_equal_blend_ref_on_their_source_frames(backend, part):
    names = sorted(C.MULTI)[part::4]
    for name in names:
        im = C.MULTI[name]
        dec, got = decode(im, backend)
        check_outputs(im, got, C.decode_model(im), name)
        dec.close()


def test_every_mode_clamp_and_premultiplication(backend):
    for name, im in C.MULTI_FIXED.items():
        dec, got = decode(im, backend)
        check_outputs(im, got, C.decode_model(im), name)
        dec.close()


# ---- upsampled frames -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.UPSAMPLED))
def test_upsampled_frames_within_the_upsampling_bound(backend, name):
    im = C.UPSAMPLED[name]
    dec, got = decode(im, backend)
    planes = got.getBuffer()
    model = C.upsampled_model(im)
    assert len(planes) == len(model)
    for c, (x, a) in enumerate(model):
        if a is None:
            assert_bits_equal(planes[c], x, "%s plane %d" % (name, c))
        else:
            assert planes[c].dtype == np.float32 and planes[c].shape == x.shape, (name, c)
            ratio(planes[c], x, a, "%s plane %d" % (name, c), K["upsample"])


# ---- the route tables name every string the route functions return -----------------------------------------------------------
ROUTE_FUNCTIONS = ("_one_plan_chain_rule", "_int_rgb_planes_rule", "_modular_frame_route", "frame_set_rule", "patch_sets_rule", "_frame_set_route",
                   "_canvas_route")


def route_literals():
    """every string literal that the route functions return or assign to `why` / self._landed / _land(...): a text scan of decoder.py"""
    src = open(os.path.join(ROOT, "jxlatte_amd", "decoder.py")).read()
    out = {}
    for fn in ROUTE_FUNCTIONS:
        m = re.search(r"\n    def %s\(.*?(?=\n    def |\n    @staticmethod|\nclass )" % fn, src, re.S)
        assert m, fn
        body = re.sub(r'""".*?"""', "", m.group(0), flags=re.S)
        lits = re.findall(r'(?:return|why =|self\._landed =|self\._land\()\s*"([^"]+)"', body)
        assert lits, fn
        out[fn] = lits
    return out


def test_every_route_string_has_a_case_or_a_reason():
    lits = route_literals()
    assert sum(len(v) for v in lits.values()) >= 30
    known = set(C.ROUTE_CASES) | set(C.UNREACHABLE)
    missing = [(fn, s) for fn, v in lits.items() for s in v if s not in known]
    assert not missing, missing
    stale = [s for s in known if not any(s in v for v in lits.values())]
    assert not stale, stale
    assert not set(C.ROUTE_CASES) & set(C.UNREACHABLE)
    for s, why in C.UNREACHABLE.items():
        assert isinstance(why, str) and len(why) > 20 and "\n" not in why, s
    for s, (table, name, switches, (where, k)) in C.ROUTE_CASES.items():
        assert name in C.table(table) and where in ("image", "frame", "canvas", "rule") and k < len(C.table(table)[name]["frames"]), (s, table, name)
    for s, (table, name, switches, stats) in C.ACCEPTED.items():
        assert name in C.table(table), (s, table, name)


def test_float_samples(backend):
    """second tier: float samples are the stream's integers converted, as Frame.java:443-448 converts them (typed_planes)"""
    for name, im in C.FLOATS.items():
        dec, got = decode(im, backend)
        check_outputs(im, got, C.expected_planes(im), name)
        dec.close()


def test_routed_images_equal_their_model(backend):
    """the images made for a route, patches among them (tests/patches_model.py on the source frames), on the default route"""
    for name, im in C.ROUTED.items():
        dec, got = decode(im, backend)
        check_outputs(im, got, C.decode_model(im), name)
        dec.close()
