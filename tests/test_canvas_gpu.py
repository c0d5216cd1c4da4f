"""The resident canvas on the device: jxl_canvas_blend (k_canvas.hip) against tests/blend_ref.py and against a chain of host.blend
calls, bit for bit; the plane sets (clone, cast, the resident planes in and out); JXLDecoder(device_canvas=True) on every
committed bitstream against the default decoder; what crosses the bus. No tolerance anywhere: the arithmetic is jxl_blend.h's
under -ffp-contract=off; NaNs are compared as one value (conftest.assert_bits_equal, any_nan)."""
import glob
import os

import numpy as np
import pytest

import blend_ref as R
from conftest import assert_bits_equal
from jxlatte_amd import abi, frontend, host, synth
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, JXLImage, PNGWriter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
F, I = np.dtype(np.float32), np.dtype(np.int32)
HE, IA, CL, PM = abi.BLEND_FLAG_HAS_EXTRA, abi.BLEND_FLAG_IS_ALPHA, abi.BLEND_FLAG_CLAMP, abi.BLEND_FLAG_PREMULT
NAN_A, NAN_B = np.array([0x7fc12345, 0xffc00abc], np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx = host, ctx
    return be


def plane(rng, dt, shape):
    if dt == I:
        a = rng.integers(-70000, 70000, shape).astype(np.int32)
        a.reshape(-1)[::9] = np.int32(2147483647)  # the int sum wraps
        return a
    a = rng.normal(0.4, 0.9, shape).astype(np.float32)
    flat = a.reshape(-1)
    flat[::7] = NAN_A
    flat[3::19] = NAN_B
    flat[1::11] = np.float32(-0.0)
    flat[2::13] = np.float32(0.0)
    flat[4::17] = np.float32(1.75)
    flat[5::23] = np.float32(np.inf)
    return a


def expected(canvas, frame, ref, rect, chans):
    """the channels in canvas order through blend_ref's functions; `ref is canvas` for the aliased arrangement"""
    bh, bw, py, px, fy, fx, ry, rx = rect
    args = ((py, px), (fy, fx), (ry, rx), (bh, bw))
    for c, (fp, mode, flags, fa, ra) in enumerate(chans):
        he = bool(flags & HE)
        if mode == abi.BLEND_REPLACE:
            R.copy_to_canvas(canvas[c], (py, px), (fy, fx), (bh, bw), frame[fp])
        elif mode == abi.BLEND_ADD:
            R.blend_add(canvas[c], frame[fp], ref[c], *args)
        elif mode == abi.BLEND_MULT:
            R.blend_mult(canvas[c], frame[fp], ref[c], *args, bool(flags & CL))
        elif mode == abi.BLEND_BLEND:
            R.blend_blend(canvas[c], frame[fp], ref[c], frame[fa] if he else None, ref[ra] if he else None, *args, bool(flags & IA), he,
                          bool(flags & CL), bool(flags & PM))
        else:
            R.blend_muladd(canvas[c], frame[fp], ref[c], frame[fa] if he else None, *args, bool(flags & IA), he, bool(flags & CL))


def blend_chain(ctx, canvas, frame, ref, rect, chans):
    """the same through one host.blend call per channel (what JXLDecoder._blend_frame does without the switch); `ref is canvas`
    for the aliased arrangement: a later channel reads the planes the calls before it returned"""
    for c, (fp, mode, flags, fa, ra) in enumerate(chans):
        he = bool(flags & HE)
        canvas[c] = host.blend(ctx, mode, canvas[c], frame[fp], None if ref is None else ref[c], rect,
                               frameAlpha=frame[fa] if he and frame[fa].dtype == F else None,
                               refAlpha=ref[ra] if he and ref is not None and ref[ra].dtype == F else None,
                               isAlpha=bool(flags & IA), hasExtra=he, clamp=bool(flags & CL), premult=bool(flags & PM))
    return canvas


def draw_case(rng, n_extra, arrangement):
    """plane types and a descriptor that jxl_canvas_blend_check accepts: per channel one type for canvas, frame and reference;
    int32 planes take the copy, the int sum and blendMulAdd's alpha copy only; the alpha planes a float function reads are float"""
    n = 3 + n_extra
    he = HE if n_extra else 0
    alpha_of = [int(rng.integers(0, n_extra)) if n_extra else 0 for _ in range(n)]
    is_alpha = [False] * 3 + [bool(rng.integers(0, 2)) or e == 0 for e in range(n_extra)]
    types_, chans = [None] * n, []
    need_float = set()
    modes = [int(rng.integers(0, 5)) for _ in range(n)]
    if arrangement == "null":
        modes = [abi.BLEND_REPLACE] * n
    for c in range(n):
        m = modes[c]
        reads_alpha = bool(n_extra) and not is_alpha[c] and m in (abi.BLEND_BLEND, abi.BLEND_MULADD)
        if reads_alpha:
            need_float.add(3 + alpha_of[c])
    for c in range(n):
        m = modes[c]
        int_ok = m in (abi.BLEND_REPLACE, abi.BLEND_ADD) or (not n_extra and m in (abi.BLEND_BLEND, abi.BLEND_MULADD)) or \
            (bool(n_extra) and m == abi.BLEND_MULADD and is_alpha[c])
        types_[c] = I if int_ok and c not in need_float and rng.random() < 0.5 else F
        flags = he | (IA if is_alpha[c] else 0) | (CL if rng.integers(0, 2) else 0) | (PM if rng.integers(0, 2) else 0)
        chans.append((c, m, flags, 3 + alpha_of[c] if n_extra else 0, 3 + alpha_of[c] if n_extra else 0))
    copies_alpha = any(bool(n_extra) and modes[c] == abi.BLEND_MULADD and is_alpha[c] for c in range(n))
    return types_, chans, copies_alpha


def run_case(ctx, rng, cshape, fshape, rshape, arrangement, size, offs, n_extra, chain):
    types_, chans, copies_alpha = draw_case(rng, n_extra, arrangement)
    (cy, cx), (fy, fx), (ry, rx) = offs
    if arrangement == "alias":
        if copies_alpha:  # blendMulAdd's alpha copy reads the reference at frameOffset: in place only at the written pixel
            cy, cx = fy, fx
        ry, rx = cy, cx
    rect = (size[0], size[1], cy, cx, fy, fx, ry, rx)
    n = 3 + n_extra
    canvas = [plane(rng, types_[c], cshape) for c in range(n)]
    frame = [plane(rng, types_[c], fshape) for c in range(n)]
    ref = None if arrangement == "null" else canvas if arrangement == "alias" else [plane(rng, types_[c], rshape) for c in range(n)]
    what = "%s %s canvas %s frame %s rect %s chans %s types %s" % (arrangement, n_extra, cshape, fshape, rect, chans, [t.name for t in types_])
    # the model
    e_canvas = [R.Buf(a) for a in canvas]
    e_ref = None if ref is None else e_canvas if ref is canvas else [R.Buf(a) for a in ref]
    expected(e_canvas, [R.Buf(a) for a in frame], e_ref, rect, chans)
    # the launch
    cv = host.DeviceCanvas.fromArrays(ctx, canvas)
    fs = host.DeviceCanvas.fromArrays(ctx, frame)
    rf = None if ref is None else cv if ref is canvas else host.DeviceCanvas.fromArrays(ctx, ref)
    try:
        host.canvas_blend(cv, fs, rf, rect, chans)
        got = [cv.download(c) for c in range(n)]
        if rf is not None and rf is not cv:
            for c in range(n):
                assert_bits_equal(rf.download(c), ref[c], what + ": the reference set is read only, plane %d" % c)
        for c in range(n):
            assert_bits_equal(fs.download(c), frame[c], what + ": the frame set is read only, plane %d" % c)
    finally:
        for s_ in {id(s_): s_ for s_ in (cv, fs, rf) if s_ is not None}.values():
            s_.release()
    inside = np.zeros(cshape, bool)
    inside[cy:cy + size[0], cx:cx + size[1]] = True
    for c in range(n):
        assert got[c].dtype == types_[c]
        assert_bits_equal(got[c], e_canvas[c].a, what + " plane %d vs blend_ref" % c, any_nan=True)
        # pixels outside the rectangle keep their bits, NaN payloads included
        assert np.array_equal(got[c].view(np.uint32)[~inside], canvas[c].view(np.uint32)[~inside]), what + " plane %d outside" % c
    if chain:
        h_canvas = [a.copy() for a in canvas]
        h_ref = None if ref is None else h_canvas if ref is canvas else [a.copy() for a in ref]
        h_canvas = blend_chain(ctx, h_canvas, frame, h_ref, rect, chans)
        for c in range(n):
            assert_bits_equal(got[c], h_canvas[c], what + " plane %d vs host.blend" % c, any_nan=True)


@pytest.mark.parametrize("n_extra", [0, 1, 2])
def test_kernel_against_the_model_and_the_blend_calls(ctx, n_extra):
    """canvas 37 x 53, frame 20 x 45, reference of either size; rect widths 1, 3, 4, 5 there and 63, 64, 65 on a 40 x 131
    canvas; canvas, frame and reference x offsets 0..3 independently; every mode per channel, mixed in one call; int32 and float
    planes; NaN, +-0, values outside 0..1 and infinities with clamp on and off; the three reference arrangements. One case in
    eight also runs the chain of host.blend calls."""
    rng = np.random.default_rng(100 + n_extra)
    k = 0
    for width in (1, 3, 4, 5, 63, 64, 65):
        wide = width > 5
        cshape, fshape = ((40, 131), (20, 72)) if wide else ((37, 53), (20, 45))
        for cx in range(4):
            for fx in range(4):
                for rx in range(4):
                    arrangement = ("other", "alias", "null")[k % 3]
                    rshape = cshape if (k // 3) % 2 or arrangement != "other" else fshape
                    height = (1, 7, 18)[k % 3]
                    cy, fy = int(rng.integers(0, cshape[0] - height + 1)), int(rng.integers(0, fshape[0] - height + 1))
                    ry = cy if rshape == cshape else fy
                    run_case(ctx, rng, cshape, fshape, rshape, arrangement, (height, width), ((cy, cx), (fy, fx), (ry, rx)), n_extra,
                             chain=k % 8 == 0)
                    k += 1


def test_every_mode_on_every_kind_of_channel(ctx):
    """each mode once on the colours, on an alpha channel and on a non-alpha extra channel, float planes, clamp and premult on
    and off, whole-canvas and clipped rectangles -- drawn cases above may miss a combination; these do not"""
    rng = np.random.default_rng(7)
    shape = (37, 53)
    for mode in range(5):
        for ec_mode in range(5):
            for flags_extra in (0, CL, PM, CL | PM):
                chans = [(c, mode, HE | flags_extra, 4, 4) for c in range(3)] + \
                        [(3, ec_mode, HE | flags_extra, 4, 4), (4, ec_mode, HE | IA | flags_extra, 4, 4)]
                canvas = [plane(rng, F, shape) for _ in range(5)]
                frame = [plane(rng, F, (20, 45)) for _ in range(5)]
                for arrangement in ("alias", "other"):
                    rect = (20, 45, 9, 5, 0, 0, 9, 5) if arrangement == "other" else (11, 30, 9, 5, 9, 5, 9, 5)
                    ref = canvas if arrangement == "alias" else [plane(rng, F, shape) for _ in range(5)]
                    e_canvas = [R.Buf(a) for a in canvas]
                    e_ref = e_canvas if ref is canvas else [R.Buf(a) for a in ref]
                    expected(e_canvas, [R.Buf(a) for a in frame], e_ref, rect, chans)
                    cv, fs = host.DeviceCanvas.fromArrays(ctx, canvas), host.DeviceCanvas.fromArrays(ctx, frame)
                    rf = cv if ref is canvas else host.DeviceCanvas.fromArrays(ctx, ref)
                    try:
                        host.canvas_blend(cv, fs, rf, rect, chans)
                        for c in range(5):
                            assert_bits_equal(cv.download(c), e_canvas[c].a, "mode %d ec %d flags %d %s plane %d" % (mode, ec_mode, flags_extra, arrangement, c),
                                              any_nan=True)
                    finally:
                        for s_ in {id(s_): s_ for s_ in (cv, fs, rf)}.values():
                            s_.release()


def test_clone_gives_independent_sets_and_aliased_use_does_not(ctx):
    rng = np.random.default_rng(11)
    shape = (37, 53)
    canvas = [plane(rng, F, shape) for _ in range(4)]
    frames = [[plane(rng, F, (20, 45)) for _ in range(4)] for _ in range(2)]
    chans = [(c, abi.BLEND_BLEND, HE, 3, 3) for c in range(3)] + [(3, abi.BLEND_BLEND, HE | IA, 3, 3)]
    # alpha FIRST in memory order is not what the reference does: channel 3 comes last, so the colours see the OLD alpha; a
    # second blend then sees the alpha the first one left -- one aliased array in the model
    rects = [(20, 45, 3, 2, 0, 0, 3, 2), (12, 40, 20, 9, 5, 1, 20, 9)]
    e_canvas = [R.Buf(a) for a in canvas]
    cv = host.DeviceCanvas.fromArrays(ctx, canvas)
    snap = cv.clone()
    sets = [cv, snap]
    try:
        for fr, rect in zip(frames, rects):
            fs = host.DeviceCanvas.fromArrays(ctx, fr)
            sets.append(fs)
            host.canvas_blend(cv, fs, cv, rect, chans)
            expected(e_canvas, [R.Buf(a) for a in fr], e_canvas, rect, chans)
        for c in range(4):
            assert_bits_equal(cv.download(c), e_canvas[c].a, "aliased twice, plane %d" % c, any_nan=True)
            assert_bits_equal(snap.download(c), canvas[c], "the clone kept the samples it was made from, plane %d" % c)
        # the clone as the reference of a third blend into the canvas: read only
        fs = host.DeviceCanvas.fromArrays(ctx, frames[0])
        sets.append(fs)
        host.canvas_blend(cv, fs, snap, rects[0], chans)
        expected(e_canvas, [R.Buf(a) for a in frames[0]], [R.Buf(a) for a in canvas], rects[0], chans)
        for c in range(4):
            assert_bits_equal(cv.download(c), e_canvas[c].a, "from the clone, plane %d" % c, any_nan=True)
            assert_bits_equal(snap.download(c), canvas[c], "the clone is untouched, plane %d" % c)
        assert snap.id != cv.id and snap.types == cv.types and snap.shape == cv.shape
    finally:
        for s_ in sets:
            s_.release()
    with pytest.raises(Exception):
        cv.download(0)  # released


@pytest.mark.parametrize("depth", [1, 8, 12, 16, 31])
def test_cast_equals_modular_to_float(ctx, depth):
    rng = np.random.default_rng(depth)
    maxv = (1 << depth) - 1
    a = rng.integers(-5, min(maxv, 2 ** 31 - 6) + 5, (37, 53), dtype=np.int64).astype(np.int32)
    a.reshape(-1)[:4] = [0, maxv, -2147483648, 2147483647]
    fl = plane(rng, F, (37, 53))
    cv = host.DeviceCanvas.fromArrays(ctx, [a, fl])
    try:
        cv.cast(0, depth)
        cv.cast(1, depth)  # nothing happens to a float plane
        assert cv.types == [abi.PLANE_FLOAT, abi.PLANE_FLOAT]
        got = cv.download(0)
        exp = host.modularToFloat(ctx, a, None, float(np.float32(1) / np.float32(maxv)))
        assert_bits_equal(got, exp.reshape(a.shape), "depth %d" % depth)
        assert_bits_equal(cv.download(1), fl, "float plane")
        bad = host.DeviceCanvas.fromArrays(ctx, [a])
        try:
            with pytest.raises(Exception) as e:
                bad.cast(0, 32)  # invalid Max Value (ImageBuffer.java:115-116)
            assert getattr(e.value, "status", None) == abi.JXL_ERR_INVALID_ARGUMENT
        finally:
            bad.release()
    finally:
        cv.release()


def test_resident_planes_round_trip_and_plane_limit(ctx):
    rng = np.random.default_rng(3)
    planes = np.stack([plane(rng, F, (19, 23)) for _ in range(3)])
    rp = host.ResidentPlanes.upload(ctx, planes)
    alpha = rng.integers(0, 255, (19, 23)).astype(np.int32)
    fs = host.DeviceCanvas.fromPlanes(ctx, [I])
    try:
        assert fs.shape == (19, 23) and fs.types == [0, 0, 0, 1]
        assert not fs.download(3).any()
        fs.upload(3, alpha)
        for c in range(3):
            assert_bits_equal(fs.download(c), planes[c], "from_planes %d" % c)
        assert_bits_equal(fs.download(3), alpha, "extra plane")
        # other samples into the resident planes, then the set back over them
        host.ResidentPlanes.upload(ctx, np.zeros((3, 5, 7), np.float32))
        back = fs.toPlanes()
        assert back.shape == (19, 23) and not rp.live()
        assert_bits_equal(back.download(), planes, "to_planes")
        # int colour planes do not become resident planes
        ints = host.DeviceCanvas.fromArrays(ctx, [alpha, alpha, alpha])
        with pytest.raises(Exception):
            ints.toPlanes()
        ints.release()
        with pytest.raises(Exception) as e:
            host.DeviceCanvas.create(ctx, [F] * 17, 4, 4)
        assert getattr(e.value, "status", None) == abi.JXL_ERR_UNSUPPORTED
    finally:
        fs.release()


# ---- the decoder ----------------------------------------------------------------------------------------------------------
def _decode(path, backend, orientation=None, **kw):
    dec = JXLDecoder(path, backend=backend, **kw)
    if orientation is not None:
        dec.info.orientation = orientation
    return dec, dec.decode()


def _compare(path, backend, orientation=None):
    name = os.path.splitext(os.path.basename(path))[0]
    dec, im = _decode(path, backend, orientation, device_canvas=True)
    writers = {hdr: PNGWriter(im, hdr=hdr, deviceSamples=True) for hdr in (False, True)}  # (while the planes are the image's)
    buf = im.getBuffer()
    ref_dec, ref_im = _decode(path, backend, orientation)
    assert [s["canvas"] for s in ref_dec.stats] == ["host"] * len(ref_dec.stats)
    exp = ref_im.getBuffer()
    assert len(buf) == len(exp)
    for c in range(len(buf)):
        assert buf[c].dtype == exp[c].dtype and buf[c].shape == exp[c].shape, (name, c, buf[c].dtype, exp[c].dtype)
        assert_bits_equal(buf[c], exp[c], "%s plane %d" % (name, c), any_nan=True)
    for hdr, w in writers.items():
        r = PNGWriter(ref_im, hdr=hdr, deviceColor=True)
        assert (w.bitDepth, w.colorMode, w.width, w.height) == (r.bitDepth, r.colorMode, r.width, r.height), (name, hdr)
        assert w.samples.dtype == r.samples.dtype and w.samples.shape == r.samples.shape, (name, hdr)
        assert np.array_equal(w.samples, r.samples), "%s hdr %d: %d samples differ" % (name, hdr, int((w.samples != r.samples).sum()))
    stats = dec.stats
    dec.close()
    return stats, ref_dec.stats, im


@pytest.mark.parametrize("path", SAMPLES, ids=NAMES)
def test_decoder_on_every_sample_equals_the_default_decoder(backend, path):
    name = os.path.splitext(os.path.basename(path))[0]
    stats, ref_stats, im = _compare(path, backend)
    print(name, [s["canvas"] for s in stats], [s.get("blend_bus") for s in stats], [s.get("blend_bus") for s in ref_stats])
    assert len(stats) == len(ref_stats)
    if name in ("blendmodes_5", "wb-rainbow"):
        assert [s["canvas"] for s in stats] == ["device"] * 5, name
        assert stats[-1]["output"] == "device" and im.resident is not None
    elif name == "patches-lossless":
        assert stats[-1]["canvas"] == "landed: a frame with patches", stats[-1]["canvas"]
        assert stats[-1]["output"] == "host" and im.resident is None
    else:  # single-frame images: the frame goes onto a device canvas or lands with a reason; the pixels are those above
        assert len(stats) == 1 and (stats[0]["canvas"] == "device" or stats[0]["canvas"].startswith("landed: ")), stats[0]["canvas"]


@pytest.mark.parametrize("path", SAMPLES, ids=NAMES)
def test_device_output_alone_reports_what_it_reported(backend, path):
    """the switch of its own: device_output=True is what it was -- lenna and bbb stay on the device, the multi-frame images are
    host images (tests/test_png_device_output_gpu.py), and its frames never report a device canvas; both switches together:
    the single-frame path takes precedence"""
    name = os.path.splitext(os.path.basename(path))[0]
    dec, im = _decode(path, backend, device_output=True)
    out = dec.stats[-1]["output"]
    assert [s["canvas"] for s in dec.stats] == ["host"] * len(dec.stats)
    if name in ("lenna", "bbb"):
        assert out == "device" and im.onDevice()
    if name in ("blendmodes_5", "wb-rainbow", "patches-lossless"):
        assert out == "host" and not im.onDevice()
    assert out in ("device", "host") and (out == "device") == im.onDevice()
    if out != "device":  # (both switches on such an image: device_canvas alone, the test above)
        return
    both, im2 = _decode(path, backend, device_output=True, device_canvas=True)
    assert both.stats[-1]["output"] == "device" and both.stats[-1]["canvas"] == "host" and "d2h" not in both.stats[-1]["plane_moves"]
    got = im2.getBuffer()
    exp = _decode(path, backend)[1].getBuffer()
    for c, b in enumerate(got):
        assert b.dtype == exp[c].dtype
        assert_bits_equal(b, exp[c], "%s both switches, plane %d" % (name, c), any_nan=True)
    both.close()


@pytest.mark.parametrize("orientation", [3, 6])
def test_orientation_forced_on_wb_rainbow(backend, orientation):
    stats, _, im = _compare(os.path.join(ROOT, "tests", "golden", "samples", "wb-rainbow.jxl"), backend, orientation)
    assert [s["canvas"] for s in stats] == ["device"] * 5
    assert (im.getHeight(), im.getWidth()) == ((1152, 2048) if orientation == 3 else (2048, 1152))


def test_the_canvas_never_comes_down_before_the_last_frame(backend):
    """blendmodes_5 (1024 x 1024, RGB + alpha, five frames): with the switch the blend path brings nothing down in any frame
    and sends up only the frame's own planes; without it every frame's blend calls bring every canvas plane down"""
    path = os.path.join(ROOT, "tests", "golden", "samples", "blendmodes_5.jxl")
    plane_bytes = 4 * 1024 * 1024
    ctx = backend.ctx
    ctx.blend_bus = [0, 0]
    dec, im = _decode(path, backend, device_canvas=True)
    on = [s["blend_bus"] for s in dec.stats]
    total_on = tuple(ctx.blend_bus)
    assert all(down == 0 for _, down in on), on
    assert all(up <= 4 * plane_bytes for up, _ in on), on  # at most the frame's four planes, once each
    # after the last frame: the alpha plane for the image, and the colour planes only where they are not float (then no resident image)
    assert total_on[1] == (plane_bytes if im.onDevice() else 4 * plane_bytes), total_on
    dec.close()
    ctx.blend_bus = [0, 0]
    ref_dec, _ = _decode(path, backend)
    off = [s["blend_bus"] for s in ref_dec.stats]
    assert all(down == 4 * plane_bytes for _, down in off), off
    assert all(up >= 8 * plane_bytes for up, _ in off), off
    print("blend path bytes per frame (up, down): device canvas %s; host canvas %s" % (on, off))


def test_synthetic_float_sequence_through_the_host_layer(backend):
    """three 64 x 48 VarDCT frames with resident colour planes and a float alpha plane: REPLACE, then BLEND and MULADD at non-zero
    origins, the last clipped by the canvas edge. The canvas equals the chain of host.blend calls on the downloaded planes; it
    ends as a resident image whose PNGWriter(deviceSamples=True) moves only the alpha up and the samples down"""
    ctx = backend.ctx
    rng = np.random.default_rng(5)
    ch, cw = 60, 80
    steps = [(abi.BLEND_REPLACE, (0, 0), (48, 64)), (abi.BLEND_BLEND, (7, 9), (48, 64)), (abi.BLEND_MULADD, (20, 30), (40, 50))]
    cv = host.DeviceCanvas.create(ctx, [F] * 4, ch, cw)
    h_canvas = [np.zeros((ch, cw), np.float32) for _ in range(4)]
    dead = []
    try:
        for k, (mode, (y0, x0), (bh, bw)) in enumerate(steps):
            fr = host.Frame.from_synth(ctx, synth.make_vardct_frame(64, 48, seed=40 + k))
            rp = fr.keepPlanes(48, 64)
            alpha = rng.random((48, 64)).astype(np.float32)
            alpha[::5, ::3] = np.float32(1.25)
            ctx.blend_bus = [0, 0]
            fs = host.DeviceCanvas.fromPlanes(ctx, [F])
            fs.upload(3, alpha)
            dead.append(fs)
            rect = (bh, bw, y0, x0, 0, 0, y0, x0)
            # (the alpha channel has a blending info of its own: BLEND where the colours take MULADD -- blendMulAdd would copy it out
            # of the canvas at frameOffset, :390, which no in-place launch replays and the type plan lands)
            a_mode = abi.BLEND_BLEND if mode == abi.BLEND_MULADD else mode
            chans = [(c, mode, HE | CL, 3, 3) for c in range(3)] + [(3, a_mode, HE | IA | CL, 3, 3)]
            host.canvas_blend(cv, fs, cv if mode != abi.BLEND_REPLACE else None, rect, chans)
            assert ctx.blend_bus == [alpha.nbytes, 0], ctx.blend_bus  # the colours never crossed the bus
            planes = list(rp.download()) + [alpha]
            h_canvas = blend_chain(ctx, h_canvas, planes, h_canvas if mode != abi.BLEND_REPLACE else None, rect, chans)
        for c in range(4):
            assert_bits_equal(cv.download(c), h_canvas[c], "synthetic sequence, plane %d" % c, any_nan=True)
        info = frontend.ImageInfo()
        info.width, info.height, info.orientation, info.bits_per_sample, info.num_extra = cw, ch, 1, 8, 1
        ref_info = JXLDecoder(SAMPLES[NAMES.index("lenna")], backend=backend).info  # (colour tags of a real header)
        info.colour_space, info.transfer = 0, ref_info.transfer
        info.white_xy, info.prim_xy, info.white_point, info.primaries = ref_info.white_xy, ref_info.prim_xy, ref_info.white_point, ref_info.primaries
        info.ec_type[0], info.ec_bits[0] = 0, 8
        a_plane = cv.download(3)
        im = JXLImage([None] * 3 + [a_plane], info, backend, resident=cv.toPlanes())
        w = PNGWriter(im, deviceSamples=True)
        assert w.bus_bytes == (a_plane.nbytes, w.samples.nbytes), w.bus_bytes
        r = PNGWriter(JXLImage([a.copy() for a in h_canvas], info, backend), deviceColor=True)
        assert w.samples.dtype == r.samples.dtype and np.array_equal(w.samples, r.samples)
    finally:
        for s_ in dead + [cv]:
            s_.release()
