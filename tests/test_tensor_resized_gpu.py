"""The image resampled to a device tensor in one pass (jxl_stage_tensor_resized / jxl_planes_tensor_resized /
jxl_canvas_tensor_resized, csrc/k_tensor_resize.hip), bit for bit against pinned entries around the numpy model:
  1. jxl_stage_color_convert with a linear output: the stage 1-5 planes
  2. tests/resize_ref.py on them and on the cast alpha: the filter, vertical pass first, sequential f32 sums
  3. jxl_stage_color_convert from linear to the target curve: stage 6
  4. tests/tensor_ref.py: un-premultiplication, normalisation, rounding, layout (the U8 quantiser: jxl_stage_tensor_samples on
     the model's float planes, itself pinned against the PNG entry)
Outputs are 0xA5-filled torch memory with guard bytes around the tensor. NaNs compare as one value."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import resize_ref as rr
import tensor_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import abi, host
from jxlatte_amd.decoder import PRI_P3, PRI_SRGB, WP_D65, get_conversion_matrix

pytestmark = pytest.mark.gpu
F = np.float32
DTYPES = ["uint8", "float16", "bfloat16", "float32"]
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
VIEW = {1: np.uint8, 2: np.uint16, 4: np.uint32}
GRID_TF = [(abi.TF_LINEAR, 0), (abi.TF_SRGB, 0), (abi.TF_BT709, 0), (abi.TF_PQ, 0), (abi.TF_GAMMA, 4545455)]
MATRIX = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65)
# (source (h, w), output (h, w), box (x0, y0, w, h) or None)
CASES = [((1, 1), (1, 1), None), ((1, 1), (3, 2), None), ((5, 7), (2, 3), None), ((5, 7), (13, 11), None), ((33, 67), (8, 5), None),
         ((64, 48), (4, 3), None), ((3, 2100), (2, 5), None), ((67, 33), (67, 33), None), ((33, 67), (6, 4), (3, 2, 20, 9))]
SOURCES = sorted({c[0] for c in CASES})
FILTERS = [("triangle", rr.TRIANGLE), ("box", rr.BOX)]


def _float_plane(seed, shape):
    """finite: [0, 1), some above 1, negatives, tiny values and f32 denormals"""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    v = np.concatenate([rng.uniform(0, 1, n).astype(F), rng.uniform(1, 4, n // 8 + 1).astype(F), -rng.uniform(0, 2, n // 8 + 1).astype(F),
                        (10 ** rng.uniform(-12, 0, n // 8 + 1)).astype(F), np.array([1e-45, -1e-45, 3e-39, 0.0, -0.0], F)])
    rng.shuffle(v)
    return np.ascontiguousarray(v[:n].reshape(shape))


def _alpha(kind, seed, shape, mx=255):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    a = rng.uniform(0.05, 1, n).astype(F) if kind == "float" else rng.integers(1, mx + 1, n).astype(np.int32)
    if n > 64:
        a[:4] = [0.0, 1.0, 1.5, 1e-30] if kind == "float" else [0, mx, mx + 45, -1]
    rng.shuffle(a)
    return a.reshape(shape)


def _alpha_float(alpha, depth):
    if alpha.dtype == np.float32:
        return alpha
    return (alpha.astype(F) * F(F(1) / F((1 << depth) - 1))).astype(F)


@pytest.fixture(scope="module")
def data():
    """the inputs of every test here, made once and never written"""
    d = {}
    for shape in SOURCES:
        d[shape] = dict(f=[_float_plane(s, shape) for s in (1, 2, 3)],
                        i=[np.random.default_rng(s).integers(0, 256, shape).astype(np.int32) for s in (4, 5, 6)],
                        af=_alpha("float", 7, shape), a8=_alpha("int", 8, shape), a10=_alpha("int", 9, shape, 1023))
        for v in d[shape].values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return d


def _pin(src):
    return (C.c_void_p * 3)(*([a.ctypes.data for a in src] + [None] * (3 - len(src))))


def _raw(ctx, src, alpha, size, box, resample, dtype, layout, lead=0, entry=None, **params):
    """one call into torch memory pre-filled with 0xA5, the tensor `lead` elements into it: (status, channels, the bytes before,
    the tensor's elements, the bytes after)"""
    shape = src[0].shape
    p = host.tensorParams(src, shape, alpha=alpha, dtype=dtype, layout=layout, **params)
    r = host.resizeParams(shape, size, box, resample)
    e = ELEM[dtype]
    nbytes = size[0] * size[1] * host.tensorChannels(p) * e
    buf = torch.empty(lead * e + nbytes + 64, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)
    ptr = buf.data_ptr() + lead * e
    if entry is None:
        st = ctx.lib.jxl_stage_tensor_resized(ctx.h, _pin(src), alpha.ctypes.data if alpha is not None else None, C.byref(p), C.byref(r), C.c_void_p(ptr))
    else:
        st = entry(p, r, ptr)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return st, host.tensorChannels(p), b[:lead * e], b[lead * e:lead * e + nbytes].copy().view(VIEW[e]), b[lead * e + nbytes:]


def _resized(ctx, src, alpha, size, box, resample, dtype, layout, **kw):
    """the tensor's element bits, [C][H][W] or [H][W][C]; nothing written around it"""
    st, c, before, body, after = _raw(ctx, src, alpha, size, box, resample, dtype, layout, **kw)
    assert st == abi.JXL_OK, (st, ctx.lib.jxl_last_error(ctx.h))
    assert np.all(before == 0xA5) and np.all(after == 0xA5), "a store outside the tensor"
    return body.reshape((c,) + tuple(size) if layout == "CHW" else tuple(size) + (c,))


def _unresized(ctx, src, alpha, dtype, layout, **params):
    """jxl_stage_tensor_samples: the pinned entry beside the new ones"""
    shape = src[0].shape
    p = host.tensorParams(src, shape, alpha=alpha, dtype=dtype, layout=layout, **params)
    c, e = host.tensorChannels(p), ELEM[dtype]
    buf = torch.empty(shape[0] * shape[1] * c * e, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    st = ctx.lib.jxl_stage_tensor_samples(ctx.h, _pin(src), alpha.ctypes.data if alpha is not None else None, C.byref(p), C.c_void_p(buf.data_ptr()))
    assert st == abi.JXL_OK, (st, ctx.lib.jxl_last_error(ctx.h))
    return buf.cpu().numpy().view(VIEW[e]).reshape((c,) + shape if layout == "CHW" else shape + (c,))


def _filtered(ctx, src, alpha, size, box, filt, premultiplied=False, writeAlpha=False, alphaDepth=8, tfOut=abi.TF_LINEAR, gammaOut=0, **front):
    """steps 1-3 and the un-premultiplication: the float planes of the output channels (colours, then alpha when written)"""
    h, w = src[0].shape
    bx = (0, 0, w, h) if box is None else box
    ty, tx = rr.taps(bx[3], size[0], filt), rr.taps(bx[2], size[1], filt)
    with np.errstate(all="ignore"):
        lin = host.colorConvert(ctx, src, maxValue=0, tfOut=abi.TF_LINEAR, **front)
        mid = [rr.resample(p, ty, tx, bx) for p in lin]
        planes = host.colorConvert(ctx, mid, maxValue=0, tfIn=abi.TF_LINEAR, tfOut=tfOut, gammaOut=gammaOut)
        fa = rr.resample(_alpha_float(alpha, alphaDepth), ty, tx, bx) if alpha is not None and (premultiplied or writeAlpha) else None
        if premultiplied:
            planes = ref.unpremultiply(planes, fa)
    return planes + ([fa] if writeAlpha else []), mid


def _expected(ctx, chans, dtype, layout, mean=None, invStd=None):
    """step 4 on the float planes of the output channels: element bits in the layout"""
    if dtype == "uint8":  # castToInt0(v, 255) of every channel: the unresized entry with every stage off, a float alpha as it is
        n = len(chans)
        colors, alpha = (chans[:-1], chans[-1]) if n in (2, 4) else (chans, None)
        return _unresized(ctx, [np.ascontiguousarray(c) for c in colors], alpha, "uint8", layout, writeAlpha=alpha is not None)
    if mean is not None:
        chans = ref.normalise(chans, mean, invStd)
    return ref.layout(ref.convert(chans, dtype), layout)


def _same(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.dtype == np.uint32:
        assert_bits_equal(got.view(F), np.ascontiguousarray(exp).view(F), what, any_nan=True)
    else:
        assert np.array_equal(got, exp), "%s: %d of %d elements differ" % (what, int((got != exp).sum()), got.size)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d%s" % (c[0] + c[1] + ("-box" if c[2] else "",)))
def test_every_shape_filter_dtype_and_layout(ctx, data, case):
    shape, size, box = case
    d = data[shape]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB, matrix=MATRIX, scale=F(1.37))
    for name, filt in FILTERS:
        chans, _ = _filtered(ctx, d["f"], None, size, box, filt, **kw)
        for dtype, layout in itertools.product(DTYPES, ("CHW", "HWC")):
            got = _resized(ctx, d["f"], None, size, box, name, dtype, layout, lead=1 if layout == "HWC" else 0, **kw)
            _same(got, _expected(ctx, chans, dtype, layout), "%s %s %s %s" % (case, name, dtype, layout))
        # grey, grey through the matrix, RGB without one, integer planes
        for src, extra in ((d["f"][:1], dict()), (d["f"][:1], dict(matrix=MATRIX)), (d["f"], dict()), (d["i"], dict(inMax=[255] * 3)), (d["i"][:1], dict(inMax=[255]))):
            k2 = dict(tfIn=abi.TF_BT709, tfOut=abi.TF_SRGB, **extra)
            chans, _ = _filtered(ctx, src, None, size, box, filt, **k2)
            assert len(chans) == (3 if len(src) == 3 or "matrix" in extra else 1)
            got = _resized(ctx, src, None, size, box, name, "float32", "CHW", **k2)
            _same(got, _expected(ctx, chans, "float32", "CHW"), "%s %s %d planes %s" % (case, name, len(src), sorted(extra)))


def test_identity_equals_the_unresized_entry(ctx, data):
    d = data[(67, 33)]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_PQ, matrix=MATRIX, writeAlpha=True, premultiplied=True)
    for (name, _), dtype, layout in itertools.product(FILTERS, ("float32", "float16", "bfloat16"), ("CHW", "HWC")):
        got = _resized(ctx, d["f"], d["af"], (67, 33), None, name, dtype, layout, **kw)
        _same(got, _unresized(ctx, d["f"], d["af"], dtype, layout, **kw), "identity %s %s %s" % (name, dtype, layout))
    # and a crop at the identity ratio is the unresized tensor's window
    full = _unresized(ctx, d["f"], None, "float32", "CHW", tfOut=abi.TF_SRGB)
    got = _resized(ctx, d["f"], None, (40, 20), (5, 9, 20, 40), "triangle", "float32", "CHW", tfOut=abi.TF_SRGB)
    _same(got, np.ascontiguousarray(full[:, 9:49, 5:25]), "crop")


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[8], CASES[3]], ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_alpha_premultiplication_and_normalisation(ctx, data, case):
    shape, size, box = case
    d = data[shape]
    mean, std = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
    inv = [F(1) / F(s) for s in std]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_BT709)
    for (name, filt), n, (akey, depth), (premult, write) in itertools.product(FILTERS, (1, 3), (("af", 8), ("a8", 8), ("a10", 10)),
                                                                           ((True, True), (False, True), (True, False))):
        src, alpha = d["f"][:n], d[akey]
        chans, _ = _filtered(ctx, src, alpha, size, box, filt, premultiplied=premult, writeAlpha=write, alphaDepth=depth, **kw)
        for dtype, layout in (("float32", "CHW"), ("uint8", "HWC"), ("float16", "HWC"), ("bfloat16", "CHW")):
            what = "%s %s n %d alpha %s premult %d write %d %s %s" % (case, name, n, akey, premult, write, dtype, layout)
            got = _resized(ctx, src, alpha, size, box, name, dtype, layout, premultiplied=premult, writeAlpha=write, alphaDepth=depth, **kw)
            _same(got, _expected(ctx, chans, dtype, layout), what)
            if dtype != "uint8":
                got = _resized(ctx, src, alpha, size, box, name, dtype, layout, premultiplied=premult, writeAlpha=write, alphaDepth=depth,
                               mean=mean[:len(chans)], invStd=inv[:len(chans)], **kw)
                _same(got, _expected(ctx, chans, dtype, layout, mean, inv), what + " normalised")


def test_every_curve_pair(ctx):
    """planes in [0.01, 1]: below that PQ and gamma inputs make NaNs by the reference's own rule"""
    rng = np.random.default_rng(31)
    src = [rng.uniform(0.01, 1, (33, 67)).astype(F) for _ in range(3)]
    for (tf_in, g_in), (tf_out, g_out), use_matrix in itertools.product(GRID_TF, GRID_TF, (False, True)):
        kw = dict(tfIn=tf_in, gammaIn=g_in, tfOut=tf_out, gammaOut=g_out, matrix=MATRIX if use_matrix else None)
        chans, mid = _filtered(ctx, src, None, (8, 5), None, rr.TRIANGLE, **kw)
        assert all(np.isfinite(m).all() for m in mid)
        got = _resized(ctx, src, None, (8, 5), None, "triangle", "float32", "HWC", **kw)
        _same(got, _expected(ctx, chans, "float32", "HWC"), "curves %d -> %d matrix %d" % (tf_in, tf_out, use_matrix))


def test_non_finite_samples_spread_only_as_far_as_their_taps(ctx):
    rng = np.random.default_rng(32)
    src = [rng.uniform(0, 1, (33, 67)).astype(F) for _ in range(3)]
    special = np.array([np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, np.inf, np.nan, 3.4e38], F)
    where = [(2, 3), (9, 40), (16, 11), (20, 60), (27, 25), (31, 5), (5, 55), (12, 30)]
    for k, (y, x) in enumerate(where):
        src[k % 3][y, x] = special[k]
    for name, filt in FILTERS:
        chans, _ = _filtered(ctx, src, None, (30, 60), None, filt, tfOut=abi.TF_SRGB)
        bad = ~np.isfinite(np.stack(chans))
        assert 0 < bad.sum() <= 128 and bad.sum() <= 0.1 * bad.size, "the model's own result: at most 16 outputs per special value"
        for dtype in ("float32", "float16"):
            got = _resized(ctx, src, None, (30, 60), None, name, dtype, "CHW", tfOut=abi.TF_SRGB)
            _same(got, _expected(ctx, chans, dtype, "CHW"), "non-finite %s %s" % (name, dtype))


def test_forced_tiles_change_no_bit(ctx, data):
    d = data[(33, 67)]
    hook = ctx.lib.jxl_debug_tensor_resize_tile
    hook.restype, hook.argtypes = C.c_int32, [C.c_int32, C.c_int32]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB, matrix=MATRIX, writeAlpha=True, premultiplied=True)
    try:
        for (name, _), (size, box) in itertools.product(FILTERS, (((8, 5), None), ((30, 60), None), ((67, 130), None), ((6, 4), (3, 2, 20, 9)))):
            assert hook(0, 0) == abi.JXL_OK
            exp = {dt: _resized(ctx, d["f"], d["af"], size, box, name, dt, "HWC", **kw) for dt in ("float32", "uint8")}
            for tw, th in ((8, 1), (16, 2), (64, 4), (1, 1), (32, 4)):
                assert hook(tw, th) == abi.JXL_OK
                for dt in exp:
                    got = _resized(ctx, d["f"], d["af"], size, box, name, dt, "HWC", lead=1, **kw)
                    assert np.array_equal(got, exp[dt]), (name, size, tw, th, dt)
        assert hook(24, 2) == abi.JXL_ERR_INVALID_ARGUMENT and hook(8, 3) == abi.JXL_ERR_INVALID_ARGUMENT
    finally:
        assert hook(0, 0) == abi.JXL_OK


def test_resident_and_set_entries_equal_the_stage_entry(ctx, data):
    shape = (33, 67)
    d = data[shape]
    kw = dict(tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB, writeAlpha=True, premultiplied=True)
    dev = "cuda:%d" % ctx.device
    rp = host.ResidentPlanes.upload(ctx, d["f"])
    cv_f = host.DeviceCanvas.fromArrays(ctx, d["f"] + [d["af"]])
    cv_i = host.DeviceCanvas.fromArrays(ctx, d["i"] + [d["a10"]])
    try:
        for (size, box), dtype, layout in itertools.product((((8, 5), None), ((6, 4), (3, 2, 20, 9))), DTYPES, ("CHW", "HWC")):
            exp = _resized(ctx, d["f"], d["af"], size, box, "triangle", dtype, layout, **kw)
            st, _, before, body, after = _raw(ctx, d["f"], d["af"], size, box, "triangle", dtype, layout, lead=1, **kw,
                                              entry=lambda p, r, ptr: ctx.lib.jxl_planes_tensor_resized(ctx.h, d["af"].ctypes.data, C.byref(p), C.byref(r), C.c_void_p(ptr)))
            assert st == abi.JXL_OK and np.array_equal(body, exp.reshape(-1)), ("resident", size, dtype, layout)
            assert np.all(before == 0xA5) and np.all(after == 0xA5)
            out = torch.empty(exp.size * ELEM[dtype], dtype=torch.uint8, device=dev)
            cv_f.tensorResized(out.data_ptr(), size, box, "triangle", nColor=3, alphaPlane=3, dtype=dtype, layout=layout, **kw)
            assert np.array_equal(out.cpu().numpy().view(VIEW[ELEM[dtype]]), exp.reshape(-1)), ("set", size, dtype, layout)
            exp = _resized(ctx, d["i"], d["a10"], size, box, "box", dtype, layout, alphaDepth=10, inMax=[255] * 3, **kw)
            cv_i.tensorResized(out.data_ptr(), size, box, "box", nColor=3, alphaPlane=3, dtype=dtype, layout=layout, alphaDepth=10, inMax=[255] * 3, **kw)
            assert np.array_equal(out.cpu().numpy().view(VIEW[ELEM[dtype]]), exp.reshape(-1)), ("int set", size, dtype, layout)
        # the python front end of the resident planes; one plane of the set as a grey image
        exp = _resized(ctx, d["f"], None, (8, 5), None, "box", "bfloat16", "HWC")
        out = torch.empty((8, 5, 3), dtype=torch.bfloat16, device=dev)
        rp.tensorResized(out.data_ptr(), (8, 5), resample="box", dtype="bfloat16", layout="HWC")
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), exp)
        exp = _resized(ctx, d["f"][:1], None, (8, 5), None, "triangle", "float16", "CHW")
        out = torch.empty(exp.size, dtype=torch.float16, device=dev)
        cv_f.tensorResized(out.data_ptr(), (8, 5), nColor=1, dtype="float16")
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), exp.reshape(-1))
        # what the set and the resident entries refuse of their own
        sent = torch.empty(4 * 4 * 40 + 64, dtype=torch.uint8, device=dev).fill_(0xA5)
        r = host.resizeParams(shape, (8, 5))
        for bad in (lambda p: setattr(p, "height", shape[0] + 1), lambda p: setattr(p.color, "in_is_int", 1), lambda p: setattr(p, "alpha_is_int", 1)):
            p = host.tensorParams(d["f"], shape, alpha=d["af"], writeAlpha=True)
            bad(p)
            assert ctx.lib.jxl_canvas_tensor_resized(ctx.h, cv_f.id, 3, C.byref(p), C.byref(r), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        p = host.tensorParams(d["f"], shape, alpha=d["af"], writeAlpha=True)
        for sid, ap in ((cv_f.id, 4), (cv_f.id, -1), (1 << 20, 3)):
            assert ctx.lib.jxl_canvas_tensor_resized(ctx.h, sid, ap, C.byref(p), C.byref(r), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        p.height += 1
        assert ctx.lib.jxl_planes_tensor_resized(ctx.h, d["af"].ctypes.data, C.byref(p), C.byref(r), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert bool((sent == 0xA5).all())
    finally:
        cv_f.release()
        cv_i.release()


def test_refusals_leave_the_output_untouched(ctx, data):
    shape = (33, 67)
    d = data[shape]
    src, ialpha = d["f"], d["a10"]
    dev = "cuda:%d" % ctx.device
    sent = torch.empty(4 * 4 * 40 + 64, dtype=torch.uint8, device=dev).fill_(0xA5)

    def call(p, r, src=src, alpha=None, ptr=None):
        st = ctx.lib.jxl_stage_tensor_resized(ctx.h, _pin(src), alpha.ctypes.data if alpha is not None else None, C.byref(p) if p is not None else None,
                                              C.byref(r) if r is not None else None, C.c_void_p(sent.data_ptr() if ptr is None else ptr))
        torch.cuda.synchronize()
        assert bool((sent == 0xA5).all()), "a refused call wrote to the output"
        return st
    P = lambda **kw: host.tensorParams(src, shape, **kw)  # noqa: E731
    R = lambda size=(8, 5), box=None, resample="triangle": host.resizeParams(shape, size, box, resample)  # noqa: E731
    bad = [("box past the right edge", P(), R(box=(60, 0, 8, 8))), ("box past the bottom", P(), R(box=(0, 30, 8, 8))), ("negative box origin", P(), R(box=(-1, 0, 8, 8))),
           ("empty box", P(), R(box=(0, 0, 0, 8))), ("out height 0", P(), R(size=(0, 5))), ("out width < 0", P(), R(size=(8, -3))),
           ("unknown filter", P(), R(resample=2)), ("negative filter", P(), R(resample=-1)),
           ("unknown dtype", P(dtype=4), R()), ("norm with U8", P(dtype="uint8", mean=[0] * 3, invStd=[1] * 3), R()), ("max_value not 0", P(maxValue=255), R())]
    for name, p, r in bad:
        assert call(p, r) == abi.JXL_ERR_INVALID_ARGUMENT, name
    for depth, dtype in ((0, "uint8"), (0, "float32"), (32, "uint8")):
        p = host.tensorParams(src, shape, alpha=ialpha, writeAlpha=True, dtype=dtype, alphaDepth=depth)
        assert call(p, R(), alpha=ialpha) == abi.JXL_ERR_INVALID_ARGUMENT, ("int alpha depth", depth, dtype)
    assert call(None, R()) == abi.JXL_ERR_INVALID_ARGUMENT and call(P(), None) == abi.JXL_ERR_INVALID_ARGUMENT
    assert call(P(), R(), ptr=0) == abi.JXL_ERR_INVALID_ARGUMENT
    # more than 1024 taps: 1 x 2100 -> 1 x 3
    wide = [np.zeros((1, 2100), F)]
    p, r = host.tensorParams(wide, (1, 2100)), host.resizeParams((1, 2100), (1, 3))
    assert call(p, r, src=wide) == abi.JXL_ERR_INVALID_ARGUMENT
    assert b"1024 taps" in ctx.lib.jxl_last_error(ctx.h)
    # a host pointer never reaches a kernel
    host_out = np.full(4 * 4 * 40 + 64, 0xA5, np.uint8)
    assert call(P(), R(), ptr=host_out.ctypes.data) == abi.JXL_ERR_INVALID_ARGUMENT and np.all(host_out == 0xA5)
    # a short allocation (test_tensor_samples_gpu's construction: a segment of its own of exactly 12 MiB), asked for a tensor of
    # 12 MiB + 4 bytes by upscaling one row
    big = 12 << 20
    torch.cuda.empty_cache()
    short = torch.empty(big, dtype=torch.uint8, device=dev).fill_(0xA5)
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= short.data_ptr() < s["address"] + s["total_size"]]
    row = [np.zeros((1, 1024), F)]
    p = host.tensorParams(row, (1, 1024))
    if len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] < short.data_ptr() + big + 4:
        r = host.resizeParams((1, 1024), (1, big // 4 + 1))
        st = ctx.lib.jxl_stage_tensor_resized(ctx.h, _pin(row), None, C.byref(p), C.byref(r), C.c_void_p(short.data_ptr()))
        assert st == abi.JXL_ERR_INVALID_ARGUMENT and bool((short == 0xA5).all())
    r = host.resizeParams((1, 1024), (1, big // 4))
    assert ctx.lib.jxl_stage_tensor_resized(ctx.h, _pin(row), None, C.byref(p), C.byref(r), C.c_void_p(short.data_ptr())) == abi.JXL_OK
    assert not bool(short.any())
