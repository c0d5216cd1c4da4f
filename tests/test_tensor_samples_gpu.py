"""The image as a device tensor in one pass (jxl_stage_tensor_samples / jxl_planes_tensor_samples / jxl_canvas_tensor_samples,
csrc/k_tensor.hip) against the entries the parent commit pins: U8 against jxl_stage_png_samples at 8 bits, F32 against
jxl_stage_color_convert's float planes, and F16 / BF16 / normalisation / un-premultiplication / layout against the numpy model of
tests/tensor_ref.py applied to those. Outputs are torch memory; every comparison is bit for bit (NaNs as one value where a curve or
a division makes them). Five shapes: 1x1, 1x3, 1x5 (a tail of 1 after a full group), 3x7 (21 pixels: the CHW planes 1 and 2 are
misaligned for every dtype) and 33x67 (2211 pixels: more than two workgroups; through the debug hook with one workgroup, the
grid-stride loop)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import tensor_ref as ref
from conftest import assert_bits_equal
from jxlatte_amd import abi, host
from jxlatte_amd.decoder import PRI_P3, PRI_SRGB, WP_D65, get_conversion_matrix

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1), (1, 3), (1, 5), (3, 7), (33, 67)]
DTYPES = ["uint8", "float16", "bfloat16", "float32"]
ELEM = {"uint8": 1, "float16": 2, "bfloat16": 2, "float32": 4}
VIEW = {1: np.uint8, 2: np.uint16, 4: np.uint32}
GRID_TF = [(abi.TF_LINEAR, 0), (abi.TF_SRGB, 0), (abi.TF_BT709, 0), (abi.TF_PQ, 0), (abi.TF_GAMMA, 4545455)]  # test_png_samples_gpu's
MATRIX = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65)
PQ_EDGE = F(math.pow(0.8359375, 1.0 / 0.012683313515655965121))
SPECIAL = np.array([0.0, -0.0, -1e-45, -1e-3, -0.5, -2.0, 1.0, 4.0, np.inf, -np.inf, np.nan, 1e-45, 1.1754942e-38, 3.4e38, 65504.0, 65520.0,
                    6e-8, 3e-8, 2.9802322e-8, 6.1e-5, 0.0404482362771082, 0.081242858298635133, 0.018053968510807807, 0.00313066844250063,
                    PQ_EDGE], F)


def _float_plane(seed, shape):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    v = np.concatenate([rng.uniform(0, 1, n).astype(F), rng.uniform(1, 4, n // 8).astype(F), (10 ** rng.uniform(-12, 0, n // 8)).astype(F)])
    if n > 4 * SPECIAL.size:
        v = np.concatenate([v, SPECIAL])
    rng.shuffle(v)
    return np.ascontiguousarray(v[:n].reshape(shape))


def _int_plane(seed, shape, mx=255):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    v = rng.integers(0, mx + 1, n).astype(np.int32)
    if n > 64:
        v[:8] = [0, mx, mx + 1, -1, -300, 2 ** 31 - 1, -2 ** 31, 1]
    rng.shuffle(v)
    return v.reshape(shape)


def _alpha(kind, seed, shape, mx=255):
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    if kind == "float":
        a = rng.uniform(0, 1, n).astype(F)
        sp = [0.0, -0.0, 1.0, 1.5, np.nan, np.inf, 0.5, 1e-30]
    else:
        a = rng.integers(0, mx + 1, n).astype(np.int32)
        sp = [0, mx, mx + 45, -1, 1, 2 ** 31 - 1, 0, 0]
    if n > 64:
        a[:8] = sp
    elif n > 2:
        a[1] = 0  # a zero alpha at every size but the smallest
    rng.shuffle(a)
    return a.reshape(shape)


def _alpha_float(alpha, depth):
    """the model's alpha: a float plane as it is, an int32 plane cast with its depth (ImageBuffer.castToFloat0)"""
    if alpha.dtype == np.float32:
        return alpha
    return (alpha.astype(F) * F(F(1) / F((1 << depth) - 1))).astype(F)


@pytest.fixture(scope="module")
def data():
    """the inputs of every test here, made once and never written"""
    d = {}
    for shape in SHAPES:
        d[shape] = dict(f=[_float_plane(s, shape) for s in (1, 2, 3)], i=[_int_plane(s, shape) for s in (4, 5, 6)],
                        af=_alpha("float", 7, shape), a8=_alpha("int", 8, shape), a10=_alpha("int", 9, shape, 1023))
        for v in d[shape].values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return d


def _pin(src):
    return (C.c_void_p * 3)(*([a.ctypes.data for a in src] + [None] * (3 - len(src))))


def _raw(ctx, src, alpha, dtype, layout, lead=0, entry=None, **params):
    """one call into torch memory pre-filled with 0xA5, the tensor `lead` elements into it: (status, params, the bytes before,
    the tensor's bytes as [n * channels] elements, the bytes after). entry(p, ptr) replaces the stage entry"""
    shape = src[0].shape
    p = host.tensorParams(src, shape, alpha=alpha, dtype=dtype, layout=layout, **params)
    e = ELEM[dtype] if dtype in ELEM else 4
    nbytes = shape[0] * shape[1] * host.tensorChannels(p) * e
    buf = torch.empty(lead * e + nbytes + 64, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)
    ptr = buf.data_ptr() + lead * e
    if entry is None:
        st = ctx.lib.jxl_stage_tensor_samples(ctx.h, _pin(src), alpha.ctypes.data if alpha is not None else None, C.byref(p), C.c_void_p(ptr))
    else:
        st = entry(p, ptr)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return st, p, b[:lead * e], b[lead * e:lead * e + nbytes].copy().view(VIEW[e]), b[lead * e + nbytes:]


def _tensor(ctx, src, alpha, dtype, layout, **kw):
    """the tensor's element bits, [C][H][W] or [H][W][C]"""
    st, p, _, body, _ = _raw(ctx, src, alpha, dtype, layout, **kw)
    assert st == abi.JXL_OK, (st, ctx.lib.jxl_last_error(ctx.h))
    c, (h, w) = host.tensorChannels(p), src[0].shape
    return body.reshape((c, h, w) if layout == "CHW" else (h, w, c))


# (name, colour kind, planes, alpha key, alpha depth, premultiplied, write alpha) -> 1 .. 4 channels
U8_CASES = [("rgb float", "f", 3, None, 8, False, False), ("rgb int", "i", 3, None, 8, False, False), ("grey float", "f", 1, None, 8, False, False),
            ("grey int", "i", 1, None, 8, False, False), ("rgba int alpha 8: clamped as it is", "f", 3, "a8", 8, False, True),
            ("rgba int alpha 10: coerced", "i", 3, "a10", 10, False, True), ("rgba float alpha", "f", 3, "af", 8, False, True),
            ("rgba premultiplied, zero alphas among them", "f", 3, "af", 8, True, True), ("rgba premultiplied int alpha 8", "i", 3, "a8", 8, True, True),
            ("grey + alpha", "f", 1, "af", 8, False, True), ("grey + int alpha 10 premultiplied", "i", 1, "a10", 10, True, True),
            ("rgb, premultiplied alpha dropped", "f", 3, "af", 8, True, False), ("grey, premultiplied int alpha dropped", "f", 1, "a10", 10, True, False)]


@pytest.mark.parametrize("shape", SHAPES)
def test_u8_hwc_equals_the_png_samples_at_8_bits(ctx, data, shape):
    d = data[shape]
    for (name, kind, n, akey, adepth, premult, write), (tf_in, tf_out) in itertools.product(U8_CASES, [(abi.TF_LINEAR, abi.TF_LINEAR), (abi.TF_LINEAR, abi.TF_SRGB), (abi.TF_SRGB, abi.TF_PQ)]):
        src, alpha = d[kind][:n], d[akey] if akey else None
        color = dict(tfIn=tf_in, tfOut=tf_out, inMax=[255] * n)
        with np.errstate(all="ignore"):
            exp = host.pngSamples(ctx, src, alpha, premultiplied=premult, bitDepth=8, alphaDepth=adepth, colorDepth=8, **color)
        if not write:
            exp = exp[:, :, :3 if n == 3 else 1]
        got = _tensor(ctx, src, alpha, "uint8", "HWC", premultiplied=premult, writeAlpha=write, alphaDepth=adepth, colorDepth=8, **color)
        assert got.shape == exp.shape and np.array_equal(got, exp), "%s %s tf %d -> %d: %d samples differ" % (shape, name, tf_in, tf_out, int((got != exp).sum()))
    # grey through a matrix: three channels, as the PNG entry gives them
    exp = host.pngSamples(ctx, d["f"][:1], None, bitDepth=8, matrix=MATRIX, tfOut=abi.TF_SRGB)
    assert np.array_equal(_tensor(ctx, d["f"][:1], None, "uint8", "HWC", matrix=MATRIX, tfOut=abi.TF_SRGB), exp) and exp.shape[2] == 3
    # integer colour planes without a maximum of their own: cast with the tagged depth
    exp = host.pngSamples(ctx, d["i"], None, bitDepth=8, colorDepth=10)
    assert np.array_equal(_tensor(ctx, d["i"], None, "uint8", "HWC", colorDepth=10), exp)


@pytest.fixture(scope="module")
def f32_grid(ctx, data):
    """F32 / HWC of the 33x67 planes for every tf pair x {float, int} colours x {matrix}: computed once, compared by several tests"""
    d = data[(33, 67)]
    out = {}
    for (tf_in, g_in), (tf_out, g_out), is_int, use_matrix in itertools.product(GRID_TF, GRID_TF, (False, True), (False, True)):
        src = d["i"] if is_int else d["f"]
        kw = dict(tfIn=tf_in, gammaIn=g_in, tfOut=tf_out, gammaOut=g_out, inMax=[255] * 3, matrix=MATRIX if use_matrix else None,
                  scale=F(1.37) if use_matrix else None)
        out[(tf_in, tf_out, is_int, use_matrix)] = (src, kw, _tensor(ctx, src, None, "float32", "HWC", **kw))
    return out


def test_f32_equals_the_colour_stage_planes_for_every_curve_pair(ctx, f32_grid):
    assert len(f32_grid) == 100
    for key, (src, kw, got) in f32_grid.items():
        planes = host.colorConvert(ctx, src, maxValue=0, **kw)
        assert_bits_equal(got.view(F), ref.layout(planes, "HWC"), "F32 HWC %s" % (key,), any_nan=True)
        if key[2] or key[3]:
            continue
        chw = _tensor(ctx, src, None, "float32", "CHW", **kw)
        assert_bits_equal(chw.view(F), np.stack(planes), "F32 CHW %s" % (key,), any_nan=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_alpha_unpremultiply_and_grey_in_f32(ctx, data, shape):
    d = data[shape]
    for n, (akey, adepth), premult, write, layout in itertools.product((1, 3), (("af", 8), ("a8", 8), ("a10", 10)), (False, True), (False, True), ("CHW", "HWC")):
        if not premult and not write:
            continue
        src, alpha = d["f"][:n], d[akey]
        kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_BT709)
        planes = host.colorConvert(ctx, src, maxValue=0, **kw)
        fa = _alpha_float(alpha, adepth)
        if premult:
            planes = ref.unpremultiply(planes, fa)
        exp = ref.layout(ref.convert(planes + ([fa] if write else []), "float32"), layout)
        got = _tensor(ctx, src, alpha, "float32", layout, premultiplied=premult, writeAlpha=write, alphaDepth=adepth, **kw)
        assert_bits_equal(got.view(F), exp.view(F), "%s n %d alpha %s premult %d write %d %s" % (shape, n, akey, premult, write, layout), any_nan=True)


def test_f16_and_bf16_are_the_model_rounding_of_the_f32_result(ctx, f32_grid):
    for key, (src, kw, f32) in f32_grid.items():
        if key[2] and key[3]:
            continue
        for dtype in ("float16", "bfloat16"):
            got = _tensor(ctx, src, None, dtype, "HWC", **kw)
            exp = ref.convert([f32.view(F)], dtype)[0]
            assert np.array_equal(got, exp), "%s %s: %d elements differ" % (dtype, key, int((got != exp).sum()))
    # values chosen for the rounding itself, through the identity chain: ties, overflow, subnormals, NaNs with payloads
    bits = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001,
                     0xFFC12345, 0x477FE000, 0x477FF000, 0x477FEFFF, 0x33800000, 0x33000000, 0x33000001, 0x33C00000, 0x387FC000, 0x387FE000,
                     0x38800000, 0x00000001, 0x80000000, 0x3F801000, 0x3F803000], np.uint32)
    plane = np.resize(bits, 28).view(F).reshape(4, 7)
    f32 = _tensor(ctx, [plane], None, "float32", "CHW")
    assert_bits_equal(f32[0].view(F), host.colorConvert(ctx, [plane])[0], "F32: the colour stages' bits as they are", any_nan=True)
    assert np.array_equal(f32[0][~np.isnan(plane)], plane.view(np.uint32)[~np.isnan(plane)])
    for dtype, layout in itertools.product(("float16", "bfloat16"), ("CHW", "HWC")):
        got = _tensor(ctx, [plane], None, dtype, layout)
        assert np.array_equal(got.reshape(4, 7), ref.convert([plane], dtype)[0]), dtype


@pytest.mark.parametrize("shape", SHAPES)
def test_normalisation_equals_the_model_on_the_f32_result(ctx, data, shape):
    d = data[shape]
    mean, std = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
    inv = [F(1) / F(s) for s in std]
    kw = dict(tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB)
    for n, write in ((3, True), (3, False), (1, True), (1, False)):
        src, alpha = d["f"][:n], d["af"]
        base = _tensor(ctx, src, alpha, "float32", "CHW", writeAlpha=write, **kw).view(F)
        with np.errstate(all="ignore"):
            normed = ref.normalise(list(base), mean, inv)
        for dtype, layout in itertools.product(("float32", "float16", "bfloat16"), ("CHW", "HWC")):
            got = _tensor(ctx, src, alpha, dtype, layout, writeAlpha=write, mean=mean, invStd=inv, **kw)
            exp = ref.layout(ref.convert(normed, dtype), layout)
            if dtype == "float32":
                assert_bits_equal(got.view(F), exp.view(F), "norm %s n %d" % (shape, n), any_nan=True)
            else:
                assert np.array_equal(got, exp), "norm %s %s %s n %d write %d" % (shape, dtype, layout, n, write)


@pytest.mark.parametrize("shape", SHAPES)
def test_chw_is_the_transposed_hwc_and_nothing_is_written_around_an_offset_tensor(ctx, data, shape):
    d = data[shape]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_LINEAR, matrix=MATRIX)
    for dtype, (n, write) in itertools.product(DTYPES, ((3, False), (3, True), (1, False), (1, True))):
        src, alpha = d["f"][:n], d["af"] if write else None
        per = {}
        for layout, lead in itertools.product(("CHW", "HWC"), (0, 1)):
            st, p, before, body, after = _raw(ctx, src, alpha, dtype, layout, lead=lead, writeAlpha=write, premultiplied=write, **kw)
            what = "%s %s %s n %d alpha %d lead %d" % (shape, dtype, layout, n, write, lead)
            assert st == abi.JXL_OK, what
            assert np.all(before == 0xA5) and np.all(after == 0xA5), what + ": a store outside the tensor"
            c = host.tensorChannels(p)
            body = body.reshape((c,) + shape if layout == "CHW" else shape + (c,))
            per.setdefault(layout, body)
            assert np.array_equal(per[layout], body), what + ": the offset tensor differs from the aligned one"
        assert np.array_equal(per["CHW"], np.moveaxis(per["HWC"], -1, 0)), "%s %s n %d alpha %d: CHW is not HWC transposed" % (shape, dtype, n, write)


def test_one_workgroup_walks_the_whole_image(ctx, data):
    d = data[(33, 67)]
    hook = ctx.lib.jxl_debug_tensor_samples_grid
    hook.restype, hook.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(abi.TensorParams), C.c_void_p, C.c_int32]
    kw = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_PQ, writeAlpha=True)
    for dtype, layout, grid in itertools.product(DTYPES, ("CHW", "HWC"), (1, 2)):
        exp = _tensor(ctx, d["f"], d["af"], dtype, layout, **kw)
        st, _, before, body, after = _raw(ctx, d["f"], d["af"], dtype, layout, lead=1, **kw,
                                          entry=lambda p, ptr: hook(ctx.h, _pin(d["f"]), d["af"].ctypes.data, C.byref(p), C.c_void_p(ptr), grid))
        assert st == abi.JXL_OK and np.array_equal(body, exp.reshape(-1)), (dtype, layout, grid)
        assert np.all(before == 0xA5) and np.all(after == 0xA5)
    p = host.tensorParams(d["f"], (33, 67))
    assert hook(ctx.h, _pin(d["f"]), None, C.byref(p), C.c_void_p(0), 0) == abi.JXL_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("shape", [(3, 7), (33, 67)])
def test_resident_and_set_entries_equal_the_stage_entry(ctx, data, shape):
    d = data[shape]
    kw = dict(tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB, writeAlpha=True, premultiplied=True)
    rp = host.ResidentPlanes.upload(ctx, d["f"])
    cv_f = host.DeviceCanvas.fromArrays(ctx, d["f"] + [d["af"]])
    cv_i = host.DeviceCanvas.fromArrays(ctx, d["i"] + [d["a10"]])
    try:
        for dtype, layout in itertools.product(DTYPES, ("CHW", "HWC")):
            exp = _tensor(ctx, d["f"], d["af"], dtype, layout, **kw)
            st, _, _, body, _ = _raw(ctx, d["f"], d["af"], dtype, layout, **kw,
                                     entry=lambda p, ptr: ctx.lib.jxl_planes_tensor_samples(ctx.h, d["af"].ctypes.data, C.byref(p), C.c_void_p(ptr)))
            assert st == abi.JXL_OK and np.array_equal(body, exp.reshape(-1)), ("resident", dtype, layout)
            bus = list(getattr(ctx, "blend_bus", [0, 0]))
            n = shape[0] * shape[1] * 4
            out = torch.empty(n * ELEM[dtype], dtype=torch.uint8, device="cuda:%d" % ctx.device)
            cv_f.tensorSamples(out.data_ptr(), nColor=3, alphaPlane=3, dtype=dtype, layout=layout, **kw)
            assert np.array_equal(out.cpu().numpy().view(VIEW[ELEM[dtype]]), exp.reshape(-1)), ("set", dtype, layout)
            assert list(getattr(ctx, "blend_bus", [0, 0])) == bus, "the set entry moved the bus counter"
            # int32 planes and an int alpha plane of depth 10, and one plane of the set as a grey image
            exp = _tensor(ctx, d["i"], d["a10"], dtype, layout, alphaDepth=10, inMax=[255] * 3, **kw)
            cv_i.tensorSamples(out.data_ptr(), nColor=3, alphaPlane=3, dtype=dtype, layout=layout, alphaDepth=10, inMax=[255] * 3, **kw)
            assert np.array_equal(out.cpu().numpy().view(VIEW[ELEM[dtype]]), exp.reshape(-1)), ("int set", dtype, layout)
        exp = _tensor(ctx, d["f"][:1], None, "float16", "CHW")
        out = torch.empty(exp.size, dtype=torch.float16, device="cuda:%d" % ctx.device)
        cv_f.tensorSamples(out.data_ptr(), nColor=1, dtype="float16")
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), exp.reshape(-1))
        # python front ends: the resident planes
        exp = _tensor(ctx, d["f"], None, "bfloat16", "HWC")
        out = torch.empty(shape + (3,), dtype=torch.bfloat16, device="cuda:%d" % ctx.device)
        rp.tensorSamples(out.data_ptr(), dtype="bfloat16", layout="HWC")
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), exp)
        # what the set and the resident entries refuse of their own: another geometry, other tags, a plane the set has not
        for bad in (lambda p: setattr(p, "height", shape[0] + 1), lambda p: setattr(p.color, "in_is_int", 1), lambda p: setattr(p, "alpha_is_int", 1)):
            p = host.tensorParams(d["f"], shape, alpha=d["af"], writeAlpha=True)
            bad(p)
            sent = torch.empty(4 * 4 * shape[0] * shape[1] + 64, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)
            assert ctx.lib.jxl_canvas_tensor_samples(ctx.h, cv_f.id, 3, C.byref(p), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
            assert bool((sent == 0xA5).all())
        p = host.tensorParams(d["f"], shape, alpha=d["af"], writeAlpha=True)
        assert ctx.lib.jxl_canvas_tensor_samples(ctx.h, cv_f.id, 4, C.byref(p), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        assert ctx.lib.jxl_canvas_tensor_samples(ctx.h, cv_f.id, -1, C.byref(p), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        assert ctx.lib.jxl_canvas_tensor_samples(ctx.h, 1 << 20, 3, C.byref(p), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        p.height += 1
        assert ctx.lib.jxl_planes_tensor_samples(ctx.h, d["af"].ctypes.data, C.byref(p), C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        assert bool((sent == 0xA5).all())
    finally:
        cv_f.release()
        cv_i.release()


def test_refusals_leave_the_output_untouched(ctx, data):
    d = data[(3, 7)]
    src, alpha, ialpha = d["f"], d["af"], d["a10"]
    dev = "cuda:%d" % ctx.device
    sent = torch.empty(4 * 4 * 21 + 64, dtype=torch.uint8, device=dev).fill_(0xA5)

    def call(p, src=src, alpha=None, ptr=None):
        st = ctx.lib.jxl_stage_tensor_samples(ctx.h, _pin(src) if src is not None else None, alpha.ctypes.data if alpha is not None else None,
                                              C.byref(p) if p is not None else None, C.c_void_p(sent.data_ptr() if ptr is None else ptr))
        torch.cuda.synchronize()
        assert bool((sent == 0xA5).all()), "a refused call wrote to the output"
        return st
    ok = lambda **kw: host.tensorParams(src, (3, 7), **kw)  # noqa: E731
    bad = []

    def edit(p, **fields):
        for k, v in fields.items():
            setattr(p, k, v)
        return p
    bad.append(("unknown dtype", edit(ok(), dtype=4), None))
    bad.append(("negative dtype", edit(ok(), dtype=-1), None))
    bad.append(("unknown layout", edit(ok(), layout=2), None))
    bad.append(("norm with U8", ok(dtype="uint8", mean=[0] * 3, invStd=[1] * 3), None))
    bad.append(("infinite inv_std", ok(mean=[0] * 3, invStd=[1, float("inf"), 1]), None))
    bad.append(("NaN inv_std", ok(mean=[0] * 3, invStd=[1, 1, float("nan")]), None))
    bad.append(("write_alpha without has_alpha", edit(ok(), write_alpha=1), None))
    bad.append(("premultiplied without has_alpha", edit(ok(), premultiplied=1), None))
    bad.append(("has_alpha without a plane", edit(ok(), has_alpha=1, write_alpha=1), None))
    bad.append(("int alpha of depth 32, float output", ok(alpha=ialpha, writeAlpha=True, alphaDepth=32), ialpha))
    bad.append(("int alpha of depth 0, premultiplied U8", ok(alpha=ialpha, premultiplied=True, dtype="uint8", alphaDepth=0), ialpha))
    bad.append(("height 0", edit(ok(), height=0), None))
    bad.append(("max_value not 0", ok(maxValue=255), None))
    bad.append(("unknown curve", ok(tfOut=99), None))
    bad.append(("two planes", edit(ok(), color=edit(ok().color, n_planes=2)), None))
    for name, p, a in bad:
        assert call(p, alpha=a) == abi.JXL_ERR_INVALID_ARGUMENT, name
    assert call(None) == abi.JXL_ERR_INVALID_ARGUMENT
    assert call(ok(), src=None) == abi.JXL_ERR_INVALID_ARGUMENT
    assert call(ok(), ptr=0) == abi.JXL_ERR_INVALID_ARGUMENT
    # a host pointer never reaches a kernel
    host_out = np.full(4 * 4 * 21 + 64, 0xA5, np.uint8)
    assert call(ok(), ptr=host_out.ctypes.data) == abi.JXL_ERR_INVALID_ARGUMENT and np.all(host_out == 0xA5)
    # a tensor on the right device, one element short, in a fresh allocation. The library asks the runtime for the extent of the
    # ALLOCATION, and torch's caching allocator carves its tensors out of larger ones; a request of 12 MiB after empty_cache() is
    # a segment of its own of exactly that size (requests above 10 MiB are rounded to 2 MiB). The refusal is asserted where the
    # allocator's own snapshot says that the segment ends before the tensor would (else only the extent rule's stand-alone
    # program pins it: tools/native/tensor_check.cpp)
    big = 12 << 20
    plane = np.zeros((1, big // 4 + 1), F)  # a float32 grey tensor of 12 MiB + 4 bytes
    torch.cuda.empty_cache()
    short = torch.empty(big, dtype=torch.uint8, device=dev).fill_(0xA5)
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= short.data_ptr() < s["address"] + s["total_size"]]
    p = host.tensorParams([plane], plane.shape)
    if len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] < short.data_ptr() + plane.nbytes:
        st = ctx.lib.jxl_stage_tensor_samples(ctx.h, _pin([plane]), None, C.byref(p), C.c_void_p(short.data_ptr()))
        assert st == abi.JXL_ERR_INVALID_ARGUMENT and bool((short == 0xA5).all())
    # and a tensor that fits the same allocation to the byte is taken
    plane = plane[:, :-1]
    p = host.tensorParams([plane], plane.shape)
    assert ctx.lib.jxl_stage_tensor_samples(ctx.h, _pin([plane]), None, C.byref(p), C.c_void_p(short.data_ptr())) == abi.JXL_OK
    assert not bool(short.any())
