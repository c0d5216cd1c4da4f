"""N images resampled into one batch tensor in one launch (jxl_tensor_resized_batch, csrc/k_tensor_resize_batch.hip). The
yardstick throughout is the single-image entry of each item's source kind -- jxl_stage_tensor_resized, jxl_planes_tensor_resized,
jxl_canvas_tensor_resized, themselves pinned by tests/test_tensor_resized_gpu.py -- called per item with the item's own
jxl_tensor_params and jxl_resize_params: bit for bit, NaNs as one value, no tolerance.
The batch goes to torch memory pre-filled with 0xA5, one element into it, with guard bytes before and after."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_bits_equal
from jxlatte_amd import abi, host
from jxlatte_amd.decoder import PRI_P3, PRI_SRGB, WP_D65, get_conversion_matrix

pytestmark = pytest.mark.gpu
F = np.float32
ELEM = {abi.TENSOR_U8: 1, abi.TENSOR_F16: 2, abi.TENSOR_BF16: 2, abi.TENSOR_F32: 4}
DTYPES = ["uint8", "float16", "bfloat16", "float32"]
MATRIX = get_conversion_matrix(PRI_SRGB, WP_D65, PRI_P3, WP_D65)
GUARD = 64
# batch A: (source (h, w), box) -> 2 x 5: upscaling, single-tile items, a footprint of two 1024-column chunks, a width that takes
# the dword loads (5 x 7: 7 % 4) beside 16-byte ones, a box
SIZE_A = (2, 5)
BATCH_A = [((1, 1), None), ((5, 7), None), ((33, 67), None), ((64, 48), None), ((3, 2100), None), ((33, 67), (3, 2, 20, 9))]
SIZE_B = (13, 11)
BATCH_B = [((5, 7), "triangle"), ((33, 67), "box"), ((67, 33), "triangle"), ((33, 67), "triangle"), ((5, 7), "box")]
SHAPES = sorted({s for s, _ in BATCH_A} | {s for s, _ in BATCH_B})
COLOR = dict(tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB, matrix=MATRIX, scale=F(1.37))


def _plane(seed, shape):
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


@pytest.fixture(scope="module")
def data():
    """the inputs of every test here, made once and never written"""
    d = {}
    for k, shape in enumerate(SHAPES):
        d[shape] = dict(f=[_plane(10 * k + s, shape) for s in (1, 2, 3)], af=_alpha("float", 10 * k + 7, shape), a8=_alpha("int", 10 * k + 8, shape),
                        a10=_alpha("int", 10 * k + 9, shape, 1023))
        for v in d[shape].values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def singles():
    """the single-image entries' results, computed once per distinct item and shared by the tests. An item is known by its
    parameter blocks and the addresses of its planes: only items over the `data` fixture's arrays, which live as long, go here"""
    return {}


def _key(it):
    return (it.source, it.set_id, it.alpha_plane, tuple(it.in_), it.alpha, bytes(it.p), bytes(it.r))


def _single(ctx, it, cache=None):
    """the item through the single-image entry of its source kind, into 0xA5-filled memory: the tensor's bytes"""
    key = _key(it)
    if cache is not None and key in cache:
        return cache[key]
    p, r = it.p, it.r
    n = r.out_height * r.out_width * host.tensorChannels(p) * ELEM[p.dtype]
    buf = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)
    out = C.c_void_p(buf.data_ptr())
    if it.source == abi.BATCH_HOST:
        st = ctx.lib.jxl_stage_tensor_resized(ctx.h, it.in_, it.alpha, C.byref(p), C.byref(r), out)
    elif it.source == abi.BATCH_RESIDENT:
        st = ctx.lib.jxl_planes_tensor_resized(ctx.h, it.alpha, C.byref(p), C.byref(r), out)
    else:
        st = ctx.lib.jxl_canvas_tensor_resized(ctx.h, it.set_id, it.alpha_plane, C.byref(p), C.byref(r), out)
    assert st == abi.JXL_OK, (st, ctx.lib.jxl_last_error(ctx.h))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[n:] == 0xA5)
    if cache is not None:
        cache[key] = b[:n].copy()
    return b[:n].copy()


def _call(ctx, items, n=None, lead=1, ptr=None):
    """one batch call into 0xA5-filled memory, the batch `lead` elements behind the front guard: (status, the bytes before, the
    items' bytes, the bytes after)"""
    p, r = items[0].p, items[0].r
    e = ELEM.get(p.dtype, 4)
    each = max(1, r.out_height) * max(1, r.out_width) * host.tensorChannels(p) * e
    front = GUARD + lead * e
    buf = torch.empty(front + len(items) * each + GUARD, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)
    arr = (abi.TensorBatchItem * len(items))(*items)
    st = ctx.lib.jxl_tensor_resized_batch(ctx.h, len(items) if n is None else n, arr, C.c_void_p(buf.data_ptr() + front if ptr is None else ptr))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return st, b[:front], [b[front + i * each:front + (i + 1) * each].copy() for i in range(len(items))], b[front + len(items) * each:]


def _same(got, exp, dtype, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if dtype == abi.TENSOR_F32:
        assert_bits_equal(got.view(F), exp.view(F), what, any_nan=True)
    else:
        assert np.array_equal(got, exp), "%s: %d of %d bytes differ" % (what, int((got != exp).sum()), got.size)


def _check(ctx, items, cache=None, what="", lead=1):
    """the batch equals the single-image entry per item, and nothing is written around it"""
    st, before, bodies, after = _call(ctx, items, lead=lead)
    assert st == abi.JXL_OK, (what, st, ctx.lib.jxl_last_error(ctx.h))
    assert np.all(before == 0xA5) and np.all(after == 0xA5), "%s: a store outside the batch" % what
    for i, it in enumerate(items):
        _same(bodies[i], _single(ctx, it, cache), it.p.dtype, "%s item %d" % (what, i))


def _batch_a(data, **kw):
    kw = dict(COLOR, **kw)
    return [host.tensorBatchItem(SIZE_A, box, "triangle", planes=data[shape]["f"], **kw) for shape, box in BATCH_A]


def _grid_hook(ctx):
    hook = ctx.lib.jxl_debug_tensor_batch_grid
    hook.restype, hook.argtypes = C.c_int32, [C.c_int32]
    return hook


def _tile_hook(ctx):
    hook = ctx.lib.jxl_debug_tensor_resize_tile
    hook.restype, hook.argtypes = C.c_int32, [C.c_int32, C.c_int32]
    return hook


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_a_every_dtype_and_layout(ctx, data, singles, dtype, layout):
    _check(ctx, _batch_a(data, dtype=dtype, layout=layout), singles, "A %s %s" % (dtype, layout))


def test_batch_b_both_filters_mixed(ctx, data, singles):
    for dtype, layout in (("float32", "CHW"), ("uint8", "HWC"), ("float16", "HWC")):
        items = [host.tensorBatchItem(SIZE_B, None, f, planes=data[shape]["f"], dtype=dtype, layout=layout, **COLOR) for shape, f in BATCH_B]
        _check(ctx, items, singles, "B %s %s" % (dtype, layout))


def test_a_batch_of_one_and_the_same_item_three_times(ctx, data, singles):
    for dtype in ("float32", "uint8"):
        it = host.tensorBatchItem(SIZE_B, (3, 2, 20, 9), "box", planes=data[(33, 67)]["f"], dtype=dtype, layout="HWC", **COLOR)
        _check(ctx, [it], singles, "one")
        _check(ctx, [it, it, it], singles, "thrice")
        one = host.tensorBatchItem((1, 1), None, "triangle", planes=data[(1, 1)]["f"], dtype=dtype, **COLOR)  # a batch of one tile
        _check(ctx, [one], singles, "1x1 -> 1x1")


def test_parameters_differ_per_item(ctx, data, singles):
    d = data[(33, 67)]
    small = data[(5, 7)]
    for dtype, layout in (("float32", "CHW"), ("uint8", "HWC"), ("bfloat16", "CHW")):
        kw = dict(dtype=dtype, layout=layout)
        # alpha written: float, int8 and int10 alpha planes, premultiplied on one item only, two curve pairs, matrix on and off
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], alpha=d["af"], writeAlpha=True, tfIn=abi.TF_PQ, tfOut=abi.TF_SRGB, **kw),
                 host.tensorBatchItem(SIZE_A, None, "box", planes=d["f"], alpha=d["a8"], writeAlpha=True, premultiplied=True, tfIn=abi.TF_GAMMA, gammaIn=4545455,
                                      tfOut=abi.TF_BT709, matrix=MATRIX, **kw),
                 host.tensorBatchItem(SIZE_A, (3, 2, 20, 9), "triangle", planes=d["f"], alpha=d["a10"], alphaDepth=10, writeAlpha=True, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=small["f"], alpha=small["a10"], alphaDepth=10, writeAlpha=True, matrix=MATRIX, scale=F(0.75), **kw)]
        _check(ctx, items, singles, "alpha written %s %s" % (dtype, layout))
        # alpha dropped: the premultiplied items read an alpha plane, their neighbours read none
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], alpha=d["af"], premultiplied=True, tfOut=abi.TF_SRGB, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=small["f"], alpha=small["af"], **kw),
                 host.tensorBatchItem(SIZE_A, None, "box", planes=d["f"], alpha=d["a10"], alphaDepth=10, premultiplied=True, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=small["f"], **kw)]
        assert [bool(it.p.has_alpha and it.p.premultiplied) for it in items] == [False, True, False, True, False]  # who reads an alpha plane
        _check(ctx, items, singles, "alpha dropped %s %s" % (dtype, layout))


def test_normalisation_per_item(ctx, data, singles):
    mean, std = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
    inv = [F(1) / F(s) for s in std]
    d = data[(33, 67)]
    for dtype, layout in (("float32", "HWC"), ("float16", "CHW"), ("bfloat16", "HWC")):
        kw = dict(dtype=dtype, layout=layout, tfIn=abi.TF_SRGB, tfOut=abi.TF_BT709)
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], mean=mean[:3], invStd=inv[:3], **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], **kw),
                 host.tensorBatchItem(SIZE_A, None, "box", planes=data[(64, 48)]["f"], mean=[0.1, 0.2, 0.3], invStd=[F(2), F(3), F(4)], **kw)]
        _check(ctx, items, singles, "normalised %s %s" % (dtype, layout))
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], alpha=d["a8"], writeAlpha=True, premultiplied=True, mean=mean, invStd=inv, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], alpha=d["af"], writeAlpha=True, **kw)]
        _check(ctx, items, singles, "normalised with alpha %s %s" % (dtype, layout))


def test_non_finite_samples(ctx):
    rng = np.random.default_rng(32)
    src = [rng.uniform(0, 1, (33, 67)).astype(F) for _ in range(3)]
    clean = [a.copy() for a in src]
    special = np.array([np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, np.inf, np.nan, 3.4e38], F)
    where = [(2, 3), (9, 40), (16, 11), (20, 60), (27, 25), (31, 5), (5, 55), (12, 30)]
    for k, (y, x) in enumerate(where):
        src[k % 3][y, x] = special[k]
    for dtype in ("float32", "float16", "uint8"):
        items = [host.tensorBatchItem((30, 60), None, "triangle", planes=clean, dtype=dtype, tfOut=abi.TF_SRGB),
                 host.tensorBatchItem((30, 60), None, "triangle", planes=src, dtype=dtype, tfOut=abi.TF_SRGB),
                 host.tensorBatchItem((30, 60), None, "box", planes=src, dtype=dtype, tfOut=abi.TF_SRGB)]
        _check(ctx, items, None, "non-finite %s" % dtype)  # (planes of this test's own: not in the shared results, which go by address)
    # the planted values reach the yardstick too: its float32 tensor is not all finite
    it = host.tensorBatchItem((30, 60), None, "triangle", planes=src, dtype="float32", tfOut=abi.TF_SRGB)
    assert not np.isfinite(_single(ctx, it).view(F)).all()


def test_grey_sources_with_and_without_alpha(ctx, data, singles):
    d, small = data[(33, 67)], data[(5, 7)]
    for dtype, layout in (("float32", "CHW"), ("uint8", "HWC"), ("float16", "HWC")):
        kw = dict(dtype=dtype, layout=layout, tfIn=abi.TF_BT709, tfOut=abi.TF_SRGB)
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"][:1], **kw),
                 host.tensorBatchItem(SIZE_A, None, "box", planes=small["f"][1:2], **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"][2:], alpha=d["af"], premultiplied=True, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=data[(3, 2100)]["f"][:1], **kw)]
        _check(ctx, items, singles, "grey %s %s" % (dtype, layout))
        items = [host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"][:1], alpha=d["a10"], alphaDepth=10, writeAlpha=True, **kw),
                 host.tensorBatchItem(SIZE_A, None, "triangle", planes=small["f"][:1], alpha=small["af"], writeAlpha=True, premultiplied=True, **kw)]
        _check(ctx, items, singles, "grey + alpha %s %s" % (dtype, layout))


def test_mixed_homes_in_one_batch(ctx, data, singles):
    d = data[(33, 67)]
    other = data[(64, 48)]
    rp = host.ResidentPlanes.upload(ctx, other["f"])
    cv = host.DeviceCanvas.fromArrays(ctx, list(d["f"]) + [d["af"]])
    cvi = host.DeviceCanvas.fromArrays(ctx, [np.random.default_rng(s).integers(0, 256, (5, 7)).astype(np.int32) for s in (4, 5, 6)] + [data[(5, 7)]["a10"]])
    try:
        for dtype, layout in (("float32", "CHW"), ("uint8", "HWC"), ("bfloat16", "HWC")):
            kw = dict(dtype=dtype, layout=layout, tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB, writeAlpha=True, premultiplied=True)
            items = [host.tensorBatchItem(SIZE_A, None, "triangle", canvas=cv, nColor=3, alphaPlane=3, **kw),
                     host.tensorBatchItem(SIZE_A, None, "triangle", resident=rp, alpha=other["af"], **kw),
                     host.tensorBatchItem(SIZE_A, None, "box", planes=d["f"], alpha=d["a8"], **kw),
                     host.tensorBatchItem(SIZE_A, (3, 2, 20, 9), "triangle", canvas=cv, nColor=3, alphaPlane=3, **kw),  # the same set again
                     host.tensorBatchItem(SIZE_A, None, "triangle", canvas=cvi, nColor=3, alphaPlane=3, alphaDepth=10, inMax=[255] * 3, **kw)]
            assert [it.source for it in items] == [abi.BATCH_SET, abi.BATCH_RESIDENT, abi.BATCH_HOST, abi.BATCH_SET, abi.BATCH_SET]
            _check(ctx, items, None, "homes %s %s" % (dtype, layout))  # (set ids and device planes: not shared beyond this test)
    finally:
        cv.release()
        cvi.release()


def test_a_small_grid_walks_tiles_of_several_items(ctx, data, singles):
    hook = _grid_hook(ctx)
    try:
        for g in (1, 3):
            assert hook(g) == abi.JXL_OK
            for dtype, layout in (("float32", "CHW"), ("uint8", "HWC")):
                _check(ctx, _batch_a(data, dtype=dtype, layout=layout), singles, "A grid %d %s" % (g, dtype))
            items = [host.tensorBatchItem(SIZE_B, None, f, planes=data[shape]["f"], dtype="float16", layout="HWC", **COLOR) for shape, f in BATCH_B]
            _check(ctx, items, singles, "B grid %d" % g)
        assert hook(-1) == abi.JXL_ERR_INVALID_ARGUMENT
    finally:
        assert hook(0) == abi.JXL_OK


def test_forced_tiles_change_no_bit(ctx, data, singles):
    tile, grid = _tile_hook(ctx), _grid_hook(ctx)
    try:
        assert tile(0, 0) == abi.JXL_OK
        a = _batch_a(data, dtype="float32", layout="HWC")
        b = [host.tensorBatchItem(SIZE_B, None, f, planes=data[shape]["f"], alpha=data[shape]["af"] if k % 2 else None, premultiplied=bool(k % 2),
                                  dtype="uint8", layout="HWC", **COLOR) for k, (shape, f) in enumerate(BATCH_B)]
        exp = [[_single(ctx, it, singles) for it in items] for items in (a, b)]  # (with the host's own tiles)
        for (tw, th), g in (((64, 4), 0), ((8, 1), 0), ((1, 1), 0), ((8, 1), 3)):
            assert tile(tw, th) == abi.JXL_OK and grid(g) == abi.JXL_OK
            for items, want in zip((a, b), exp):
                if items is a and (tw, th) == (64, 4):  # four rows of 3 x 2100's footprint are 100 KB: refused, and with it the batch
                    _refused(ctx, items, needle=["item 4", "does not fit the LDS"])
                    continue
                st, before, bodies, after = _call(ctx, items)
                assert st == abi.JXL_OK, (tw, th, ctx.lib.jxl_last_error(ctx.h))
                assert np.all(before == 0xA5) and np.all(after == 0xA5)
                for i, it in enumerate(items):
                    _same(bodies[i], want[i], it.p.dtype, "tile %dx%d grid %d item %d" % (tw, th, g, i))
    finally:
        assert tile(0, 0) == abi.JXL_OK and grid(0) == abi.JXL_OK


def _refused(ctx, items, status=abi.JXL_ERR_INVALID_ARGUMENT, needle=None, **kw):
    st, before, bodies, after = _call(ctx, items, **kw)
    assert st == status, (st, ctx.lib.jxl_last_error(ctx.h))
    assert np.all(before == 0xA5) and np.all(after == 0xA5) and all(np.all(b == 0xA5) for b in bodies), "a refused call wrote to the output"
    msg = ctx.lib.jxl_last_error(ctx.h).decode()
    if needle is not None:
        for s in ([needle] if isinstance(needle, str) else needle):
            assert s in msg, (s, msg)
    return msg


def test_refusals_leave_the_output_untouched(ctx, data):
    d, small = data[(33, 67)], data[(5, 7)]
    good = lambda **kw: host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"], **kw)  # noqa: E731
    dev = "cuda:%d" % ctx.device
    _refused(ctx, [good(), good()], n=0, needle="item count")
    _refused(ctx, [good(), good()], n=abi.TENSOR_BATCH_MAX + 1, needle="item count")
    _refused(ctx, [good(), good()], n=-3, needle="item count")
    arr = (abi.TensorBatchItem * 2)(good(), good())
    sent = torch.empty(4096, dtype=torch.uint8, device=dev).fill_(0xA5)
    assert ctx.lib.jxl_tensor_resized_batch(ctx.h, 2, None, C.c_void_p(sent.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
    assert ctx.lib.jxl_tensor_resized_batch(ctx.h, 2, arr, None) == abi.JXL_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((sent == 0xA5).all())
    bad = good()
    bad.source = 3
    _refused(ctx, [good(), bad], needle=["item 1", "unknown source"])
    # disagreement: size, dtype, layout, channel count
    _refused(ctx, [good(), host.tensorBatchItem((2, 4), None, "triangle", planes=d["f"])], needle=["item 1", "output size"])
    _refused(ctx, [good(), good(), host.tensorBatchItem((3, 5), None, "triangle", planes=d["f"])], needle=["item 2", "output size"])
    _refused(ctx, [good(), good(dtype="float16")], needle=["item 1", "dtype"])
    _refused(ctx, [good(), good(layout="HWC")], needle=["item 1", "layout"])
    _refused(ctx, [good(), host.tensorBatchItem(SIZE_A, None, "triangle", planes=d["f"][:1])], needle=["item 1", "channel count"])
    _refused(ctx, [good(), good(alpha=d["af"], writeAlpha=True)], needle=["item 1", "channel count"])
    # the resident planes: twice; once on a context that has none; an unknown set
    rp = host.ResidentPlanes.upload(ctx, d["f"])
    res = lambda: host.tensorBatchItem(SIZE_A, None, "triangle", resident=rp)  # noqa: E731
    _refused(ctx, [res(), good(), res()], needle=["item 2", "resident"])
    from jxlatte_amd import _lib
    other = _lib.Context(ctx.device)
    try:
        _refused(other, [good(), res()], status=abi.JXL_ERR_STATE, needle="item 1")
    finally:
        other.close()
    ghost = good()
    ghost.source, ghost.set_id = abi.BATCH_SET, 1 << 20
    _refused(ctx, [good(), good(), ghost], needle=["item 2", "unknown set"])
    # one bad item among good ones: a box outside its image, more than 1024 taps, a null plane, an int alpha of depth 0
    _refused(ctx, [good(), host.tensorBatchItem(SIZE_A, (60, 0, 8, 8), "triangle", planes=d["f"]), good()], needle=["item 1", "box"])
    wide = [np.zeros((1, 2100), F)] * 3
    _refused(ctx, [host.tensorBatchItem((1, 3), None, "triangle", planes=small["f"]), host.tensorBatchItem((1, 3), None, "triangle", planes=small["f"]),
                   host.tensorBatchItem((1, 3), None, "triangle", planes=wide)], needle=["item 2", "1024 taps"])
    hole = good()
    hole.in_[1] = None
    _refused(ctx, [hole, good()], needle="item 0")
    _refused(ctx, [good(alpha=d["a10"], premultiplied=True), good(alpha=d["a10"], alphaDepth=0, premultiplied=True)], needle=["item 1", "invalid Max Value"])
    odd = good()
    odd.r.filter = 2
    _refused(ctx, [good(), odd], needle=["item 1", "filter"])
    # a host pointer never reaches a kernel
    host_out = np.full(4096, 0xA5, np.uint8)
    _refused(ctx, [good(), good()], ptr=host_out.ctypes.data, needle="device memory")
    assert np.all(host_out == 0xA5)
    # an allocation that holds one tensor but not two (test_tensor_resized_gpu's construction: a segment of its own of exactly
    # 12 MiB; a tensor is 6 MiB + 4 bytes, one upscaled row)
    big = 12 << 20
    torch.cuda.empty_cache()
    short = torch.empty(big, dtype=torch.uint8, device=dev).fill_(0xA5)
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= short.data_ptr() < s["address"] + s["total_size"]]
    row = [np.zeros((1, 1024), F)]
    one = host.tensorBatchItem((1, big // 8 + 1), None, "triangle", planes=row)
    arr = (abi.TensorBatchItem * 2)(one, one)
    if len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] < short.data_ptr() + big + 8:
        assert ctx.lib.jxl_tensor_resized_batch(ctx.h, 2, arr, C.c_void_p(short.data_ptr())) == abi.JXL_ERR_INVALID_ARGUMENT
        assert b"ends before" in ctx.lib.jxl_last_error(ctx.h)
        torch.cuda.synchronize()
        assert bool((short == 0xA5).all())
    assert ctx.lib.jxl_tensor_resized_batch(ctx.h, 1, arr, C.c_void_p(short.data_ptr())) == abi.JXL_OK
    torch.cuda.synchronize()
    assert not bool(short[:big // 2 + 4].any()) and bool((short[big // 2 + 4:] == 0xA5).all())
