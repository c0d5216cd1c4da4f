"""GPU, C ABI: every way a decoded image leaves the library, from each of its three homes -- host planes (jxl_stage_*), the
context's resident planes (jxl_planes_*), a plane set (jxl_canvas_*, JXL_BATCH_SET) -- as ONE table: the PNG, PFM, colour peak,
tensor and resized tensor entries, the PNG guard hook, and the batch with one item of each source kind.

A refusal is pinned by its status code, the exact text of jxl_last_error (written out below, from the entries' source: the JNI
shim makes it the Java exception's message) and by the output still holding its 0xA5 fill. An accepted call equals the same image
through the family's jxl_stage_* entry bit for bit.

The fixture is that of tests/test_canvas_samples_gpu.py: 5 x 7; a set of three float colour planes, an int32 plane at 3 and a
float plane at 4; resident planes of 5 x 7 with the set's colours. A second context has no resident planes and no set."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from jxlatte_amd import _lib, abi, host

pytestmark = pytest.mark.gpu
F = np.float32
SHAPE = (5, 7)
SIZE = (3, 4)  # of the resized tensors
INV, STATE = abi.JXL_ERR_INVALID_ARGUMENT, abi.JXL_ERR_STATE
FAMILIES = ("png", "pfm", "peak", "tensor", "resized")


@pytest.fixture(scope="module")
def env(ctx):
    rng = np.random.default_rng(57)
    fl = [rng.uniform(0, 1, SHAPE).astype(F) for _ in range(3)]
    ai = rng.integers(1, 256, SHAPE).astype(np.int32)
    af = rng.uniform(0.1, 1, SHAPE).astype(F)
    for a in fl + [ai, af]:
        a.setflags(write=False)
    cv = host.DeviceCanvas.fromArrays(ctx, fl + [ai, af])
    grey = host.DeviceCanvas.fromArrays(ctx, [fl[0]])
    rp = host.ResidentPlanes.upload(ctx, fl)
    bare = _lib.Context(ctx.device)
    guard = ctx.lib.jxl_debug_png_samples_guard
    guard.restype = C.c_int32
    guard.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(abi.PngParams), C.c_void_p, C.c_int32]
    yield types.SimpleNamespace(ctx=ctx, bare=bare, fl=fl, ai=ai, af=af, cv=cv, grey=grey, rp=rp, guard=guard, stage={})
    bare.close()
    grey.release()
    cv.release()


# ---- the parameters of a family: good ones for the fixture, and what a refusal has wrong ----
def _good(env, family, alpha, write_alpha=False):
    a = env.ai if alpha else None
    if family == "png":
        return host.pngParams(env.fl, SHAPE, alpha=a, bitDepth=8)
    if family == "pfm":
        return host.pfmParams(env.fl, SHAPE, [8, 8, 8])
    if family == "peak":
        return host.colorParams(env.fl, tfIn=abi.TF_SRGB)
    return host.tensorParams(env.fl, SHAPE, alpha=a, writeAlpha=write_alpha, tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB)


def _spoil(family, p, what):
    if what == "colour tag":
        if family == "pfm":
            p.is_int[0], p.tagged_depth[0] = 1, 8
        else:
            col = p if family == "peak" else p.color
            col.in_is_int = 1
            for i in range(3):
                col.in_max[i] = 255
    elif what in ("alpha tag float", "has_alpha without a plane"):
        pass  # (the parameters are good: the plane asked for is not)
    elif what == "alpha tag int":
        p.alpha_is_int = 0
    elif what == "a plane without has_alpha":
        p.has_alpha = p.alpha_is_int = 0
    elif what == "transposed":
        p.height, p.width = SHAPE[1], SHAPE[0]
    elif what == "width + 1":
        p.width = SHAPE[1] + 1
    elif what == "one plane":
        p.n_planes = 1
    return p


def _alpha_plane(what, has_alpha):
    if not has_alpha:
        return -1
    return {"alpha plane 5": 5, "alpha plane -2": -2, "has_alpha without a plane": -1, "alpha tag float": 4}.get(what, 3)


def _rz(p):
    return host.resizeParams((p.height, p.width), SIZE)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _device_out(ctx, n=4096):
    return torch.empty(n, dtype=torch.uint8, device="cuda:%d" % ctx.device).fill_(0xA5)


def _entry(env, family, home, p, ctx=None, set_id=None, alpha_plane=-1, null_out=False, null_rz=False, guard=None):
    """one call of the family's entry for `home` into 0xA5-filled memory: (status, jxl_last_error, the output's bytes)"""
    ctx = env.ctx if ctx is None else ctx
    lib, h = ctx.lib, ctx.h
    ref = None if p is None else C.byref(p)
    has_alpha = family in ("png", "tensor", "resized") and p is not None and p.has_alpha
    alpha = _ptr(env.ai) if has_alpha else None
    planes = host._pv(env.fl)
    set_id = env.cv.id if set_id is None else set_id
    if family in ("tensor", "resized"):
        buf = _device_out(ctx)
        out = None if null_out else C.c_void_p(buf.data_ptr())
        rz = None if (null_rz or p is None) else C.byref(_rz(p))
        args = (ref, out) if family == "tensor" else (ref, rz, out)
        name = "samples" if family == "tensor" else "resized"
        if home == "stage":
            st = getattr(lib, "jxl_stage_tensor_" + name)(h, planes, alpha, *args)
        elif home == "resident":
            st = getattr(lib, "jxl_planes_tensor_" + name)(h, alpha, *args)
        else:
            st = getattr(lib, "jxl_canvas_tensor_" + name)(h, set_id, alpha_plane, *args)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
    else:
        got = np.full(4 if family == "peak" else 1024, 0xA5, np.uint8)
        out = None if null_out else got.ctypes.data
        if family == "peak":
            out = None if null_out else C.cast(got.ctypes.data, C.POINTER(C.c_float))
            if home == "stage":
                st = lib.jxl_stage_color_peak(h, planes, SHAPE[0], SHAPE[1], ref, out)
            elif home == "resident":
                st = lib.jxl_planes_color_peak(h, ref, out)
            else:
                st = lib.jxl_canvas_color_peak(h, set_id, ref, out)
        elif family == "pfm":
            if home == "stage":
                st = lib.jxl_stage_pfm_samples(h, planes, ref, out)
            elif home == "resident":
                st = lib.jxl_planes_pfm_samples(h, ref, out)
            else:
                st = lib.jxl_canvas_pfm_samples(h, set_id, ref, out)
        elif home == "stage":
            st = lib.jxl_stage_png_samples(h, planes, alpha, ref, out)
        elif home == "guard":
            st = env.guard(h, planes, alpha, ref, out, 16 if guard is None else guard)
        elif home == "resident":
            st = lib.jxl_planes_png_samples(h, alpha, ref, out)
        else:
            st = lib.jxl_canvas_png_samples(h, set_id, alpha_plane, ref, out)
    return st, (lib.jxl_last_error(h) or b"").decode(), got


# ---- the refusals: (family, home, what is wrong, status, jxl_last_error) ----
NULL = {"png": "png samples: null argument", "pfm": "pfm samples: null argument", "tensor": "tensor samples: null argument"}
RESIDENT_SIZE = {"png": "png samples: the resident planes are three 5 x 7 float planes",
                 "pfm": "pfm samples: the resident planes are three 5 x 7 float planes",
                 "tensor": "tensor samples: the resident planes are three float planes of another size",
                 "resized": "tensor samples: the resident planes are three float planes of another size"}
SET_PLANES = {"png": "png samples: the set has no such planes", "peak": "color peak: the set has no such planes",
              "tensor": "tensor samples: the set has no such planes", "resized": "tensor samples: the set has no such planes"}
SET_DESCRIBE = {"png": "png samples: the parameters do not describe the set's 5 x 7 planes",
                "pfm": "pfm samples: the parameters do not describe the set's 5 x 7 planes",
                "peak": "color peak: the parameters do not describe the set's planes",
                "tensor": "tensor samples: the parameters do not describe the set's planes",
                "resized": "tensor samples: the parameters do not describe the set's planes"}
REFUSALS = []
for fam in FAMILIES:
    REFUSALS += [(fam, "resident", "no resident planes", STATE, "no resident planes"),
                 (fam, "resident", "no resident planes, null p", STATE, "no resident planes"),
                 (fam, "set", "unknown set", INV, "canvas: unknown set"),
                 (fam, "set", "unknown set, null p", INV, "canvas: unknown set")]
for fam in ("png", "pfm", "tensor", "resized"):
    for what in ("colour tag", "transposed", "width + 1"):
        REFUSALS += [(fam, "resident", what, INV, RESIDENT_SIZE[fam]), (fam, "set", what, INV, SET_DESCRIBE[fam])]
for fam in ("png", "tensor", "resized"):
    for what in ("alpha plane 5", "alpha plane -2", "has_alpha without a plane", "a plane without has_alpha", "more planes than the set"):
        REFUSALS.append((fam, "set", what, INV, SET_PLANES[fam]))
    for what in ("alpha tag int", "alpha tag float"):
        REFUSALS.append((fam, "set", what, INV, SET_DESCRIBE[fam]))
for fam in ("png", "pfm", "tensor"):
    for home in ("stage", "resident", "set") + (("guard",) if fam == "png" else ()):
        REFUSALS += [(fam, home, "null p", INV, NULL[fam]), (fam, home, "null out", INV, NULL[fam])]
REFUSALS += [
    ("png", "guard", "negative guard", INV, "png samples: bad guard size"),
    ("pfm", "set", "more planes than the set", INV, SET_DESCRIBE["pfm"]),
    # the colour peak: the resident entry has one text for its whole second half; the set entry refuses a null p as planes
    # the set does not have
    ("peak", "stage", "null p", INV, "color: null argument"),
    ("peak", "stage", "null out", INV, "color peak: bad arguments"),
    ("peak", "resident", "null p", INV, "color: null argument"),
    ("peak", "resident", "null out", INV, "color peak: bad arguments"),
    ("peak", "resident", "colour tag", INV, "color peak: bad arguments"),
    ("peak", "resident", "one plane", INV, "color peak: bad arguments"),
    ("peak", "set", "null p", INV, SET_PLANES["peak"]),
    ("peak", "set", "more planes than the set", INV, SET_PLANES["peak"]),
    ("peak", "set", "null out", INV, "color peak: bad arguments"),
    ("peak", "set", "colour tag", INV, SET_DESCRIBE["peak"]),
    # the resized entries: the resize's own check meets a null p first where no set is asked before it
    ("resized", "stage", "null p", INV, "tensor resized: null argument"),
    ("resized", "resident", "null p", INV, "tensor resized: null argument"),
    ("resized", "set", "null p", INV, "tensor samples: null argument"),
    ("resized", "stage", "null out", INV, "tensor samples: null argument"),
    ("resized", "resident", "null out", INV, "tensor samples: null argument"),
    ("resized", "set", "null out", INV, "tensor samples: null argument"),
    ("resized", "stage", "null resize", INV, "tensor resized: null argument"),
    ("resized", "resident", "null resize", INV, "tensor resized: null argument"),
    ("resized", "set", "null resize", INV, "tensor resized: null argument"),
]


@pytest.mark.parametrize("family,home,what,status,text", REFUSALS, ids=["%s-%s-%s" % r[:3] for r in REFUSALS])
def test_refusal(env, family, home, what, status, text):
    has_alpha = family in ("png", "tensor", "resized") and home == "set" or what.startswith("alpha")
    p = None if what.endswith("null p") else _spoil(family, _good(env, family, has_alpha), what)
    kw = {}
    if what.startswith("no resident planes"):
        kw["ctx"] = env.bare
    if what.startswith("unknown set"):
        kw["set_id"] = env.cv.id + 100
    if what == "more planes than the set":
        kw["set_id"] = env.grey.id
    if what == "negative guard":
        kw["guard"] = -1
    alpha_plane = -1 if (what == "more planes than the set" and family != "pfm") else _alpha_plane(what, has_alpha)
    if what == "more planes than the set" and p is not None and family in ("png", "tensor", "resized"):
        p.has_alpha = p.alpha_is_int = 0
    st, err, out = _entry(env, family, home, p, alpha_plane=alpha_plane, null_out=what == "null out", null_rz=what == "null resize", **kw)
    assert (st, err) == (status, text)
    assert np.all(out == 0xA5), "the output was written"


# ---- the accepted calls: every home's output is the stage entry's ----
def _accepted(env, family, home):
    alpha = family in ("png", "tensor", "resized")
    p = _good(env, family, alpha, write_alpha=True)
    st, err, out = _entry(env, family, home, p, alpha_plane=3 if alpha else -1)
    assert st == abi.JXL_OK, (st, err)
    return out


def _bytes(family):
    n = SHAPE[0] * SHAPE[1]
    return {"png": n * 4, "pfm": n * 3 * 4, "peak": 4, "tensor": n * 4 * 4, "resized": SIZE[0] * SIZE[1] * 4 * 4}[family]


def _stage(env, family):
    if family not in env.stage:
        out = _accepted(env, family, "stage")
        n = _bytes(family)
        assert np.all(out[n:] == 0xA5) and not np.all(out[:n] == 0xA5)
        env.stage[family] = out
    return env.stage[family]


@pytest.mark.parametrize("family,home", [(f, h) for f in FAMILIES for h in ("resident", "set")] + [("png", "guard")])
def test_accepted_call_equals_the_stage_entry(env, family, home):
    exp = _stage(env, family)
    got = _accepted(env, family, home)
    n = _bytes(family)
    assert np.array_equal(got[:n], exp[:n]), "%d bytes differ" % int((got[:n] != exp[:n]).sum())
    assert np.all(got[n:] == 0xA5), "bytes behind the output were written"  # (the guard hook's 16 bytes are 0xA5 too)


# ---- the batch: one item of each source kind ----
def _items(env, alpha, write_alpha=False):
    kw = dict(writeAlpha=write_alpha, tfIn=abi.TF_SRGB, tfOut=abi.TF_SRGB)
    a = env.ai if alpha else None
    return [host.tensorBatchItem(SIZE, planes=env.fl, alpha=a, **kw), host.tensorBatchItem(SIZE, resident=env.rp, alpha=a, **kw),
            host.tensorBatchItem(SIZE, canvas=env.cv, alphaPlane=3 if alpha else None, **kw)]


def _batch(env, items, ctx=None, null_out=False, null_items=False):
    ctx = env.ctx if ctx is None else ctx
    buf = _device_out(ctx)
    arr = (abi.TensorBatchItem * len(items))(*items)
    st = ctx.lib.jxl_tensor_resized_batch(ctx.h, len(items), None if null_items else arr, None if null_out else C.c_void_p(buf.data_ptr()))
    torch.cuda.synchronize()
    return st, (ctx.lib.jxl_last_error(ctx.h) or b"").decode(), buf.cpu().numpy()


ITEM = "tensor batch: item %d: "
BATCH_REFUSALS = [
    (1, "no resident planes", STATE, ITEM % 1 + "no resident planes"),
    (2, "unknown set", INV, ITEM % 2 + "canvas: unknown set"),
    (2, "alpha plane 5", INV, ITEM % 2 + SET_PLANES["tensor"]),
    (2, "alpha plane -2", INV, ITEM % 2 + SET_PLANES["tensor"]),
    (2, "has_alpha without a plane", INV, ITEM % 2 + SET_PLANES["tensor"]),
    (2, "a plane without has_alpha", INV, ITEM % 2 + SET_PLANES["tensor"]),
    (2, "more planes than the set", INV, ITEM % 2 + SET_PLANES["tensor"]),
    (2, "alpha tag int", INV, ITEM % 2 + SET_DESCRIBE["tensor"]),
    (2, "alpha tag float", INV, ITEM % 2 + SET_DESCRIBE["tensor"]),
    (None, "null out", INV, "tensor batch: null argument"),
    (None, "null items", INV, "tensor batch: null argument"),
]
for _what in ("colour tag", "transposed", "width + 1"):
    BATCH_REFUSALS += [(1, _what, INV, ITEM % 1 + RESIDENT_SIZE["tensor"]), (2, _what, INV, ITEM % 2 + SET_DESCRIBE["tensor"])]


@pytest.mark.parametrize("bad,what,status,text", BATCH_REFUSALS, ids=["item %s-%s" % r[:2] for r in BATCH_REFUSALS])
def test_batch_refusal(env, bad, what, status, text):
    items = _items(env, alpha=True)
    ctx = None
    if what == "no resident planes":
        ctx, items = env.bare, items[:2]
    elif bad is not None:
        it = items[bad]
        _spoil("tensor", it.p, what)
        it.r = _rz(it.p)
        if bad == 2:
            it.alpha_plane = _alpha_plane(what, True)
        if what == "unknown set":
            it.set_id = env.cv.id + 100
        if what == "more planes than the set":
            it.set_id, it.alpha_plane, it.p.has_alpha, it.p.alpha_is_int = env.grey.id, -1, 0, 0
    st, err, out = _batch(env, items, ctx=ctx, null_out=what == "null out", null_items=what == "null items")
    assert (st, err) == (status, text)
    assert np.all(out == 0xA5), "the output was written"


def test_batch_items_equal_the_stage_entry(env):
    exp = _stage(env, "resized")
    n = _bytes("resized")
    st, err, out = _batch(env, _items(env, alpha=True, write_alpha=True))
    assert st == abi.JXL_OK, (st, err)
    for i in range(3):
        assert np.array_equal(out[i * n:(i + 1) * n], exp[:n]), "item %d" % i
    assert np.all(out[3 * n:] == 0xA5)
