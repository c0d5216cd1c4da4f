"""The pooled IDCT-output planes are cell-tiled (jxlatte_amd/csrc/plane_tiled.h): the 256-thread IDCT launch stores
whole 8x8 cells into them and the fused restoration launch of the same call gathers its input tile from cells. The layout moves
where samples sit between two launches and never a value, so every comparison here is bit for bit: the frame on two contexts that
share a stream (pooled planes: tiled), the same frame on a context with a stream of its own (private planes: raster), and the
oracle. jxl_debug_last_plane_a_tiled tells which layout a run took, jxl_debug_set_plane_a_tiled is what JXL_PLANE_A_TILED=0 sets
(jxlatte_amd/_lib.py).

Sizes: the restoration tile grid (62 x 30 output tiles, 70 x 38 input tiles) and the 8 x 8 cell grid disagree in every way --
64 x 32 is one tile, at 72 x 40 cells cross the tile's right and bottom halo, 136 x 72 has an interior tile (the cell-gather
loader) with all four neighbours, 256 x 256 is a whole group, in which a 64 x 64 block fits."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import switch_cases as sc
from conftest import ROOT, assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

SIZES = ((64, 32), (72, 40), (136, 72), (256, 256))
# name -> (mix, the type the frame must contain). The shares of the large types are chosen so that synth places them wherever they fit.
MIXES = {
    "default": (None, None),  # the default mix restricted to the types that fit the frame
    "dct8": ({"DCT8": 1.0}, "DCT8"),
    "hornuss": ({"HORNUSS": 1.0}, "HORNUSS"),
    "dct2": ({"DCT2": 1.0}, "DCT2"),
    "dct4": ({"DCT4": 1.0}, "DCT4"),
    "dct4_8": ({"DCT4_8": 1.0}, "DCT4_8"),
    "dct8_4": ({"DCT8_4": 1.0}, "DCT8_4"),
    "afv": ({"AFV1": 1.0}, "AFV1"),
    "dct16_8": ({"DCT16_8": 0.6, "DCT8": 0.4}, "DCT16_8"),  # rectangles whose rows split across cells
    "dct8_32": ({"DCT8_32": 0.6, "DCT8": 0.4}, "DCT8_32"),
    "dct32": ({"DCT32": 0.7, "DCT8": 0.3}, "DCT32"),
    "dct64": ({"DCT64": 0.95, "DCT8": 0.05}, "DCT64"),
}


def _fits(name, w, h):
    t = abi.TRANSFORM_TYPES[abi.TT_BY_NAME[name]]
    return t[5] <= h and t[6] <= w


def _grid():
    out = []
    for w, h in SIZES:
        for m, (mix, need) in MIXES.items():
            names = (need,) if isinstance(need, str) else (need or ())
            if all(_fits(n, w, h) for n in names):
                out.append((w, h, m))
    return out


_cache = {}


def _case(w, h, m, **kw):
    """(frame, raster result on a private stream, oracle result), made once"""
    key = (w, h, m, tuple(sorted(kw.items())))
    if key not in _cache:
        mix, need = MIXES[m]
        if mix is None:
            mix = {n: s for n, s in synth.MIX_DEFAULT.items() if _fits(n, w, h)}
        f = synth.make_vardct_frame(w, h, seed=500 + zlib.crc32(repr(key).encode()) % 1000, mix=mix, **kw)
        hist = synth.type_histogram(f)
        for n in ((need,) if isinstance(need, str) else (need or ())):
            assert hist.get(n, 0) > 0, (n, hist)
        with _lib.Context(0) as c:
            fr = host.Frame.from_synth(c, f)
            raster = fr.decodeFrame().copy()
            assert _last_tiled(c) == 0  # a context alone on its stream keeps private raster planes
        _cache[key] = (f, raster, orc.vardct_frame(f))
    return _cache[key]


def _hook(name, res, args):
    fn = getattr(_lib.load(), name)
    fn.restype, fn.argtypes = res, args
    return fn


def _last_tiled(ctx):
    return _hook("jxl_debug_last_plane_a_tiled", C.c_int, [C.c_void_p])(ctx.h)


def _set_tiled(on):
    return _hook("jxl_debug_set_plane_a_tiled", C.c_int, [C.c_int])(on)


class _Shared:
    """two contexts on the stream of a third that runs nothing: their IDCT output goes to the stream's pooled planes"""

    def __init__(self, n=2):
        self.holder = _lib.Context(0)
        self.ctxs = [_lib.Context(0) for _ in range(n)]
        for c in self.ctxs:
            c.call("jxl_ctx_set_stream", self.holder.stream)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for c in self.ctxs:
            c.close()
        self.holder.close()


def _run_shared(sh, f, expect_tiled, what, exp, raster=None):
    """the frame on both contexts of the pool, interleaved; every result against the oracle (and the raster run)"""
    frs = [host.Frame.from_synth(c, f) for c in sh.ctxs]
    for fr in frs:
        fr.run()
    for c, fr in zip(sh.ctxs, frs):
        got = sc.planar(fr.readOutput())
        assert _last_tiled(c) == expect_tiled, what
        assert_bits_equal(got, exp, what + ": shared stream against the oracle")
        if raster is not None:
            assert_bits_equal(got, sc.planar(raster), what + ": shared stream against a stream of its own")


@pytest.fixture(autouse=True)
def _tiled_default():
    was = _set_tiled(1)
    yield
    _set_tiled(was)


@pytest.mark.parametrize("w,h,m", _grid(), ids=lambda v: str(v))
def test_tiled_path_equals_raster_path_and_oracle(w, h, m):
    f, raster, exp = _case(w, h, m)
    assert_bits_equal(raster, exp, "%dx%d %s: private stream against the oracle" % (w, h, m))
    with _Shared() as sh:
        _run_shared(sh, f, 1, "%dx%d %s" % (w, h, m), exp, raster)


@pytest.mark.parametrize("gab", (1, 0))
@pytest.mark.parametrize("it", (0, 1, 2))
def test_restoration_variants(gab, it):
    f, raster, exp = _case(136, 72, "default", gab=bool(gab), epf_iters=it)
    with _Shared() as sh:
        _run_shared(sh, f, 1, "136x72 gab %d epf %d" % (gab, it), exp, raster)


def test_quantising_sink_reads_tiled_planes():
    base, _, _ = _case(136, 72, "default")
    f = sc.with_params(base, 31, transfer=abi.TRANSFER_SRGB, out_format=abi.OUT_RGB8)
    with _Shared() as sh:
        _run_shared(sh, f, 1, "136x72 sRGB RGB8", orc.vardct_frame(f))


def test_three_epf_iterations_keep_raster():
    f, raster, exp = _case(136, 72, "default", epf_iters=3)
    with _Shared() as sh:
        _run_shared(sh, f, 0, "136x72 epf 3", exp, raster)


def test_switch_off_equals_default():
    f, raster, exp = _case(136, 72, "default")
    with _Shared() as sh:
        _run_shared(sh, f, 1, "tiled", exp, raster)
        _set_tiled(0)
        _run_shared(sh, f, 0, "raster in the same pooled planes", exp, raster)
        _set_tiled(1)
        _run_shared(sh, f, 1, "tiled again", exp, raster)


def test_environment_switch_reaches_the_library():
    """JXL_PLANE_A_TILED=0 in a fresh process (read once, when the package loads the library): raster on the shared path, same bits"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_tiled_plane_a_gpu as t\n"
            "f, raster, exp = t._case(136, 72, 'default')\n"
            "with t._Shared() as sh:\n"
            "    t._run_shared(sh, f, int(sys.argv[1]), 'child', exp, raster)\n"
            "print('CHILD OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    for value, tiled in (("0", 0), ("1", 1)):
        r = subprocess.run([sys.executable, "-c", code, str(tiled)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, JXL_PLANE_A_TILED=value))
        assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_two_sizes_share_one_pool_back_to_back():
    """the pool holds one set per size; a set is rewritten by frames of either layout (a frame that keeps raster between two tiled ones)"""
    big = _case(136, 72, "default")
    small = _case(72, 40, "default")
    e3 = _case(136, 72, "default", epf_iters=3)  # same size class as `big`, raster
    with _Shared(3) as sh:
        frs = [host.Frame.from_synth(c, x[0]) for c, x in zip(sh.ctxs, (big, small, e3))]
        for order in ((0, 1, 2, 0, 1), (2, 0, 0, 1, 2)):
            for i in order:
                frs[i].run()
            for i, x in enumerate((big, small, e3)):
                assert_bits_equal(frs[i].readOutput(), x[2], "frame %d after runs %s" % (i, order))
        assert [_last_tiled(c) for c in sh.ctxs] == [1, 1, 0]
        # a context whose frame changes size moves to the other set
        fr = host.Frame.from_synth(sh.ctxs[0], small[0])
        fr.run()
        frs[1].run()
        assert_bits_equal(fr.readOutput(), small[2], "72x40 on the context that ran 136x72")
        assert_bits_equal(frs[1].readOutput(), small[2], "72x40 beside it")


def test_frame_with_a_512_thread_side_launch_keeps_raster():
    """a DCT64_32 block belongs to the 512-thread launch, which stores raster: the whole frame keeps raster in the pooled planes"""
    f = synth.make_vardct_frame(136, 72, seed=77, mix={"DCT64_32": 0.95, "DCT8": 0.05})
    assert synth.type_histogram(f).get("DCT64_32", 0) > 0
    exp = orc.vardct_frame(f)
    with _Shared() as sh:
        _run_shared(sh, f, 0, "136x72 with DCT64_32", exp)
