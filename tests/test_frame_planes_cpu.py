"""CPU-only, no library: decoder.FramePlanes on fake backends, 4 x 6 planes. With a backend that keeps planes resident: the
crossings are idempotent and logged once each, `keep` leaves the colours up, dtypes / shape / land() answer for each of the
three residencies. With a host-only backend: _chained_tail's stages reach the backend's stage calls in the order, and with the
arrays, of the inline code they replace (restated below), for a three-colour and a one-colour frame."""
import types

import numpy as np
import pytest

from jxlatte_amd import decoder
from jxlatte_amd.decoder import FramePlanes

F = np.float32
H, W = 4, 6


class Info:
    bits_per_sample, xyb_encoded, intensity_target, colour_space = 8, 0, 255.0, decoder.CE_RGB
    prim_xy, white_xy = list(decoder.PRI_SRGB), list(decoder.WP_D65)
    opsin_matrix = [11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                    -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863]
    opsin_bias = [-0.0037930732552754493] * 3
    custom_up = [0, 0, 0]
    num_extra, ec_bits = 1, [10]


def _frame(**kw):
    rec = dict(upsampling=1, ec_upsampling=[1], num_patches=0, has_splines=0, has_noise=0, save_before_ct=0, save_as_reference=0,
               do_ycbcr=0, group_dim=256, base_corr_x=0.0, base_corr_b=1.0, noise=[0.01 * (i + 1) for i in range(8)])
    rec.update(kw)
    return types.SimpleNamespace(**rec)


def _planes(colors, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W)).astype(np.int32) for _ in range(colors)] + [rng.uniform(0, 1, (H, W)).astype(F)]


def _shell(backend, info=Info):
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.backend, dec.info, dec.stats, dec.reference = backend, info, [{}], [None] * 4
    dec.visibleFrames, dec.invisibleFrames = 2, 1
    return dec


# ---- a backend that keeps planes resident ----------------------------------------------------------------------------
class FakeResident:
    def __init__(self, planes):
        self.planes, self.calls = np.array(planes, F), []

    @property
    def shape(self):
        return self.planes.shape[1:]

    def download(self):
        self.calls.append("download")
        return self.planes.copy()

    def noise(self, *a):
        self.calls.append("noise")
        self.planes = self.planes + F(1)


class ResidentBackend:
    resident = True

    def __init__(self):
        self.uploads = []

    def keep_planes(self, planes):
        self.uploads.append(np.array(planes))
        return FakeResident(planes)


class FakeSet:
    shape = (H, W)
    dtypes = [np.dtype(np.int32)] * 3 + [np.dtype(np.float32)]

    def __len__(self):
        return 4

    def download(self, c):
        return np.full(self.shape, c, self.dtypes[c])


def test_crossings_are_idempotent_and_logged_once():
    be, host = ResidentBackend(), _planes(3)
    want = [decoder._to_float(b, 8) for b in host[:3]]
    fp = FramePlanes(be, Info, host, 3)
    assert fp.resident and fp.moves == []
    rp = fp.to_device()
    assert fp.to_device() is rp and fp.moves == ["h2d"] and len(be.uploads) == 1
    assert be.uploads[0].dtype == F and all(np.array_equal(be.uploads[0][c], want[c]) for c in range(3))  # castToFloat first
    assert fp.to_host() is host and fp.to_host() is host and fp.moves == ["h2d", "d2h"] and rp.calls == ["download"]
    assert fp.rp is None and all(host[c].dtype == F and np.array_equal(host[c], want[c]) for c in range(3))


@pytest.mark.parametrize("keep", [True, False])
def test_keep_leaves_the_colours_up(keep):
    be, host = ResidentBackend(), _planes(3)
    dec = _shell(be)
    fp = FramePlanes(be, Info, host, 3)
    dec._chained_tail(_frame(has_noise=1), fp, False, False, keep=keep)
    assert (fp.rp is not None) == keep and fp.moves == (["h2d"] if keep else ["h2d", "d2h"])
    assert dec.stats[-1]["plane_moves"] is fp.moves
    if not keep:
        assert all(np.array_equal(host[c], be.uploads[0][c] + F(1)) for c in range(3))


def test_dtypes_shape_and_land_for_each_residency():
    f32, i32 = np.dtype(np.float32), np.dtype(np.int32)
    be, host = ResidentBackend(), _planes(3)
    on_host = FramePlanes(be, Info, host, 3)
    assert on_host.dtypes == [i32, i32, i32, f32] and tuple(on_host.shape) == (H, W) and on_host.one_size()
    assert on_host.land() is host and on_host.moves == []
    up = FramePlanes(be, Info, [None] * 3 + host[3:], 3, rp=FakeResident(np.stack(host[:3])))
    assert up.dtypes == [f32, f32, f32, f32] and tuple(up.shape) == (H, W) and up.one_size()
    snap = up.snapshot("trace")  # a copy comes down, the planes stay
    assert up.rp is not None and up.moves == ["trace"] and up.host[0] is None and all(isinstance(a, np.ndarray) for a in snap)
    landed = up.land()
    assert up.rp is None and len(landed) == 4 and all(isinstance(a, np.ndarray) and a.shape == (H, W) for a in landed)
    assert all(np.array_equal(landed[c], host[c]) for c in range(4)) and up.moves == ["trace"]  # (landing is no move of the tail)
    ready = FramePlanes(be, Info, [None] * 3, 3, fset=FakeSet())
    assert ready.dtypes == FakeSet.dtypes and tuple(ready.shape) == (H, W) and ready.one_size() and ready.blend_set() is ready.set
    landed = ready.land()
    assert [a.dtype for a in landed] == FakeSet.dtypes and [int(a[0, 0]) for a in landed] == [0, 1, 2, 3]


# ---- a host-only backend: the stage calls --------------------------------------------------------------------------------
class HostBackend:
    """no `resident`: every stage is a stage call on host arrays. Each call is logged with copies of its array arguments"""

    def __init__(self):
        self.calls = []

    def _log(self, name, *args):
        self.calls.append((name,) + tuple(np.array(a) if isinstance(a, np.ndarray) else a for a in args))

    def upsample(self, plane, k, weights):
        self._log("upsample", plane, k, weights)
        return np.kron(plane, np.ones((k, k), F)).astype(F)

    def noise_init(self, h, w, seed0, group_dim, colors):
        self._log("noise_init", h, w, seed0, group_dim, colors)
        return np.full((3, h, w), 0.5, F)

    def noise_add(self, planes, noise, lut, bcx, bcb):
        self._log("noise_add", planes, noise, lut, bcx, bcb)
        return planes + noise

    def xyb(self, planes, matrix, bias, cbrt, intensity_target):
        self._log("xyb", planes, matrix, bias, cbrt, intensity_target)
        return planes * F(2)

    def ycbcr(self, planes):
        self._log("ycbcr", planes)
        return planes[::-1] + F(3)


def _inline(dec, fr, buffers, colors, xyb_done):
    """the host flavour of JXLCodestreamDecoder.java:628-637 as decode() spelled it out before FramePlanes"""
    info, be = dec.info, dec.backend
    for c in range(len(buffers)):
        k = fr.upsampling if c < colors else fr.ec_upsampling[c - colors]
        if k > 1:
            depth = info.bits_per_sample if c < colors else info.ec_bits[c - colors]
            buffers[c] = be.upsample(dec._to_float(buffers[c], depth), k, dec._up_weights(k))
    if fr.has_noise:
        h, w = buffers[0].shape
        noise = be.noise_init(h, w, (dec.visibleFrames << 32) | dec.invisibleFrames, fr.group_dim, colors)
        planes = np.stack([dec._to_float(buffers[c], info.bits_per_sample) for c in range(3)])
        planes = be.noise_add(planes, noise, np.array(fr.noise, F), fr.base_corr_x, fr.base_corr_b)
        for c in range(3):
            buffers[c] = np.ascontiguousarray(planes[c])
    if (info.xyb_encoded and not xyb_done) or fr.do_ycbcr:
        planes = np.stack([dec._to_float(buffers[c], info.bits_per_sample) for c in range(3)])
        if info.xyb_encoded and not xyb_done:
            m, bias, cbrt = dec._opsin()
            planes = be.xyb(planes, m, bias, cbrt, info.intensity_target)
        if fr.do_ycbcr:
            planes = be.ycbcr(planes)
        for c in range(3):
            buffers[c] = np.ascontiguousarray(planes[c])
    return buffers


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@pytest.mark.parametrize("colors", [3, 1])
def test_host_only_stages_call_the_backend_as_the_inline_code_did(colors):
    class XYB(Info):
        xyb_encoded = 1
        num_extra, ec_bits = (1, [10]) if colors == 3 else (2, [10, 10])
    info = XYB if colors == 3 else type("Grey", (XYB,), dict(xyb_encoded=0, colour_space=decoder.CE_GRAY))
    fr = _frame(upsampling=2, ec_upsampling=[2] * info.num_extra, has_noise=1, do_ycbcr=1)
    start = _planes(3)[:colors + info.num_extra] if colors == 3 else _planes(1) + [np.arange(H * W, dtype=np.int32).reshape(H, W)]
    want_be, got_be = HostBackend(), HostBackend()
    want = _inline(_shell(want_be, info), fr, [b.copy() for b in start], colors, False)
    dec = _shell(got_be, info)
    host = [b.copy() for b in start]
    fp = FramePlanes(got_be, info, host, colors)
    assert not fp.resident
    dec._chained_tail(fr, fp, False, False)
    names = [c[0] for c in got_be.calls]
    assert names == ["upsample"] * len(start) + ["noise_init", "noise_add"] + (["xyb"] if colors == 3 else []) + ["ycbcr"]
    assert names == [c[0] for c in want_be.calls]
    for g, w in zip(got_be.calls, want_be.calls):
        assert len(g) == len(w) and all(_same(a, b) for a, b in zip(g, w)), g[0]
    assert fp.host is host and len(host) == len(want) and all(_same(a, b) for a, b in zip(host, want))
    assert "plane_moves" not in dec.stats[-1] and fp.moves == [] and fp.rp is None
