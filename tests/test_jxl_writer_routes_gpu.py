"""GPU: the bitstreams of tests/jxl_writer_cases.py through JXLDecoder on the device backend, under the default switches, each opt-in
set the project documents as a unit (device_image; device_canvas; device_canvas + device_frames; the five of
test_device_chains_gpu.SWITCHES; device_palette; device_output) and all of them together. What comes out -- planes (dtype, shape,
bits), PNGWriter's samples, PFMWriter's bytes, toTensor in both layouts as float32 and uint8 -- is compared with what
jxl_writer_cases computes from the SOURCE pixels, never with another decode of the same bytes; only an upsampled frame, which is
not exact, is held to K["upsample"] of test_pixel_ref64_cpu.py AND to bit-equality with the default decode.

The route tables (jxl_writer_cases.ROUTE_CASES, ACCEPTED) are run here: every string a route function can return shows up in the
stats of a real decode of the image listed for it, and every accepted route is taken by the image built for it.

One bitstream is encoded once (a cache) and decoded once per switch set."""
import io

import numpy as np
import pytest
import torch

import jxl_writer as W
import jxl_writer_cases as C
import jxl_writer_lossy_run as RUN
from conftest import assert_bits_equal
from jxlatte_amd import frontend
from jxlatte_amd.decoder import JXLDecoder, PFMWriter, PNGWriter
from test_device_frames_gpu import CountingBackend
from test_jxl_writer_cpu import png_of
from test_pixel_ref64_cpu import K, ratio

pytestmark = pytest.mark.gpu
F = np.float32
_bytes, _default_up = {}, {}


@pytest.fixture(scope="module")
def backend(ctx):
    return CountingBackend(ctx)


def encoded(table, name):
    if (table, name) not in _bytes:
        _bytes[table, name] = W.encode(C.table(table)[name])
    return _bytes[table, name]


def decode(table, name, backend, switches):
    kw = dict(switches)
    trace = kw.pop("trace", False)
    dec = JXLDecoder(encoded(table, name), backend=backend, **kw)
    if trace:
        dec.trace = lambda k, stage, planes, fused: None
    backend.calls.clear()
    return dec, dec.decode()


def tensor_expectation(im, planes):
    """(float32 [C][H][W], uint8 [C][H][W]) of toTensor(target="as-is", alpha dropped): the colour planes cast with their depth, a
    premultiplied image's divided by its alpha (PNGWriter.java:94-104), and the quantiser of ImageBuffer.castToInt0 at 255"""
    n_col, ai = 1 if im.get("grey") else 3, C.alpha_index(im)
    depths = C.depths_of(im)
    f = [C.cast_to_float(planes[c], depths[c]) for c in range(n_col)]
    if ai >= 0 and im["extra"][ai].get("alpha_associated", False):
        a = C.cast_to_float(planes[n_col + ai], depths[n_col + ai])
        with np.errstate(all="ignore"):
            f = [(p / a).astype(F) for p in f]
    f = np.stack(f)
    with np.errstate(all="ignore"):
        q = (f * F(255) + F(0.5)).astype(F)
    u8 = np.clip(np.nan_to_num(np.trunc(q.astype(np.float64)), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)
    return f, u8


def check_image(im, got, exp_planes, what, exact=True):
    """the writers and the tensors first (while the planes are the image's), then the planes"""
    if exact:
        bit_depth, exp_png = C.png_samples(im, exp_planes)
        w = PNGWriter(got, deviceSamples=True)
        assert w.bitDepth == bit_depth, what
        got_png = png_of(w)
        assert got_png.shape == exp_png.shape and np.array_equal(got_png, exp_png), "%s: %d PNG samples differ" % (what, int((got_png != exp_png).sum()))
        buf = io.BytesIO()
        PFMWriter(got, deviceSamples=True).write(buf)
        assert buf.getvalue() == C.pfm_bytes(im, exp_planes), what + ": PFM bytes"
        exp_f, exp_u8 = tensor_expectation(im, exp_planes)
        for layout in ("CHW", "HWC"):
            t = got.toTensor(torch.float32, layout=layout, target="as-is").cpu().numpy()
            e = exp_f if layout == "CHW" else np.ascontiguousarray(np.moveaxis(exp_f, 0, -1))
            assert_bits_equal(t, e, "%s tensor float32 %s" % (what, layout), any_nan=True)
            t = got.toTensor(torch.uint8, layout=layout, target="as-is").cpu().numpy()
            e = exp_u8 if layout == "CHW" else np.ascontiguousarray(np.moveaxis(exp_u8, 0, -1))
            assert t.dtype == np.uint8 and t.shape == e.shape and np.array_equal(t, e), "%s tensor uint8 %s: %d differ" % (what, layout, int((t != e).sum()))
    planes = got.getBuffer()
    assert len(planes) == len(exp_planes), what
    for c, (a, b) in enumerate(zip(planes, exp_planes)):
        if exact:
            assert_bits_equal(a, b, "%s plane %d" % (what, c), any_nan=True)
    return planes


GROUPS = list(C.SINGLE) + ["multi", "multi_fixed", "routed", "floats"]


@pytest.mark.parametrize("config", list(C.CONFIGS))
@pytest.mark.parametrize("group", GROUPS)
def test_images_equal_their_source(backend, group, config):
    for name, im in C.table(group).items():
        dec, got = decode(group, name, backend, C.CONFIGS[config])
        try:
            check_image(im, got, C.expected_planes(im), "%s under %s" % (name, config))
        finally:
            dec.close()


@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_upsampled_frames(backend, config):
    """within K["upsample"] of the float64 model of the source, and bit for bit what the default switches give"""
    for name, im in C.UPSAMPLED.items():
        dec, got = decode("upsampled", name, backend, C.CONFIGS[config])
        try:
            model = C.upsampled_model(im)
            planes = check_image(im, got, [m[0] for m in model], name, exact=False)
            for c, (x, a) in enumerate(model):
                if a is None:
                    assert_bits_equal(planes[c], x, "%s plane %d under %s" % (name, c, config))
                else:
                    assert planes[c].dtype == np.float32 and planes[c].shape == x.shape, (name, c)
                    ratio(planes[c], x, a, "%s plane %d under %s" % (name, c, config), K["upsample"])
            if config == "default":
                _default_up[name] = [p.copy() for p in planes]
            else:
                assert name in _default_up, "the default configuration runs first"
                for c, p in enumerate(planes):
                    assert_bits_equal(p, _default_up[name][c], "%s plane %d: %s against the default decode" % (name, c, config))
        finally:
            dec.close()


# ---- the route tables ---------------------------------------------------------------------------------------------------------
def _stats_of(dec, key):
    return [s.get(key) for s in dec.stats]


@pytest.mark.parametrize("reason", list(C.ROUTE_CASES))
def test_a_real_decode_reaches_the_refusal(backend, reason, monkeypatch):
    table, name, switches, (where, k) = C.ROUTE_CASES[reason]
    heard = []
    real = JXLDecoder.patch_sets_rule
    monkeypatch.setattr(JXLDecoder, "patch_sets_rule", staticmethod(lambda *a: (heard.append(real(*a)), heard[-1])[1]))
    dec, got = decode(table, name, backend, switches)
    try:
        im = C.table(table)[name]
        print(reason, "|", _stats_of(dec, "image"), _stats_of(dec, "frame"), _stats_of(dec, "canvas"), heard)
        assert len(dec.stats) > k
        if where == "rule":
            assert reason in heard, heard
        elif where == "canvas":
            assert dec.stats[k]["canvas"] == "landed: " + reason
        elif "%s" in reason:
            head, tail = reason.split("%s")
            said = dec.stats[k][where]
            assert said.startswith("host: " + head) and said.endswith(tail) and len(said) > len("host: " + head + tail), said
        else:
            assert dec.stats[k][where] == "host: " + reason
        if table == "lossy":  # within the bound of its expectation from the SOURCE
            RUN.check(name, dict(planes=got.getBuffer()), "%s, refused for %r" % (name, reason), cuts=False)
        elif table != "upsampled":  # and the image is still its source's
            check_image(im, got, C.expected_planes(im), name)
    finally:
        dec.close()


@pytest.mark.parametrize("route", list(C.ACCEPTED))
def test_a_real_decode_takes_the_accepted_route(backend, route):
    table, name, switches, want = C.ACCEPTED[route]
    dec, got = decode(table, name, backend, switches)
    try:
        im = C.table(table)[name]
        print(route, "|", dec.stats)
        for key, per_frame in want.items():
            if key == "patches_path":
                said = [(s.get("patches") or {}).get("path") if isinstance(s.get("patches"), dict) else None for s in dec.stats]
            elif key == "chain_has_palette":
                said = [frontend.TRANSFORM_PALETTE in (s.get("chain") or {}).get("kinds", []) for s in dec.stats]
            else:
                said = _stats_of(dec, key)
            assert said == per_frame, (route, key, said)
        if table != "upsampled":
            check_image(im, got, C.expected_planes(im), name)
    finally:
        dec.close()


@pytest.mark.parametrize("config", ["default", "all"])
def test_a_wrong_sample_is_seen(backend, config):
    """the comparisons discriminate: one expected sample changed by one code value is told from the decode by every output"""
    im = C.SINGLE["depths"]["depth_8"]
    exp = C.expected_planes(im)
    dec, got = decode("depths", "depth_8", backend, C.CONFIGS[config])
    try:
        check_image(im, got, exp, "unchanged")
        bad = [p.copy() for p in exp]
        bad[2][16, 32] ^= 1
        _, good_png = C.png_samples(im, exp)
        assert (C.png_samples(im, bad)[1] != good_png).sum() == 1 and C.pfm_bytes(im, bad) != C.pfm_bytes(im, exp)
        assert all((a != b).sum() == 1 for a, b in zip(tensor_expectation(im, bad), tensor_expectation(im, exp)))
        with pytest.raises(AssertionError, match="PNG samples differ"):
            check_image(im, got, bad, "changed")
    finally:
        dec.close()
