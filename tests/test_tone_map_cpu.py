"""HDR -> SDR tone mapping without a GPU: the model's own properties (tests/tone_map_model.py), the mutations its two witnesses
must tell apart, csrc/tone_map_check.h and csrc/tone_map_ops.h as a stand-alone host program under AddressSanitizer + UBSan
(tools/native/tone_map_check.cpp), ToneMap's defaults, every ValueError of the toneMap= entries over fake backends (raised before
any backend call), the arming discipline (armed around the one call, cleared after it, after an exception too), the argument
parser, and the declarations, bindings and struct size."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import tone_map_model as tm
from jxlatte_amd import __main__ as cli
from jxlatte_amd import _lib, abi
from jxlatte_amd.decoder import (CE_GRAY, CE_RGB, PRI_BT2100, PRI_SRGB, TF_BT709, TF_LINEAR, TF_PQ, TF_SRGB, WP_D65, JXLImage, PNGWriter,
                                 ToneMap, _primaries_to_xyz, toTensorBatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
UNIT, SOURCE, TARGET = 10000.0, 1000.0, 203.0


def witness_bound(v, lum, unit, source, target, gamut):
    """the worst |float32 restatement - float64 model| over the finite results: what the formats cost, measured, never the device"""
    a, b = tm.restated(v, lum, unit, source, target, gamut), tm.model(v, lum, unit, source, target, gamut)
    worst = 0.0
    for x, y in zip(a, b):
        ok = np.isfinite(y)
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64)[ok] - y[ok]))))
    return worst


# ---- the model's properties ----
def test_a_grey_pixel_at_the_source_peak_comes_out_at_the_target_peak():
    for unit, source, target in ((10000.0, 1000.0, 203.0), (10000.0, 10000.0, 100.0), (4000.0, 4000.0, 203.0), (255.0, 255.0, 80.0)):
        g = np.array([source / unit], np.float64)
        for gamut in (False, True):
            out = tm.model([g, g, g], (0.25, 0.5, 0.25), unit, source, target, gamut)
            assert all(abs(o[0] - 1.0) < 1e-12 for o in out), (unit, source, target, out)


def test_a_grey_ramp_is_non_decreasing_and_linear_below_the_knee():
    ramp = np.linspace(0.0, 1.0, 20001)
    out = tm.model([ramp] * 3, tm.LUM_2020, UNIT, SOURCE, TARGET, False)[0]
    assert np.all(np.diff(out) >= -1e-15) and out[-1] == pytest.approx(1.0, abs=1e-12)
    knee = tm.knee_luminance(UNIT, SOURCE, TARGET) / sum(tm.LUM_2020)
    below = ramp < knee * (1 - 1e-9)
    assert below.sum() > 50 and np.array_equal(out[below], ramp[below] * (UNIT / TARGET))  # v * norm, exactly
    assert np.all(out[~below][1:] < (ramp[~below] * (UNIT / TARGET))[1:])  # and compressed above it
    # continuous at the knee and at the clamp: neighbours differ by what the slope allows
    assert np.max(np.abs(np.diff(out))) < 2 * (UNIT / TARGET) * (ramp[1] - ramp[0])


def test_a_source_no_brighter_than_the_target_is_the_identity_times_norm():
    v = tm.pixels(16, 16, 5)
    for source, target in ((203.0, 203.0), (100.0, 203.0)):
        out = tm.model(v, tm.LUM_2020, UNIT, source, target, False)
        rst = tm.restated(v, tm.LUM_2020, UNIT, source, target, False)
        for o, r, a in zip(out, rst, v):
            assert np.array_equal(o, a.astype(np.float64) * (UNIT / target), equal_nan=True)
            assert np.array_equal(r, a * F(UNIT / target), equal_nan=True)
    same = tm.restated(v, tm.LUM_2020, 203.0, 203.0, 203.0, False)  # norm == 1: bit for bit
    assert all(np.array_equal(s.view(np.uint32), a.view(np.uint32)) for s, a in zip(same, v))


def test_gamut_step_lands_in_range_and_keeps_the_luminance():
    v = tm.pixels(64, 64, 6)
    lum = np.array(tm.LUM_2020) / sum(tm.LUM_2020)  # weights that sum to 1 exactly enough for the closed form
    off, on = tm.model(v, lum, UNIT, SOURCE, TARGET, False), tm.model(v, lum, UNIT, SOURCE, TARGET, True)
    fin = np.isfinite(off[0]) & np.isfinite(off[1]) & np.isfinite(off[2])
    for o in on:
        assert np.all((o[fin] >= -1e-12) & (o[fin] <= 1 + 1e-12))
    y_off = sum(w * o for w, o in zip(lum, off))
    y_on = sum(w * o for w, o in zip(lum, on))
    inside = fin & (y_off >= 0) & (y_off <= 1)
    assert inside.sum() > 1000 and np.max(np.abs(y_on[inside] - y_off[inside])) < 1e-12
    untouched = fin & np.all([(o >= 0) & (o <= 1) for o in off], axis=0)
    assert untouched.sum() > 100 and all(np.array_equal(a[untouched], b[untouched]) for a, b in zip(on, off))
    assert (fin & ~untouched).sum() > 100  # (the inputs do reach the step)


def test_without_the_gamut_step_the_channel_ratios_are_kept():
    v = tm.pixels(32, 32, 7)
    out = tm.model(v, tm.LUM_2020, UNIT, SOURCE, TARGET, False)
    with np.errstate(all="ignore"):
        r = [o / a.astype(np.float64) for o, a in zip(out, v)]
    ok = np.all([np.isfinite(x) & (np.abs(a) > 1e-6) for x, a in zip(r, v)], axis=0)
    assert ok.sum() > 500 and np.allclose(r[0][ok], r[1][ok], rtol=1e-12) and np.allclose(r[0][ok], r[2][ok], rtol=1e-12)


def test_zero_negative_and_nan_luminance_take_the_identity_branch():
    v = [np.array([0.0, -0.01, np.nan, -0.5], F), np.array([0.0, 0.002, 0.2, 0.1], F), np.array([0.0, 0.001, 0.3, 0.1], F)]
    out = tm.restated(v, tm.LUM_2020, UNIT, SOURCE, TARGET, False)
    for o, a in zip(out, v):
        assert np.array_equal(o, a * F(UNIT / TARGET), equal_nan=True)
    assert np.isnan(out[0][2]) and not np.isnan(out[1][2])


def test_the_two_witnesses_agree_and_every_mutation_misses():
    """the float32 restatement stays within a few float ulps of the output range of the float64 model; each mutation of the model
    misses it by more than the device's bound (4 x that distance) on the very inputs of the device tests"""
    for shape, seed in (((8, 8), 1), ((67, 83), 2), ((264, 40), 3)):
        v = tm.pixels(shape[0], shape[1], seed)
        for gamut in (False, True):
            bound = witness_bound(v, tm.LUM_2020, UNIT, SOURCE, TARGET, gamut)
            assert 0 < bound < 64 * 2.0 ** -24 * (UNIT / TARGET), bound  # a PQ slope of about 20 on float roundings of values up to norm
            exact = tm.model(v, tm.LUM_2020, UNIT, SOURCE, TARGET, gamut)
            for m in tm.MUTATIONS:
                if (m == "gamut_to_zero" and not gamut) or (m == "no_clamp" and gamut):
                    continue  # (the gamut step needs to run to be wrong; and it folds every overshoot of an unclamped E1 back to 1)
                wrong = tm.model(v, tm.LUM_2020, UNIT, SOURCE, TARGET, gamut, mutate=m)
                miss = max(float(np.nanmax(np.abs(w - e))) for w, e in zip(wrong, exact))
                assert miss > 4 * bound, (shape, gamut, m, miss, bound)


# ---- the header as a program of its own, under the sanitizers ----
def test_check_program_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tone_map_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "tone_map_check.cpp"), "-o", exe])
    v = tm.pixels(8, 8, 1)
    px = [(float(v[0].flat[i]), float(v[1].flat[i]), float(v[2].flat[i])) for i in range(64) if np.isfinite(v[0].flat[i])]
    rows = [(UNIT, SOURCE, TARGET, g) + p for g in (0, 1) for p in px] + [(UNIT, 20000.0, TARGET, 1, 0.1, 0.1, 0.1)]
    r = subprocess.run([exe] + ["%.9g" % x for row in rows for x in row], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("PIXEL", "REFUSED"))]
    assert len(lines) == len(rows) and lines[-1].startswith("REFUSED tone map: source_nits")
    got = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[:-1]])
    # the host-compiled header against the model, at the device's bound
    for g in (0, 1):
        part = got[g * len(px):(g + 1) * len(px)]
        planes = [np.array([p[c] for p in px], F) for c in range(3)]
        exact = tm.model(planes, tm.LUM_2020, UNIT, SOURCE, TARGET, bool(g))
        bound = witness_bound(planes, tm.LUM_2020, UNIT, SOURCE, TARGET, bool(g))
        for c in range(3):
            assert np.max(np.abs(part[:, c] - exact[c])) <= 4 * bound


# ---- declarations, bindings, struct size ----
def test_entry_declared_bound_and_exported(tmp_path):
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    assert re.search(r"jxl_status\s+jxl_ctx_set_tone_map\s*\(\s*jxl_ctx\s*\*\s*ctx\s*,\s*const\s+jxl_tone_map\s*\*\s*tm\s*\)", header)
    for name in ("jxl_ctx_set_tone_map", "jxl_ctx_tone_map_armed"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(abi.ToneMapParams) == 28 and C.sizeof(abi.ColorParams) == 88
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "jxlatte_amd.h"\nint main(void) { printf("%zu %zu\\n", sizeof(jxl_tone_map), sizeof(jxl_color_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["28", "88"]
    jni = open(os.path.join(ROOT, "integration", "jni", "jxlatte_amd_jni.c")).read()
    assert "NativeBackend_setToneMap" in jni and "jxl_ctx_set_tone_map(c, &t)" in jni
    for f in ("tone_map_ops.h", "tone_map_check.h"):
        assert "getenv" not in open(os.path.join(ROOT, "jxlatte_amd", "csrc", f)).read()  # no environment switch


# ---- ToneMap and the toneMap= entries over fake backends ----
def _info(gray=False, transfer=TF_PQ, xyb=False, intensity=4000.0, icc=False, prim=PRI_BT2100, bits=16):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[],
                                 prim_xy=list(prim), white_xy=list(WP_D65), transfer=transfer, xyb_encoded=xyb, bits_per_sample=bits,
                                 use_icc=icc, intensity_target=intensity)


def _fake(calls, tone=True, fail=False):
    def record(name):
        def call(*a, **kw):
            calls.append((name, a, kw))
            if fail and name != "set_tone_map":
                raise RuntimeError("the backend call failed")
            if name == "color_convert":
                return [np.zeros(a[0][0].shape, F) for _ in range(3)]
            if name in ("png_samples", "pack"):
                return np.zeros(a[0][0].shape + (3,), np.uint8)
            if name == "color_peak":
                return F(1)
        return call
    names = ["color_convert", "color_peak", "png_samples", "pack", "tensor_samples", "tensor_resized", "tensor_resized_batch"] + (["set_tone_map"] if tone else [])
    return types.SimpleNamespace(tensor_device=lambda: "cpu", **{n: record(n) for n in names})


def _image(be, shape=(4, 6), **info):
    planes = [np.full(shape, 0.25, F) for _ in range(1 if info.get("gray") else 3)]
    return JXLImage(planes, _info(**info), be)


def test_tone_map_defaults_resolve_per_image():
    t = ToneMap()
    assert (t.targetNits, t.sourceNits, t.unitNits, t.gamut) == (203.0, None, None, True)
    assert t.resolve(_image(None, transfer=TF_PQ, intensity=4000.0)) == (10000.0, 4000.0, 203.0, True)  # tagged PQ: a sample is 10000 nits
    assert t.resolve(_image(None, transfer=TF_PQ, xyb=True, intensity=4000.0)) == (4000.0, 4000.0, 203.0, True)  # XYB: the intensity target
    assert t.resolve(_image(None, transfer=TF_SRGB, intensity=255.0)) == (255.0, 255.0, 203.0, True)
    assert ToneMap(100, sourceNits=1000, unitNits=500, gamut=False).resolve(_image(None)) == (500.0, 1000.0, 100.0, False)
    for bad in (dict(targetNits=0), dict(targetNits=-1), dict(targetNits=float("nan")), dict(targetNits=float("inf")), dict(targetNits=None),
                dict(targetNits="203"), dict(sourceNits=0), dict(sourceNits=10001), dict(unitNits=float("inf")), dict(unitNits=-5)):
        with pytest.raises(ValueError):
            ToneMap(**bad)


def test_every_value_error_is_raised_before_any_backend_call():
    calls = []
    be, old = _fake(calls), _fake(calls, tone=False)
    im, im_old, icc = _image(be), _image(old), _image(be, icc=True, xyb=False)
    t = ToneMap()
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        im.transform(PRI_SRGB, WP_D65, TF_SRGB, toneMap=t)  # device=False
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        im_old.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True, toneMap=t)  # a backend without set_tone_map
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        PNGWriter(im, toneMap=t)  # no device switch
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        PNGWriter(im_old, deviceSamples=True, toneMap=t)
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        im_old.toTensor(toneMap=t)
    with pytest.raises(ValueError, match="toneMap needs the device path"):
        toTensorBatch([im_old], (2, 2), toneMap=t)
    with pytest.raises(ValueError):
        im.transform(PRI_BT2100, WP_D65, TF_PQ, device=True, toneMap=t)
    with pytest.raises(ValueError):
        PNGWriter(im, hdr=True, deviceColor=True, toneMap=t)
    for target in ("pq", "as-is"):
        with pytest.raises(ValueError):
            im.toTensor(target=target, toneMap=t)
        with pytest.raises(ValueError):
            toTensorBatch([im], (2, 2), target=target, toneMap=t)
    with pytest.raises(ValueError):
        icc.toTensor(toneMap=t)
    with pytest.raises(ValueError):
        PNGWriter(icc, deviceColor=True, toneMap=t)
    with pytest.raises(ValueError):
        im.toTensor(toneMap=203.0)  # not a ToneMap
    other = _image(be, intensity=1000.0)
    with pytest.raises(ValueError, match=r"image 0 .* image 1 "):
        toTensorBatch([im, other], (2, 2), toneMap=t)  # the defaults resolve differently inside one batch
    assert calls == []


def test_arming_surrounds_the_one_call_and_is_always_cleared():
    lum = [float(x) for x in _primaries_to_xyz(PRI_SRGB, WP_D65)[1]]
    assert lum == pytest.approx(tm.LUM_709, abs=2e-4)
    for fail in (False, True):
        for use in ("transform", "png", "png_color", "tensor", "resized", "batch"):
            calls = []
            im = _image(_fake(calls, fail=fail))
            t = ToneMap(300.0, gamut=False)

            def go():
                if use == "transform":
                    im.transform(PRI_SRGB, WP_D65, TF_BT709, device=True, toneMap=t)
                elif use == "png":
                    PNGWriter(im, deviceSamples=True, toneMap=t)
                elif use == "png_color":
                    PNGWriter(im, deviceColor=True, toneMap=t)
                elif use == "tensor":
                    im.toTensor(toneMap=t)
                elif use == "resized":
                    im.toTensor(size=(2, 3), toneMap=t)
                else:
                    toTensorBatch([im, _image(im.backend)], (2, 3), toneMap=t)
            if fail:
                with pytest.raises(RuntimeError):
                    go()
            else:
                go()
            names = [c[0] for c in calls]
            work = {"transform": "color_convert", "png": "png_samples", "png_color": "color_convert", "tensor": "tensor_samples",
                    "resized": "tensor_resized", "batch": "tensor_resized_batch"}[use]
            assert names[:3] == ["set_tone_map", work, "set_tone_map"], (use, fail, names)  # no peak call: peak detection is not consulted
            assert "color_peak" not in names and names.count("set_tone_map") == 2
            armed, cleared = calls[0], calls[2]
            assert armed[1][0] == lum and armed[1][1:] == (10000.0, 4000.0, 300.0, False) and cleared[1] == (None,)
            kw = calls[1][2] if use != "batch" else calls[1][1][0][0]
            assert kw.get("scale") is None and kw["matrix"] is not None and kw["tfIn"] == abi.TF_PQ


def test_a_grey_image_gives_three_channels():
    calls = []
    im = _image(_fake(calls), gray=True, transfer=TF_SRGB, prim=PRI_SRGB, intensity=255.0, bits=8)
    out = im.toTensor(toneMap=ToneMap(100.0))
    assert tuple(out.shape) == (3, 4, 6)
    assert tuple(im.toTensor().shape) == (1, 4, 6)  # and one without, as before
    res = im.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True, toneMap=ToneMap(100.0))
    assert res.getColorChannelCount() == 3 and len(res.buffer) == 3
    assert im.transform(PRI_SRGB, WP_D65, TF_SRGB, device=True) is im  # nothing to do without: the image itself, as before


# ---- the argument parser ----
def test_argument_parser():
    p = cli.parser()
    a = p.parse_args(["in.jxl", "out.png", "--tone-map=203"])
    assert a.tone_map == (203.0, None) and not a.no_gamut_map and not a.device_color
    t = cli.tone_map_of(a)
    assert (t.targetNits, t.sourceNits, t.gamut) == (203.0, None, True) and a.device_color  # turned on: no device colour switch was given
    a = p.parse_args(["in.jxl", "out.png", "--tone-map=100,4000", "--no-gamut-map", "--device-png"])
    t = cli.tone_map_of(a)
    assert (t.targetNits, t.sourceNits, t.gamut) == (100.0, 4000.0, False) and a.device_png and not a.device_color
    a = p.parse_args(["in.jxl", "out.png"])
    assert a.tone_map is None and cli.tone_map_of(a) is None and not a.device_color
    for bad in ("--tone-map=", "--tone-map=abc", "--tone-map=0", "--tone-map=-5", "--tone-map=1,2,3", "--tone-map=100,20000", "--tone-map=inf", "--tone-map=nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["in.jxl", "out.png", bad])
