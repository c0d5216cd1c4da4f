"""The tensor exit without a GPU: the numpy model of tests/tensor_ref.py on known vectors; the three C-ABI entries' declarations,
bindings and struct size; jxlatte_amd/csrc/tensor_check.h as a stand-alone host program under AddressSanitizer + UBSan
(tools/native/tensor_check.cpp; the sanitizer runtimes are linked statically, so the program needs nothing from its environment);
JXLImage.toTensor's argument refusals, raised before any backend call, and its single backend call on host arrays."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import tensor_ref as ref
from jxlatte_amd import _lib, abi
from jxlatte_amd.decoder import CE_GRAY, CE_RGB, PRI_SRGB, TF_SRGB, WP_D65, JXLImage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the model's rounding on known vectors ----
def test_model_bf16_rounding():
    x = ref.f32([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0x80000000, 0x00000001])
    assert ref.to_bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x7F80, 0xFF80, 0x7F80, 0x8000, 0x0000]
    nans = ref.f32([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0xFFC12345])
    assert ref.to_bf16_bits(nans).tolist() == [ref.BF16_NAN] * 4


def test_model_f16_rounding_subnormals_and_overflow():
    cases = [
        (1.0, 0x3C00), (-2.0, 0xC000), (65504.0, 0x7BFF), (65519.996, 0x7BFF), (65520.0, 0x7C00), (1e9, 0x7C00), (-1e9, 0xFC00),
        (2.0 ** -14, 0x0400),              # the least normal
        (2.0 ** -24, 0x0001),              # the least subnormal
        (2.0 ** -25, 0x0000),              # a tie between 0 and the least subnormal: to even
        (2.0 ** -25 * 1.0000001, 0x0001),  # just above it
        (2.0 ** -24 * 1.5, 0x0002),        # a tie between 1 and 2 units: to even
        (2.0 ** -24 * 2.5, 0x0002),        # a tie between 2 and 3 units: to even
        (2.0 ** -14 * (1023.5 / 1024), 0x0400),  # the largest subnormal's upper tie carries into the least normal
        (1.0 + 2.0 ** -11, 0x3C00),        # a tie at 1.0: to even
        (1.0 + 3 * 2.0 ** -11, 0x3C02),    # a tie above an odd significand: up
        (1e-40, 0x0000), (-0.0, 0x8000),
    ]
    x = np.array([c[0] for c in cases], F)
    assert ref.to_f16_bits(x).tolist() == [c[1] for c in cases]
    assert ref.to_f16_bits(ref.f32([0x7F800000, 0xFF800000])).tolist() == [0x7C00, 0xFC00]
    assert ref.to_f16_bits(ref.f32([0x7FC00000, 0x7F800001, 0xFFFFFFFF])).tolist() == [ref.F16_NAN] * 3
    # and against numpy's own cast wherever no NaN is involved: every f16 value, its two neighbouring ties and a spread of floats
    rng = np.random.default_rng(11)
    every = np.arange(0x10000, dtype=np.uint16).view(np.float16)
    every = every[np.isfinite(every)].astype(F)
    with np.errstate(over="ignore"):
        ties = ((every.astype(np.float64) + np.nextafter(every.astype(np.float16), np.float16(np.inf)).astype(np.float64)) / 2).astype(F)
    spread = np.concatenate([rng.normal(0, 1, 4096), rng.normal(0, 1e-6, 4096), rng.normal(0, 3e4, 4096)]).astype(F)
    for v in (every, ties[np.isfinite(ties)], spread):
        with np.errstate(over="ignore"):
            assert np.array_equal(ref.to_f16_bits(v), v.astype(np.float16).view(np.uint16))


def test_model_layout_normalise_unpremultiply():
    planes = [np.arange(6, dtype=F).reshape(2, 3) + 10 * c for c in range(3)]
    assert ref.layout(planes, "CHW").shape == (3, 2, 3) and ref.layout(planes, "HWC").shape == (2, 3, 3)
    assert ref.layout(planes, "HWC")[1, 2].tolist() == [5.0, 15.0, 25.0]
    n = ref.normalise(planes, [1, 2, 3], [F(0.5), F(2), F(1) / F(3)])
    assert n[0][0, 0] == F(-0.5) and n[1][1, 2] == F(26) and n[2][0, 1] == F(F(21) - F(3)) * (F(1) / F(3))
    alpha = np.array([[0.5, 0.0, 1.0]] * 2, F)
    u = ref.unpremultiply([planes[0]], alpha)[0]
    assert u[0, 0] == 0 and np.isnan(ref.unpremultiply([np.zeros((2, 3), F)], alpha)[0][0, 1]) and np.isinf(u[1, 1]) and u[1, 2] == 5


# ---- declarations, bindings, struct size ----
def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    for name in ("jxl_stage_tensor_samples", "jxl_planes_tensor_samples", "jxl_canvas_tensor_samples"):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert hasattr(lib, "jxl_debug_tensor_samples_grid") and "jxl_debug_tensor_samples_grid" not in header
    for name, value in (("U8", 0), ("F16", 1), ("BF16", 2), ("F32", 3), ("CHW", 0), ("HWC", 1)):
        assert re.search(r"#define\s+JXL_TENSOR_%s\s+%d\b" % (name, value), header) and getattr(abi, "TENSOR_" + name) == value


def test_struct_size_matches_the_c_layout():
    # jxl_color_params: 22 four-byte members; then 11 int32 and 2 x 4 floats
    assert C.sizeof(abi.ColorParams) == 88 and C.sizeof(abi.TensorParams) == 88 + 4 * 11 + 4 * 8
    assert abi.TensorParams.dtype.offset == 88 + 4 * 8 and abi.TensorParams.mean.offset == 88 + 4 * 11


def test_library_reads_no_tensor_switch():
    for f in ("k_tensor.hip", "tensor_host.hip", "tensor_check.h"):
        assert "getenv" not in open(os.path.join(ROOT, "jxlatte_amd", "csrc", f)).read()


# ---- tensor_check.h as a program of its own, under the sanitizers ----
def test_check_program_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tensor_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "tensor_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    assert "LAYOUT rgb_f32 3 3 4 252" in r.stdout and "LAYOUT ga_bf16 1 2 2 4" in r.stdout


# ---- toTensor over a fake backend ----
def _info(gray=False, bits=8, n_extra=0, ec_bits=(), icc=False):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=n_extra, ec_type=[0] * n_extra,
                                 ec_alpha_associated=[0] * n_extra, ec_bits=list(ec_bits), prim_xy=list(PRI_SRGB), white_xy=list(WP_D65),
                                 transfer=TF_SRGB, xyb_encoded=False, bits_per_sample=bits, use_icc=icc)


def _fake(calls):
    def tensor_samples(planes, alpha, out_ptr, **kw):
        calls.append((planes, alpha, out_ptr, kw))

    def color_peak(planes, **kw):
        calls.append(("peak", planes, kw))
        return F(1)
    return types.SimpleNamespace(tensor_samples=tensor_samples, tensor_device=lambda: "cpu", color_peak=color_peak)


def test_to_tensor_refuses_bad_arguments_before_any_backend_call():
    calls = []
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (4, 6)).astype(np.int32) for _ in range(3)]
    im = JXLImage(planes, _info(), _fake(calls))
    with_alpha = JXLImage(planes + [rng.uniform(0, 1, (4, 6)).astype(F)], _info(n_extra=1, ec_bits=[8]), _fake(calls))
    bad = [
        dict(dtype=torch.float64), dict(dtype=torch.int8), dict(dtype="float32"), dict(layout="NCHW"), dict(layout="hwc"),
        dict(target="rec709"), dict(alpha="keep"), dict(alpha="append"),  # (no alpha channel)
        dict(mean=[0, 0, 0]), dict(std=[1, 1, 1]), dict(mean=[0, 0], std=[1, 1]), dict(mean=[0, 0, 0], std=[1, 0, 1]),
        dict(mean=[0, 0, 0], std=[1, float("nan"), 1]), dict(dtype=torch.uint8, mean=[0, 0, 0], std=[1, 1, 1]),
        dict(out=np.zeros((3, 4, 6), F)), dict(out=torch.zeros((3, 4, 6), dtype=torch.float16)), dict(out=torch.zeros((3, 4, 7))),
        dict(out=torch.zeros((4, 6, 3))), dict(out=torch.zeros((3, 4, 12))[:, :, ::2]), dict(out=torch.zeros((4, 4, 6))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            im.toTensor(**kw)
    with pytest.raises(ValueError):
        with_alpha.toTensor(alpha="append", mean=[0, 0, 0], std=[1, 1, 1])  # four output channels
    with pytest.raises(ValueError):
        with_alpha.toTensor(alpha="append", out=torch.zeros((3, 4, 6)))
    assert calls == []
    with pytest.raises(TypeError):
        JXLImage(planes, _info(), types.SimpleNamespace()).toTensor()


def test_to_tensor_makes_one_backend_call_on_host_arrays():
    calls = []
    rng = np.random.default_rng(4)
    planes = [rng.integers(0, 256, (4, 6)).astype(np.int32) for _ in range(3)]
    alpha = rng.uniform(0, 1, (4, 6)).astype(F)
    im = JXLImage(planes + [alpha], _info(n_extra=1, ec_bits=[8]), _fake(calls))
    t = im.toTensor()  # sRGB planes to the sRGB target: the image as it is
    assert len(calls) == 1 and t.shape == (3, 4, 6) and t.dtype == torch.float32
    pl, a, ptr, kw = calls[0]
    assert all(x is y for x, y in zip(pl, planes)) and a is alpha and ptr == t.data_ptr()
    assert kw["dtype"] == "float32" and kw["layout"] == "CHW" and not kw["writeAlpha"] and not kw["premultiplied"]
    assert kw["inMax"] == [255] * 3 and kw["mean"] is None and kw["invStd"] is None and kw["alphaDepth"] == 8 and kw["colorDepth"] == 8
    assert im.tensor_bus_bytes == (3 * 4 * 6 * 4, 0)  # the alpha plane is not read: it does not go up
    # into a slice of a batch, with alpha, normalised, to the linear target: still one call, the caller's memory
    del calls[:]
    batch = torch.zeros((2, 4, 6, 4), dtype=torch.bfloat16)
    t = im.toTensor(torch.bfloat16, "HWC", target="linear", alpha="append", mean=[0.5] * 4, std=[0.25, 0.5, 1, 3], out=batch[1])
    assert len(calls) == 1 and t.data_ptr() == batch[1].data_ptr() == calls[0][2]
    kw = calls[0][3]
    assert kw["dtype"] == "bfloat16" and kw["layout"] == "HWC" and kw["writeAlpha"] and kw["tfIn"] == abi.TF_SRGB and kw.get("tfOut", abi.TF_LINEAR) == abi.TF_LINEAR
    assert kw["mean"] == [0.5] * 4 and [F(v) for v in kw["invStd"]] == [F(4), F(2), F(1), F(1) / F(3)]
    assert im.tensor_bus_bytes == (4 * 4 * 6 * 4, 0)
    # an image with an ICC profile is taken as it is whatever is asked
    del calls[:]
    icc = JXLImage(planes, _info(icc=True), _fake(calls))
    icc.toTensor(torch.uint8, target="pq")
    assert len(calls) == 1 and "tfOut" not in calls[0][3] and "matrix" not in calls[0][3]
    # a grey image to another gamut: three channels, through the matrix
    del calls[:]
    grey = JXLImage([planes[0]], _info(gray=True), _fake(calls))
    assert grey.toTensor().shape == (1, 4, 6)
    t = grey.toTensor(target="pq", peakDetect=0)
    assert t.shape == (3, 4, 6) and calls[-1][3].get("matrix") is not None
