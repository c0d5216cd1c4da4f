"""PFM output without a GPU: the numpy model of tests/pfm_ref.py against hand-written byte strings, PFMWriter's default path
against the model, the CLI's choice of format, and the two C-ABI entries' declarations and bindings."""
import ctypes as C
import io
import os
import re
import struct
import types

import numpy as np
import pytest

import pfm_ref
from jxlatte_amd import _lib, abi
from jxlatte_amd.decoder import CE_GRAY, CE_RGB, PRI_SRGB, TF_SRGB, WP_D65, JXLImage, PFMWriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _info(gray=False, bits=8, n_extra=0, ec_bits=()):
    return types.SimpleNamespace(colour_space=CE_GRAY if gray else CE_RGB, num_extra=n_extra, ec_type=[0] * n_extra,
                                 ec_alpha_associated=[0] * n_extra, ec_bits=list(ec_bits), prim_xy=list(PRI_SRGB), white_xy=list(WP_D65),
                                 transfer=TF_SRGB, xyb_encoded=False, bits_per_sample=bits, use_icc=False)


# ---- the model against bytes written by hand ----
def test_model_grey_2x1_header_endianness_nan_and_negative_zero():
    # width 2, height 1: a signalling NaN with a payload and the sign set, then -0.0
    plane = np.array([[0xff800001, 0x80000000]], np.uint32).view(np.float32)
    assert pfm_ref.pfm([plane]) == b"Pf\n2 1\n1.0\n" + bytes([0x7f, 0xc0, 0x00, 0x00]) + bytes([0x80, 0x00, 0x00, 0x00])


def test_model_rgb_1x2_row_order_channel_order_and_int_cast():
    # width 1, height 2. Row 0 (top): R = 1.0f, G = int 255 at depth 8, B = 2.0f; row 1 (bottom): R = -2.0f, G = int 0, B = a quiet NaN
    # with a payload. The bottom row is written first.
    r = np.array([[1.0], [-2.0]], np.float32)
    g = np.array([[255], [0]], np.int32)
    b = np.array([[0x40000000], [0x7fc12345]], np.uint32).view(np.float32)
    exp = b"PF\n1 2\n1.0\n" + \
        bytes([0xc0, 0, 0, 0]) + bytes([0, 0, 0, 0]) + bytes([0x7f, 0xc0, 0, 0]) + \
        bytes([0x3f, 0x80, 0, 0]) + bytes([0x3f, 0x80, 0, 0]) + bytes([0x40, 0, 0, 0])
    assert pfm_ref.pfm([r, g, b], [8, 8, 8]) == exp


def test_model_java_int_arithmetic_of_the_depth():
    assert [pfm_ref.java_depth_max(d) for d in (0, 1, 8, 12, 16, 24, 31, 32, 33)] == [0, 1, 255, 4095, 65535, (1 << 24) - 1, (1 << 31) - 1, 0, 1]
    for bad in (0, 32):
        with pytest.raises(ValueError):
            pfm_ref.cast(np.zeros((1, 1), np.int32), bad)
    # the conversion rounds first: 2^24 + 1 is no float, and at depth 31 the maximum itself rounds to 2^31, so max gives exactly 1.0
    v = np.array([[(1 << 24) + 1, (1 << 31) - 1]], np.int32)
    assert pfm_ref.cast(v, 31).view(np.uint32).tolist() == [[0x3c000000, 0x3f800000]]  # 2^24 * 2^-31 and 2^31 * 2^-31
    assert struct.pack(">f", 1.0) == bytes([0x3f, 0x80, 0, 0])


# ---- PFMWriter's default path against the model ----
def _random_planes(rng, shape, kinds, depths):
    out = []
    for kind, d in zip(kinds, depths):
        if kind == "f":
            p = rng.normal(0, 4, shape).astype(F)
            p.reshape(-1)[::7] = _f(0x7fa00001)  # signalling NaNs among them
            p.reshape(-1)[3::11] = F(-0.0)
        else:
            p = rng.integers(-5, (1 << d) + 5, shape, dtype=np.int64).astype(np.int32)
        out.append(p)
    return out


@pytest.mark.parametrize("gray,kinds,bits", [(False, "fff", 8), (False, "iii", 8), (False, "ifi", 12), (True, "f", 8), (True, "i", 16),
                                             (False, "iii", 31)])
def test_writer_default_path_equals_the_model(gray, kinds, bits):
    rng = np.random.default_rng(5)
    for shape in [(1, 1), (3, 5), (17, 9)]:
        planes = _random_planes(rng, shape, kinds, [bits] * len(kinds))
        extra = [rng.uniform(0, 1, shape).astype(F)]  # an alpha channel: never written
        im = JXLImage(planes + extra, _info(gray, bits, 1, [8]), None)
        out = io.BytesIO()
        w = PFMWriter(im)
        w.write(out)
        assert w.bus_bytes is None
        assert out.getvalue() == pfm_ref.pfm(planes, [bits] * len(kinds)), (shape, kinds)


def test_writer_refuses_a_depth_without_a_maximum():
    im = JXLImage([np.zeros((2, 2), np.int32)] * 3, _info(bits=32), None)
    with pytest.raises(ValueError):
        PFMWriter(im)


def test_device_samples_makes_one_call_on_host_arrays_and_needs_the_backend_entry():
    rng = np.random.default_rng(6)
    planes = _random_planes(rng, (4, 6), "ifi", [12] * 3)
    calls = []

    def pfm_samples(pl, tagged):
        calls.append((pl, tagged))
        return np.frombuffer(pfm_ref.payload(pl, tagged), np.uint8).reshape(4, 6, 3, 4)
    w = PFMWriter(JXLImage(planes, _info(bits=12), types.SimpleNamespace(pfm_samples=pfm_samples)), deviceSamples=True)
    assert len(calls) == 1 and calls[0][1] == [12, 12, 12] and all(a is b for a, b in zip(calls[0][0], planes))
    assert w.bus_bytes == (3 * 4 * 6 * 4, 3 * 4 * 6 * 4)
    out = io.BytesIO()
    w.write(out)
    assert out.getvalue() == pfm_ref.pfm(planes, [12] * 3)
    with pytest.raises(TypeError):
        PFMWriter(JXLImage(planes, _info(bits=12), types.SimpleNamespace()), deviceSamples=True)


# ---- the CLI's choice of format ----
def test_cli_format_option_and_extension():
    from jxlatte_amd.__main__ import output_format, parser
    ap = parser()

    def fmt(*argv):
        return output_format(ap.parse_args(list(argv)))
    assert fmt("a.jxl", "out.pfm") == "pfm"
    assert fmt("a.jxl", "OUT.PfM") == "pfm"
    assert fmt("a.jxl", "out.png") == "png"
    assert fmt("a.jxl", "out.pfm", "--format=png") == "png"
    assert fmt("a.jxl", "out.png", "--format", "pfm") == "pfm"
    assert fmt("a.jxl", "out.bin", "--format=pfm", "--device-png") == "pfm"
    # an unknown extension, a name that merely contains ".pfm", and no extension at all still give a PNG
    assert fmt("a.jxl", "out.xyz") == "png" and fmt("a.jxl", "out.pfm.bak") == "png" and fmt("a.jxl", "out") == "png"
    assert fmt("a.jxl") == "png"
    with pytest.raises(SystemExit):
        ap.parse_args(["a.jxl", "o", "--format=ppm"])
    a = ap.parse_args(["a.jxl", "o.pfm", "--device-png"])
    assert a.device_png and a.format is None


# ---- declarations and bindings ----
def test_header_declares_both_entries_and_python_binds_them():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    for name in ("jxl_stage_pfm_samples", "jxl_planes_pfm_samples"):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "typedef struct jxl_pfm_params" in header and "PFMWriter.java" in header
    vp = C.c_void_p
    res, args = _lib.SIGNATURES["jxl_stage_pfm_samples"]
    assert res is C.c_int32 and args[0] is vp and args[2] is C.POINTER(abi.PfmParams) and args[3] is vp and len(args) == 4
    res, args = _lib.SIGNATURES["jxl_planes_pfm_samples"]
    assert res is C.c_int32 and args == [vp, C.POINTER(abi.PfmParams), vp]
    # struct jxl_pfm_params: height, width, n_planes, is_int[3], tagged_depth[3], all int32, in the header's order
    body = re.search(r"typedef struct jxl_pfm_params \{(.*?)\} jxl_pfm_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in re.findall(r"[a-z_]+", decl)]
    assert names == [f[0] for f in abi.PfmParams._fields_] == ["height", "width", "n_planes", "is_int", "tagged_depth"]
    assert C.sizeof(abi.PfmParams) == 4 * 9


def test_no_context_is_refused_without_a_crash():
    lib = _lib.load()
    p = abi.PfmParams()
    out = (C.c_uint8 * 16)()
    assert lib.jxl_planes_pfm_samples(None, C.byref(p), out) != 0
    assert lib.jxl_stage_pfm_samples(None, None, C.byref(p), out) != 0
