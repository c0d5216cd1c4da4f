"""Draw varblocks without a GPU: the numpy model of tests/varblocks_ref.py against values worked out by hand; the factor table,
the validator and the cell-map builder of jxlatte_amd/csrc/varblock_check.h as a stand-alone host program under AddressSanitizer
+ UBSan (tools/native/varblock_check.cpp; the sanitizer runtimes are linked statically, so the program needs nothing from its
environment); the CLI's flag; the two C-ABI entries' declarations and bindings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import varblocks_cases
import varblocks_ref as ref
from jxlatte_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the model against values worked out by hand ----
def test_model_factors_of_type_0():
    # hue = 0: rFactor = (cos 0 + 0.5) / 1.5 = 1; g and b: (cos(-+2 pi / 3) + 1) / 2 = 0.25 in exact arithmetic. The float
    # nearest 2 pi / 3 is off by about 6e-8, and the slope of cos there is 0.87: the float result may miss 0.25 by an ulp or two
    r, g, b = ref.factors(0)
    assert r == F(1.0)
    assert abs(np.float64(g) - 0.25) <= 2 * np.spacing(F(0.25)) and abs(np.float64(b) - 0.25) <= 8 * np.spacing(F(0.25))
    # PHI_BAR is the float of the golden ratio's fractional part; type 1 turns the hue by it
    assert ref.PHI_BAR == F(0.6180339887498949)
    r1 = ref.factors(1)[0]
    assert abs(np.float64(r1) - (np.cos(2 * np.pi * 0.6180339887498949) + 0.5) / 1.5) < 1e-6


def test_model_one_dct8_block_by_hand():
    planes = [np.ones((8, 8), F) for _ in range(3)]
    out = ref.draw(planes, [(0, 0, 0)])
    fac = ref.factors(0)
    for c in range(3):
        assert not out[c][0, :].any() and not out[c][:, 0].any()  # the top row and the left column are black
        # R = G = B = 1: light = 0.25 * 2 + 0.5 = 1, cbrt 1, * 0.5 + 0.25 = 0.75; out = factor * 0.5 + 0.5 / 0.75
        want = F(F(fac[c] * F(0.5)) + F(F(0.5) / F(0.75)))
        assert (out[c][1:, 1:] == want).all()
    assert out[0][1, 1] == F(F(0.5) + F(F(0.5) / F(0.75)))  # rFactor = 1
    assert all(p.min() == 1 and p.max() == 1 for p in planes)  # the input is not written


def test_model_leaves_pixels_outside_every_block_and_clips_at_the_plane():
    rng = np.random.default_rng(3)
    planes = [rng.uniform(0, 1, (13, 30)).astype(F) for _ in range(3)]
    out = ref.draw(planes, [(0, 1, 4), (1, 5, 0)])  # a 16x16 at pixel (0, 8), cut at row 13; an 8x8 at column 40, right of the plane
    for c in range(3):
        assert np.array_equal(out[c][:, :8], planes[c][:, :8]) and np.array_equal(out[c][:, 24:], planes[c][:, 24:])
        assert not out[c][0, 8:24].any() and not out[c][:, 8].any()
        assert out[c][8, 9:24].all()  # row 8 is inside the 16x16 block: no border there
    out2 = ref.draw(planes, [(2, 0, 0)])  # starts at row 16: wholly below the plane
    assert all(np.array_equal(a, b) for a, b in zip(out2, planes))


def test_model_division_by_a_zero_light():
    planes = [np.full((8, 8), -0.125, F) for _ in range(3)]
    with np.errstate(all="ignore"):
        out = ref.draw(planes, [(0, 0, 0)])
    assert all(np.isneginf(out[c][1:, 1:]).all() for c in range(3))  # 0.5 * -0.125 / 0


# ---- varblock_check.h as a program of its own, under the sanitizers ----
@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("varblock_check")
    exe = str(tmp / "varblock_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "varblock_check.cpp"), "-o", exe])
    names = sorted(varblocks_cases.CASES)
    # the tilings of the GPU test, then a block that hangs over the plane edge (the grid is the frame's, not the plane's) and a
    # 256x256 block beside a 128x256
    extra = [((3, 2), [(1, 0, 4)]), ((32, 64), [(0, 0, 24), (0, 32, 26), (16, 32, 26)])]
    cases = [(varblocks_cases.CASES[n][2], varblocks_cases.CASES[n][3]) for n in names] + extra
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for (ch, cw), blocks in cases:
            f.write("%d %d %d\n" % (ch, cw, len(blocks)))
            for b in blocks:
                f.write("%d %d %d\n" % tuple(b))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return r, cases


def test_validator_and_cell_maps_under_asan(check_run):
    r, cases = check_run
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failure(s)" in r.stdout and "FAIL" not in r.stdout and "%d case(s)" % len(cases) in r.stdout
    maps = dict(re.findall(r"^MAP (\d+) ([0-9a-f]+)$", r.stdout, re.M))
    assert len(maps) == len(cases)
    for i, ((ch, cw), blocks) in enumerate(cases):
        want = np.full((ch, cw), 0xff, np.uint8)
        for cy, cx, t in blocks:
            bh, bw = ref.TYPE_SIZES[t][0] // 8, ref.TYPE_SIZES[t][1] // 8
            want[cy:cy + bh, cx:cx + bw] = t
            want[cy, cx:cx + bw] |= 0x20
            want[cy:cy + bh, cx] |= 0x40
        assert bytes.fromhex(maps[str(i)]) == want.tobytes(), i
    # the mixed tiling meets every kind of cell: both bits, one of them, neither; the all-types tiling leaves cells unowned
    mix = np.frombuffer(bytes.fromhex(maps[str(sorted(varblocks_cases.CASES).index("b_24x40_mix"))]), np.uint8)
    assert {0x60, 0x20, 0x40, 0x00} <= {int(m) & 0x60 for m in mix}
    alltypes = np.frombuffer(bytes.fromhex(maps[str(sorted(varblocks_cases.CASES).index("d_512x512_all_types"))]), np.uint8)
    assert (alltypes == 0xff).any() and {int(m) & 0x1f for m in alltypes if m != 0xff} == set(range(27))


def test_factor_table_equals_the_model_bit_for_bit(check_run):
    r, _ = check_run
    rows = re.findall(r"^FACTOR (\d+) ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8})$", r.stdout, re.M)
    assert [int(t[0]) for t in rows] == list(range(27))
    for t, *bits in rows:
        want = [int(np.array([v], F).view(np.uint32)[0]) for v in ref.factors(int(t))]
        assert [int(b, 16) for b in bits] == want, t


# ---- the CLI's flag ----
def test_cli_knows_draw_varblocks():
    from jxlatte_amd.__main__ import parser
    ap = parser()
    assert ap.parse_args(["a.jxl", "o.png"]).draw_varblocks is False
    a = ap.parse_args(["a.jxl", "o.png", "--draw-varblocks", "--device-png"])
    assert a.draw_varblocks is True and a.device_png


def test_decoder_keyword_defaults_to_off():
    import inspect
    from jxlatte_amd.decoder import JXLDecoder
    assert inspect.signature(JXLDecoder.__init__).parameters["draw_varblocks"].default is False


# ---- declarations and bindings ----
def test_header_python_shim_and_java_declare_both_entries():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    shim = open(os.path.join(ROOT, "integration", "jni", "jxlatte_amd_jni.c")).read()
    java = open(os.path.join(ROOT, "integration", "jni", "NativeBackend.java")).read()
    for name, native in (("jxl_stage_varblocks", "stageVarblocks"), ("jxl_planes_varblocks", "planesVarblocks")):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
        assert re.search(r"\b%s\s*\(" % name, shim) and ("NativeBackend_%s(" % native) in shim
        assert re.search(r"native\s+void\s+%s\s*\(" % native, java) and name in java
    assert "typedef struct jxl_varblock_desc" in header and "Frame.java:464-503" in header and "JXLCodestreamDecoder.java:638-639" in header
    vp, i32 = C.c_void_p, C.c_int32
    res, args = _lib.SIGNATURES["jxl_stage_varblocks"]
    assert res is i32 and len(args) == 6 and args[0] is vp and args[2] is i32 and args[3] is i32 and args[4] is C.POINTER(abi.VarblockDesc)
    assert _lib.SIGNATURES["jxl_planes_varblocks"] == (i32, [vp, C.POINTER(abi.VarblockDesc)])
    # struct jxl_varblock_desc: int32 n_blocks, const int32* blocks, int32 cells_h, cells_w, in the header's order
    body = re.search(r"typedef struct jxl_varblock_desc \{(.*?)\} jxl_varblock_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"int32_t\*?\s+([^;]+);", body) for n in re.findall(r"[a-z_]+", decl)]
    assert names == [f[0] for f in abi.VarblockDesc._fields_] == ["n_blocks", "blocks", "cells_h", "cells_w"]
    assert C.sizeof(abi.VarblockDesc) == 24 and abi.VarblockDesc.blocks.offset == 8 and abi.VarblockDesc.cells_h.offset == 16


def test_no_context_is_refused_without_a_crash():
    lib = _lib.load()
    d, keep = abi.make_varblock_desc([(0, 0, 0)], (1, 1))
    assert lib.jxl_planes_varblocks(None, C.byref(d)) != 0
    assert lib.jxl_stage_varblocks(None, None, 8, 8, C.byref(d), None) != 0
