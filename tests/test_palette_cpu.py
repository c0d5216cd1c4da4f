"""The inverse Palette transform without a GPU: the Python model of tests/palette_ref.py against values worked out by hand and
against the front-end's own loop on a real file; the per-sample arithmetic of jxlatte_amd/csrc/palette_ops.h and the validator of
palette_check.h as a stand-alone host program under AddressSanitizer + UBSan (tools/native/palette_check.cpp; the sanitizer
runtimes are linked statically, so the program needs nothing from its environment), bit for bit against the model on every case
of tests/palette_cases.py; the declarations, the bindings and the CLI's flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import palette_cases
import palette_ref as ref
from jxlatte_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ---- the model against values worked out by hand ----
def _one(index, c, bit_depth, nb_colors=4):
    palette = [[10, 11, 12, 13], [20, 21, 22, 23], [30, 31, 32, 33], [40, 41, 42, 43]]
    return ref.value(index, c, palette, nb_colors, bit_depth)


def test_model_one_pixel_per_index_class_at_8_bits():
    assert [_one(2, c, 8) for c in range(4)] == [12, 22, 32, 42]                    # inside the palette
    # the cube: index - 4 = 27 = 0b011011 -> digits 3, 2, 1 (two bits per channel), c = 3: 27 >> 6 = 0; * 255 / 4 + (1 << 5)
    assert [_one(4 + 27, c, 8) for c in range(4)] == [3 * 255 // 4 + 32, 2 * 255 // 4 + 32, 1 * 255 // 4 + 32, 32]
    assert [_one(4 + 27, c, 8) for c in range(4)] == [223, 159, 95, 32]
    # the ladder: index - 4 - 64 = 117 = 4 * 25 + 3 * 5 + 2 -> digits 2, 3, 4, 0 in base 5; * 255 / 4
    assert [_one(4 + 64 + 117, c, 8) for c in range(4)] == [2 * 255 // 4, 3 * 255 // 4, 255, 0] == [127, 191, 255, 0]
    # negative: -1 -> 0 -> row 0, sign flipped: (0, 0, 0); -2 -> 1 -> row 1 as it is: (4, 4, 4); -3 -> 2 -> row 1 negated
    assert [_one(-1, c, 8) for c in range(4)] == [0, 0, 0, 0]
    assert [_one(-2, c, 8) for c in range(4)] == [4, 4, 4, 0]
    assert [_one(-3, c, 8) for c in range(4)] == [-4, -4, -4, 0]
    assert [_one(-4, c, 8) for c in range(4)] == [11, 0, 0, 0]                      # 3 -> row 2
    # -143 -> 142 -> row 71 negated, -144 -> 143 % 143 = 0 -> row 0 again, -145 -> 1
    assert [_one(-143, c, 8) for c in range(3)] == [24, -45, 45]
    assert [_one(-144, c, 8) for c in range(3)] == [0, 0, 0]
    assert [_one(-145, c, 8) for c in range(3)] == [4, 4, 4]
    # INT32_MIN: -index wraps to INT32_MIN, - 1 wraps to INT32_MAX = 143 * 15017368 + 23 -> 23 -> row 12 as it is
    assert I32_MAX % 143 == 23
    assert [_one(I32_MIN, c, 8) for c in range(4)] == [0, -32, -32, 0]


def test_model_one_pixel_per_index_class_at_12_bits():
    assert [_one(3, c, 12) for c in range(4)] == [13, 23, 33, 43]
    # the cube: * 4095 / 4 + (1 << 9)
    assert [_one(4 + 27, c, 12) for c in range(4)] == [3 * 4095 // 4 + 512, 2 * 4095 // 4 + 512, 4095 // 4 + 512, 512] == [3583, 2559, 1535, 512]
    assert [_one(4 + 64 + 117, c, 12) for c in range(4)] == [2047, 3071, 4095, 0]
    # the delta palette is shifted left by min(12, 24) - 8 = 4
    assert [_one(-2, c, 12) for c in range(4)] == [64, 64, 64, 0]
    assert [_one(-3, c, 12) for c in range(4)] == [-64, -64, -64, 0]
    assert [_one(-143, c, 12) for c in range(3)] == [24 * 16, -45 * 16, 45 * 16]
    assert [_one(I32_MIN, c, 12) for c in range(4)] == [0, -512, -512, 0]


def test_model_wraps_like_a_java_int():
    # bit_depth 32: 1 << 32 is 1 << 0, so (1 << 32) - 1 = 0 and the shift 1 << 29; bit_depth 31: (1 << 31) - 1 = INT32_MAX and
    # 3 * INT32_MAX wraps to INT32_MAX - 2 (= 2^31 - 3), / 4 = 536870911, + (1 << 28)
    assert _one(4 + 3, 0, 32) == 1 << 29
    assert _one(4 + 3, 0, 31) == ((I32_MAX - 2) // 4) + (1 << 28) == 536870911 + 268435456
    # the delta palette stops shifting at 24 bits
    assert _one(-2, 0, 31) == 4 << 16 and _one(-2, 0, 24) == 4 << 16 and _one(-2, 0, 16) == 4 << 8
    # shift counts count mod 32: channel 16 shifts by 32 = 0, so it sees the low digit again
    assert ref.value(4 + 27, 16, [[0] * 4] * 17, 4, 8) == _one(4 + 27, 0, 8)
    assert ref.tdiv(-7, 2) == -3 and ref.trem(-7, 2) == -1 and ref.jabs(I32_MIN) == I32_MIN and ref.i32(I32_MAX + 1) == I32_MIN


@pytest.mark.parametrize("d_pred,want", [
    # indices: (0, 0) = 1 -> 100; (0, 1) = -2: delta, 4 + pred; (1, 0) = -2; (1, 1) = -2. nb_deltas 0, palette (7, 100), 8 bits
    (1, [[100, 104], [104, 108]]),   # west (north in column 0): 4 + 100, 4 + 100, 4 + 104
    # 5: gradient. (0, 1): w = n = nw = 100 -> 100 -> 104. (1, 0): w = n = nw = 100 (column 0 falls back to north) -> 104.
    # (1, 1): w = 104, n = 104, nw = 100: 108 clamped to [104, 104] -> 104 -> 108
    (5, [[100, 104], [104, 108]]),
    # 13: (6 n - 2 nn + 7 w + ww + nee + 3 ne + 8) / 16. (0, 1): all six are 100 -> (1600 + 8) / 16 = 100 -> 104.
    # (1, 0): n = nn = w = ww = 100, ne = nee = 104: (600 - 200 + 700 + 100 + 104 + 312 + 8) / 16 = 1624 / 16 = 101 -> 105.
    # (1, 1): n = nn = ne = nee = 104, w = ww = 105: (624 - 208 + 735 + 105 + 104 + 312 + 8) / 16 = 1680 / 16 = 105 -> 109
    (13, [[100, 104], [105, 109]]),
])
def test_model_2x2_chain_by_hand(d_pred, want):
    out = ref.inverse_palette([[1, -2], [-2, -2]], [[7, 100]], 1, 2, 0, d_pred, 8)
    assert out.tolist() == [want]


def test_delta_palette_table_equals_the_frontends_copy_and_the_reference_source():
    """the 72 x 3 table of include/jxl_tables.h, which the model and palette_ops.h read, against the copy the front-end has always
    had (jxlatte_amd/frontend/modular.cc) and, where a checkout of the reference is present, against its source text"""
    def triples(text, start):
        body = text[text.index(start):]
        return [tuple(int(v) for v in r) for r in re.findall(r"\{(-?\d+), (-?\d+), (-?\d+)\}", body[:body.index("};")])]
    assert len(ref.K_DELTA_PALETTE) == 72 and ref.K_DELTA_PALETTE[1] == (4, 4, 4) and ref.K_DELTA_PALETTE[71] == (-24, 45, -45)
    front = open(os.path.join(ROOT, "jxlatte_amd", "frontend", "modular.cc")).read()
    assert triples(front, "kDeltaPalette[72][3]") == ref.K_DELTA_PALETTE
    java = "/root/reference/java/com/traneptora/jxlatte/frame/modular/ModularStream.java"
    if os.path.exists(java):
        assert triples(open(java).read(), "kDeltaPalette =") == ref.K_DELTA_PALETTE


# ---- the model against the front-end's own loop on a real file ----
def test_model_as_the_frontend_hook_equals_the_frontends_loop():
    """patches-lossless.jxl undoes four frame-level palettes in each of its two frames and needs neither Squeeze nor RCT: a decode
    whose palette hook is the model gives the channels of a decode without hooks"""
    from jxlatte_amd import frontend
    data = open(os.path.join(SAMPLES, "patches-lossless.jxl"), "rb").read()
    calls = []

    def hook(index, palette, pred, num_c, nb_colors, nb_deltas, d_pred, bit_depth):
        calls.append((index.shape, num_c, nb_colors, nb_deltas, d_pred))
        return ref.inverse_palette(index, palette, num_c, nb_colors, nb_deltas, d_pred, bit_depth, pred)
    plain, hooked = frontend.Frontend(data), frontend.Frontend(data)
    try:
        frames = 0
        while True:
            a = plain.next_frame(None, None)
            before = len(calls)
            b = hooked.next_frame(None, None, hook)
            if a is None:
                assert b is None
                break
            frames += 1
            assert len(calls) - before == 4 and calls[before][1] == 4 and [c[1] for c in calls[before + 1:]] == [1, 1, 1]
            assert a.num_modular_channels == b.num_modular_channels > 0
            for i in range(a.num_modular_channels):
                ca, cb = plain.modular_channel(i), hooked.modular_channel(i)
                assert ca[1] == cb[1] and np.array_equal(ca[0], cb[0]), (frames, i)
        assert frames == 2
        assert sorted({c[0] for c in calls}) == [(198, 198), (1096, 1600)]
    finally:
        plain.close()
        hooked.close()


# ---- palette_ops.h and palette_check.h as a program of their own, under the sanitizers ----
REFUSALS = {"null_desc", "null_index", "null_out", "null_out_plane", "null_palette", "height_0", "width_0", "height_negative",
            "width_negative", "too_many_samples", "too_many_samples_max", "num_c_0", "num_c_negative", "nb_colors_negative",
            "nb_deltas_negative", "pal_w_below_nb_colors", "pal_h_below_num_c", "d_pred_negative", "d_pred_14", "d_pred_6_without_pred",
            "bit_depth_0", "bit_depth_33", "bit_depth_negative"}


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("palette_check")
    exe = str(tmp / "palette_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "palette_check.cpp"), "-o", exe])
    names = sorted(palette_cases.CASES)
    cases, result = str(tmp / "cases.bin"), str(tmp / "result.bin")
    palette_cases.write_case_file(cases, names)
    r = subprocess.run([exe, cases, result], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return r, names, result


def test_host_arithmetic_equals_the_model_bit_for_bit_under_asan_and_ubsan(check_run):
    r, names, result = check_run
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failure(s)" in r.stdout and "FAIL" not in r.stdout and "%d case(s)" % len(names) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = np.fromfile(result, np.int32)
    at = 0
    for name in names:
        want = palette_cases.expected(name)
        assert np.array_equal(got[at:at + want.size].reshape(want.shape), want), name
        at += want.size
    assert at == got.size


def test_validator_refuses_what_the_entry_must_refuse(check_run):
    r, _, _ = check_run
    assert set(re.findall(r"^REFUSAL (\w+) ok$", r.stdout, re.M)) == REFUSALS


def test_cases_cover_what_they_promise():
    cs = palette_cases.CASES
    assert {c["num_c"] for c in cs.values()} >= {1, 3, 4}
    assert {c["bit_depth"] for c in cs.values()} >= {1, 3, 8, 10, 16, 24, 31, 32}
    assert {c["d_pred"] for c in cs.values()} == set(range(14))
    assert {(c["h"], c["w"]) for c in cs.values()} >= {(1, 1), (1, 7), (7, 1), (2, 5), (21, 37), (33, 70), (257, 769)}
    assert {palette_cases.launches(n) for n in cs} == {1, 2}
    for name, c in cs.items():
        idx, nc = c["index"].astype(np.int64), c["nb_colors"]
        assert c["palette"].shape[0] >= c["num_c"] and c["palette"].shape[1] >= nc, name
        if idx.size < 100:
            continue
        assert (idx >= nc + 64).any() and ((idx >= nc) & (idx < nc + 64)).any() and (idx == I32_MAX).any(), name
        assert nc == 0 or ((idx >= 0) & (idx < nc)).any(), name
        assert c["nb_deltas"] == 0 or ((idx >= 0) & (idx < c["nb_deltas"])).any(), name
        if name != "no_delta_pixel_pred05":
            assert {-1, -143, -144, I32_MIN} <= set(idx[idx < 0].tolist()), name
    # the constants the shapes were chosen by are the kernels'
    internal = open(os.path.join(ROOT, "jxlatte_amd", "csrc", "jxl_internal.h")).read()
    assert int(re.search(r"constexpr int kPaletteLdsInts = (\d+);", internal).group(1)) == palette_cases.LDS_INTS
    assert int(re.search(r"constexpr int kPaletteChainThreads = (\d+);", internal).group(1)) == palette_cases.CHAIN_THREADS
    h, w = cs["front_257x769"]["h"], cs["front_257x769"]["w"]
    longest = max(sum(1 for y in range(h) if 0 <= t - 3 * y < w) for t in range(w + 3 * h - 3))
    assert longest == palette_cases.CHAIN_THREADS + 1
    exact, over = cs["lds_exact_4x2048"], cs["lds_over_4x2049"]
    assert exact["num_c"] * exact["nb_colors"] == palette_cases.LDS_INTS < over["num_c"] * over["nb_colors"]
    assert (exact["index"] == exact["nb_colors"] - 1).any() and (over["index"] == over["nb_colors"] - 1).any()


# ---- declarations, bindings, the CLI's flag ----
def test_header_python_shim_and_java_declare_the_entry():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    shim = open(os.path.join(ROOT, "integration", "jni", "jxlatte_amd_jni.c")).read()
    java = open(os.path.join(ROOT, "integration", "jni", "NativeBackend.java")).read()
    assert re.search(r"jxl_status\s+jxl_stage_palette\s*\(", header) and "ModularStream.java:327-378" in header
    assert "jxl_stage_palette" in _lib.SIGNATURES and hasattr(_lib.load(), "jxl_stage_palette")
    assert re.search(r"\bjxl_stage_palette\s*\(", shim) and "NativeBackend_stagePalette(" in shim
    assert re.search(r"native\s+void\s+stagePalette\s*\(", java) and "jxl_stage_palette" in java
    vp, i32, pi = C.c_void_p, C.c_int32, C.POINTER(C.c_int32)
    assert _lib.SIGNATURES["jxl_stage_palette"] == (i32, [vp, C.POINTER(abi.PaletteDesc), pi, i32, i32, C.POINTER(pi)])
    body = re.search(r"typedef struct jxl_palette_desc \{(.*?)\} jxl_palette_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"int32_t\*?\s+([^;]+);", body) for n in re.findall(r"[a-z_]+", decl)]
    assert names == [f[0] for f in abi.PaletteDesc._fields_] == ["num_c", "nb_colors", "nb_deltas", "d_pred", "bit_depth", "pal_h", "pal_w",
                                                                 "palette", "pred"]
    assert C.sizeof(abi.PaletteDesc) == 48 and abi.PaletteDesc.palette.offset == 32 and abi.PaletteDesc.pred.offset == 40
    # the debug hook is exported, and stays outside the C ABI
    assert hasattr(_lib.load(), "jxl_debug_last_palette") and "jxl_debug_last_palette" not in header


def test_frontend_hook_is_appended_and_optional():
    from jxlatte_amd import frontend
    assert [f[0] for f in frontend.Hooks._fields_] == ["user", "squeeze", "rct", "palette"]
    header = open(os.path.join(ROOT, "include", "jxlatte_frontend.h")).read()
    body = re.search(r"typedef struct jxf_hooks \{(.*?)\} jxf_hooks;", header, re.S).group(1)
    assert re.findall(r"\(\*(\w+)\)", body) == ["squeeze", "rct", "palette"]
    fuzz = open(os.path.join(ROOT, "jxlatte_amd", "frontend", "fuzz_main.cc")).read()
    assert "jxf_hooks h{nullptr, sq, rct};" in fuzz  # two hooks named: the third stays null


def test_cli_and_decoder_switch_default_to_off():
    import inspect
    from jxlatte_amd.__main__ import parser
    from jxlatte_amd.decoder import DeviceBackend, JXLDecoder
    ap = parser()
    assert ap.parse_args(["a.jxl", "o.png"]).device_palette is False
    assert ap.parse_args(["a.jxl", "o.png", "--device-palette"]).device_palette is True
    assert inspect.signature(JXLDecoder.__init__).parameters["device_palette"].default is False
    assert callable(getattr(DeviceBackend, "palette"))


def test_no_context_is_refused_without_a_crash():
    d, keep = abi.make_palette_desc(np.zeros((1, 2), np.int32), None, 1, 2, 0, 0, 8)
    assert _lib.load().jxl_stage_palette(None, C.byref(d), None, 1, 1, None) != 0
