"""JXLDecoder(downsample=8) without a GPU: the image at 1:8 from the LF image of its VarDCT frame.

* front-end: jxf_set_lf_only hands out the source's LF integers and nothing behind them, from a prefix of the file that a full decode
  refuses; the same under AddressSanitizer + UBSan as a program of its own (tools/native/lf_only_check.cpp);
* decoder: on an oracle backend that has `lf_image` (LFBackend below: pyoracle.lf_dequant per LF group at a 256-cell pitch, cropped,
  pyoracle.xyb) the image is that composition bit for bit, made here from the SOURCE of the writer cases or from a full decode's
  integers, and before the inverse XYB it is the float64 model's (jxl_writer_vardct_cases.lf_planes) within the LF stage's K;
* the rule table over every sample; a refused decode never asks for a coefficient;
* fidelity of the definition against the 8 x 8 box mean of the full decode (tools/lf_preview_fidelity.py), with the mutants that
  must miss it;
* plumbing: jxlatte_amd/csrc/lf_image_check.h under the sanitizers, the ctypes mirror, the declarations, the CLI switch.

The case two_lf_groups_2056x16 of the writer is two cells high: no cell of it has four neighbours, so nothing in it is ever smoothed
and a smoothing across the LF-group seam cannot show there (test_the_16_pixel_case_cannot_show_a_seam holds that down). SEAM_CASE
below is the same frame four cells high under lf_rough's scales, where the seam's columns are smoothed by a wrong composition."""
import ctypes as C_
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import jxl_writer_vardct as V
import jxl_writer_vardct_cases as C
import jxl_writer_vardct_run as R
import pixel_ref64 as P
import vardct_ref64 as M
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, frontend
from jxlatte_amd.decoder import JXLDecoder, UnsupportedOperationException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
F = np.float32
WRITER = ("one_dct8", "ragged_67x83", "groups_264x264", "two_lf_groups_2056x16", "passes_2", "lf_rough", "corr", "rgb",
          "noise_40x40", "ycbcr_444", "opsin_custom")  # (noise is left out, YCbCr without subsampling and any opsin matrix are accepted)
# the writer cases that downsample=8 refuses, with the reason preview_rule gives (the first condition that fails, in its order)
WRITER_RULE = dict(up2_19x15_of_37x29="not the image's only frame",  # 2 x 19 is not 37: the size test comes before the factor's
                   up4_ragged="the frame is upsampled", up8_40x40="the frame is upsampled", up2_custom_weights="the frame is upsampled",
                   noise_up2="the frame is upsampled", noise_up2_of_271x39="not the image's only frame", opsin_custom_up2="the frame is upsampled",
                   alpha_40x40="the image has extra channels", alpha_264x264="the image has extra channels",
                   alpha_up2="the image has extra channels", s420="chroma subsampling", s422="chroma subsampling",
                   s440="chroma subsampling")
FILES = ("white", "lenna", "bbb", "bench")
SEAM_CASE = "two_lf_groups_2056x32"

_spec = importlib.util.spec_from_file_location("lf_preview_fidelity", os.path.join(ROOT, "tools", "lf_preview_fidelity.py"))
fidelity = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fidelity)


def sample(name):
    with open(os.path.join(SAMPLES, name + ".jxl"), "rb") as f:
        return f.read()


_seam = {}


def source(name):
    if name != SEAM_CASE:
        return C.source(name)
    if "src" not in _seam:  # lf_rough's scales: the smoothing gap lies in all three regimes
        _seam["src"] = C.fit(lambda seed: C.draw(seed, 2056, 32, allowed=(0, 1, 2, 3, 4, 7, 12, 14), density=0.03, lf_amp=2000,
                                                 extra_precision=3, global_scale=221, quant_lf=16), 31)
    return _seam["src"]


def encoded(name):
    if name != SEAM_CASE:
        return C.encoded(name)
    if "data" not in _seam:
        _seam["data"] = V.encode(source(name), None)
    return _seam["data"]


# ---- the composition, made here --------------------------------------------------------------------------------------------------
MUTANTS = ("xb_exchanged", "no_cfl", "seam_smoothed")


def compose(orc, groups, cells, bcx, bcb, color_factor, mut=None):
    """the LF image before the colour transform: pyoracle.lf_dequant per LF group, assembled at a 256-cell pitch, cropped. mut: one
    of MUTANTS -- X and B exchanged, the LF chroma-from-luma left out, smoothing across the LF-group seams"""
    rows, cols = -(-cells[0] // 256), -(-cells[1] // 256)
    if mut == "no_cfl":
        bcx = bcb = 0.0
    full = np.zeros((3, rows * 256, cols * 256), F)
    if mut == "seam_smoothed":  # one dequantisation of the assembled integers (the groups of the cases it runs on share their scales)
        q = np.zeros((3, rows * 256, cols * 256), np.int32)
        for g in groups:
            a = np.stack(g["lf_quant"])
            q[:, g["lfg_y"] * 256:g["lfg_y"] * 256 + a.shape[1], g["lfg_x"] * 256:g["lfg_x"] * 256 + a.shape[2]] = a
        g = groups[0]
        assert all(h["extra_precision"] == g["extra_precision"] for h in groups)
        return orc.lf_dequant(np.ascontiguousarray(q[:, :cells[0], :cells[1]]), g["scaled_dequant"], g["extra_precision"], g["x_factor_lf"],
                              g["b_factor_lf"], g["adaptive_smoothing"], bcx, bcb, color_factor)
    for g in groups:
        q = np.stack(g["lf_quant"]).astype(np.int32)
        if mut == "xb_exchanged":
            q = np.ascontiguousarray(q[::-1])
        xf, bf = (128, 128) if mut == "no_cfl" else (g["x_factor_lf"], g["b_factor_lf"])
        lf = orc.lf_dequant(q, g["scaled_dequant"], g["extra_precision"], xf, bf, g["adaptive_smoothing"], bcx, bcb, color_factor)
        full[:, g["lfg_y"] * 256:g["lfg_y"] * 256 + lf.shape[1], g["lfg_x"] * 256:g["lfg_x"] * 256 + lf.shape[2]] = lf
    return np.ascontiguousarray(full[:, :cells[0], :cells[1]])


def make_backend(orc, mut=None):
    from oracle.pybackend import OracleBackend

    class LFBackend(OracleBackend):
        """the oracle backend with the one call downsample=8 makes"""
        def __init__(self):
            super().__init__()
            self.lf_calls = []
            self.vardct_calls = 0

        def vardct(self, *a, **kw):
            self.vardct_calls += 1
            return super().vardct(*a, **kw)

        def lf_image(self, groups, cells, bcx, bcb, color_factor, xyb, keep=False):
            assert not keep  # (this backend has no resident planes)
            self.lf_calls.append(dict(groups=groups, cells=cells, xyb=xyb))
            self.last_pre = compose(orc, groups, cells, bcx, bcb, color_factor, mut)
            if xyb is None:
                return self.last_pre
            m, bias, cbrt, it = xyb
            return orc.xyb(self.last_pre, list(m), list(bias), list(cbrt), it)
    return LFBackend()


def groups_of_source(src):
    """what the decoder must hand to lf_image, from the SOURCE alone"""
    p, geo = C.params_of(src), V.geometry(src)
    groups = [dict(lfg_y=i // geo["lcols"], lfg_x=i % geo["lcols"], lf_quant=[np.ascontiguousarray(a, np.int32) for a in g["lf_quant"]],
                   extra_precision=g.get("extra_precision", 0), scaled_dequant=list(p.scaled_dequant), x_factor_lf=p.x_factor_lf,
                   b_factor_lf=p.b_factor_lf, adaptive_smoothing=not src.get("skip_smoothing", False)) for i, g in enumerate(src["lfgroups"])]
    xyb = (p.opsin_matrix, p.opsin_bias, p.cbrt_opsin_bias, p.intensity_target) if src.get("xyb", True) else None
    return groups, (geo["ph"] >> 3, geo["pw"] >> 3), p, xyb


def lf_only(data, on=True):
    fe = frontend.Frontend(data)
    fe.set_lf_only(on)
    fr = fe.next_frame()
    return fe, fr, [fe.lfgroup(i) for i in range(fr.num_lf_groups)]


# ---- front-end: the same integers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WRITER + (SEAM_CASE,))
def test_lf_only_hands_out_the_source_integers(name):
    src, data = source(name), encoded(name)
    fe, fr, views = lf_only(data)
    _, fr_full, full = lf_only(data, False)
    assert len(views) == len(src["lfgroups"]) == len(full)
    for g, v, w in zip(src["lfgroups"], views, full):
        for c in range(3):  # buffer order X, Y, B, as the full decode's view has them (test_jxl_writer_vardct_cpu.views_differ)
            assert v["lf_quant"][c].dtype == np.int32 and np.array_equal(v["lf_quant"][c], g["lf_quant"][c])
            assert np.array_equal(v["lf_quant"][c], w["lf_quant"][c])
        assert v["extra_precision"] == g.get("extra_precision", 0) == w["extra_precision"]
        assert (v["cells_h"], v["cells_w"]) == (w["cells_h"], w["cells_w"]) == np.asarray(g["hf_mul"]).shape
        assert v["n_blocks"] == 0 and w["n_blocks"] == len(g["blocks"]) > 0
        assert v["block_yx"].shape == (0, 2) and not v["dct_select"].any() and not v["hf_mul"].any()  # (null maps read as zeros)
    # LfGlobal was read
    assert list(fr.scaled_dequant) == list(fr_full.scaled_dequant) and fr.colour_factor == fr_full.colour_factor
    assert (fr.x_factor_lf, fr.b_factor_lf, fr.base_corr_x, fr.base_corr_b) == (fr_full.x_factor_lf, fr_full.b_factor_lf, fr_full.base_corr_x, fr_full.base_corr_b)
    for call in (fe.coeffs, fe.coeffs_sparse):
        with pytest.raises(frontend.FrontendError) as e:
            call(0, 0)
        assert e.value.status == -6 and "jxf_set_lf_only" in str(e.value)
    assert fe.next_frame() is None  # the frame was the last one


def test_the_switch_is_per_decoder_and_off_by_default():
    data = encoded("ragged_67x83")
    fe = frontend.Frontend(data)
    fe.next_frame()
    assert fe.lfgroup(0)["n_blocks"] > 0 and fe.coeffs(0, 0)[0].any()
    fe = frontend.Frontend(data)
    fe.set_lf_only(True)
    fe.set_lf_only(False)
    fe.next_frame()
    assert fe.lfgroup(0)["n_blocks"] > 0


def test_a_modular_frame_ignores_the_switch(orc):
    be = make_backend(orc)
    a, b = frontend.Frontend(sample("art")), frontend.Frontend(sample("art"))
    b.set_lf_only(True)
    fa, fb = a.next_frame(be.squeeze, be.rct), b.next_frame(be.squeeze, be.rct)
    assert fa.encoding == fb.encoding == 1 and bytes(fa) == bytes(fb)
    for i in range(fa.num_modular_channels):
        assert np.array_equal(a.modular_channel(i)[0], b.modular_channel(i)[0])


# ---- front-end: truncation -----------------------------------------------------------------------------------------------------------
def _accepts(data, on):
    try:
        return lf_only(data, on)
    except frontend.FrontendError:
        return None


@pytest.mark.parametrize("name", ("groups_264x264", "passes_2", "lenna"))
def test_lf_only_needs_only_a_prefix_of_the_file(name):
    data = sample(name) if name == "lenna" else encoded(name)
    whole = lf_only(data)[2]
    lo, hi = 0, len(data)  # the shortest accepted prefix: lo is refused, hi accepted
    assert _accepts(data[:lo], True) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _accepts(data[:mid], True) is None:
            lo = mid
        else:
            hi = mid
    assert hi < len(data), "LF-only decoding needs the whole file"
    cut = _accepts(data[:hi], True)
    assert cut is not None and _accepts(data[:hi - 1], True) is None
    for v, w in zip(cut[2], whole):
        assert all(np.array_equal(a, b) for a, b in zip(v["lf_quant"], w["lf_quant"])) and v["extra_precision"] == w["extra_precision"]
    assert cut[0].next_frame() is None  # (is_last: the missing tail is nobody's business)
    with pytest.raises(frontend.FrontendError):  # the full decode wants the sections behind the LF groups
        lf_only(data[:hi], False)


def test_lf_only_is_clean_under_the_sanitizers(tmp_path):
    """tools/native/lf_only_check.cpp over the front-end's sources, as a process of its own: the cases above and lenna.jxl, LF-only
    against the full decode, and every prefix length of one_dct8"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path / "lf_only_check")
    fdir = os.path.join(ROOT, "jxlatte_amd", "frontend")
    flags = ["-O1", "-g", "-std=c++17", "-fwrapv", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]
    srcs = [os.path.join(ROOT, "tools", "native", "lf_only_check.cpp")] + [os.path.join(fdir, f) for f in ("entropy.cc", "headers.cc", "modular.cc", "frame.cc", "api.cc")]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    cxx = os.environ.get("CXX", "g++")
    with ThreadPoolExecutor(len(srcs)) as ex:  # (one translation unit per core: the build is most of this test's time)
        list(ex.map(lambda so: subprocess.check_call([cxx] + flags + ["-c", so[0], "-o", so[1]]), zip(srcs, objs)))
    subprocess.check_call([cxx] + flags + ["-static-libasan", "-static-libubsan"] + objs + ["-o", exe])
    paths = []
    for name in WRITER + (SEAM_CASE, "s420"):
        paths.append(str(tmp_path / (name + ".jxl")))
        with open(paths[-1], "wb") as f:
            f.write(encoded(name))
    paths.append(os.path.join(SAMPLES, "lenna.jxl"))
    r = subprocess.run([exe] + paths + ["--prefixes", paths[0]], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(paths) + 1


# ---- the decoder against the model ---------------------------------------------------------------------------------------------------
def preview(data, orc, mut=None, **kw):
    be = make_backend(orc, mut)
    dec = JXLDecoder(data, backend=be, downsample=8, **kw)
    im = dec.decode()
    return dec, be, im


@pytest.mark.parametrize("name", WRITER + (SEAM_CASE,))
def test_preview_of_a_writer_case_is_the_composition_of_its_source(orc, name):
    src = source(name)
    groups, cells, p, xyb = groups_of_source(src)
    dec, be, im = preview(encoded(name), orc)
    assert be.vardct_calls == 0 and len(be.lf_calls) == 1
    pre = compose(orc, groups, cells, float(p.base_corr_x), float(p.base_corr_b), p.color_factor)
    want = pre if xyb is None else orc.xyb(pre, *[list(v) for v in xyb[:3]], xyb[3])
    if src.get("do_ycbcr", False):
        want = orc.ycbcr(want)
    assert (im.getHeight(), im.getWidth()) == cells == (-(-src["height"] // 8), -(-src["width"] // 8))
    assert_bits_equal(np.stack(im.getBuffer(copy=False)), want, name)
    note = "lf image (1:8)" + (", noise left out" if src.get("noise") is not None else "")
    assert dec.stats[-1]["preview"] == note and dec.stats[-1]["output"] == "host" and dec.decode() is None
    # before the inverse XYB: the float64 model of the SOURCE, within the LF stage's K (jxl_writer_vardct_run.K_LF)
    for g, d in zip(src["lfgroups"], groups):
        x = np.stack(C.lf_planes(src, g, p))
        h, w = x.shape[1:]
        smoothed = d["adaptive_smoothing"] and min(h, w) >= 3
        a = P.lf_stage(np.stack([np.asarray(q, np.int64) for q in g["lf_quant"]]), p.scaled_dequant, d["extra_precision"], p.x_factor_lf,
                       p.b_factor_lf, d["adaptive_smoothing"], float(p.base_corr_x), float(p.base_corr_b), p.color_factor)[1]
        got = be.last_pre[:, d["lfg_y"] * 256:d["lfg_y"] * 256 + h, d["lfg_x"] * 256:d["lfg_x"] * 256 + w]
        ratio = M.error_ratio(got, x, a)
        print("%s LF group (%d, %d): K %.2f of %d" % (name, d["lfg_y"], d["lfg_x"], ratio, R.K_LF[smoothed]))
        assert ratio <= R.K_LF[smoothed]


@pytest.mark.parametrize("name", FILES)
def test_preview_of_a_sample_is_the_composition_of_its_integers(orc, name):
    data = sample(name)
    fe, fr, _ = lf_only(data, False)  # the full decode's integers
    info = fe.image
    groups, cells = fidelity.lf_groups(fe, fr), (-(-fr.height // 8), -(-fr.width // 8))
    dec, be, im = preview(data, orc)
    assert be.vardct_calls == 0 and len(be.lf_calls) == 1
    want = compose(orc, groups, cells, fr.base_corr_x, fr.base_corr_b, fr.colour_factor)
    if info.xyb_encoded:
        m, bias, cbrt = dec._opsin()
        want = orc.xyb(want, list(m), list(bias), list(cbrt), info.intensity_target)
    if fr.do_ycbcr:
        want = orc.ycbcr(want)
    if info.orientation != 1:
        want = np.stack([orc.orient(np.ascontiguousarray(want[c]), info.orientation) for c in range(3)])
    assert_bits_equal(np.stack(im.getBuffer(copy=False)), want, name)
    assert dec.stats[-1]["preview"] == "lf image (1:8)"
    if name == "bench":  # orientation 5 of a 500 x 606 frame: 63 x 76 cells, transposed
        assert (info.orientation, fr.width, fr.height, bool(fr.do_ycbcr)) == (5, 500, 606, True)
        assert (im.getWidth(), im.getHeight()) == (76, 63)
    else:
        assert (im.getWidth(), im.getHeight()) == (cells[1], cells[0])


def test_the_preview_image_is_an_ordinary_image(orc):
    """the writers and transform() take it as they take any image"""
    import io
    from jxlatte_amd.decoder import PNGWriter
    _, _, im = preview(sample("bbb"), orc)
    out = io.BytesIO()
    PNGWriter(im).write(out)
    png = out.getvalue()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:24] == (160).to_bytes(4, "big") + (90).to_bytes(4, "big")
    assert not im.onDevice() and im.getColorChannelCount() == 3 and not im.hasAlpha()


# ---- the rule table ------------------------------------------------------------------------------------------------------------------
RULE = dict(art="not a VarDCT frame", quilt="not a VarDCT frame", blendmodes_5="the image has extra channels",
            **{"wb-rainbow": "the image has extra channels", "patches-lossless": "the image has extra channels"},
            white=None, lenna=None, bbb=None, bench=None)


def test_every_sample_has_a_row_in_the_rule_table():
    assert sorted(RULE) == sorted(f[:-4] for f in os.listdir(SAMPLES) if f.endswith(".jxl"))


@pytest.mark.parametrize("name", sorted(RULE))
def test_preview_rule_on_the_samples(orc, name):
    be = make_backend(orc)
    fe = frontend.Frontend(sample(name))
    fr = fe.next_frame(be.squeeze, be.rct)
    assert JXLDecoder.preview_rule(fe.image, fr) == RULE[name]
    assert JXLDecoder.preview_rule(fe.image, None) == (RULE[name] if fe.image.num_extra else None)


def test_preview_rule_on_header_fields():
    import types
    info = types.SimpleNamespace(num_extra=0, width=40, height=24)
    ok = dict(encoding=0, type=0, lf_level=0, flags=0, is_last=1, x0=0, y0=0, width=40, height=24, upsampling=1, jpeg_up_y=[0, 0, 0],
              jpeg_up_x=[0, 0, 0], num_patches=0, has_splines=0, has_noise=0, do_ycbcr=0)

    def rule(**kw):
        return JXLDecoder.preview_rule(info, types.SimpleNamespace(**dict(ok, **kw)))
    assert rule() is None and rule(has_noise=1, flags=1) is None and rule(do_ycbcr=1) is None and rule(flags=128) is None
    assert rule(encoding=1) == "not a VarDCT frame"
    for kw in (dict(type=1), dict(type=2), dict(type=3), dict(lf_level=1), dict(flags=32)):
        assert rule(**kw) == "not a regular frame of LF level 0 with LF coefficients of its own"
    for kw in (dict(is_last=0), dict(x0=8), dict(y0=-8), dict(width=32), dict(height=16)):
        assert rule(**kw) == "not the image's only frame"
    assert rule(upsampling=2, width=20, height=12) == "the frame is upsampled"
    assert rule(jpeg_up_x=[1, 0, 1]) == rule(jpeg_up_y=[0, 0, 1]) == "chroma subsampling"
    assert rule(num_patches=2, flags=2) == "patches" and rule(has_splines=1, flags=16) == "splines"
    assert JXLDecoder.preview_rule(types.SimpleNamespace(num_extra=1, width=40, height=24), types.SimpleNamespace(**ok)) == "the image has extra channels"


@pytest.mark.parametrize("name", sorted(WRITER_RULE))
def test_preview_rule_on_the_writer_cases(orc, name):
    """every writer case outside WRITER is refused for the reason the rule gives, by the rule and by a decode; the others pass it"""
    fe, fr, _ = lf_only(encoded(name), False)
    assert JXLDecoder.preview_rule(fe.image, fr) == WRITER_RULE[name]
    be = make_backend(orc)
    with pytest.raises(UnsupportedOperationException) as e:
        JXLDecoder(encoded(name), backend=be, downsample=8).decode()
    assert str(e.value) == "downsample=8: " + WRITER_RULE[name] and be.vardct_calls == 0 and not be.lf_calls


def test_the_writer_rule_table_covers_the_tail_cases():
    also = ("noise_264x264", "noise_corr", "opsin_custom_epf2")  # accepted like their siblings in WRITER; not decoded here
    assert set(C.TAIL_CASES) == (set(WRITER) | set(WRITER_RULE) | set(also)) & set(C.TAIL_CASES)
    for name in WRITER + also:
        fe, fr, _ = lf_only(encoded(name), False)
        assert JXLDecoder.preview_rule(fe.image, fr) is None, name


def test_s420_is_refused_for_its_subsampling():
    fe, fr, _ = lf_only(encoded("s420"), False)
    assert JXLDecoder.preview_rule(fe.image, fr) == "chroma subsampling"


@pytest.mark.parametrize("name,reason", [("s420", "chroma subsampling"), ("art", "not a VarDCT frame"),
                                         ("patches-lossless", "the image has extra channels")])
def test_a_refused_decode_never_asks_for_a_coefficient(orc, monkeypatch, name, reason):
    asked = []
    for fn in ("coeffs", "coeffs_sparse", "quant_params"):
        monkeypatch.setattr(frontend.Frontend, fn, lambda self, *a, _fn=fn: asked.append(_fn) or pytest.fail("asked for " + _fn))
    be = make_backend(orc)
    dec = JXLDecoder(encoded(name) if name == "s420" else sample(name), backend=be, downsample=8)
    with pytest.raises(UnsupportedOperationException) as e:
        dec.decode()
    assert str(e.value) == "downsample=8: " + reason
    assert asked == [] and be.lf_calls == [] and be.vardct_calls == 0


def test_an_accepted_decode_never_asks_for_a_coefficient(orc, monkeypatch):
    asked = []
    for fn in ("coeffs", "coeffs_sparse", "quant_params"):
        monkeypatch.setattr(frontend.Frontend, fn, lambda self, *a, _fn=fn: asked.append(_fn))
    preview(sample("lenna"), orc)
    assert asked == []


def test_bad_arguments_are_refused_up_front(orc):
    data = sample("white")
    for bad in (0, 2, 4, 16, -8, "8", None):
        with pytest.raises(ValueError):
            JXLDecoder(data, backend=make_backend(orc), downsample=bad)
    for kw in (dict(draw_varblocks=True), dict(device_canvas=True), dict(device_frames=True)):
        with pytest.raises(ValueError):
            JXLDecoder(data, backend=make_backend(orc), downsample=8, **kw)
    dec = JXLDecoder(data, backend=make_backend(orc), downsample=8)
    dec.trace = lambda *a: None
    with pytest.raises(ValueError):
        dec.decode()
    from oracle.pybackend import OracleBackend
    with pytest.raises(RuntimeError):  # a backend without `lf_image` is an error, never a full decode
        JXLDecoder(data, backend=OracleBackend(), downsample=8).decode()
    assert JXLDecoder(data, backend=make_backend(orc)).downsample == 1 and JXLDecoder.downsample == 1


def test_without_the_switch_nothing_changes(orc):
    """downsample=1 is the decoder as it was: the same planes and stats as a decoder made without the argument"""
    for name in ("lenna", "bench"):
        a, b = JXLDecoder(sample(name), backend=make_backend(orc)), JXLDecoder(sample(name), backend=make_backend(orc), downsample=1)
        ia, ib = a.decode(), b.decode()
        assert a.stats == b.stats and "preview" not in a.stats[-1] and a.backend.lf_calls == b.backend.lf_calls == []
        assert_bits_equal(np.stack(ia.getBuffer(copy=False)), np.stack(ib.getBuffer(copy=False)), name)


# ---- fidelity of the definition ------------------------------------------------------------------------------------------------------
def _measure(orc, name, mut=None):
    return fidelity.measure(sample(name), orc, make_backend(orc), compose=lambda o, *a: compose(o, *a, mut=mut))


def test_the_lf_cell_of_a_dct8_jpeg_is_the_block_mean(orc):
    """bench.jxl: DCT8 only, no Gaborish, no EPF -- the LF coefficient IS the block's mean. 1e-6 is 16 float32 ulps at magnitude 1;
    1.5e-8 was measured"""
    m = _measure(orc, "bench")
    print("bench.jxl: max |LF cell - 8 x 8 mean| %.3g on a range of %.3f (%s)" % (m["max_abs"], m["range"], m["domain"]))
    assert m["domain"] == "YCbCr" and m["cells"] == (75, 62) and m["max_abs"] <= 1e-6


# linear-RGB PSNR (peak 1.0) measured on the CPU oracle: the definition and what the two arithmetic mutants give
MEASURED_PSNR = dict(lenna=dict(definition=38.3, xb_exchanged=7.3, no_cfl=10.0), bbb=dict(definition=38.9, xb_exchanged=10.9, no_cfl=3.0))


@pytest.mark.parametrize("name", ("lenna", "bbb"))
def test_the_preview_is_the_box_mean_of_the_full_decode_to_37_db(orc, name):
    m = _measure(orc, name)
    print("%s.jxl: %.2f dB; XYB mean |diff| %.2f %% of the range, max %.1f %%" % (name, m["psnr_rgb"], 100 * m["mean_abs"] / m["range"],
                                                                                 100 * m["max_abs"] / m["range"]))
    assert m["psnr_rgb"] >= 37.0
    assert abs(m["psnr_rgb"] - MEASURED_PSNR[name]["definition"]) < 0.1  # (the oracle is deterministic: the recorded figure)


@pytest.mark.parametrize("mut", ("xb_exchanged", "no_cfl"))
@pytest.mark.parametrize("name", ("lenna", "bbb"))
def test_an_arithmetic_mutant_misses_37_db_by_far(orc, name, mut):
    m = _measure(orc, name, mut)
    print("%s.jxl, %s: %.2f dB" % (name, mut, m["psnr_rgb"]))
    assert m["psnr_rgb"] < 37.0 - 15.0  # "far below": 15 dB under the pin is 30 times its mean squared error
    assert abs(m["psnr_rgb"] - MEASURED_PSNR[name][mut]) < 0.1


@pytest.mark.parametrize("mut", MUTANTS)
def test_a_mutant_composition_is_not_the_decoders_image(orc, mut):
    """each mutant fails the bit-for-bit test of the case that can show it"""
    name = SEAM_CASE if mut == "seam_smoothed" else "corr"
    src = source(name)
    groups, cells, p, _ = groups_of_source(src)
    _, be, _ = preview(encoded(name), orc)
    good = compose(orc, groups, cells, float(p.base_corr_x), float(p.base_corr_b), p.color_factor)
    bad = compose(orc, groups, cells, float(p.base_corr_x), float(p.base_corr_b), p.color_factor, mut)
    assert_bits_equal(be.last_pre, good, name)
    differ = np.argwhere(be.last_pre.view(np.uint32) != bad.view(np.uint32))
    assert differ.size, mut
    if mut == "seam_smoothed":  # only the seam's cells that have four neighbours in the assembled image: column 255, rows 1 and 2
        assert set(differ[:, 2].tolist()) == {255} and set(differ[:, 1].tolist()) <= {1, 2}


def test_the_16_pixel_case_cannot_show_a_seam(orc):
    """two_lf_groups_2056x16 is two cells high: no cell has four neighbours, nothing is smoothed, the seam mutant is the definition.
    (The mutant is shown on SEAM_CASE above.)"""
    src = source("two_lf_groups_2056x16")
    groups, cells, p, _ = groups_of_source(src)
    assert cells == (2, 257)
    for g in groups:
        g["extra_precision"] = 0  # (the mutant dequantises once: give the groups one scale, for both sides)
    args = (groups, cells, float(p.base_corr_x), float(p.base_corr_b), p.color_factor)
    assert_bits_equal(compose(orc, *args), compose(orc, *args, "seam_smoothed"))


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lf_image_check") / "lf_image_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "lf_image_check.cpp"), "-o", exe])
    return exe


def _run_check(exe, pairs=()):
    r = subprocess.run([exe] + [str(v) for p in pairs for v in p], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    return r.stdout


def test_validator_is_clean_under_the_sanitizers(check_program):
    """the program's own table: accepted tilings with their plans, and the refusals -- overlap, a group outside the grid, a 257-cell
    group, a null plane, color_factor 0, extra_precision, the group count, the output size"""
    _run_check(check_program)


def test_the_plan_of_the_gpu_tests_grids(check_program):
    """PLAN of (cells_h, cells_w) descriptors whose groups come in reverse order, against the sums made here"""
    grids = [(1, 1), (33, 288), (257, 2), (260, 300)]
    lines = [ln.split()[1:] for ln in _run_check(check_program, grids).splitlines() if ln.startswith("PLAN")]
    assert len(lines) == len(grids)
    for (ch, cw), ln in zip(grids, lines):
        v = [int(x) for x in ln]
        gr, gc = -(-ch // 256), -(-cw // 256)
        n = gr * gc
        assert v[:3] == [gr, gc, 3 * ch * cw] and v[3:3 + n] == list(range(n - 1, -1, -1))
        sizes = [min(256, ch - 256 * (p // gc)) * min(256, cw - 256 * (p % gc)) for p in range(n) for _ in range(3)]
        assert v[3 + n:] == [sum(sizes[:k]) for k in range(3 * n)]


def test_descriptor_has_the_c_layout(tmp_path):
    src = tmp_path / "layout.cpp"
    fields = ("n_groups", "cells_h", "cells_w", "color_factor", "groups", "base_corr_x", "base_corr_b", "xyb", "opsin_matrix", "opsin_bias",
              "cbrt_opsin_bias", "intensity_target")
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "jxlatte_amd.h"\nint main() {\n    printf("%zu %zu", sizeof(jxl_lf_image_desc), '
                   'sizeof(jxl_lfquant_desc));\n' + "".join('    printf(" %%zu", offsetof(jxl_lf_image_desc, %s));\n' % f for f in fields) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    T = abi.LFImageDesc
    assert out == [C_.sizeof(T), C_.sizeof(abi.LFQuantDesc)] + [getattr(T, f).offset for f in fields]


def test_descriptor_binding():
    rng = np.random.default_rng(2)
    groups = [dict(lfg_y=0, lfg_x=x, lf_quant=[rng.integers(-9, 9, (5, w)).astype(np.int32) for _ in range(3)], extra_precision=x + 1,
                   scaled_dequant=[0.5, 0.25, 0.125], x_factor_lf=120 + x, b_factor_lf=131, adaptive_smoothing=bool(x)) for x, w in ((0, 256), (1, 7))]
    d, keep = abi.make_lf_image_desc(groups, (5, 263), 0.25, 0.75, 90, xyb=(np.arange(9, dtype=F), [1, 2, 3], [4, 5, 6], 255.0))
    assert (d.n_groups, d.cells_h, d.cells_w, d.color_factor, d.base_corr_x, d.base_corr_b, d.xyb) == (2, 5, 263, 90, 0.25, 0.75, 1)
    assert list(d.opsin_matrix) == list(range(9)) and list(d.opsin_bias) == [1, 2, 3] and list(d.cbrt_opsin_bias) == [4, 5, 6] and d.intensity_target == 255.0
    for i, g in enumerate(groups):
        q = d.groups[i]
        assert (q.lfg_y, q.lfg_x, q.cells_h, q.cells_w, q.extra_precision, q.x_factor_lf, q.b_factor_lf, q.adaptive_smoothing) == \
            (0, i, 5, g["lf_quant"][0].shape[1], i + 1, 120 + i, 131, i)
        assert list(q.scaled_dequant) == [0.5, 0.25, 0.125]
        for c in range(3):
            assert np.array_equal(np.ctypeslib.as_array(q.lf_quant[c], shape=(5 * q.cells_w,)).reshape(5, q.cells_w), g["lf_quant"][c])
    assert abi.make_lf_image_desc(groups, (5, 263))[0].xyb == 0
    groups[0]["lf_quant"][1] = groups[0]["lf_quant"][1][:, :8]
    with pytest.raises(ValueError):
        abi.make_lf_image_desc(groups, (5, 263))


def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    vp = C_.c_void_p
    for name in ("jxl_planes_from_lf", "jxl_stage_lf_image"):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["jxl_planes_from_lf"] == (C_.c_int32, [vp, C_.POINTER(abi.LFImageDesc)])
    assert _lib.SIGNATURES["jxl_stage_lf_image"][1][:2] == [vp, C_.POINTER(abi.LFImageDesc)]
    fheader = open(os.path.join(ROOT, "include", "jxlatte_frontend.h")).read()
    assert re.search(r"int32_t\s+jxf_set_lf_only\s*\(", fheader) and "jxf_set_lf_only" in frontend.SIGNATURES
    csrc = os.path.join(ROOT, "jxlatte_amd", "csrc")
    for f in ("k_lf_image.hip", "lf_image_host.hip", "lf_image_check.h", "lf_image.h", "lf_cell.h"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()  # no environment switch
    # one definition each: the LF cell and the inverse XYB are called, not restated
    kernel = open(os.path.join(csrc, "k_lf_image.hip")).read()
    assert "lf_cell(" in kernel and "invert_xyb_px(" in kernel and "0.05226273532324128f" not in kernel and "gammaL" not in kernel
    assert "lf_cell(" in open(os.path.join(csrc, "k_lf.hip")).read() and open(os.path.join(csrc, "lf_cell.h")).read().count("0.05226273532324128f") == 1
    assert kernel.count("hipLaunchKernelGGL") == 1 and open(os.path.join(csrc, "lf_image_host.hip")).read().count("hipMemcpyHostToDevice") == 1


def test_the_cli_has_the_switch():
    from jxlatte_amd.__main__ import parser
    a = parser().parse_args(["--downsample=8", "in.jxl", "out.png"])
    assert a.downsample == 8 and parser().parse_args(["in.jxl"]).downsample == 1
    with pytest.raises(SystemExit):
        parser().parse_args(["--downsample=4", "in.jxl"])
