"""CPU-only: JXLDecoder(region=) on the oracle backend.

  * the region decode of every frame and box of tests/region_cases.py equals the crop of the full decode bit for bit, and reads
    exactly the groups and LF groups that the box, the margin M and the geometry give (computed here);
  * a margin of M - 1 (jxf_debug_set_region_margin) is wrong: on each margin setting a box differs from the crop, and M + 8 is right;
  * the front-end touches no unselected section (overwritten or missing ones decode), refuses what it did not read, decodes a
    single-section frame whole; the same under AddressSanitizer + UBSan as a program of its own (tools/native/region_check.cpp);
  * region_rule's reasons on the writer cases and the nine sample files; a refused decode never reaches backend.vardct;
  * region_in_frame against numpy's eight transforms; the ValueErrors, the refused combinations, the CLI, the struct's layout;
  * the windowed noise validator (jxlatte_amd/csrc/noise_window_check.h) under the sanitizers.

A region of a frame whose TOC is permuted is test_jxl_writer_lfframe_cpu.py's (the group sections are looked up through the
permutation). No generated or sample file carries an orientation: that is tested through the image header's field
(test_an_oriented_image_end_to_end)."""
import ctypes as C_
import functools
import io
import os
import re
import subprocess
import types

import numpy as np
import pytest

import jxl_writer_vardct_cases as C
import region_cases as RC
from conftest import assert_bits_equal
from jxlatte_amd import _lib, frontend
from jxlatte_amd.decoder import JXLDecoder, JXLImage, PFMWriter, PNGWriter, UnsupportedOperationException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
FILES = ("lenna", "bbb", "bench", "white")
JXF_ERR_STATE = -6


def sample(name):
    with open(os.path.join(SAMPLES, name + ".jxl"), "rb") as f:
        return f.read()


def make_backend():
    from oracle import pyoracle as orc
    from oracle.pybackend import OracleBackend

    class RegionBackend(OracleBackend):
        """the oracle backend with the one call a region with noise makes: the whole frame's noise, cropped"""
        def __init__(self):
            super().__init__()
            self.vardct_sizes = []

        def vardct(self, params, *a, **kw):
            self.vardct_sizes.append((params.width, params.height))
            return super().vardct(params, *a, **kw)

        def noise_window(self, planes, group_dim, seed0, lut, bcx, bcb, frame_h, frame_w, y0, x0):
            h, w = planes.shape[1:]
            noise = orc.noise_init(frame_h, frame_w, seed0, group_dim, 3)
            return orc.noise_add(planes, np.ascontiguousarray(noise[:, y0:y0 + h, x0:x0 + w]), lut, bcx, bcb)
    return RegionBackend()


def data_of(name):
    return RC.encoded(name) if name in RC.FRAMES else C.encoded(name) if name in C.CASES else sample(name)


@functools.lru_cache(maxsize=None)
def full_decode(name):
    """the full decode's planes, computed once per file and never written to"""
    planes = JXLDecoder(data_of(name), backend=make_backend()).decode().getBuffer(copy=False)
    for p in planes:
        p.setflags(write=False)
    return planes


def region_decode(name, box, margin=None, data=None, **kw):
    dec = JXLDecoder(data_of(name) if data is None else data, backend=make_backend(), region=box, **kw)
    if margin is not None:
        assert dec.fe.lib.jxf_debug_set_region_margin(dec.fe.h, margin) == 0
    return dec, dec.decode()


def assert_is_crop(image, name, box, what=""):
    full = full_decode(name)
    assert (image.getWidth(), image.getHeight()) == (box[2], box[3]) and len(image.buffer) == len(full) and image.region == tuple(box)
    for c, (a, b) in enumerate(zip(image.getBuffer(copy=False), RC.crop(full, box))):
        assert_bits_equal(a, b, "%s %s plane %d %s" % (name, box, c, what))


def differs_from_crop(image, name, box):
    return any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(image.getBuffer(copy=False), RC.crop(full_decode(name), box)))


# ---- region equals crop, and reads what the formula says ----------------------------------------------------------------------------
CASES = [(name, i) for name, n in RC.BOX_COUNT.items() for i in range(n)]


def test_the_case_list_is_complete():
    assert sorted(RC.BOX_COUNT) == sorted(RC.FRAMES) and all(len(RC.boxes(name)) == n for name, n in RC.BOX_COUNT.items())


@pytest.mark.parametrize("name,i", CASES)
def test_region_equals_crop(name, i):
    box = RC.boxes(name)[i]
    w, h = RC.size(name)
    m = RC.margin(name)
    dec, im = region_decode(name, box)
    assert_is_crop(im, name, box)
    r = dec.stats[-1]["region"]
    groups, lf_groups = RC.expected_reads(w, h, box, m)
    assert (r["groups_read"], r["lf_groups_read"], r["margin"]) == (groups, lf_groups, m)
    assert (r["groups_total"], r["lf_groups_total"]) == (-(-w // 256) * -(-h // 256), -(-w // 2048) * -(-h // 2048))
    assert r["box"] == r["frame_box"] == tuple(box) and r["path"] == "groups"
    assert 0 < r["section_bytes_read"] <= r["section_bytes_total"] and (r["section_bytes_read"] == r["section_bytes_total"]) == (groups == r["groups_total"])
    # the sub-frame is the LF-group rectangle: its origin a multiple of 2048, and backend.vardct saw exactly it
    sx, sy, sw, sh = r["subframe"]
    assert sx % 2048 == 0 and sy % 2048 == 0 and dec.backend.vardct_sizes == [(sw, sh)]
    assert sx <= box[0] and sy <= box[1] and box[0] + box[2] <= sx + sw and box[1] + box[3] <= sy + sh


def test_the_table_of_the_issue():
    """the counts the issue states for its boxes"""
    reads = {name: [RC.expected_reads(*RC.size(name), b, RC.margin(name)) for b in RC.boxes(name)] for name in ("A", "B", "C")}
    assert RC.margin("A") == 7 and RC.margin("A1") == 2 and RC.margin("A2") == 3
    assert [g for g, _ in reads["A"]] == [1, 4, 1, 1, 4, 9]
    assert [lf for _, lf in reads["B"]] == [1, 2, 1] and [lf for _, lf in reads["C"]] == [1, 2, 1]
    for name in ("B", "C"):  # the sub-frame of LF group 1 begins at 2048; LF group 0 alone for the box at 1000
        decs = [region_decode(name, b)[0] for b in RC.boxes(name)]
        origins = [d.stats[-1]["region"]["subframe"][:2] for d in decs]
        assert origins == ([(2048, 0), (0, 0), (0, 0)] if name == "B" else [(0, 2048), (0, 0), (0, 0)])


@pytest.mark.parametrize("name", ["D"])
def test_every_pass_of_a_selected_group_is_read(name):
    fe = frontend.Frontend(RC.encoded(name))
    fe.set_region((0, 0, 16, 16))
    fr = fe.next_frame()
    assert fr.num_passes == 2 and fe.region_plan()["groups_read"] == 1
    for p in range(2):
        assert any(np.any(q) for q in fe.coeffs(p, 0))
        with pytest.raises(frontend.FrontendError) as e:
            fe.coeffs(p, 3)
        assert e.value.status == JXF_ERR_STATE


# ---- a smaller margin is wrong -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "A1", "A2"])
def test_a_smaller_margin_is_wrong_and_a_larger_one_is_right(name):
    m = RC.margin(name)
    four = RC.boxes(name)[1]  # one pixel inside the margin of the centre group: four groups under M, one under M - 1
    w, h = RC.size(name)
    assert RC.expected_reads(w, h, four, m)[0] == 4 and RC.expected_reads(w, h, four, m - 1)[0] == 1
    dec, im = region_decode(name, four, margin=m - 1)
    r = dec.stats[-1]["region"]
    assert (r["margin"], r["groups_read"]) == (m - 1, 1)
    assert differs_from_crop(im, name, four), "M - 1 gives the crop: the margin is not pinned from below"
    for box in RC.boxes(name):
        dec, im = region_decode(name, box, margin=m + 8)
        assert dec.stats[-1]["region"]["margin"] == m + 8 and dec.stats[-1]["region"]["groups_read"] == RC.expected_reads(w, h, box, m + 8)[0]
        assert_is_crop(im, name, box, "under M + 8")


# ---- the front-end -------------------------------------------------------------------------------------------------------------------
def plan_of(data, box, margin=None):
    fe = frontend.Frontend(data)
    fe.set_region(box)
    if margin is not None:
        assert fe.lib.jxf_debug_set_region_margin(fe.h, margin) == 0
    fr = fe.next_frame()
    return fe, fr, fe.region_plan()


@functools.lru_cache(maxsize=None)
def sections_of_A():
    """frame A's sections from the plans alone: (offset of the first pass-group section in the file, the nine groups' lengths).
    One box per group gives base + its length, a box over groups 0 and 1 gives base + both: base = LfGlobal + LF group + HfGlobal"""
    data = RC.encoded("A")
    one = [plan_of(data, (256 * (g % 3) + 1, 256 * (g // 3) + 1, 1, 1), margin=0)[2] for g in range(9)]
    assert all(p["groups_read"] == 1 and (p["group_x0"], p["group_y0"]) == (g % 3, g // 3) for g, p in enumerate(one))
    pair = plan_of(data, (255, 1, 2, 1), margin=0)[2]
    assert pair["groups_read"] == 2
    base = one[0]["section_bytes_read"] + one[1]["section_bytes_read"] - pair["section_bytes_read"]
    lengths = [p["section_bytes_read"] - base for p in one]
    total = one[0]["section_bytes_total"]
    assert base > 0 and all(n > 0 for n in lengths) and base + sum(lengths) == total
    return len(data) - total + base, lengths


def test_unselected_sections_are_never_touched():
    data = RC.encoded("A")
    first, lengths = sections_of_A()
    starts = [first + sum(lengths[:g]) for g in range(9)]
    centre = RC.boxes("A")[0]
    bad = bytearray(data)
    for g in range(9):
        if g != 4:
            bad[starts[g]:starts[g] + lengths[g]] = b"\xff" * lengths[g]
    dec, im = region_decode("A", centre, data=bytes(bad))
    assert dec.stats[-1]["region"]["groups_read"] == 1
    assert_is_crop(im, "A", centre, "with every other group overwritten")
    # a file that ends behind the last selected section decodes; one that ends inside it does not
    corner = (0, 0, 8, 8)
    dec, im = region_decode("A", corner, data=data[:starts[0] + lengths[0]])
    assert_is_crop(im, "A", corner, "of a truncated file")
    dec, im = region_decode("A", centre, data=data[:starts[4] + lengths[4]])
    assert_is_crop(im, "A", centre, "of a truncated file")
    with pytest.raises(Exception):
        region_decode("A", centre, data=data[:starts[4] + lengths[4] - 1])
    with pytest.raises(Exception):  # without a region the same file is truncated
        JXLDecoder(data[:starts[4] + lengths[4]], backend=make_backend()).decode()


def test_what_was_not_read_is_refused():
    fe, fr, plan = plan_of(RC.encoded("A"), RC.boxes("A")[0])
    assert plan["applied"] == 1 and (plan["group_x0"], plan["group_y0"], plan["group_w"], plan["group_h"]) == (1, 1, 1, 1)
    assert [np.shape(q) for q in fe.coeffs(0, 4)] == [(256, 256)] * 3 and fe.coeffs_sparse(0, 4)
    for g in (0, 1, 3, 5, 8):
        for fn in (fe.coeffs, fe.coeffs_sparse):
            with pytest.raises(frontend.FrontendError) as e:
                fn(0, g)
            assert e.value.status == JXF_ERR_STATE
    fe, fr, plan = plan_of(RC.encoded("B"), RC.boxes("B")[0])
    assert (plan["lf_group_x0"], plan["lf_group_w"], plan["lf_groups_read"], plan["lf_groups_total"]) == (1, 1, 1, 2)
    assert fe.lfgroup(1)["n_blocks"] > 0
    with pytest.raises(frontend.FrontendError) as e:
        fe.lfgroup(0)
    assert e.value.status == JXF_ERR_STATE


def test_clearing_and_combining():
    data = RC.encoded("A")
    fe = frontend.Frontend(data)
    fe.set_region((0, 0, 8, 8))
    fe.set_region(None)  # w == 0 clears it
    fe.next_frame()
    plan = fe.region_plan()
    assert plan["applied"] == 0 and plan["groups_read"] == plan["groups_total"] == 9 and plan["section_bytes_read"] == plan["section_bytes_total"]
    assert fe.coeffs(0, 8)
    fe = frontend.Frontend(data)
    fe.set_region((0, 0, 8, 8))
    fe.set_lf_only(True)
    with pytest.raises(frontend.FrontendError) as e:
        fe.next_frame()
    assert e.value.status == JXF_ERR_STATE
    fe = frontend.Frontend(data)
    for bad in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, -8, 8), (0, 0, 8, 0)):
        with pytest.raises(frontend.FrontendError):
            fe.set_region(bad)
    fe.set_region((600, 0, 8, 8))  # not inside the frame: the frame is decoded whole
    fe.next_frame()
    assert fe.region_plan()["applied"] == 0


def test_a_single_section_frame_is_decoded_whole():
    box = (2, 3, 5, 4)
    dec, im = region_decode("one_dct8", box)
    r = dec.stats[-1]["region"]
    assert r["path"] == "whole frame (single section)" and r["groups_read"] == r["groups_total"] == 1
    assert r["section_bytes_read"] == r["section_bytes_total"] and r["subframe"] == (0, 0, 8, 8)
    assert_is_crop(im, "one_dct8", box)


def test_a_modular_frame_is_decoded_whole_by_the_front_end():
    be = make_backend()
    fe = frontend.Frontend(sample("art"))
    fe.set_region((0, 0, 8, 8))
    fr = fe.next_frame(be.squeeze, be.rct)
    assert fr.encoding == 1 and fe.region_plan()["applied"] == 0


def _sanitizer_flags():
    return ["-O1", "-g", "-std=c++17", "-fwrapv", "-fopenmp", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined"]


def test_region_selection_is_clean_under_the_sanitizers(tmp_path):
    """tools/native/region_check.cpp over the front-end's sources, as a process of its own, on files written here: every box of A,
    B and D against the full decode, a margin of 0, and A cut right behind the last section a box needs"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path / "region_check")
    fdir = os.path.join(ROOT, "jxlatte_amd", "frontend")
    srcs = [os.path.join(ROOT, "tools", "native", "region_check.cpp")] + [os.path.join(fdir, f) for f in ("entropy.cc", "headers.cc", "modular.cc", "frame.cc", "api.cc")]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]
    cxx = os.environ.get("CXX", "g++")
    with ThreadPoolExecutor(len(srcs)) as ex:  # (one translation unit per core: the build is most of this test's time)
        list(ex.map(lambda so: subprocess.check_call([cxx] + _sanitizer_flags() + ["-c", so[0], "-o", so[1]]), zip(srcs, objs)))
    subprocess.check_call([cxx] + _sanitizer_flags() + ["-static-libasan", "-static-libubsan"] + objs + ["-o", exe])
    paths = {}
    for name in ("A", "B", "D"):
        paths[name] = str(tmp_path / (name + ".jxl"))
        with open(paths[name], "wb") as f:
            f.write(RC.encoded(name))
    paths["one_dct8"] = str(tmp_path / "one_dct8.jxl")
    with open(paths["one_dct8"], "wb") as f:
        f.write(C.encoded("one_dct8"))
    args, expect = [], []
    for name in ("A", "B", "D"):
        for box in RC.boxes(name):
            args += [paths[name]] + [str(v) for v in box]
            expect.append((1,) + RC.expected_reads(*RC.size(name), box, RC.margin(name)))
    args += [paths["one_dct8"], "1", "1", "4", "4", os.path.join(SAMPLES, "lenna.jxl"), "300", "300", "100", "100"]
    expect += [(0, 1, 1), (1, 1, 1)]
    first, lengths = sections_of_A()
    args += ["--margin", "0", paths["A"], "255", "255", "2", "2", "--cut", str(first + lengths[0]), paths["A"], "3", "3", "9", "9"]
    expect += [(1, 4, 1), (1, 1, 1)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert [(int(v[2]), int(v[3]), int(v[5])) for v in lines] == expect


# ---- the rule table ------------------------------------------------------------------------------------------------------------------
RULE = dict(art="not a VarDCT frame", quilt="not a VarDCT frame", blendmodes_5="the image has extra channels",
            **{"wb-rainbow": "the image has extra channels", "patches-lossless": "the image has extra channels"},
            white=None, lenna=None, bbb=None, bench=None)
WRITER_OK = ("one_dct8", "ragged_67x83", "groups_264x264", "two_lf_groups_2056x16", "passes_2", "lf_rough", "corr", "rgb", "noise_40x40",
             "noise_264x264", "noise_corr", "ycbcr_444", "opsin_custom", "opsin_custom_epf2", "epf3")
WRITER_RULE = dict(up2_19x15_of_37x29="not the image's only frame", up4_ragged="the frame is upsampled", up8_40x40="the frame is upsampled",
                   up2_custom_weights="the frame is upsampled", noise_up2="the frame is upsampled", noise_up2_of_271x39="not the image's only frame",
                   opsin_custom_up2="the frame is upsampled", alpha_40x40="the image has extra channels", alpha_264x264="the image has extra channels",
                   alpha_up2="the image has extra channels", s420="chroma subsampling", s422="chroma subsampling", s440="chroma subsampling")


def test_every_sample_has_a_row_in_the_rule_table():
    assert sorted(RULE) == sorted(f[:-4] for f in os.listdir(SAMPLES) if f.endswith(".jxl"))
    assert set(C.TAIL_CASES) <= set(WRITER_OK) | set(WRITER_RULE)


@pytest.mark.parametrize("name", sorted(RULE) + sorted(WRITER_RULE) + list(WRITER_OK))
def test_region_rule(name):
    want = RULE[name] if name in RULE else WRITER_RULE.get(name)
    be = make_backend()
    fe = frontend.Frontend(data_of(name))
    fr = fe.next_frame(be.squeeze, be.rct)
    assert JXLDecoder.region_rule(fe.image, fr) == want
    assert JXLDecoder.region_rule(fe.image, None) == (want if fe.image.num_extra else None)
    if want is not None:  # a refused decode raises before backend.vardct is called
        dec = JXLDecoder(data_of(name), backend=be, region=(0, 0, 4, 4))
        with pytest.raises(UnsupportedOperationException) as e:
            dec.decode()
        assert str(e.value) == "region: " + want and be.vardct_sizes == []


def test_region_rule_on_header_fields():
    info = types.SimpleNamespace(num_extra=0, width=40, height=24)
    ok = dict(encoding=0, type=0, lf_level=0, flags=0, is_last=1, x0=0, y0=0, width=40, height=24, upsampling=1, jpeg_up_y=[0, 0, 0],
              jpeg_up_x=[0, 0, 0], num_patches=0, has_splines=0, has_noise=0, do_ycbcr=0, blend_mode=0)

    def rule(**kw):
        return JXLDecoder.region_rule(info, types.SimpleNamespace(**dict(ok, **kw)))
    assert rule() is None and rule(has_noise=1, flags=1) is None and rule(do_ycbcr=1) is None and rule(flags=128) is None
    assert rule(encoding=1) == "not a VarDCT frame"
    for kw in (dict(type=1), dict(type=2), dict(type=3), dict(lf_level=1), dict(flags=32)):
        assert rule(**kw) == "not a regular frame of LF level 0 with LF coefficients of its own"
    for kw in (dict(is_last=0), dict(x0=8), dict(y0=-8), dict(width=32), dict(height=16), dict(blend_mode=2)):
        assert rule(**kw) == "not the image's only frame"
    assert rule(upsampling=2, width=20, height=12) == "the frame is upsampled"
    assert rule(jpeg_up_x=[1, 0, 1]) == rule(jpeg_up_y=[0, 0, 1]) == "chroma subsampling"
    assert rule(num_patches=2, flags=2) == "patches" and rule(has_splines=1, flags=16) == "splines"
    assert JXLDecoder.region_rule(types.SimpleNamespace(num_extra=1, width=40, height=24), types.SimpleNamespace(**ok)) == "the image has extra channels"


# ---- the samples ---------------------------------------------------------------------------------------------------------------------
def sample_boxes(name):
    h, w = full_decode(name)[0].shape
    return [(0, 0, 40, 30), (w // 2 - 20, h // 2 - 20, 40, 40), (236, min(200, h - 80), 40, 70)]  # a corner, the centre, over the group edge at x = 256


@pytest.mark.parametrize("name", FILES)
def test_samples(name):
    h, w = full_decode(name)[0].shape
    fe = frontend.Frontend(sample(name))
    fr = fe.next_frame()
    m = (1 if fr.gab else 0) + RC.EPF_REACH[fr.epf_iters]
    for box in sample_boxes(name):
        dec, im = region_decode(name, box)
        assert_is_crop(im, name, box)
        r = dec.stats[-1]["region"]
        assert (r["groups_read"], r["lf_groups_read"]) == RC.expected_reads(w, h, box, m, padded=(fr.padded_width, fr.padded_height))
        assert r["margin"] == m and r["groups_total"] == fr.num_groups
    assert RC.expected_reads(w, h, sample_boxes(name)[2], m)[0] >= 2


def test_the_sparse_feed_gives_the_same(monkeypatch):
    """sparse_coeffs reaches the backend as entry lists: this backend takes dense planes, so the lists are made dense on the way"""
    from jxlatte_amd import decoder as D
    box = RC.boxes("A")[1]
    asked = []
    real = D.JXLDecoder._vardct_inputs

    def inputs(self, fr, fuse_xyb, sub=None):
        p, weights, woffs, lfgroups, groups, hist = real(self, fr, fuse_xyb, sub)

        def dense(sparse=False):
            asked.append(sparse)
            for (pass_, grp, sp), (_, grp2, q) in zip(groups(True), groups(False)):
                assert grp == grp2
                out = [np.zeros(shape, np.int32) for _, _, shape in sp]
                for c, (e, wide, _) in enumerate(sp):
                    if wide:
                        pos, val = e[0::2], e[1::2].view(np.int32)
                    else:
                        pos, val = e & 0xffff, (e >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
                    out[c][pos >> 8, pos & 0xff] = val
                    assert np.array_equal(out[c], q[c])
                yield pass_, grp, out
        return p, weights, woffs, lfgroups, dense, hist
    monkeypatch.setattr(D.JXLDecoder, "_vardct_inputs", inputs)

    class Be(type(make_backend())):
        def vardct(self, params, weights, woffs, lfgroups, groups, sparse=False):
            return super().vardct(params, weights, woffs, lfgroups, groups)
    dec = JXLDecoder(RC.encoded("A"), backend=Be(), region=box, sparse_coeffs=True)
    assert_is_crop(dec.decode(), "A", box)
    assert asked == [True]


# ---- orientation ---------------------------------------------------------------------------------------------------------------------
def numpy_orient(a, o):
    """JXLCodestreamDecoder.transposeBuffer with numpy"""
    return {1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: a.T, 6: a[::-1].T, 7: a[::-1, ::-1].T, 8: a.T[::-1]}[o]


@pytest.mark.parametrize("o", range(1, 9))
def test_region_in_frame_against_numpy(o):
    H, W = 11, 17
    grid = np.arange(H * W).reshape(H, W)  # the frame: every pixel its own index
    delivered = numpy_orient(grid, o)
    info = types.SimpleNamespace(height=H, width=W, orientation=o)
    dh, dw = delivered.shape
    rng = np.random.default_rng(o)
    boxes = [(0, 0, dw, dh), (0, 0, 1, 1), (dw - 1, dh - 1, 1, 1)]
    for _ in range(40):
        x0, y0 = int(rng.integers(0, dw)), int(rng.integers(0, dh))
        boxes.append((x0, y0, int(rng.integers(1, dw - x0 + 1)), int(rng.integers(1, dh - y0 + 1))))
    for x0, y0, w, h in boxes:
        fx, fy, fw, fh = JXLDecoder.region_in_frame(info, (x0, y0, w, h))
        assert 0 <= fx and 0 <= fy and fx + fw <= W and fy + fh <= H
        # orienting the frame's box gives the delivered image's box
        assert np.array_equal(numpy_orient(grid[fy:fy + fh, fx:fx + fw], o), delivered[y0:y0 + h, x0:x0 + w])
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 1), (dw, 0, 1, 1), (0, 0, dw + 1, 1), (0, 0, 1, dh + 1), (0, dh - 1, 1, 2)):
        with pytest.raises(ValueError):
            JXLDecoder.region_in_frame(info, bad)


@pytest.mark.parametrize("o", [2, 5, 6, 8])
def test_an_oriented_image_end_to_end(o):
    """no file here carries an orientation: the image header's field is set on the decoder, for the full decode and for the region"""
    data = RC.encoded("D")
    full = JXLDecoder(data, backend=make_backend())
    full.info.orientation = o
    planes = full.decode().getBuffer(copy=False)
    box = (30, 3, 200, 100) if o < 5 else (3, 30, 100, 200)
    dec = JXLDecoder(data, backend=make_backend(), region=box)
    dec.info.orientation = o
    im = dec.decode()
    r = dec.stats[-1]["region"]
    assert r["box"] == box and r["frame_box"] == JXLDecoder.region_in_frame(dec.info, box) and r["frame_box"] != box
    for a, b in zip(im.getBuffer(copy=False), RC.crop(planes, box)):
        assert_bits_equal(a, b, "orientation %d" % o)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_up_front():
    data = sample("white")  # 320 x 240
    for bad in ((0, 0, 0, 10), (0, 0, 10, 0), (-1, 0, 10, 10), (0, -1, 10, 10), (311, 0, 10, 10), (0, 231, 10, 10), (0, 0, 321, 1),
                (0, 0, 10), (0, 0, 10, 10, 1), "0,0,10,10", (0.5, 0, 10, 10), 7):
        with pytest.raises(ValueError):
            JXLDecoder(data, backend=make_backend(), region=bad)
    for kw in (dict(downsample=8), dict(draw_varblocks=True), dict(device_canvas=True), dict(device_frames=True), dict(device_image=True)):
        with pytest.raises(ValueError):
            JXLDecoder(data, backend=make_backend(), region=(0, 0, 10, 10), **kw)
    dec = JXLDecoder(data, backend=make_backend(), region=(0, 0, 10, 10))
    dec.trace = lambda *a: None
    with pytest.raises(ValueError):
        dec.decode()
    assert JXLDecoder.region is None and JXLDecoder(data, backend=make_backend()).region is None
    assert JXLDecoder(data, backend=make_backend(), region=[np.int64(1), 2, 3, 4]).region == (1, 2, 3, 4)
    from oracle.pybackend import OracleBackend
    with pytest.raises(RuntimeError):  # noise on a region without `noise_window` is an error, never the window's own noise
        JXLDecoder(RC.encoded("E"), backend=OracleBackend(), region=(0, 0, 8, 8)).decode()


def test_without_the_switch_nothing_changes():
    for name in ("lenna", "bench"):
        a, b = JXLDecoder(sample(name), backend=make_backend()), JXLDecoder(sample(name), backend=make_backend(), region=None)
        ia, ib = a.decode(), b.decode()
        assert a.stats == b.stats and "region" not in a.stats[-1] and ia.region is None and ib.region is None
        assert a.fe.region_plan()["applied"] == 0
        assert_bits_equal(np.stack(ia.getBuffer(copy=False)), np.stack(ib.getBuffer(copy=False)), name)


def test_the_region_image_is_an_ordinary_image():
    """the writers and transform() take it as they take the crop of the full image"""
    box = sample_boxes("bbb")[1]
    dec, im = region_decode("bbb", box)
    ref = JXLImage([p.copy() for p in RC.crop(full_decode("bbb"), box)], dec.info, dec.backend)
    for writer in (PNGWriter, PFMWriter):
        a, b = io.BytesIO(), io.BytesIO()
        writer(im).write(a)
        writer(ref).write(b)
        assert a.getvalue() == b.getvalue() and len(a.getvalue()) > 100
    assert not im.onDevice() and im.getColorChannelCount() == 3 and not im.hasAlpha()


def test_the_cli_has_the_switch(monkeypatch, tmp_path, capsys):
    from jxlatte_amd import __main__ as cli
    from jxlatte_amd import decoder as D
    a = cli.parser().parse_args(["--region=3,4,50,60", "in.jxl", "out.png"])
    assert a.region == (3, 4, 50, 60) and cli.parser().parse_args(["in.jxl"]).region is None
    for bad in ("--region=1,2,3", "--region=a,b,c,d", "--region=1,2,3,4,5"):
        with pytest.raises(SystemExit):
            cli.parser().parse_args([bad, "in.jxl"])
    monkeypatch.setattr(D, "DeviceBackend", lambda device=0: make_backend())  # (no device here: the decoder's path is the same)
    out = str(tmp_path / "out.png")
    assert cli.main(["--region=236,100,40,70", os.path.join(SAMPLES, "lenna.jxl"), out]) == 0
    with open(out, "rb") as f:
        png = f.read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:24] == (40).to_bytes(4, "big") + (70).to_bytes(4, "big")
    assert "region: 2 of 4 groups read (groups)" in capsys.readouterr().err
    assert cli.main(["--region=0,0,8,8", os.path.join(SAMPLES, "art.jxl"), out]) == 2  # a frame that does not qualify
    assert "region: not a VarDCT frame" in capsys.readouterr().err
    assert cli.main(["--region=500,500,40,40", os.path.join(SAMPLES, "lenna.jxl"), out]) == 2  # not inside the image
    assert "not inside" in capsys.readouterr().err


def test_the_plan_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "layout.cpp"
    fields = [f for f, _ in frontend.RegionPlan._fields_]
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "jxlatte_frontend.h"\nint main() {\n    printf("%zu", sizeof(jxf_region_plan));\n' +
                   "".join('    printf(" %%zu", offsetof(jxf_region_plan, %s));\n' % f for f in fields) + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C_.sizeof(frontend.RegionPlan)] + [getattr(frontend.RegionPlan, f).offset for f in fields]
    assert C_.sizeof(frontend.RegionPlan) == 14 * 4 + 2 * 8 and len(fields) == 16


def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    i32, vp = C_.c_int32, C_.c_void_p
    for name in ("jxl_planes_from_frame_at", "jxl_planes_noise_at", "jxl_stage_noise_window"):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["jxl_planes_from_frame_at"] == (i32, [vp, i32, i32, i32, i32])
    fheader = open(os.path.join(ROOT, "include", "jxlatte_frontend.h")).read()
    flib = frontend.load()
    for name in ("jxf_set_region", "jxf_get_region_plan", "jxf_debug_set_region_margin"):
        assert re.search(r"int32_t\s+%s\s*\(" % name, fheader) and name in frontend.SIGNATURES and hasattr(flib, name)
    csrc = os.path.join(ROOT, "jxlatte_amd", "csrc")
    for f in ("k_noise_window.hip", "noise_window_host.hip", "noise_window_check.h", "noise_window.h", "noise_ops.h"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()  # no environment switch
    for f in ("frame.cc", "api.cc"):
        assert open(os.path.join(ROOT, "jxlatte_amd", "frontend", f)).read().count("getenv") == (1 if f == "frame.cc" else 0)  # (JXF_TIMING, as before)
    # synthesizeNoise's arithmetic has one statement: both kernels call it
    kernel, post, ops = (open(os.path.join(csrc, f)).read() for f in ("k_noise_window.hip", "k_post.hip", "noise_ops.h"))
    assert "noise_add_px(" in kernel and "noise_add_px(" in post and ops.count("0.21828125f") == 2
    assert "0.21828125f" not in kernel and "0.21828125f" not in post and "-3.84f" not in kernel
    assert kernel.count("hipLaunchKernelGGL") == 2 and "asm" not in kernel


# ---- the windowed noise validator ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("noise_window_check") / "noise_window_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "noise_window_check.cpp"), "-o", exe])
    return exe


def _run_noise_check(exe, rows=()):
    r = subprocess.run([exe] + [str(v) for row in rows for v in row], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    return r.stdout


def test_noise_window_validator_is_clean_under_the_sanitizers(noise_check_program):
    """the program's own table: the device tests' windows, every window of every frame up to 6 x 6, windows around group corners --
    each with both launches' index arithmetic replayed on allocations of the plan's sizes -- and the refusals"""
    _run_noise_check(noise_check_program)


def test_the_plan_of_noise_windows(noise_check_program):
    """PLAN of (group_dim, frame_h, frame_w, y0, x0, win_h, win_w) rows against the apron and group arithmetic made here"""
    rows = [(256, 264, 520, y0, x0, h, w) for x0, y0, w, h in RC.boxes("E")] + [(16, 37, 39, 14, 15, 3, 18), (256, 4000, 6000, 2046, 2047, 224, 224),
                                                                             (256, 264, 520, 0, 0, 265, 1), (256, 264, 520, 0, 519, 1, 2), (100, 64, 64, 0, 0, 8, 8)]
    lines = [ln.split() for ln in _run_noise_check(noise_check_program, rows).splitlines() if ln.startswith(("PLAN", "REFUSED"))]
    assert len(lines) == len(rows)
    for (gd, fh, fw, y0, x0, h, w), ln in zip(rows, lines):
        if y0 + h > fh or x0 + w > fw or gd & (gd - 1):
            assert ln[0] == "REFUSED"
            continue
        ay0, ax0, ay1, ax1 = max(0, y0 - 2), max(0, x0 - 2), min(fh, y0 + h + 2), min(fw, x0 + w + 2)
        gy0, gx0, gy1, gx1 = ay0 // gd, ax0 // gd, (ay1 - 1) // gd, (ax1 - 1) // gd
        want = [ay0, ax0, ay1 - ay0, ax1 - ax0, gy0, gx0, gy1 - gy0 + 1, gx1 - gx0 + 1, (gy1 - gy0 + 1) * (gx1 - gx0 + 1), (ay1 - ay0) * (ax1 - ax0), h * w]
        assert ln[0] == "PLAN" and [int(v) for v in ln[1:]] == want
