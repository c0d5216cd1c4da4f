"""The resized tensor exit without a GPU: jxlatte_amd/csrc/tensor_resize_check.h as a stand-alone host program under
AddressSanitizer + UBSan (tools/native/tensor_resize_check.cpp), its tap tables bit for bit against the numpy model of
tests/resize_ref.py; the model against Pillow's resize of mode-F images within a derived bound; declarations and bindings;
JXLImage.toTensor(size=, box=, resample=) over a fake backend."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import resize_ref as rr
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import CE_RGB, PRI_SRGB, TF_SRGB, WP_D65, JXLImage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# source (h, w) -> output (h, w) of the GPU tests' shapes, and the boxed lengths (9 -> 6, 20 -> 4)
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 7), (2, 3)), ((5, 7), (13, 11)), ((33, 67), (8, 5)), ((64, 48), (4, 3)),
          ((3, 2100), (2, 5)), ((67, 33), (67, 33)), ((9, 20), (6, 4)), ((33, 67), (30, 60))]
AXES = sorted({(s[0], o[0]) for s, o in SHAPES} | {(s[1], o[1]) for s, o in SHAPES})


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize_check") / "tensor_resize_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "tensor_resize_check.cpp"), "-o", exe])
    return exe


def _run(exe, triples=()):
    args = [str(v) for t in triples for v in t]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    return r.stdout


def test_check_program_is_clean_under_the_sanitizers(program):
    """every refusal of the pure check, the cap, the tile picker and the load rule: the program's own table"""
    _run(program)


def test_tables_equal_the_model_bit_for_bit(program):
    triples = [(L, O, f) for L, O in AXES for f in (rr.TRIANGLE, rr.BOX)]
    lines = iter(_run(program, triples).splitlines())
    seen = 0
    for line in lines:
        if not line.startswith("TAPS"):
            continue
        _, L, O, f, total = line.split()
        model = rr.taps(int(L), int(O), int(f))
        n = 0
        for o in range(int(O)):
            row = next(lines).split()
            assert row[0] == "T"
            first, count = int(row[1]), int(row[2])
            bits = np.array([int(v, 16) for v in row[3:]], np.uint32)
            assert (first, count) == (model[o][0], len(model[o][1])), (L, O, f, o)
            assert np.array_equal(bits, model[o][1].view(np.uint32)), (L, O, f, o)
            assert 0 <= first and first + count <= int(L)
            n += count
        assert n == int(total)
        seen += 1
    assert seen == len(triples)


def test_refused_axes_are_reported(program):
    out = _run(program, [(2100, 3, rr.TRIANGLE), (2100, 2, rr.BOX)])
    assert out.count("refused: tensor resized: more than 1024 taps") == 2


@pytest.mark.parametrize("filt", [rr.TRIANGLE, rr.BOX])
def test_identity_is_one_tap_of_weight_one(filt):
    for n in (1, 33, 67):
        for o, (first, w) in enumerate(rr.taps(n, n, filt)):
            assert first == o and w.tolist() == [1.0]
    rng = np.random.default_rng(5)
    plane = rng.normal(0, 1, (67, 33)).astype(F)
    out = rr.resample(plane, rr.taps(67, 67, filt), rr.taps(33, 33, filt))
    assert np.array_equal(out.view(np.uint32), plane.view(np.uint32))


def test_model_matches_pillow_within_the_derived_bound():
    """|model - Pillow| <= K u (A + |model|), u = 2^-24, A the model on |plane|, K = ny + nx + 4: one product and one sum per tap
    and pass, the weight's rounding, and the rounding of the witness (Pillow keeps float64 weights and a float64 accumulator per
    pass, rounded to f32 between the passes). Prints the measured multiple of u (A + |model|) per case."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(21)
    u = 2.0 ** -24
    worst = 0.0
    for (h, w), (oh, ow) in SHAPES:
        plane = rng.normal(0.3, 1.0, (h, w)).astype(F)
        for filt, pil in ((rr.TRIANGLE, Image.BILINEAR), (rr.BOX, Image.BOX)):
            ty, tx = rr.taps(h, oh, filt), rr.taps(w, ow, filt)
            model = rr.resample(plane, ty, tx).astype(np.float64)
            A = rr.resample(np.abs(plane), ty, tx).astype(np.float64)
            witness = np.asarray(Image.fromarray(plane).resize((ow, oh), pil), F).astype(np.float64)
            K = max(len(t[1]) for t in ty) + max(len(t[1]) for t in tx) + 4
            ratio = float(np.max(np.abs(model - witness) / (u * (A + np.abs(model)))))
            worst = max(worst, ratio)
            print("%dx%d -> %dx%d filter %d: %.2f u (A + |v|), K = %d" % (h, w, oh, ow, filt, ratio, K))
            assert ratio <= K, ((h, w), (oh, ow), filt, ratio, K)
    print("worst: %.2f" % worst)


def test_model_against_torch_antialiased_bilinear_is_recorded():
    """not asserted beyond sanity: torch forms its weights in f32. The figure is printed for DESIGN's table"""
    rng = np.random.default_rng(22)
    plane = rng.uniform(0, 1, (33, 67)).astype(F)
    model = rr.resample(plane, rr.taps(33, 8, rr.TRIANGLE), rr.taps(67, 5, rr.TRIANGLE))
    other = torch.nn.functional.interpolate(torch.from_numpy(plane)[None, None], size=(8, 5), mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
    A = rr.resample(np.abs(plane), rr.taps(33, 8, rr.TRIANGLE), rr.taps(67, 5, rr.TRIANGLE))
    ratio = float(np.max(np.abs(model.astype(np.float64) - other) / (2.0 ** -24 * A)))
    print("torch antialiased bilinear 33x67 -> 8x5: %.1f u A" % ratio)
    assert ratio < 1e4  # the same filter, not the same roundings


# ---- declarations, bindings ----
def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    for name in ("jxl_stage_tensor_resized", "jxl_planes_tensor_resized", "jxl_canvas_tensor_resized"):
        assert re.search(r"jxl_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert hasattr(lib, "jxl_debug_tensor_resize_tile") and "jxl_debug_tensor_resize_tile" not in header
    for name, value in (("TRIANGLE", 0), ("BOX", 1)):
        assert re.search(r"#define\s+JXL_RESIZE_%s\s+%d\b" % (name, value), header) and getattr(abi, "RESIZE_" + name) == value
    assert C.sizeof(abi.ResizeParams) == 28 and abi.ResizeParams.out_height.offset == 16 and abi.ResizeParams.filter.offset == 24
    r = host.resizeParams((33, 67), (8, 5))
    assert (r.box_x0, r.box_y0, r.box_width, r.box_height, r.out_height, r.out_width, r.filter) == (0, 0, 67, 33, 8, 5, 0)
    r = host.resizeParams((33, 67), (6, 4), box=(3, 2, 20, 9), resample="box")
    assert (r.box_x0, r.box_y0, r.box_width, r.box_height, r.out_height, r.out_width, r.filter) == (3, 2, 20, 9, 6, 4, 1)
    for f in ("k_tensor_resize.hip", "tensor_resize_host.hip", "tensor_resize_check.h"):
        assert "getenv" not in open(os.path.join(ROOT, "jxlatte_amd", "csrc", f)).read()


# ---- toTensor over a fake backend ----
def _info(n_extra=0, ec_bits=()):
    return types.SimpleNamespace(colour_space=CE_RGB, num_extra=n_extra, ec_type=[0] * n_extra, ec_alpha_associated=[0] * n_extra,
                                 ec_bits=list(ec_bits), prim_xy=list(PRI_SRGB), white_xy=list(WP_D65), transfer=TF_SRGB, xyb_encoded=False,
                                 bits_per_sample=8, use_icc=False)


def _fake(calls, resized=True):
    def tensor_samples(planes, alpha, out_ptr, **kw):
        calls.append(("samples", planes, alpha, out_ptr, kw))

    def tensor_resized(planes, alpha, out_ptr, size, box, resample, **kw):
        calls.append(("resized", planes, alpha, out_ptr, size, box, resample, kw))
    be = types.SimpleNamespace(tensor_samples=tensor_samples, tensor_device=lambda: "cpu", color_peak=lambda planes, **kw: F(1))
    if resized:
        be.tensor_resized = tensor_resized
    return be


def _image(calls, resized=True):
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (9, 20)).astype(np.int32) for _ in range(3)]
    return JXLImage(planes, _info(), _fake(calls, resized)), planes


def test_to_tensor_refuses_bad_resize_arguments_before_any_backend_call():
    calls = []
    im, _ = _image(calls)
    bad = [
        dict(size=(0, 4)), dict(size=(4, -1)), dict(size=4), dict(size=(4,)), dict(size=(4, 4, 4)), dict(size=(4.5, 4)), dict(size=("a", 4)),
        dict(box=(0, 0, 21, 9)), dict(box=(0, 0, 20, 10)), dict(box=(-1, 0, 4, 4)), dict(box=(0, -1, 4, 4)), dict(box=(0, 0, 0, 4)),
        dict(box=(0, 0, 4, 0)), dict(box=(17, 0, 4, 4)), dict(box=(0, 6, 4, 4)), dict(box=(0, 0, 4)), dict(box=(0.5, 0, 4, 4)), dict(box=7),
        dict(size=(4, 4), resample="lanczos"), dict(size=(4, 4), resample=0), dict(resample="cubic"),
        dict(size=(4, 4), out=torch.zeros((3, 9, 20))), dict(box=(1, 1, 4, 5), out=torch.zeros((3, 4, 5))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            im.toTensor(**kw)
    assert calls == []
    im, _ = _image(calls, resized=False)
    with pytest.raises(TypeError):
        im.toTensor(size=(4, 4))
    assert calls == []


def test_to_tensor_with_defaults_takes_the_unresized_path():
    calls = []
    im, planes = _image(calls)
    t = im.toTensor()
    assert [c[0] for c in calls] == ["samples"] and t.shape == (3, 9, 20) and "resize" not in calls[0][4]
    del calls[:]
    im.toTensor(resample="box")  # (no size, no box: nothing to resample)
    assert [c[0] for c in calls] == ["samples"]


def test_to_tensor_resized_shapes_and_the_out_rule():
    calls = []
    im, planes = _image(calls)
    t = im.toTensor(size=(4, 6))
    assert t.shape == (3, 4, 6) and len(calls) == 1
    kind, pl, a, ptr, size, box, resample, kw = calls[0]
    assert kind == "resized" and size == (4, 6) and box == (0, 0, 20, 9) and resample == "triangle" and ptr == t.data_ptr()
    assert all(x is y for x, y in zip(pl, planes)) and kw["dtype"] == "float32" and kw["inMax"] == [255] * 3
    assert im.tensor_bus_bytes == (3 * 9 * 20 * 4, 0)
    del calls[:]
    t = im.toTensor(torch.uint8, "HWC", box=(3, 2, 5, 4), resample="box")  # a crop: the box's own size
    assert t.shape == (4, 5, 3) and calls[0][4] == (4, 5) and calls[0][5] == (3, 2, 5, 4) and calls[0][6] == "box"
    del calls[:]
    batch = torch.zeros((2, 3, 8, 8), dtype=torch.float16)
    t = im.toTensor(torch.float16, size=(8, 8), box=(1, 1, 10, 7), out=batch[1])
    assert t.data_ptr() == batch[1].data_ptr() == calls[0][3] and calls[0][4] == (8, 8) and calls[0][5] == (1, 1, 10, 7)
    with pytest.raises(ValueError):
        im.toTensor(torch.float16, size=(8, 8), out=batch[:, 0])  # not the tensor's shape
    assert len(calls) == 1
