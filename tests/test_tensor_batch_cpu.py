"""The batched resized tensor exit without a GPU: jxlatte_amd/csrc/tensor_batch_check.h as a stand-alone host program under
AddressSanitizer + UBSan (tools/native/tensor_batch_check.cpp); the ctypes mirror of jxl_tensor_batch_item against the C layout;
declarations and bindings; decoder.toTensorBatch over a fake backend, and JXLImage.toTensor's calls beside it."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import CE_GRAY, CE_RGB, PRI_SRGB, TF_SRGB, WP_D65, JXLImage, toTensorBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_check") / "tensor_batch_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "tensor_batch_check.cpp"), "-o", exe])
    return exe


def _run(exe, quads=()):
    args = [str(v) for q in quads for v in q]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    return r.stdout


def test_check_program_is_clean_under_the_sanitizers(program):
    """the program's own table: every batch-level refusal, the agreement rules, the offsets in 64 bits, table sharing, the prefix
    sums with their cap, the search, the LDS maximum, the grid"""
    _run(program)


def test_work_list_of_the_gpu_tests_batches(program):
    """tile_base of (oh, ow, tw, th) items as the program builds it, against the sums made here"""
    quads = [(2, 5, 8, 2), (2, 5, 8, 1), (13, 11, 8, 4), (1, 1, 64, 4), (224, 224, 32, 4), (13, 11, 1, 1)]
    tiles = [-(-ow // tw) * -(-oh // th) for oh, ow, tw, th in quads]
    assert tiles == [1, 2, 8, 1, 392, 143]
    line = [ln for ln in _run(program, quads).splitlines() if ln.startswith("BASE")]
    assert len(line) == 1
    assert [int(v) for v in line[0].split()[1:]] == [len(quads)] + [sum(tiles[:k]) for k in range(len(quads) + 1)]


def test_item_struct_has_the_c_layout(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "jxlatte_amd.h"\nint main() {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jxl_tensor_batch_item), offsetof(jxl_tensor_batch_item, source),\n'
                   '           offsetof(jxl_tensor_batch_item, set_id), offsetof(jxl_tensor_batch_item, alpha_plane), offsetof(jxl_tensor_batch_item, in),\n'
                   '           offsetof(jxl_tensor_batch_item, alpha), offsetof(jxl_tensor_batch_item, p), offsetof(jxl_tensor_batch_item, r));\n'
                   '    printf("%d %d %d %d\\n", JXL_TENSOR_BATCH_MAX, JXL_BATCH_HOST, JXL_BATCH_RESIDENT, JXL_BATCH_SET);\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    T = abi.TensorBatchItem
    assert [int(v) for v in out[0].split()] == [C.sizeof(T), T.source.offset, T.set_id.offset, T.alpha_plane.offset, T.in_.offset, T.alpha.offset,
                                                T.p.offset, T.r.offset]
    assert [int(v) for v in out[1].split()] == [abi.TENSOR_BATCH_MAX, abi.BATCH_HOST, abi.BATCH_RESIDENT, abi.BATCH_SET]
    assert abi.TENSOR_BATCH_MAX >= 256


def test_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    lib = _lib.load()
    assert re.search(r"jxl_status\s+jxl_tensor_resized_batch\s*\(", header)
    assert "jxl_tensor_resized_batch" in _lib.SIGNATURES and hasattr(lib, "jxl_tensor_resized_batch")
    for hook in ("jxl_debug_tensor_batch_grid", "jxl_debug_tensor_batch_stats"):
        assert hasattr(lib, hook) and hook not in header
    for f in ("k_tensor_resize_batch.hip", "tensor_batch_host.hip", "tensor_batch_check.h", "tensor_resize_body.h"):
        assert "getenv" not in open(os.path.join(ROOT, "jxlatte_amd", "csrc", f)).read()
    # the tile body exists once: both kernels call it, neither restates it
    csrc = os.path.join(ROOT, "jxlatte_amd", "csrc")
    for f in ("k_tensor_resize.hip", "k_tensor_resize_batch.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "resize_tile<BYTES, COLORS>(" in text and "color_front" not in text and "__syncthreads" not in text
    assert open(os.path.join(csrc, "tensor_resize_body.h")).read().count("color_front<COLORS>(") == 1


def test_batch_item_binding():
    rng = np.random.default_rng(1)
    planes = [rng.uniform(0, 1, (9, 20)).astype(F) for _ in range(3)]
    alpha = rng.integers(0, 1024, (9, 20)).astype(np.int32)
    it = host.tensorBatchItem((4, 6), (3, 2, 5, 4), "box", planes=planes, alpha=alpha, writeAlpha=True, alphaDepth=10, dtype="float16", layout="HWC")
    assert (it.source, it.set_id, it.alpha_plane) == (abi.BATCH_HOST, -1, -1)
    assert list(it.in_) == [p.ctypes.data for p in planes] and it.alpha == alpha.ctypes.data
    assert bytes(it.p) == bytes(host.tensorParams(planes, (9, 20), alpha=alpha, writeAlpha=True, alphaDepth=10, dtype="float16", layout="HWC"))
    assert bytes(it.r) == bytes(host.resizeParams((9, 20), (4, 6), (3, 2, 5, 4), "box"))
    grey = host.tensorBatchItem((4, 6), planes=planes[:1])
    assert list(grey.in_) == [planes[0].ctypes.data, None, None] and grey.alpha is None and grey.p.color.n_planes == 1
    canvas = types.SimpleNamespace(id=7, shape=(9, 20), types=[abi.PLANE_FLOAT] * 3 + [abi.PLANE_INT32], _live=lambda: None)
    canvas._stand_ins = lambda n: [np.broadcast_to(np.zeros((), F), canvas.shape)] * n
    it = host.tensorBatchItem((4, 6), canvas=canvas, nColor=3, alphaPlane=3, premultiplied=True)
    assert (it.source, it.set_id, it.alpha_plane) == (abi.BATCH_SET, 7, 3) and list(it.in_) == [None] * 3 and it.alpha is None
    assert (it.p.has_alpha, it.p.alpha_is_int, it.p.height, it.p.width) == (1, 1, 9, 20)
    for bad in (dict(), dict(planes=planes, canvas=canvas)):
        with pytest.raises(ValueError):
            host.tensorBatchItem((4, 6), **bad)


# ---- toTensorBatch over a fake backend ----
def _info(grey=False, n_extra=0, ec_bits=()):
    return types.SimpleNamespace(colour_space=CE_GRAY if grey else CE_RGB, num_extra=n_extra, ec_type=[0] * n_extra, ec_alpha_associated=[0] * n_extra,
                                 ec_bits=list(ec_bits), prim_xy=list(PRI_SRGB), white_xy=list(WP_D65), transfer=TF_SRGB, xyb_encoded=False,
                                 bits_per_sample=8, use_icc=False)


def _fake(calls):
    def tensor_samples(planes, alpha, out_ptr, **kw):
        calls.append(("samples", planes, alpha, out_ptr, kw))

    def tensor_resized(planes, alpha, out_ptr, size, box, resample, **kw):
        calls.append(("resized", planes, alpha, out_ptr, size, box, resample, kw))

    def tensor_resized_batch(items, out_ptr):
        calls.append(("batch", items, out_ptr))

    def color_peak(planes, **kw):
        calls.append(("peak", planes, kw))
        return F(1)
    return types.SimpleNamespace(tensor_samples=tensor_samples, tensor_resized=tensor_resized, tensor_resized_batch=tensor_resized_batch,
                                 tensor_device=lambda: "cpu", color_peak=color_peak)


def _image(be, shape=(9, 20), seed=3, grey=False, alpha=False):
    rng = np.random.default_rng(seed)
    planes = [rng.integers(0, 256, shape).astype(np.int32) for _ in range((1 if grey else 3) + alpha)]
    return JXLImage(planes, _info(grey, int(alpha), [8] * int(alpha)), be), planes


def test_batch_refuses_bad_arguments_before_any_backend_call():
    calls = []
    be = _fake(calls)
    (a, _), (b, _), (g, _) = _image(be), _image(be, (5, 7), 4), _image(be, (5, 7), 5, grey=True)
    other, _ = _image(_fake(calls))
    bad = [
        dict(images=[]), dict(images=[a, other]), dict(images=[a, g]), dict(images=[a, "x"]),
        dict(size=None), dict(size=(0, 4)), dict(size=(4, -1)), dict(size=4), dict(size=(4,)), dict(size=(4.5, 4)),
        dict(boxes=[None]), dict(boxes=[None, None, None]), dict(boxes=[None, (0, 0, 8, 5)]), dict(boxes=[(17, 0, 4, 4), None]), dict(boxes=[(0, 0, 4), None]),
        dict(resample="lanczos"), dict(dtype=torch.int32), dict(layout="NCHW"), dict(target="rec2020"), dict(alpha="keep"), dict(alpha="append"),
        dict(mean=[0.5] * 3), dict(mean=[0.5] * 3, std=[0.5] * 2), dict(mean=[0.5] * 3, std=[0.5, 0.0, 0.5]), dict(dtype=torch.uint8, mean=[0.5] * 3, std=[0.5] * 3),
        dict(out=torch.zeros((3, 4, 6))), dict(out=torch.zeros((2, 3, 4, 6), dtype=torch.float16)), dict(out=torch.zeros((3, 3, 4, 6))),
        dict(out=torch.zeros((2, 3, 6, 4)).permute(0, 1, 3, 2)), dict(layout="HWC", out=torch.zeros((2, 3, 4, 6))),
    ]
    for kw in bad:
        kw = dict(dict(images=[a, b], size=(4, 6)), **kw)
        with pytest.raises(ValueError):
            toTensorBatch(kw.pop("images"), kw.pop("size"), **kw)
    assert calls == []
    be2 = _fake(calls)
    del be2.tensor_resized_batch
    with pytest.raises(TypeError):
        toTensorBatch([_image(be2)[0]], (4, 6))
    assert calls == []


def test_batch_shapes_items_and_the_out_rule():
    calls = []
    be = _fake(calls)
    (a, pa), (b, pb) = _image(be), _image(be, (5, 7), 4)
    t = toTensorBatch([a, b, a], (4, 6), boxes=[None, (1, 0, 5, 4), (3, 2, 5, 4)])
    assert t.shape == (3, 3, 4, 6) and t.dtype == torch.float32 and [c[0] for c in calls] == ["batch"]
    items, ptr = calls[0][1], calls[0][2]
    assert ptr == t.data_ptr() and len(items) == 3
    assert [(it["size"], it["box"], it["resample"]) for it in items] == [((4, 6), (0, 0, 20, 9), "triangle"), ((4, 6), (1, 0, 5, 4), "triangle"),
                                                                        ((4, 6), (3, 2, 5, 4), "triangle")]
    assert all(x is y for x, y in zip(items[0]["planes"], pa)) and all(x is y for x, y in zip(items[1]["planes"], pb))
    assert all(it["dtype"] == "float32" and it["layout"] == "CHW" and it["inMax"] == [255] * 3 and it["alpha"] is None for it in items)
    assert a.tensor_bus_bytes == (3 * 9 * 20 * 4, 0) and b.tensor_bus_bytes == (3 * 5 * 7 * 4, 0)
    assert t.bus_bytes == (2 * 3 * 9 * 20 * 4 + 3 * 5 * 7 * 4, 0)
    del calls[:]
    t = toTensorBatch([b, a], (2, 5), dtype=torch.uint8, layout="HWC", resample="box")
    assert t.shape == (2, 2, 5, 3) and t.dtype == torch.uint8 and calls[0][1][0]["resample"] == "box" and calls[0][1][1]["layout"] == "HWC"
    del calls[:]
    big = torch.zeros((5, 3, 8, 8), dtype=torch.float16)
    t = toTensorBatch([a, b], (8, 8), dtype=torch.float16, out=big[2:4], mean=[0.5, 0.4, 0.3], std=[0.25, 0.5, 2.0])
    assert t.data_ptr() == big[2].data_ptr() == calls[0][2] and t.shape == (2, 3, 8, 8)
    assert calls[0][1][1]["mean"] == [0.5, 0.4, 0.3] and calls[0][1][1]["invStd"] == [F(4), F(2), F(0.5)]
    # grey images make a batch of their own; alpha appended on images that have one
    del calls[:]
    (g, _), (h, _) = _image(be, (5, 7), 5, grey=True), _image(be, (9, 20), 6, grey=True)
    assert toTensorBatch([g, h], (4, 6)).shape == (2, 1, 4, 6) and len(calls[0][1][0]["planes"]) == 1
    del calls[:]
    (x, px), (y, py) = _image(be, (5, 7), 7, alpha=True), _image(be, (9, 20), 8, alpha=True)
    t = toTensorBatch([x, y], (4, 6), alpha="append", layout="HWC")
    assert t.shape == (2, 4, 6, 4) and [c[0] for c in calls] == ["batch"]
    assert all(it["writeAlpha"] and it["alphaDepth"] == 8 for it in calls[0][1]) and np.array_equal(calls[0][1][0]["alpha"], px[3])
    assert x.tensor_bus_bytes == (4 * 5 * 7 * 4, 0)
    with pytest.raises(ValueError):
        toTensorBatch([x, _image(be)[0]], (4, 6), alpha="append")  # one image has no alpha to append


def test_each_image_gets_the_plan_to_tensor_builds_for_it():
    """per image, the keywords of the batch item are those of the image's own toTensor(size=) call; toTensor still issues exactly
    one tensor_resized (one tensor_samples without size and box) and never the batch entry"""
    calls = []
    be = _fake(calls)
    images = [_image(be)[0], _image(be, (5, 7), 4)[0], _image(be, (9, 20), 9, alpha=True)[0]]
    for kwargs in (dict(), dict(dtype=torch.float16, layout="HWC", target="linear"), dict(target="as-is", resample="box"), dict(target="pq", peakDetect=True)):
        del calls[:]
        toTensorBatch(images, (4, 6), boxes=[None, (1, 0, 5, 4), None], **kwargs)
        peaks = [c for c in calls if c[0] == "peak"]
        assert len(peaks) <= len(images) and [c[0] for c in calls if c[0] != "peak"] == ["batch"]
        items = [c for c in calls if c[0] == "batch"][0][1]
        for im, box, it in zip(images, [None, (1, 0, 5, 4), None], items):
            del calls[:]
            im.toTensor(size=(4, 6), box=box, **kwargs)
            rest = [c for c in calls if c[0] != "peak"]
            assert [c[0] for c in rest] == ["resized"] and len(calls) - 1 <= 1
            _, planes, alpha, _, size, bx, resample, kw = rest[0]
            assert (it["size"], it["box"], it["resample"]) == (size, bx, resample)
            assert len(it["planes"]) == len(planes) and all(np.array_equal(p, q) for p, q in zip(it["planes"], planes))
            assert (it["alpha"] is None) == (alpha is None) and (alpha is None or np.array_equal(it["alpha"], alpha))
            mine = {k: v for k, v in it.items() if k not in ("size", "box", "resample", "planes", "alpha")}
            assert sorted(mine) == sorted(kw)
            for k in kw:
                assert np.array_equal(np.asarray(mine[k], dtype=object), np.asarray(kw[k], dtype=object)) if isinstance(kw[k], (list, tuple, np.ndarray)) else mine[k] == kw[k], k
    del calls[:]
    images[0].toTensor()
    assert [c[0] for c in calls] == ["samples"]
