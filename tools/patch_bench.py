"""JXLCodestreamDecoder.computePatches: the default path (JXLDecoder._patches, one backend.blend call per position and channel on
the device backend) against the device stage (jxl_stage_patches, uploads and downloads included) and the kernel alone.

    python tools/patch_bench.py [--reps 3] [--kernel-reps 20] [--default-limit 400]

Cases:
  sample          the patch stage of tests/golden/samples/patches-lossless.jxl (1600 x 1096, 650 positions), cut out of a decode
  glyphs_4k       one synthetic 3840 x 2160 float frame, a glyph-dictionary reference, about 2 * 10^4 positions
  deep_overlap    512 x 512, 4000 positions stacked around a few spots
Per case it prints one JSON line:
  positions / tiles / list_entries  the table and its binning
  evals                             pixel x position evaluations (the sum of the applied rectangles' areas)
  default_ms                        wall clock of _patches on the device backend; with more than --default-limit positions it is
                                    measured on the first --default-limit positions and scaled (default_scaled: true)
  device_ms                         wall clock of the plan + jxl_stage_patches, median of --reps after one warm-up
  kernel_ms                         the kernel alone, stream events over --kernel-reps launches
  kernel_evals_per_s
  identical                         the device result equals the default path's bit for bit (only where the default ran in full)
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jxlatte_amd import _lib, abi, decoder, host  # noqa: E402

F = np.float32


def _info(n_extra):
    return types.SimpleNamespace(colour_space=decoder.CE_RGB, num_extra=n_extra, ec_type=[0] * n_extra, ec_alpha_associated=[0] * n_extra,
                                 bits_per_sample=8, ec_bits=[8] * n_extra)


def _patch(ref, y0, x0, h, w, positions, row):
    return dict(ref=ref, y0=y0, x0=x0, h=h, w=w, positions=np.asarray(positions, np.int32).reshape(-1, 2),
                blend=np.asarray([row] * len(positions), np.int32).reshape(len(positions), -1, 3))


def glyphs(h=2160, w=3840, n=20000):
    rng = np.random.default_rng(1)
    frame = [rng.uniform(0, 1, (h, w)).astype(F) for _ in range(3)]
    ref = [rng.uniform(-0.1, 0.1, (256, 1024)).astype(F) for _ in range(3)]
    patches = []
    for g in range(96):  # 96 glyphs of about 12 x 20 in a 256 x 1024 dictionary
        gh, gw = int(rng.integers(8, 17)), int(rng.integers(10, 25))
        k = n // 96
        pos = np.stack([rng.integers(0, h - gh, k), rng.integers(0, w - gw, k)], axis=1)
        patches.append(_patch(0, (g // 32) * 32, (g % 32) * 32, gh, gw, pos, [[2, 0, 0]]))
    return _info(0), patches, frame, [ref, None, None, None]


def deep(h=512, w=512, n=4000):
    rng = np.random.default_rng(2)
    frame = [rng.uniform(0, 1, (h, w)).astype(F) for _ in range(3)]
    ref = [rng.uniform(-0.01, 0.01, (64, 64)).astype(F) for _ in range(3)]
    spots = rng.integers(40, h - 100, (8, 2))
    pos = spots[rng.integers(0, 8, n)] + rng.integers(-6, 7, (n, 2))
    return _info(0), [_patch(0, 0, 0, 48, 48, pos, [[2, 0, 0]])], frame, [ref, None, None, None]


def sample(backend):
    """the inputs of the sample's patch stage, captured in a default decode"""
    dec = decoder.JXLDecoder(os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl"), backend=backend)
    got = {}
    inner = dec._patches

    def capture(fr, bufs, colors):
        got["patches"] = [dec.fe.patch(i) for i in range(fr.num_patches)]
        got["frame"] = [b.copy() for b in bufs]
        got["ref"] = [None if r is None else [None if a is None else a.copy() for a in r] for r in dec.reference]
        inner(fr, bufs, colors)
    dec._patches = capture
    dec.decode()
    return dec.info, got["patches"], got["frame"], got["ref"]


def shell(info, patches, reference, backend):
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.info, dec.reference, dec.backend, dec.stats = info, reference, backend, [{}]
    dec.fe = types.SimpleNamespace(patch=lambda i: patches[i])
    return dec


def copy_ref(reference):
    return [None if r is None else [None if a is None else a.copy() for a in r] for r in reference]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--default-limit", type=int, default=400)
    a = ap.parse_args()
    be = decoder.DeviceBackend()
    ctx = be.ctx
    fn = ctx.lib.jxl_debug_patch_kernel_ms
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(abi.PatchDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                   C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    for name, make in (("sample", lambda: sample(be)), ("glyphs_4k", glyphs), ("deep_overlap", deep)):
        info, patches, frame, reference = make()
        n_chan = len(frame)
        n_pos = sum(p["positions"].shape[0] for p in patches)
        evals = sum(p["positions"].shape[0] * p["h"] * p["w"] for p in patches if reference[p["ref"]] is not None)
        rec = types.SimpleNamespace(num_patches=len(patches), upsampling=1, ec_upsampling=[])

        def device():
            fb, ref = [b.copy() for b in frame], copy_ref(reference)
            dec = shell(info, patches, ref, types.SimpleNamespace(patches=be.patches))  # (the stage entry: no resident planes)
            t0 = time.perf_counter()
            assert dec._patches_device(rec, decoder.FramePlanes(dec.backend, info, fb, 3))
            return (time.perf_counter() - t0) * 1e3, fb, dec.stats[-1]["patches"]
        device()
        runs = [device() for _ in range(a.reps)]
        dev = runs[-1][1]
        # the default path, in full or on a prefix of the positions
        scaled = n_pos > a.default_limit
        sub, left = [], a.default_limit
        for p in patches:
            k = p["positions"].shape[0] if not scaled else min(left, p["positions"].shape[0])
            if k > 0:
                sub.append(dict(p, positions=p["positions"][:k], blend=p["blend"][:k]))
            left -= k
        fb, ref = [b.copy() for b in frame], copy_ref(reference)
        dec = shell(info, sub, ref, be)
        t0 = time.perf_counter()
        dec._patches(types.SimpleNamespace(num_patches=len(sub), upsampling=1, ec_upsampling=[]), fb, 3)
        default_ms = (time.perf_counter() - t0) * 1e3 * (n_pos / min(n_pos, a.default_limit) if scaled else 1.0)
        # the kernel alone, on planes of the plan's types
        plan = decoder.patch_type_plan(info, patches, frame, reference, 3)
        kf = [b if b.dtype == plan.frame_types[n] else dec._to_float(b, 8) for n, b in enumerate(frame)]
        kr = [None if r is None else [None if x is None else (x if x.dtype == np.float32 or plan.ref_types.get(k, [None] * n_chan)[n] != np.float32
                                                               else dec._to_float(x, 8)) for n, x in enumerate(r)] for k, r in enumerate(reference)]
        kf = [np.ascontiguousarray(b) for b in kf]
        ft = np.array([host._patch_type(b) for b in kf], np.int32)
        desc, pp, rt, keep = host._patch_call_args(ft, n_chan, kr, plan.pos, plan.blend, 3, [True] * info.num_extra, [False] * info.num_extra)
        fp = (C.c_void_p * n_chan)(*[host._vp(b) for b in kf])
        ms, counts = C.c_float(), (C.c_int64 * 3)()
        _lib.check(ctx.h, fn(ctx.h, C.byref(desc), fp, abi.iptr(ft), kf[0].shape[0], kf[0].shape[1], pp, abi.iptr(rt), a.kernel_reps, C.byref(ms), counts))
        row = dict(case=name, size="%dx%d" % (frame[0].shape[1], frame[0].shape[0]), channels=n_chan, positions=n_pos, tiles=int(counts[1]),
                   list_entries=int(counts[2]), evals=evals, segments=runs[-1][2]["segments"], default_ms=round(default_ms, 1), default_scaled=scaled,
                   device_ms=round(statistics.median(r[0] for r in runs), 2), kernel_ms=round(ms.value, 4),
                   kernel_evals_per_s=round(evals / (ms.value * 1e-3)) if ms.value > 0 else None)
        if not scaled:
            row["identical"] = all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(dev, fb))
        print(json.dumps(row), flush=True)
    be.close()


if __name__ == "__main__":
    main()
