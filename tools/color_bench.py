"""Colour management of one 3840x2160 three-plane image on the way into an 8-bit sRGB PNG: the host path of JXLImage.transform
(numpy, one plane and one stage at a time) against the device path (jxl_stage_color_peak + jxl_stage_color_convert), and the
two kernels alone.

    python tools/color_bench.py [--reps 5] [--kernel-reps 20] [--height 2160 --width 3840]

Cases: P3 8-bit integer -> sRGB, and PQ / BT.2100 float -> sRGB with peak detection. Per case it prints
  host_ms      wall clock of transform(..., device=False), median of --reps after one warm-up
  device_ms    wall clock of transform(..., device=True), uploads and downloads included, same protocol
  convert_ms / peak_ms   the kernels alone on resident planes, stream events over --kernel-reps launches
and what the kernels achieve: f64 operations per second (110 per pow, the count of csrc/jxl_fastpow.h, times the pows per
pixel of the case) and bytes per second against the 6.29 TB/s a copy kernel reaches on this chip. Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jxlatte_amd import abi, decoder, host  # noqa: E402
from jxlatte_amd.decoder import (CE_RGB, PEAK_DETECT_AUTO, PRI_BT2100, PRI_P3, PRI_SRGB, TF_PQ, TF_SRGB, WP_D65, DeviceBackend,  # noqa: E402
                                 JXLImage)

F64_OPS_PER_POW = 110
F64_PEAK = 157.3e12 / 2 / 2  # f64 VALU operations per second: half the f32 vector rate, an FMA counted once
HBM_COPY = 6.29e12


def info(transfer, prim, bits):
    return types.SimpleNamespace(colour_space=CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[], prim_xy=list(prim),
                                 white_xy=list(WP_D65), transfer=transfer, xyb_encoded=False, bits_per_sample=bits, use_icc=False)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    a = ap.parse_args()
    h, w = a.height, a.width
    rng = np.random.default_rng(1)
    be = DeviceBackend(0)
    lib = be.ctx.lib
    lib.jxl_debug_color_kernel_ms.restype = C.c_int32
    lib.jxl_debug_color_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.POINTER(abi.ColorParams), C.c_int32,
                                              C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    cases = [
        ("p3_int8_to_srgb8", [rng.integers(0, 256, (h, w)).astype(np.int32) for _ in range(3)], info(TF_SRGB, PRI_P3, 8), abi.TF_SRGB, [255] * 3, 3, 0),
        ("pq_bt2100_float_to_srgb8_peak", [rng.uniform(0.05, 0.75, (h, w)).astype(np.float32) for _ in range(3)], info(TF_PQ, PRI_BT2100, 16),
         abi.TF_PQ, None, 6, 6),
    ]
    for name, planes, inf, tf_in, in_max, pows_convert, pows_peak in cases:
        im = JXLImage(planes, inf, be)
        res = dict(case=name, height=h, width=w)
        res["host_ms"], res["host_ms_min"], res["host_ms_max"] = timed(lambda: im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO), a.reps)
        res["device_ms"], res["device_ms_min"], res["device_ms_max"] = timed(
            lambda: im.transform(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO, device=True), a.reps)
        m = decoder.get_conversion_matrix(PRI_SRGB, WP_D65, im.primariesXY, im.whiteXY)
        p = host.colorParams(planes, tfIn=tf_in, inMax=in_max, matrix=m, scale=1.5 if pows_peak else None, tfOut=abi.TF_SRGB, maxValue=255)
        cms, pms = C.c_float(0), C.c_float(0)
        pin = (C.c_void_p * 3)(*[x.ctypes.data for x in planes])
        host.check(be.ctx.h, lib.jxl_debug_color_kernel_ms(be.ctx.h, pin, h, w, C.byref(p), 1 if pows_peak else 0, a.kernel_reps, C.byref(cms), C.byref(pms)))
        res["convert_ms"], res["peak_ms"] = cms.value, pms.value
        px = h * w
        res["convert_f64_ops_per_s"] = px * pows_convert * F64_OPS_PER_POW / (cms.value * 1e-3)
        res["convert_share_of_f64_issue"] = res["convert_f64_ops_per_s"] / F64_PEAK
        res["convert_bytes_per_s"] = px * 24 / (cms.value * 1e-3)
        res["convert_share_of_hbm_copy"] = res["convert_bytes_per_s"] / HBM_COPY
        if pows_peak:
            res["peak_f64_ops_per_s"] = px * pows_peak * F64_OPS_PER_POW / (pms.value * 1e-3)
            res["peak_share_of_f64_issue"] = res["peak_f64_ops_per_s"] / F64_PEAK
            res["peak_bytes_per_s"] = px * 12 / (pms.value * 1e-3)
        res["speedup_end_to_end"] = res["host_ms"] / res["device_ms"]
        print(json.dumps(res), flush=True)
    be.close()


if __name__ == "__main__":
    main()
