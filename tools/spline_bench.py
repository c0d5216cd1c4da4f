"""Frame.renderSplines on one synthetic 3840x2160 frame: the host path (decoder.render_splines, numpy, one arc box at a time)
against the device stage (jxl_stage_splines, uploads and downloads included) and the kernel alone.

    python tools/spline_bench.py [--reps 3] [--kernel-reps 10] [--height 2160 --width 3840] [--skip-host]

Seeded spline sets: few and long, many and short, thick (large sigma), thin, crossing. Per set it prints
  arcs / tiles / list entries     the arc table and its binning
  evals                           pixel x arc evaluations (the sum of the arcs' box areas)
  host_ms                         wall clock of render_splines, one run (it is slow)
  device_ms                       wall clock of jxl_stage_splines, median of --reps after one warm-up
  kernel_ms                       the kernel alone on resident planes, stream events over --kernel-reps launches
  identical                       share of the touched samples of the device result that equal the host result bit for bit
as one JSON line each. Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jxlatte_amd import _lib, abi, decoder, host  # noqa: E402


def spline_set(seed, n, h, w, points, sigma, step=None):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(points[0], points[1] + 1))
        if step is None:
            cp = np.stack([rng.integers(0, h, k), rng.integers(0, w, k)], axis=1)
        else:
            cp = np.array([rng.integers(0, h), rng.integers(0, w)]) + np.cumsum(rng.integers(-step, step + 1, (k, 2)), axis=0)
        coeff = np.zeros((4, 32), np.int64)
        coeff[:3, :8] = rng.integers(-200, 201, (3, 8))
        coeff[3, 0] = rng.integers(sigma[0], sigma[1] + 1)
        out.append(dict(quant_adjust=0, control=[(int(y), int(x)) for y, x in cp], coeff=coeff.tolist()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    h, w = a.height, a.width
    sets = {
        "few_long": spline_set(1, 8, h, w, (4, 8), (4, 9)),
        "many_short": spline_set(2, 400, h, w, (2, 3), (3, 6), step=50),
        "thick": spline_set(3, 12, h, w, (3, 5), (40, 80)),
        "thin": spline_set(4, 24, h, w, (3, 6), (1, 2)),
        "crossing": [s for i in range(6) for s in spline_set(5 + i, 4, 400, 400, (3, 5), (6, 15))],
    }
    planes = np.random.default_rng(0).normal(0, 0.5, (3, h, w)).astype(np.float32)
    ctx = _lib.Context(0)
    lib = ctx.lib
    fn = lib.jxl_debug_spline_kernel_ms
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.c_int32, C.c_int32, C.POINTER(abi.SplineDesc), C.c_int32,
                   C.POINTER(C.c_float), C.POINTER(C.c_int64)]
    for name, sp in sets.items():
        arcs = host.spline_arcs(sp, 0.0, 1.0, h, w)
        evals = int(((arcs["x1"].astype(np.int64) - arcs["x0"] + 1) * (arcs["y1"].astype(np.int64) - arcs["y0"] + 1)).sum())
        host.renderSplines(ctx, planes, sp, 0.0, 1.0)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dev = host.renderSplines(ctx, planes, sp, 0.0, 1.0)
            ts.append((time.perf_counter() - t0) * 1e3)
        d, keep = abi.make_spline_desc(sp, 0.0, 1.0)
        p3 = (C.POINTER(C.c_float) * 3)(*[abi.fptr(planes[c]) for c in range(3)])
        ms, counts = C.c_float(), (C.c_int64 * 3)()
        _lib.check(ctx.h, fn(ctx.h, p3, h, w, C.byref(d), a.kernel_reps, C.byref(ms), counts))
        row = dict(set=name, splines=len(sp), arcs=int(counts[0]), tiles=int(counts[1]), list_entries=int(counts[2]), evals=evals,
                   device_ms=round(statistics.median(ts), 2), kernel_ms=round(ms.value, 4),
                   kernel_evals_per_s=round(evals / (ms.value * 1e-3)) if ms.value > 0 else None)
        if not a.skip_host:
            bufs = [planes[c].copy() for c in range(3)]
            t0 = time.perf_counter()
            decoder.render_splines(bufs, sp, 0.0, 1.0, w, h)
            row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            ref = np.stack(bufs)
            touched = ref.view(np.uint32) != planes.view(np.uint32)
            same = (ref.view(np.uint32) == dev.view(np.uint32)) | (np.isnan(ref) & np.isnan(dev))
            row["identical"] = float(same[touched].mean()) if touched.any() else 1.0
            row["untouched_equal"] = bool(same[~touched].all())
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
