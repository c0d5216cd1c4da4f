"""device_image against the best path before it (profiles/device_image.md). Medians of interleaved rounds; nothing here is a
pass / fail threshold.

    python tools/device_image_bench.py [--rounds N] [--kernel-only]

1. quilt.jxl (3 x 1024 x 1024 int32, frame-level chain [Squeeze]), wall time from JXLDecoder.decode() through the PNGWriter
   constructor: JXLDecoder() + PNGWriter(deviceSamples=True) on host arrays against JXLDecoder(device_image=True) + the same writer.
2. synthetic 3840 x 2160 int32 RGB with an RCT at the C ABI: jxl_modular_apply + jxl_stage_png_samples against jxl_modular_begin /
   jxl_modular_run / jxl_canvas_from_modular / jxl_canvas_png_samples.
--kernel-only: a few launches of the second chain and nothing else, for a kernel trace of its own.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jxlatte_amd import _lib, host  # noqa: E402
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PNGWriter  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def interleaved(arms, rounds):
    """arms: name -> callable; every round runs each arm once, in turn. Returns name -> list of milliseconds"""
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            out[k].append(timed(fn)[0])
    return out


def report(what, ms, **extra):
    line = dict(what=what, rounds=len(next(iter(ms.values()))), **extra)
    for k, v in ms.items():
        line[k + "_ms_median"] = round(statistics.median(v), 3)
        line[k + "_ms_min"] = round(min(v), 3)
        line[k + "_ms_max"] = round(max(v), 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    be = DeviceBackend(0)
    ctx = be.ctx

    # ---- 2. the C ABI chains on synthetic 4K ----
    h, w = 2160, 3840
    rng = np.random.default_rng(1)
    chans = [rng.integers(0, 256, (h, w)).astype(np.int32) for _ in range(3)]
    kw = dict(bitDepth=8, bigEndian=True, inMax=[255] * 3, colorDepth=8)
    planes = [(c, -1, np.int32, 1.0) for c in range(3)]

    def before():
        outs = host.ModularStream(ctx, chans, [], rctType=6).applyTransforms()
        return host.pngSamples(ctx, outs, None, **kw)

    def after():
        host.ModularStream(ctx, chans, [], rctType=6).run()
        cv = host.DeviceCanvas.fromModular(ctx, h, w, planes)
        try:
            return cv.pngSamples(nColor=3, **kw)
        finally:
            cv.release()

    if a.kernel_only:
        for _ in range(5):
            after()
        be.close()
        return 0
    assert np.array_equal(before(), after())  # (and the warm-up of both arms)
    report("4K synthetic int32 RGB + RCT, C ABI: modular_apply + stage_png_samples | begin/run/from_modular/canvas_png_samples",
           interleaved(dict(before=before, after=after), a.rounds), plane_bytes=4 * h * w, sample_bytes=3 * h * w)

    # ---- 1. quilt through the decoder ----
    path = os.path.join(ROOT, "tests", "golden", "samples", "quilt.jxl")
    data = open(path, "rb").read()

    def run(**sw):
        dec = JXLDecoder(data, backend=be, **sw)
        im = dec.decode()
        wr = PNGWriter(im, deviceSamples=True)
        route = dec.stats[-1]["image"]
        im.close()
        dec.close()
        return wr.samples, wr.bus_bytes, route

    s0, bus0, r0 = run()
    s1, bus1, r1 = run(device_image=True)
    assert np.array_equal(s0, s1)
    report("quilt.jxl, decode() through PNGWriter(deviceSamples=True): default decoder | device_image",
           interleaved(dict(before=lambda: run(), after=lambda: run(device_image=True)), a.rounds),
           route_before=r0, route_after=r1, writer_bus_before=bus0, writer_bus_after=bus1)
    # the front-end's share (entropy decoding: the same work in both arms)
    from jxlatte_amd import frontend

    def fe_only():
        fe = frontend.Frontend(data)
        fe.set_defer_transforms(True)
        fe.next_frame(None, None, None)
        fe.close()
    report("quilt.jxl, the front-end alone (transforms deferred)", interleaved(dict(frontend=fe_only), a.rounds))
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
