"""One 3840x2160 three-plane image into the samples of an 8-bit sRGB PNG: PNGWriter's constructor with deviceColor=True (peak,
colour convert and pack as three device passes with float planes crossing the bus between them) against deviceSamples=True
(one pass), on host arrays and on resident planes, as interleaved rounds in one process.

    python tools/png_bench.py [--pairs 5] [--height 2160 --width 3840]
    python tools/png_bench.py --kernels 10      # only launches, for a kernel trace: the one-pass entry and the two-pass
                                                # entries on the same inputs, 10 times each

Cases: P3 8-bit integer -> sRGB, and PQ / BT.2100 float -> sRGB with peak detection (those of tools/color_bench.py). Per case
and path: median and range of the constructor's wall clock over the rounds (after one warm-up round), and the bytes of sample
planes that cross the bus each way (recorded by PNGWriter.bus_bytes for deviceSamples; for deviceColor DERIVED from the calls
that path makes -- staged_bytes -- and marked so in the output). The resident path exists for float planes only. zlib is not timed: PNGWriter.write spends
its time there, on the host. Prints one JSON line per case. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jxlatte_amd import host  # noqa: E402
from jxlatte_amd.decoder import (CE_RGB, PEAK_DETECT_AUTO, PRI_BT2100, PRI_P3, PRI_SRGB, TF_PQ, TF_SRGB, WP_D65, DeviceBackend, JXLImage,  # noqa: E402
                                 PNGWriter)


def info(transfer, prim, bits):
    return types.SimpleNamespace(colour_space=CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[], prim_xy=list(prim),
                                 white_xy=list(WP_D65), transfer=transfer, xyb_encoded=False, bits_per_sample=bits, use_icc=False)


def cases(h, w):
    rng = np.random.default_rng(1)
    level = rng.uniform(0.2, 0.6, (h, 1))
    return {"p3-int8": ([rng.integers(0, 256, (h, w)).astype(np.int32) for _ in range(3)], info(TF_SRGB, PRI_P3, 8)),
            "pq-bt2100-float": ([(level + rng.uniform(-0.01, 0.01, (h, w))).astype(np.float32) for _ in range(3)], info(TF_PQ, PRI_BT2100, 16))}


def staged_bytes(buf, peak):
    """deviceColor=True: the peak reads all three planes (a matrix is on), convert takes three up and three float planes down,
    pack takes them up again and brings the samples down"""
    n = buf[0].size
    return (3 * 4 * n if peak else 0) + 3 * buf[0].nbytes + 3 * 4 * n, 3 * 4 * n + 3 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    be = DeviceBackend(0)
    for name, (buf, inf) in cases(a.height, a.width).items():
        image = JXLImage(buf, inf, be)
        is_float = buf[0].dtype == np.float32
        if a.kernels:
            plan = image._color_plan(PRI_SRGB, WP_D65, TF_SRGB, PEAK_DETECT_AUTO, be.color_peak)
            planes, params = plan[0], plan[1]
            for _ in range(a.kernels):
                host.pngSamples(be.ctx, planes, None, bitDepth=8, bigEndian=True, **params)
                out = host.colorConvert(be.ctx, planes, **params)
                host.packSamples(be.ctx, out, 8, taggedDepth=[inf.bits_per_sample] * 4, bigEndian=True)
            continue
        paths = {"deviceColor": lambda: PNGWriter(image, bitDepth=8, deviceColor=True),
                 "deviceSamples host arrays": lambda: PNGWriter(image, bitDepth=8, deviceSamples=True)}
        if is_float:
            rp = host.ResidentPlanes.upload(be.ctx, np.stack(buf))
            resident = JXLImage([None] * 3, inf, be, resident=rp)
            paths["deviceSamples resident"] = lambda: PNGWriter(resident, bitDepth=8, deviceSamples=True)
        times = {k: [] for k in paths}
        ref = None
        bus = {}
        for r in range(a.pairs + 1):  # round 0 warms up
            for k, fn in paths.items():
                t0 = time.perf_counter()
                wr = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    times[k].append(dt)
                bus[k] = wr.bus_bytes
                if ref is None:
                    ref = wr.samples
                assert np.array_equal(wr.samples, ref), "%s: %s differs" % (name, k)
        bus["deviceColor"] = staged_bytes(buf, inf.transfer == TF_PQ)  # DERIVED from the calls that path makes, not recorded
        print(json.dumps(dict(case=name, height=a.height, width=a.width, rounds=a.pairs, paths={
            k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), all_ms=[round(x, 3) for x in v],
                    bytes_up=bus[k][0], bytes_down=bus[k][1], bytes="derived" if k == "deviceColor" else "recorded")
            for k, v in times.items()})), flush=True)
    be.close()


if __name__ == "__main__":
    main()
