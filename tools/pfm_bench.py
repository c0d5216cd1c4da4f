"""One 3840x2160 three-plane float image into the bytes of a PFM: PFMWriter's constructor on the host (numpy: NaN
canonicalisation, row flip, interleave, byte order) against deviceSamples=True (one kernel), on host arrays and on resident
planes, as interleaved rounds in one process.

    python tools/pfm_bench.py [--rounds 6] [--height 2160 --width 3840]
    python tools/pfm_bench.py --kernels 10      # only launches, for a kernel trace: the resident entry 10 times

Paths: "host numpy" (the default writer on host arrays), "host numpy after download" (the default writer on an image whose
planes are resident: its getBuffer download is part of the time -- what a caller had to do before there was a device path),
"deviceSamples host arrays" (jxl_stage_pfm_samples), "deviceSamples resident" (jxl_planes_pfm_samples), and "download only"
(the three planes brought down, nothing else: the floor for anything that ends with these bytes on the host). Per path: median
and range of the wall clock over the rounds (after one warm-up round) and the bytes that cross the bus each way
(PFMWriter.bus_bytes where the writer records them). Writing the file is not timed. Prints one JSON line. Needs a GPU."""
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
from jxlatte_amd.decoder import CE_RGB, PRI_SRGB, TF_LINEAR, WP_D65, DeviceBackend, JXLImage, PFMWriter  # noqa: E402


def info():
    return types.SimpleNamespace(colour_space=CE_RGB, num_extra=0, ec_type=[], ec_alpha_associated=[], ec_bits=[], prim_xy=list(PRI_SRGB),
                                 white_xy=list(WP_D65), transfer=TF_LINEAR, xyb_encoded=False, bits_per_sample=32, use_icc=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    be = DeviceBackend(0)
    rng = np.random.default_rng(1)
    buf = [rng.normal(0.5, 1.0, (a.height, a.width)).astype(np.float32) for _ in range(3)]
    buf[1][::97, ::89] = np.float32("nan")
    inf = info()
    rp = host.ResidentPlanes.upload(be.ctx, np.stack(buf))
    if a.kernels:
        for _ in range(a.kernels):
            rp.pfmSamples()
        be.close()
        return
    image = JXLImage(buf, inf, be)
    n = 4 * 3 * a.height * a.width
    paths = {"host numpy": lambda: PFMWriter(image),
             "host numpy after download": lambda: PFMWriter(JXLImage([None] * 3, inf, be, resident=rp)),
             "deviceSamples host arrays": lambda: PFMWriter(image, deviceSamples=True),
             "deviceSamples resident": lambda: PFMWriter(JXLImage([None] * 3, inf, be, resident=rp), deviceSamples=True),
             "download only": lambda: rp.download()}
    derived = {"host numpy": (0, 0), "host numpy after download": (0, n), "download only": (0, n)}
    times = {k: [] for k in paths}
    bus = {}
    ref = None
    for r in range(a.rounds + 1):  # round 0 warms up
        for k, fn in paths.items():
            t0 = time.perf_counter()
            wr = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                times[k].append(dt)
            if k == "download only":
                continue
            bus[k] = wr.bus_bytes
            if ref is None:
                ref = wr.samples
            assert np.array_equal(wr.samples, ref), "%s differs" % k
    print(json.dumps(dict(height=a.height, width=a.width, rounds=a.rounds, payload_bytes=n, paths={
        k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), all_ms=[round(x, 3) for x in v],
                bytes_up=(bus.get(k) or derived[k])[0], bytes_down=(bus.get(k) or derived[k])[1],
                bytes="recorded" if bus.get(k) else "derived")
        for k, v in times.items()})), flush=True)
    be.close()


if __name__ == "__main__":
    main()
