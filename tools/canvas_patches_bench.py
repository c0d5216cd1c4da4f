"""device_patch_sets against the landing route on patches-lossless.jxl (profiles/canvas_patches.md). Measurements, no pass / fail
threshold.

    python tools/canvas_patches_bench.py [--reps N] [--sets] [--tree DIR]
    python tools/canvas_patches_bench.py --casts one|per-plane

Without --casts: JXLDecoder(device_canvas=True, device_patches=True[, device_patch_sets=True]).decode() N times after one warm-up,
each ending in a synchronise of the context; one JSON line with the wall times and every frame's stats[k]["blend_bus"],
stats[k]["canvas"] and patch path. --tree: import the package from another checkout (the parent commit, built there), which has
no --sets.
With --casts: the sample's hoisted casts alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/...): four
int32 planes of 1096 x 1600 and four of 198 x 198 in two sets, cast by ONE jxl_canvas_cast_planes call or by eight jxl_canvas_cast
calls; 5 rounds on fresh uploads. The trace's rows for k_canvas_cast / k_modular_to_float are the measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--casts", choices=["one", "per-plane"])
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from jxlatte_amd import host
    from jxlatte_amd.decoder import DeviceBackend, JXLDecoder
    be = DeviceBackend()
    try:
        if a.casts:
            rng = np.random.default_rng(1)
            for _ in range(5):
                big = host.DeviceCanvas.fromArrays(be.ctx, [rng.integers(0, 256, (1096, 1600)).astype(np.int32) for _ in range(4)])
                small = host.DeviceCanvas.fromArrays(be.ctx, [rng.integers(0, 256, (198, 198)).astype(np.int32) for _ in range(4)])
                if a.casts == "one":
                    host.canvas_cast_planes(be.ctx, [(s, n, 8) for s in (big, small) for n in range(4)])
                else:
                    for s in (big, small):
                        for n in range(4):
                            s.cast(n, 8)
                be.ctx.synchronize()
                big.release()
                small.release()
            print(json.dumps(dict(casts=a.casts, rounds=5, planes="4 x 1096x1600 + 4 x 198x198 int32")))
            return
        kw = dict(device_canvas=True, device_patches=True)
        if a.sets:
            kw["device_patch_sets"] = True
        times, rows = [], None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            dec = JXLDecoder(SAMPLE, backend=be, **kw)
            im = dec.decode()
            be.ctx.synchronize()
            t1 = time.perf_counter()
            rows = [dict(blend_bus=list(st["blend_bus"]), canvas=st["canvas"], patches=st.get("patches", {}).get("path")) for st in dec.stats]
            im.close()
            dec.close()
            if r:
                times.append(round((t1 - t0) * 1e3, 2))
        print(json.dumps(dict(tree=os.path.relpath(os.path.abspath(a.tree), ROOT), switches=sorted(kw), wall_ms=times,
                              median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), frames=rows)))
    finally:
        be.close()


if __name__ == "__main__":
    main()
