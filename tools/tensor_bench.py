"""One 3840x2160 image, three float planes resident on the device, as a torch tensor in the sRGB target: the tensor exit
(ResidentPlanes.tensorSamples: one kernel into torch memory) against the route there was before it (ResidentPlanes.pngSamples
brings the PNG's 8-bit samples down, torch.from_numpy(...).cuda() sends them up again), as interleaved rounds in one process.

    python tools/tensor_bench.py [--rounds 8] [--calls 20] [--height 2160 --width 3840]
    python tools/tensor_bench.py --kernels 10      # only launches, for a kernel trace: each of the three forms 10 times

Per path: median and range over the rounds (after one warm-up round) of the wall clock of one call, taken as the time of `--calls`
back-to-back calls over their number; every call ends in a device synchronise (the library's own, or torch's after the upload).
Bytes: what the kernel reads and writes (three float planes in, the tensor out), and what crosses the bus. `hbm_fraction_of_call`
is those kernel bytes over the CALL's time over the 8.0 TB/s the HBM3E is specified for: a lower bound of the kernel's own share,
since the call also holds the pointer queries, the launch and the synchronise; the kernel's time is a kernel trace's to give
(--kernels). The uint8 tensor is checked against the old route's bytes. Prints one JSON line. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jxlatte_amd import abi, host  # noqa: E402
from jxlatte_amd._lib import Context  # noqa: E402

HBM_PEAK = 8.0e12
FORMS = [("uint8", "HWC", 1), ("float16", "CHW", 2), ("float32", "CHW", 4)]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_bench needs a GPU")
    ctx = Context(0)
    dev = "cuda:%d" % ctx.device
    rng = np.random.default_rng(1)
    planes = np.stack([rng.uniform(0, 1, (a.height, a.width)).astype(np.float32) for _ in range(3)])
    rp = host.ResidentPlanes.upload(ctx, planes)
    color = dict(tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB)
    n = a.height * a.width
    tdt = {"uint8": torch.uint8, "float16": torch.float16, "float32": torch.float32}
    outs = {(d, l): torch.empty((a.height, a.width, 3) if l == "HWC" else (3, a.height, a.width), dtype=tdt[d], device=dev) for d, l, _ in FORMS}

    def new(d, l):
        return lambda: rp.tensorSamples(outs[(d, l)].data_ptr(), dtype=d, layout=l, **color)

    def old():
        t = torch.from_numpy(rp.pngSamples(bitDepth=8, **color)).cuda()
        torch.cuda.synchronize()
        return t
    if a.kernels:
        for d, l, _ in FORMS:
            for _ in range(a.kernels):
                new(d, l)()
        ctx.close()
        return
    paths = {"tensor %s/%s" % (d, l): new(d, l) for d, l, _ in FORMS}
    paths["png samples down, torch up (uint8/HWC)"] = old
    times = {k: [] for k in paths}
    for r in range(a.rounds + 1):  # round 0 warms up
        for k, fn in paths.items():
            t0 = time.perf_counter()
            for _ in range(a.calls):
                last = fn()
            dt = (time.perf_counter() - t0) * 1e3 / a.calls
            if r:
                times[k].append(dt)
            if k.startswith("png"):
                assert torch.equal(last, outs[("uint8", "HWC")]), "the two routes give different bytes"
    res = {}
    for k, v in times.items():
        med = statistics.median(v)
        e = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), all_ms=[round(x, 4) for x in v])
        form = next((f for f in FORMS if k == "tensor %s/%s" % f[:2]), None)
        if form:
            kb = 3 * 4 * n + 3 * form[2] * n
            e.update(kernel_bytes=kb, bytes_up=0, bytes_down=0, hbm_fraction_of_call=round(kb / (med * 1e-3) / HBM_PEAK, 4),
                     call_gbytes_per_s=round(kb / (med * 1e-3) / 1e9, 1))
        else:
            e.update(kernel_bytes=3 * 4 * n + 3 * n, bytes_up=3 * n, bytes_down=3 * n)
        res[k] = e
    print(json.dumps(dict(height=a.height, width=a.width, rounds=a.rounds, calls=a.calls, hbm_peak_bytes_per_s=HBM_PEAK, paths=res)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
