"""One 3840x2160 image, three float planes resident on the device, as a torch tensor in the sRGB target: the tensor exit
(ResidentPlanes.tensorSamples: one kernel into torch memory) against the route there was before it (ResidentPlanes.pngSamples
brings the PNG's 8-bit samples down, torch.from_numpy(...).cuda() sends them up again), as interleaved rounds in one process.

    python tools/tensor_bench.py [--rounds 8] [--calls 20] [--height 2160 --width 3840]
    python tools/tensor_bench.py --kernels 10      # only launches, for a kernel trace: each of the three forms 10 times
    python tools/tensor_bench.py --size 224x224 [--tile 64x4] [--no-skew]   # the resized leg (below); with --kernels: launches only

Per path: median and range over the rounds (after one warm-up round) of the wall clock of one call, taken as the time of `--calls`
back-to-back calls over their number; every call ends in a device synchronise (the library's own, or torch's after the upload).
Bytes: what the kernel reads and writes (three float planes in, the tensor out), and what crosses the bus. `hbm_fraction_of_call`
is those kernel bytes over the CALL's time over the 8.0 TB/s the HBM3E is specified for: a lower bound of the kernel's own share,
since the call also holds the pointer queries, the launch and the synchronise; the kernel's time is a kernel trace's to give
(--kernels). The uint8 tensor is checked against the old route's bytes. Prints one JSON line. Needs a GPU.

--size HxW: the same planes, linear -> sRGB, as an HxW tensor, F16/CHW and U8/HWC, two routes alternating in one process:
  A  what there was before: tensorSamples(float32, CHW) at full size, then torch.nn.functional.interpolate(antialias=True) and the
     conversion in torch. It filters AFTER the curve: the route a user had, not the same arithmetic.
  B  ResidentPlanes.tensorResized: one kernel, the filter in linear light, the curve per output pixel.
--tile TWxTH forces the kernel's output tile and --no-skew takes the skew out of its LDS image (the library's test hooks)."""
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
    ap.add_argument("--size", default=None)
    ap.add_argument("--tile", default=None)
    ap.add_argument("--no-skew", action="store_true")
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
    if a.size:
        resized_leg(a, ctx, rp, color, dev)
        ctx.close()
        return
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


def resized_leg(a, ctx, rp, color, dev):
    import ctypes as C

    import torch
    oh, ow = (int(v) for v in a.size.lower().split("x"))
    if a.tile:
        tw, th = (int(v) for v in a.tile.lower().split("x"))
        hook = ctx.lib.jxl_debug_tensor_resize_tile
        hook.restype, hook.argtypes = C.c_int32, [C.c_int32, C.c_int32]
        assert hook(tw, th) == 0, "no such tile"
    if a.no_skew:
        hook = ctx.lib.jxl_debug_tensor_resize_skew
        hook.restype, hook.argtypes = C.c_int32, [C.c_int32]
        hook(0)
    full = torch.empty((3, a.height, a.width), dtype=torch.float32, device=dev)
    f16 = torch.empty((3, oh, ow), dtype=torch.float16, device=dev)
    u8 = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)

    def small():
        rp.tensorSamples(full.data_ptr(), dtype="float32", layout="CHW", **color)
        return torch.nn.functional.interpolate(full[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0]

    def a_f16():
        t = small().to(torch.float16)
        torch.cuda.synchronize()
        return t

    def a_u8():
        t = (small().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous()
        torch.cuda.synchronize()
        return t

    def b_f16():
        rp.tensorResized(f16.data_ptr(), (oh, ow), dtype="float16", layout="CHW", **color)
        return f16

    def b_u8():
        rp.tensorResized(u8.data_ptr(), (oh, ow), dtype="uint8", layout="HWC", **color)
        return u8
    if a.kernels:
        for _ in range(a.kernels):
            b_f16()
            b_u8()
        return
    paths = {"A full-size tensor + interpolate F16/CHW": a_f16, "B fused resize F16/CHW": b_f16,
             "A full-size tensor + interpolate U8/HWC": a_u8, "B fused resize U8/HWC": b_u8}
    times = {k: [] for k in paths}
    last = {}
    for r in range(a.rounds + 1):  # round 0 warms up
        for k, fn in paths.items():
            t0 = time.perf_counter()
            for _ in range(a.calls):
                last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3 / a.calls
            if r:
                times[k].append(dt)
    res = {}
    for k, v in times.items():
        res[k] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), all_ms=[round(x, 4) for x in v])
    # the two routes are not the same arithmetic (A filters encoded samples): how far apart they land, in 8-bit steps
    d8 = (last["A full-size tensor + interpolate U8/HWC"].to(torch.int16) - last["B fused resize U8/HWC"].to(torch.int16)).abs()
    print(json.dumps(dict(height=a.height, width=a.width, out_height=oh, out_width=ow, tile=a.tile, skew=not a.no_skew, rounds=a.rounds, calls=a.calls,
                          plane_bytes=3 * 4 * a.height * a.width, u8_routes_max_abs_diff=int(d8.max()), u8_routes_mean_abs_diff=round(float(d8.float().mean()), 4),
                          paths=res)), flush=True)


if __name__ == "__main__":
    main()
