"""Multi-frame images with the canvas on the host (one jxl_stage_blend call per channel and frame) against the canvas on the
device (JXLDecoder(device_canvas=True): one jxl_canvas_blend launch per frame), as interleaved rounds in one process.

    python tools/canvas_bench.py [--rounds 5] [--height 2160 --width 3840]

Two inputs:
  "blendmodes_5": the committed 1024 x 1024 five-frame RGB + alpha bitstream, decode() and then PNGWriter(deviceSamples=True),
      with the switch off and on (the front-end's entropy decoding is part of both).
  "synthetic": five float RGBA frames of --height x --width through the host layer, the colour planes of every frame starting
      as the context's resident planes (where a VarDCT frame leaves them): REPLACE, then BLEND, ADD, MULT and BLEND into and from
      the same canvas. Off: the planes come down and every channel is one host.blend call, then PNGWriter(deviceSamples=True) on
      the host arrays. On: DeviceCanvas.fromPlanes + the alpha plane up + one host.canvas_blend, then the canvas becomes the
      resident planes and PNGWriter(deviceSamples=True) packs them. Placing a frame's planes on the device is not timed.
Per input and path: median and range of the wall clock over the rounds (after one warm-up round) and the bytes that crossed the
bus, from the binding's counters (host._bus for the blend path, PNGWriter.bus_bytes for the writer; the download of a frame's
resident planes in the synthetic "off" path is counted by its size). The PNG samples of both paths are compared. Prints one
JSON line. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jxlatte_amd import abi, host  # noqa: E402
from jxlatte_amd.decoder import CE_RGB, PRI_SRGB, TF_SRGB, WP_D65, DeviceBackend, JXLDecoder, JXLImage, PNGWriter  # noqa: E402

HE, IA = abi.BLEND_FLAG_HAS_EXTRA, abi.BLEND_FLAG_IS_ALPHA
MODES = [abi.BLEND_REPLACE, abi.BLEND_BLEND, abi.BLEND_ADD, abi.BLEND_MULT, abi.BLEND_BLEND]


def info():
    return types.SimpleNamespace(colour_space=CE_RGB, num_extra=1, ec_type=[0], ec_alpha_associated=[0], ec_bits=[8], prim_xy=list(PRI_SRGB),
                                 white_xy=list(WP_D65), transfer=TF_SRGB, xyb_encoded=False, bits_per_sample=8, use_icc=False)


def sample(be, device_canvas):
    ctx = be.ctx
    ctx.blend_bus = [0, 0]
    t0 = time.perf_counter()
    dec = JXLDecoder(os.path.join(ROOT, "tests", "golden", "samples", "blendmodes_5.jxl"), backend=be, device_canvas=device_canvas)
    im = dec.decode()
    t1 = time.perf_counter()
    wr = PNGWriter(im, deviceSamples=True)
    t2 = time.perf_counter()
    bus = (ctx.blend_bus[0] + wr.bus_bytes[0], ctx.blend_bus[1] + wr.bus_bytes[1])
    states = [s["canvas"] for s in dec.stats]
    dec.close()
    return dict(decode_ms=(t1 - t0) * 1e3, total_ms=(t2 - t0) * 1e3), bus, wr.samples, states


def synthetic(be, frames, alphas, shape, device_canvas):
    ctx = be.ctx
    h, w = shape
    rect = (h, w, 0, 0, 0, 0, 0, 0)
    ctx.blend_bus = [0, 0]
    extra_down = 0
    total = blend = 0.0
    canvas = host.DeviceCanvas.create(ctx, [np.float32] * 4, h, w) if device_canvas else [np.zeros(shape, np.float32) for _ in range(4)]
    dead = []
    for k, mode in enumerate(MODES):
        rp = host.ResidentPlanes.upload(ctx, frames[k])  # (where a VarDCT frame's colour planes are; not timed)
        ctx.synchronize()
        t0 = time.perf_counter()
        chans = [(c, mode, HE, 3, 3) for c in range(3)] + [(3, mode, HE | IA, 3, 3)]
        if device_canvas:
            fs = host.DeviceCanvas.fromPlanes(ctx, [np.float32])
            fs.upload(3, alphas[k])
            dead.append(fs)
            host.canvas_blend(canvas, fs, None if mode == abi.BLEND_REPLACE else canvas, rect, chans)
        else:
            planes = list(rp.download()) + [alphas[k]]
            extra_down += 3 * 4 * h * w
            for c, (fp, m, flags, fa, ra) in enumerate(chans):
                canvas[c] = host.blend(ctx, m, canvas[c], planes[fp], None if m == abi.BLEND_REPLACE else canvas[c], rect, frameAlpha=planes[fa],
                                       refAlpha=None if m == abi.BLEND_REPLACE else canvas[ra], isAlpha=bool(flags & IA), hasExtra=True)
        ctx.synchronize()  # (a launch returns before the kernel ends)
        blend += time.perf_counter() - t0
    t0 = time.perf_counter()
    if device_canvas:
        im = JXLImage([None] * 3 + [canvas.download(3)], info(), be, resident=canvas.toPlanes())
    else:
        im = JXLImage(canvas, info(), be)
    wr = PNGWriter(im, deviceSamples=True)
    total = blend + time.perf_counter() - t0
    bus = (ctx.blend_bus[0] + wr.bus_bytes[0], ctx.blend_bus[1] + wr.bus_bytes[1] + extra_down)
    for s_ in dead + ([canvas] if device_canvas else []):
        s_.release()
    return dict(blend_ms=blend * 1e3, total_ms=total * 1e3), bus, wr.samples, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    a = ap.parse_args()
    be = DeviceBackend(0)
    rng = np.random.default_rng(1)
    shape = (a.height, a.width)
    frames = [np.stack([rng.random(shape, np.float32) for _ in range(3)]) for _ in MODES]
    alphas = [rng.random(shape, np.float32) for _ in MODES]
    runs = {("blendmodes_5", "off"): lambda: sample(be, False), ("blendmodes_5", "on"): lambda: sample(be, True),
            ("synthetic", "off"): lambda: synthetic(be, frames, alphas, shape, False),
            ("synthetic", "on"): lambda: synthetic(be, frames, alphas, shape, True)}
    times = {k: {} for k in runs}
    bus, ref, states = {}, {}, {}
    for r in range(a.rounds + 1):  # round 0 warms up
        for k, fn in runs.items():
            t, b, samples, st = fn()
            if r:
                for name, ms in t.items():
                    times[k].setdefault(name, []).append(ms)
            bus[k], states[k] = b, st
            if k[0] not in ref:
                ref[k[0]] = samples
            assert np.array_equal(samples, ref[k[0]]), "%s %s: the PNG samples differ" % k
    out = {}
    for (inp, path), t in times.items():
        out.setdefault(inp, {})[path] = dict(
            {name: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), all=[round(x, 3) for x in v])
             for name, v in t.items()}, bytes_up=bus[(inp, path)][0], bytes_down=bus[(inp, path)][1], canvas=states[(inp, path)])
    print(json.dumps(dict(rounds=a.rounds, synthetic_shape=list(shape), inputs=out)), flush=True)
    be.close()


if __name__ == "__main__":
    main()
