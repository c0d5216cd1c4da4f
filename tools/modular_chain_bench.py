"""device_chains on patches-lossless.jxl (profiles/modular_chain.md). Measurements, no pass / fail threshold.

    python tools/modular_chain_bench.py [--rounds N] [--decodes N]

The chain of frame 1 (1600 x 1096: four nested Palette transforms over one index channel and four palette channels), three arms
taken in turn within every round, all on the same encoded channels:
  fused   one plan of jxl_modular_begin_chain, its Palette run as ONE k_palette_run launch: jxl_modular_run to a synchronise
  steps   the same plan with jxl_debug_set_palette_fuse(0): four k_palette_lookup launches on the plan's device channels
  stage   what the decoder does without device_chains but with device_palette: four jxl_stage_palette calls, each of which sends its index
          plane up and brings its planes down (the front-end's hook order: the 4-channel palette, then the three 1-channel ones)
`fused` and `steps` are also timed with the plan's build in front (jxl_modular_begin_chain: the upload of the encoded channels),
which is the part of a decode they stand for; `stage` has its transfers inside by construction.
Then the decoder end to end, two arms taken in turn: device_canvas + device_patches + device_patch_sets + device_frames with and
without device_chains (without it: the route of the commit before the switch), decode() to a synchronise.
One JSON line per arm with every time in ms, the median, the minimum and the maximum."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl")


def _line(arm, times, **more):
    t = [round(v * 1e3, 3) for v in times]
    print(json.dumps(dict(arm=arm, ms=t, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), **more)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--decodes", type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from jxlatte_amd import frontend, host
    from jxlatte_amd.decoder import DeviceBackend, JXLDecoder
    fe = frontend.Frontend(open(SAMPLE, "rb").read())
    fe.set_defer_transforms(True)
    fe.next_frame(None, None)
    fe.next_frame(None, None)
    transforms = fe.transforms()
    chans = [fe.modular_channel(i)[0].copy() for i in range(fe.modular_channel_count())]
    depth = fe.image.bits_per_sample
    fe.close()
    be = DeviceBackend()
    ctx = be.ctx

    def plan(fuse, build):
        host.setPaletteFuse(ctx, fuse)
        ms = host.ModularStream(ctx, chans, transforms=transforms, bitDepth=depth)
        if not build:
            ms.begin()
            ctx.synchronize()
        t0 = time.perf_counter()
        ms.run()
        ctx.synchronize()
        t1 = time.perf_counter()
        out = ms.getDecodedBuffer()
        return t1 - t0, out, host.lastPaletteRun(ctx)

    def stage():
        ch = list(chans)
        t0 = time.perf_counter()
        for t in reversed(transforms):
            first = t["begin_c"] + 1
            planes = host.inversePalette(ctx, ch[first], ch[0], t["num_c"], t["nb_colors"], t["nb_deltas"], t["d_pred"], depth)
            ch[first:first + 1] = list(planes)
            del ch[0]
        t1 = time.perf_counter()
        return t1 - t0, ch
    try:
        times = {k: [] for k in ("fused", "steps", "fused+build", "steps+build", "stage")}
        forms = {}
        for r in range(a.rounds + 2):  # two warm-up rounds
            got = {}
            for arm, fuse, build in (("fused", True, False), ("steps", False, False), ("fused+build", True, True), ("steps+build", False, True)):
                dt, got[arm], forms[arm] = plan(fuse, build)
                if r >= 2:
                    times[arm].append(dt)
            dt, got["stage"] = stage()
            if r >= 2:
                times["stage"].append(dt)
            if r == 0:
                for arm, out in got.items():
                    assert len(out) == len(got["stage"]) and all(np.array_equal(x, y) for x, y in zip(out, got["stage"])), arm
        host.setPaletteFuse(ctx, True)
        samples = int(chans[-1].size)
        for arm in times:
            _line(arm, times[arm], palette_launches=forms.get(arm), samples=samples, encoded_bytes=sum(c.nbytes for c in chans))
        kw = dict(device_canvas=True, device_patches=True, device_patch_sets=True, device_frames=True)
        wall = {True: [], False: []}
        rows = {}
        for r in range(a.decodes + 1):
            for chains in (True, False):
                t0 = time.perf_counter()
                dec = JXLDecoder(SAMPLE, backend=be, device_chains=chains, **kw)
                im = dec.decode()
                ctx.synchronize()
                t1 = time.perf_counter()
                rows[chains] = [dict(frame=st["frame"], canvas=st["canvas"], blend_bus=list(st["blend_bus"]), chain=st.get("chain")) for st in dec.stats]
                im.close()
                dec.close()
                if r:
                    wall[chains].append(t1 - t0)
        _line("decode, device_chains", wall[True], frames=rows[True])
        _line("decode, switch off", wall[False], frames=rows[False])
    finally:
        be.close()


if __name__ == "__main__":
    main()
