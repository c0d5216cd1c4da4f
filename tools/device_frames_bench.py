"""device_frames against device_canvas alone (profiles/device_frames.md). Medians of alternating rounds; nothing here is a pass / fail
threshold.

    python tools/device_frames_bench.py [--rounds N]

For blendmodes_5.jxl and wb-rainbow.jxl: JXLDecoder(device_canvas=True, device_splines=True).decode() with device_frames off and on,
in turn, each ending in a synchronise of the context; the bytes each frame moves over the bus in either arm -- the blend path's
(stats[k]["blend_bus"]) plus what the host route's backend hooks take up and bring down (rct, squeeze, upsample, modular_to_float,
keep_planes: counted here, around the hooks), with stats[k]["plane_moves"] -- and the front-end alone (entropy decoding: the same
work in both arms). The images of the two arms are compared first. Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jxlatte_amd import frontend  # noqa: E402
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder  # noqa: E402


HOOKS = ("rct", "squeeze", "upsample", "modular_to_float", "keep_planes")


def _nbytes(v):
    if isinstance(v, np.ndarray):
        return v.nbytes
    if isinstance(v, (list, tuple)):
        return sum(_nbytes(x) for x in v)
    return 0


class CountingBackend(DeviceBackend):
    """the device backend with the bytes its host-route hooks move: hook_bus = [up, down]"""
    hook_bus = [0, 0]


for _name in HOOKS:
    def _counted(self, *a, _name=_name, **kw):
        r = getattr(DeviceBackend, _name)(self, *a, **kw)
        self.hook_bus[0] += _nbytes(a)
        self.hook_bus[1] += _nbytes(r)
        return r
    setattr(CountingBackend, _name, _counted)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    be = CountingBackend(0)
    for name in ("blendmodes_5", "wb-rainbow"):
        with open(os.path.join(ROOT, "tests", "golden", "samples", name + ".jxl"), "rb") as f:
            data = f.read()

        def run(on, keep=False):
            be.hook_bus = [0, 0]
            t0 = time.perf_counter()
            dec = JXLDecoder(data, backend=be, device_canvas=True, device_splines=True, device_frames=on)
            im = dec.decode()
            be.ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            dec.stats[-1]["hook_bus_image"] = tuple(be.hook_bus)  # (the hooks of all frames of the image)
            out = (ms, dec.stats, [b.copy() for b in im.getBuffer()] if keep else None)
            im.close()
            dec.close()
            return out

        def fe_only():
            t0 = time.perf_counter()
            fe = frontend.Frontend(data)
            fe.set_defer_transforms(True)
            while True:
                fr = fe.next_frame(None, None, None)
                if fr is None or fr.is_last:
                    break
            ms = (time.perf_counter() - t0) * 1e3
            fe.close()
            return ms
        # warm-up of both arms, and the comparison of their images
        _, stats_off, planes_off = run(False, keep=True)
        _, stats_on, planes_on = run(True, keep=True)
        assert all(x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(planes_off, planes_on))
        fe_only()
        ms = dict(off=[], on=[], frontend=[])
        for _ in range(a.rounds):
            ms["off"].append(run(False)[0])
            ms["on"].append(run(True)[0])
            ms["frontend"].append(fe_only())
        line = dict(what="%s.jxl, decode() + synchronise with device_canvas + device_splines: device_frames off | on" % name,
                    rounds=a.rounds, routes_on=[s["frame"] for s in stats_on],
                    bus_off=[s["blend_bus"] for s in stats_off], bus_on=[s["blend_bus"] for s in stats_on],
                    hook_bus_image_off=stats_off[-1]["hook_bus_image"], hook_bus_image_on=stats_on[-1]["hook_bus_image"],
                    plane_moves_off=[s.get("plane_moves") for s in stats_off], plane_moves_on=[s.get("plane_moves") for s in stats_on])
        for k, v in ms.items():
            line[k + "_ms_median"] = round(statistics.median(v), 3)
            line[k + "_ms_min"] = round(min(v), 3)
            line[k + "_ms_max"] = round(max(v), 3)
        line["pairs_ms"] = [(round(x, 1), round(y, 1)) for x, y in zip(ms["off"], ms["on"])]
        print(json.dumps(line), flush=True)
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
