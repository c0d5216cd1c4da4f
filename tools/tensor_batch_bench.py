"""N distinct 3840x2160 images, three float planes each in a device plane set, as one (N, ...) batch tensor of a small size,
linear -> sRGB, F16/CHW and U8/HWC: two arms at the C ABI, alternating in one process.

  A  what there was before: N calls of jxl_canvas_tensor_resized, image i into batch[i]
  B  one call of jxl_tensor_resized_batch

    python tools/tensor_batch_bench.py [--n 1,8,32,64] [--sizes 224x224,135x240] [--pairs 6] [--calls 10] [--height 2160 --width 3840]
    python tools/tensor_batch_bench.py --kernels 5 --n 8,64     # launches only, for a kernel trace: each arm and form 5 times per N

The parameter blocks and the item array are built once, outside the timed window: both arms time the library's calls (through
ctypes), not the Python that prepares them. Per (size, N, form): median and range over `--pairs` A/B pairs (after one warm-up pair)
of the wall clock of one batch -- `--calls` batches back to back over their number; every call of either arm ends in the library's
stream synchronise -- and images per second from the median; the two arms' bytes are compared. Then what the batch call planned
(jxl_debug_tensor_batch_stats): table lookups, tables built, bytes of the one transfer, tiles, grid, LDS bytes, the tile. Prints one
JSON line per (size, N). Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jxlatte_amd import abi, host  # noqa: E402
from jxlatte_amd._lib import Context  # noqa: E402

FORMS = [("float16", "CHW"), ("uint8", "HWC")]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,8,32,64")
    ap.add_argument("--sizes", default="224x224,135x240")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_batch_bench needs a GPU")
    ns = [int(v) for v in a.n.split(",")]
    sizes = [tuple(int(v) for v in s.lower().split("x")) for s in a.sizes.split(",")]
    ctx = Context(0)
    dev = "cuda:%d" % ctx.device
    rng = np.random.default_rng(1)
    base = [rng.uniform(0, 1, (a.height, a.width)).astype(np.float32) for _ in range(3)]
    # distinct images: the base planes rolled by a different number of rows each
    sets = [host.DeviceCanvas.fromArrays(ctx, [np.roll(p, 17 * i + c, axis=0) for c, p in enumerate(base)]) for i in range(max(ns))]
    stats_fn = ctx.lib.jxl_debug_tensor_batch_stats
    stats_fn.restype, stats_fn.argtypes = C.c_int32, [C.POINTER(C.c_int64)]
    tdt = {"uint8": torch.uint8, "float16": torch.float16}
    color = dict(tfIn=abi.TF_LINEAR, tfOut=abi.TF_SRGB)
    single, batched = ctx.lib.jxl_canvas_tensor_resized, ctx.lib.jxl_tensor_resized_batch
    for size in sizes:
        for n in ns:
            res = {}
            for dtype, layout in FORMS:
                shape = (n, 3) + size if layout == "CHW" else (n,) + size + (3,)
                out_a = torch.zeros(shape, dtype=tdt[dtype], device=dev)
                out_b = torch.zeros(shape, dtype=tdt[dtype], device=dev)
                items = [host.tensorBatchItem(size, canvas=sets[i], nColor=3, dtype=dtype, layout=layout, **color) for i in range(n)]
                arr = (abi.TensorBatchItem * n)(*items)
                calls_a = [(sets[i].id, C.byref(items[i].p), C.byref(items[i].r), C.c_void_p(out_a[i].data_ptr())) for i in range(n)]
                ptr_b = C.c_void_p(out_b.data_ptr())

                def arm_a():
                    for id_, p, r, ptr in calls_a:
                        if single(ctx.h, id_, -1, p, r, ptr) != 0:
                            raise SystemExit(ctx.lib.jxl_last_error(ctx.h))

                def arm_b():
                    if batched(ctx.h, n, arr, ptr_b) != 0:
                        raise SystemExit(ctx.lib.jxl_last_error(ctx.h))
                if a.kernels:
                    for _ in range(a.kernels):
                        arm_a()
                        arm_b()
                    continue
                times = {"A": [], "B": []}
                for r in range(a.pairs + 1):  # pair 0 warms up
                    for k, fn in (("A", arm_a), ("B", arm_b)):
                        t0 = time.perf_counter()
                        for _ in range(a.calls):
                            fn()
                        dt = (time.perf_counter() - t0) * 1e3 / a.calls
                        if r:
                            times[k].append(dt)
                assert torch.equal(out_a.view(torch.uint8), out_b.view(torch.uint8)), "the two arms give different bytes"
                st = (C.c_int64 * 8)()
                stats_fn(st)
                e = {}
                for k, v in times.items():
                    med = statistics.median(v)
                    e[k] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), images_per_s=round(n / (med * 1e-3), 1),
                                all_ms=[round(x, 4) for x in v])
                e["B_over_A"] = round(e["B"]["median_ms"] / e["A"]["median_ms"], 4)
                e["batch_call"] = dict(table_lookups=st[0], tables_built=st[1], tables_shared=st[0] - st[1], transfer_bytes=st[2], tiles=st[3], grid=st[4],
                                       lds_bytes=st[5], tile="%dx%d" % (st[6], st[7]))
                res["%s/%s" % (dtype, layout)] = e
            if not a.kernels:
                print(json.dumps(dict(height=a.height, width=a.width, out_height=size[0], out_width=size[1], n=n, pairs=a.pairs, calls=a.calls,
                                      plane_bytes_per_image=3 * 4 * a.height * a.width, forms=res)), flush=True)
    for s in sets:
        s.release()
    ctx.close()


if __name__ == "__main__":
    main()
