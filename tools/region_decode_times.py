"""The measurements of profiles/region_decode.md: what the front-end no longer does for a region (CPU, no GPU).

    python tools/region_decode_times.py [--runs N] [--writer WxH | --no-writer] [file.jxl ...]
    python tools/region_decode_times.py --kernel N      N calls of jxl_planes_noise_at on a centred 224 x 224 window of a 3840 x 2160
                                                        frame, for `rocprofv3 --kernel-trace --stats -- python tools/... --kernel N`

jxf_next_frame of the whole frame against a centred 224 x 224 region (jxf_set_region), N runs each (default 9) in ONE process per
thread setting -- OpenMP pinned to one thread, and at its default -- the two decodes taking turns; the table gives the medians,
the groups, LF groups and section bytes read, and the shares. Default inputs: lenna.jxl and bbb.jxl of tests/golden/samples, what
tests/golden/samples_large holds, and a frame made by the tests' VarDCT writer (default 3840x2160: the largest it makes in under a
minute here; the time it took is printed)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHILD = """
import json, sys, time
sys.path.insert(0, %r)
from jxlatte_amd import frontend
data = open(sys.argv[1], "rb").read()
runs = int(sys.argv[2])
fe = frontend.Frontend(data)
w, h = fe.image.width, fe.image.height
box = (max(0, w // 2 - 112), max(0, h // 2 - 112), min(224, w), min(224, h))
times, plan = dict(full=[], region=[]), None
for i in range(runs + 1):  # (the first round warms the process up: tables made once, the file in the page cache)
    for mode in ("full", "region"):
        fe = frontend.Frontend(data)
        fe.set_region(box if mode == "region" else None)
        t = time.perf_counter()
        fe.next_frame(None, None)
        dt = time.perf_counter() - t
        if i:
            times[mode].append(1e3 * dt)
        if mode == "region":
            plan = fe.region_plan()
        fe.close()
print(json.dumps(dict(size=(w, h), box=box, times=times, plan=plan)))
""" % ROOT


def measure(path, runs, threads):
    env = dict(os.environ)
    env.pop("JXF_TIMING", None)
    if threads:
        env["OMP_NUM_THREADS"] = str(threads)
    else:
        env.pop("OMP_NUM_THREADS", None)
    r = subprocess.run([sys.executable, "-c", CHILD, path, str(runs)], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def writer_frame(width, height, out_dir):
    """a frame of the tests' VarDCT writer with Gaborish and two EPF iterations (M = 4), written to out_dir; returns (path, seconds)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jxl_writer_vardct as V
    import jxl_writer_vardct_cases as C
    t = time.time()
    src = C.fit(lambda s: C.draw(s, width, height, allowed=C.MID_TYPES, epf_iters=2, **C.SMOOTH), 900)
    data = V.encode(src, None)
    took = time.time() - t
    path = os.path.join(out_dir, "writer_%dx%d.jxl" % (width, height))
    with open(path, "wb") as f:
        f.write(data)
    return path, took


def kernel_runs(n):
    import numpy as np
    from jxlatte_amd import _lib, host
    frame_h, frame_w, h, w = 2160, 3840, 224, 224
    y0, x0 = (frame_h - h) // 2, (frame_w - w) // 2
    rng = np.random.default_rng(1)
    planes = np.stack([rng.uniform(-0.5, 0.5, (h, w)), rng.uniform(0, 1.5, (h, w)), rng.uniform(0, 1, (h, w))]).astype(np.float32)
    lut = np.array([0, 300, 1023, 640, 900, 120, 0, 512], np.float32) / np.float32(1024)
    ctx = _lib.Context(0)
    rp = host.ResidentPlanes.upload(ctx, planes)
    for _ in range(n):
        rp.noiseAt(256, 1 << 32, lut, 0.0, 1.0, frame_h, frame_w, y0, x0)
    rp.download()
    ctx.close()
    print("%d calls of jxl_planes_noise_at: a %d x %d window at (%d, %d) of a %d x %d frame" % (n, w, h, x0, y0, frame_w, frame_h))


def main(argv):
    import tempfile
    if argv[:1] == ["--kernel"]:
        return kernel_runs(int(argv[1]))
    runs, writer, paths = 9, (3840, 2160), []
    while argv:
        a = argv.pop(0)
        if a == "--runs":
            runs = int(argv.pop(0))
        elif a == "--writer":
            writer = tuple(int(v) for v in argv.pop(0).lower().split("x"))
        elif a == "--no-writer":
            writer = None
        else:
            paths.append(a)
    if not paths:
        paths = [os.path.join(ROOT, "tests", "golden", "samples", n) for n in ("lenna.jxl", "bbb.jxl")]
        large = os.path.join(ROOT, "tests", "golden", "samples_large")
        if os.path.isdir(large):
            paths += sorted(os.path.join(large, n) for n in os.listdir(large) if n.endswith(".jxl"))
    with tempfile.TemporaryDirectory() as tmp:
        if writer:
            path, took = writer_frame(writer[0], writer[1], tmp)
            print("the writer made %s (%d bytes) in %.1f s\n" % (os.path.basename(path), os.path.getsize(path), took))
            paths.append(path)
        print("| input | size | threads | full (ms) | region (ms) | region / full | groups | LF groups | section bytes | M |\n|---|---|---|---|---|---|---|---|---|---|")
        for p in paths:
            for threads in (1, 0):
                m = measure(p, runs, threads)
                f, r, pl = statistics.median(m["times"]["full"]), statistics.median(m["times"]["region"]), m["plan"]
                print("| `%s` | %dx%d | %s | %.1f | %.1f | %.2f | %d of %d | %d of %d | %d of %d (%.0f %%) | %d |" % (
                    os.path.basename(p), m["size"][0], m["size"][1], threads or "default", f, r, r / f, pl["groups_read"], pl["groups_total"],
                    pl["lf_groups_read"], pl["lf_groups_total"], pl["section_bytes_read"], pl["section_bytes_total"],
                    100.0 * pl["section_bytes_read"] / pl["section_bytes_total"], pl["margin"]))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
