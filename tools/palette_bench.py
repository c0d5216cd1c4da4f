"""The inverse Palette transform of the frame-level Modular stream, device stage against the front-end's own loop, on the same
inputs:

  * the four palettes of frame 2 of tests/golden/samples/patches-lossless.jxl (1096 x 1600: one of four channels, three of one),
    captured through the front-end's palette hook
  * one synthetic 4096 x 4096 four-channel palette of 256 colours without a delta pixel (one launch), and the same with one pixel
    in a hundred a delta pixel under predictor 5 (the chain kernel runs behind the lookup kernel)

    python tools/palette_bench.py [--rounds 5] [--size 4096]
    python tools/palette_bench.py --kernels 3       # only stage calls, for a kernel trace: every input 3 times
    python tools/palette_bench.py --build-only      # build the CPU harness and stop (no GPU needed)

Per input: the median and the range of the wall clock around jxl_stage_palette (uploads, launches, downloads: the call returns
with the planes on the host) after one warm-up call, its launches and delta pixels, and the front-end's loop on the same input
(tools/native/palette_cpu_bench.cpp: ModularStream::apply_transforms alone, best and median of the rounds), whose result must
hash to the device's. Prints one JSON line. The timed paths need a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "tools", "native", "palette_cpu_bench")


def build_cpu_harness():
    fe = os.path.join(ROOT, "jxlatte_amd", "frontend")
    srcs = [os.path.join(ROOT, "tools", "native", "palette_cpu_bench.cpp"), os.path.join(fe, "modular.cc"), os.path.join(fe, "entropy.cc")]
    deps = srcs + [os.path.join(fe, f) for f in ("modular.h", "entropy.h", "bits.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fwrapv", "-fopenmp", "-Wall"] + srcs + ["-o", EXE])
    return EXE


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        for c in cases:
            pal = np.ascontiguousarray(c["palette"], np.int32)
            f.write(np.array([c["index"].shape[0], c["index"].shape[1], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"],
                              pal.shape[0], pal.shape[1], int(c["pred"] is not None)], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["index"], np.int32).tobytes())
            f.write(pal.tobytes())
            if c["pred"] is not None:
                f.write(np.ascontiguousarray(c["pred"], np.int32).tobytes())


def checksum(planes_in_channel_order):
    """the hash of tools/native/palette_cpu_bench.cpp: s = s * 31 + v over every channel's samples, mod 2^32"""
    v = np.concatenate([np.asarray(p, np.int32).reshape(-1) for p in planes_in_channel_order]).view(np.uint32).astype(np.uint64)
    n = v.size
    # s = sum v[i] * 31^(n - 1 - i) mod 2^32, in blocks to keep the powers table small
    s = 0
    block = 1 << 16
    pw = np.ones(block, np.uint64)
    for i in range(1, block):
        pw[i] = (pw[i - 1] * 31) & 0xFFFFFFFF
    pw = pw[::-1].copy()
    step = int((int(pw[0]) * 31) & 0xFFFFFFFF)  # 31^block
    for at in range(0, n, block):
        chunk = v[at:at + block]
        m = chunk.size
        part = int(((chunk * pw[block - m:]) & 0xFFFFFFFF).sum() & 0xFFFFFFFF)
        s = (s * (step if m == block else pow(31, m, 1 << 32)) + part) & 0xFFFFFFFF
    return s


def inputs(size, be):
    from jxlatte_amd import frontend
    cases = []
    data = open(os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl"), "rb").read()
    fe = frontend.Frontend(data)
    seen = []

    def hook(index, palette, pred, num_c, nb_colors, nb_deltas, d_pred, bit_depth):
        seen.append(dict(index=index, palette=palette, pred=pred, num_c=num_c, nb_colors=nb_colors, nb_deltas=nb_deltas, d_pred=d_pred,
                         bit_depth=bit_depth))
        return be.palette(index, palette, pred, num_c, nb_colors, nb_deltas, d_pred, bit_depth)
    fe.next_frame(None, None, hook)
    del seen[:]
    fe.next_frame(None, None, hook)
    fe.close()
    for k, c in enumerate(seen):
        c["name"] = "patches-lossless frame 2, palette %d (%d channel%s, %d colours)" % (k + 1, c["num_c"], "s" * (c["num_c"] > 1), c["nb_colors"])
        cases.append(c)
    rng = np.random.default_rng(7)
    index = rng.integers(0, 256, (size, size)).astype(np.int32)
    palette = rng.integers(0, 256, (4, 256)).astype(np.int32)
    cases.append(dict(name="synthetic %d x %d, 4 channels, 256 colours, no delta pixel" % (size, size), index=index, palette=palette, pred=None,
                      num_c=4, nb_colors=256, nb_deltas=0, d_pred=5, bit_depth=8))
    chained = index.copy()
    at = rng.random(index.shape) < 0.01
    chained[at] = -1 - rng.integers(0, 40, int(at.sum()))
    cases.append(dict(name="synthetic %d x %d, 4 channels, 256 colours, 1 %% delta pixels, predictor 5" % (size, size), index=chained,
                      palette=palette, pred=None, num_c=4, nb_colors=256, nb_deltas=0, d_pred=5, bit_depth=8))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    exe = build_cpu_harness()
    if a.build_only:
        print(exe)
        return
    from jxlatte_amd import host
    from jxlatte_amd.decoder import DeviceBackend
    be = DeviceBackend(0)
    cases = inputs(a.size, be)

    def stage(c):
        return host.inversePalette(be.ctx, c["index"], c["palette"], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"],
                                   pred=c["pred"])
    if a.kernels:
        for c in cases:
            for _ in range(a.kernels):
                stage(c)
        be.close()
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.bin")
        write_cases(path, cases)
        cpu = subprocess.run([exe, path, str(a.rounds)], capture_output=True, text=True, check=True).stdout
    cpu_rows = {int(r.split()[1]): r.split()[2:] for r in cpu.splitlines() if r.startswith("CASE")}
    rows = []
    for i, c in enumerate(cases):
        out = stage(c)  # warm-up, and the result that is compared
        launches, deltas = host.lastPalette(be.ctx)
        ts = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            stage(c)
            ts.append((time.perf_counter() - t0) * 1e3)
        best, med, digest = cpu_rows[i]
        # the front-end leaves the stream's channels: the num_c planes (the palette channel is erased)
        same = int(digest, 16) == checksum(list(out))
        n = c["index"].size
        rows.append(dict(input=c["name"], pixels=n, launches=launches, delta_pixels=deltas,
                         stage_ms_median=round(statistics.median(ts), 3), stage_ms_min=round(min(ts), 3), stage_ms_max=round(max(ts), 3),
                         bus_bytes_up=4 * (n + c["num_c"] * c["nb_colors"]), bus_bytes_down=4 * n * c["num_c"],
                         frontend_loop_ms_best=float(best), frontend_loop_ms_median=float(med), same_samples=same))
    be.close()
    print(json.dumps(dict(rounds=a.rounds, rows=rows)))
    if not all(r["same_samples"] for r in rows):
        sys.exit("the device stage and the front-end's loop disagree")


if __name__ == "__main__":
    main()
