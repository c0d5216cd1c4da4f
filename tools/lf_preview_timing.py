"""The measurements of profiles/lf_preview.md.

    python tools/lf_preview_timing.py [--runs N] [file.jxl ...]     front-end: jxf_next_frame in full and LF-only (CPU, no GPU)
    python tools/lf_preview_timing.py --kernel N                    N launches of k_lf_image at 480 x 270 cells (a 3840 x 2160 frame),
                                                                    for `rocprofv3 --kernel-trace --stats -- python tools/... --kernel N`

Front-end: every run is a process of its own with JXF_TIMING=1 and OMP_NUM_THREADS=1 (the front-end prints its phases to stderr);
the table gives the median of the runs per phase and every run's total. Default files: lenna.jxl and bbb.jxl of
tests/golden/samples, and what tests/golden/samples_large holds."""
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHILD = """
import sys
sys.path.insert(0, %r)
from jxlatte_amd import frontend
fe = frontend.Frontend(open(sys.argv[1], "rb").read())
fe.set_lf_only(sys.argv[2] == "lf")
fe.next_frame(None, None)
""" % ROOT
PHASES = ("LfGlobal", "LF groups", "HfGlobal", "pass groups")


def one_run(path, mode):
    r = subprocess.run([sys.executable, "-c", CHILD, path, mode], capture_output=True, text=True,
                       env=dict(os.environ, JXF_TIMING="1", OMP_NUM_THREADS="1"))
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[jxf\] (.{12}) ([\d.]+) ms", r.stderr)}


def frontend_table(paths, runs):
    print("| sample | decode | " + " | ".join(PHASES) + " | total, every run |\n|---|---|" + "---|" * (len(PHASES) + 1))
    for p in paths:
        for mode, label in (("full", "full"), ("lf", "LF-only")):
            rs = [one_run(p, mode) for _ in range(runs)]
            med = ["%.1f" % statistics.median(r[k] for r in rs) if k in rs[0] else "-" for k in PHASES]
            totals = ", ".join("%.1f" % sum(v for k, v in r.items() if k in PHASES) for r in rs)
            print("| `%s` | %s | %s | %s |" % (os.path.basename(p), label, " | ".join(med), totals))


def kernel_runs(n):
    import numpy as np
    from jxlatte_amd import _lib, host
    cells = (270, 480)
    q = np.random.default_rng(1).integers(-200, 200, size=(3,) + cells).astype(np.int32)
    groups = []
    for gy in range(2):
        for gx in range(2):
            groups.append(dict(lfg_y=gy, lfg_x=gx, lf_quant=[np.ascontiguousarray(q[c, gy * 256:gy * 256 + 256, gx * 256:gx * 256 + 256]) for c in range(3)],
                               extra_precision=1, scaled_dequant=[0.0004, 0.0032, 0.0064], x_factor_lf=128, b_factor_lf=128, adaptive_smoothing=True))
    xyb = ([11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863, -0.16462299647058826,
            -3.6588512862745097, 2.7129230470588235, 1.9459282392156863], [-0.0037930732552754493] * 3, [-0.15595420054924863] * 3, 255.0)
    ctx = _lib.Context(0)
    for _ in range(n):
        host.lfImage(ctx, groups, cells, 0.0, 1.0, 84, xyb=xyb, keep=True)
    ctx.close()
    print("%d launches of k_lf_image at %d x %d cells" % (n, cells[1], cells[0]))


def main(argv):
    if argv[:1] == ["--kernel"]:
        return kernel_runs(int(argv[1]))
    runs = 3
    if argv[:1] == ["--runs"]:
        runs, argv = int(argv[1]), argv[2:]
    paths = argv
    if not paths:
        paths = [os.path.join(ROOT, "tests", "golden", "samples", n) for n in ("lenna.jxl", "bbb.jxl")]
        large = os.path.join(ROOT, "tests", "golden", "samples_large")
        if os.path.isdir(large):
            paths += sorted(os.path.join(large, n) for n in os.listdir(large) if n.endswith(".jxl"))
    frontend_table(paths, runs)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
