#!/usr/bin/env python3
"""Vector-instruction budget of one kernel from its gfx950 assembly listing: a counting aid for
profiles/restore_valu_budget.md.

    hipcc <the library's flags for k_restore_fused.hip> --offload-device-only -S k_restore_fused.hip -o k.s
    python tools/restore_valu_budget.py k.s --kernel 'k_restore_fusedILb1ELi2ELi0ELi1E' \
        --stages load,gab,gab-writeback,epf1,epf1-writeback,epf2+sink --skip %bb.12...LBB18_15 ...

It classifies mnemonics by regular expression and prints a table; it judges nothing.

  * The kernel's text is cut into segments at every s_barrier; --stages names the segments in order (equal names are summed,
    missing names become seg<N>).
  * Dynamic count = static count x trip count. A loop is a label that a later branch jumps back to; every instruction between
    the label and that branch is weighted by --trip LABEL=N (default --default-trip, the channel loops' 3). Nested loops multiply.
  * Forward branches are ignored: an exec-masked block counts for every lane. Code that a workgroup-uniform branch keeps an
    interior tile out of (edge loads, mirror fix-up) is taken out with --skip FROM..TO (two labels or basic-block
    comments such as %bb.12, FROM inclusive, TO exclusive).
  * The labels are the compiler's and change with every build: --branches lists the barriers, the workgroup-uniform branches and
    the labels, from which the edge-only ranges are read off (the tile load's `else` arm, each mirror fix-up between a uniform branch
    and its target, and since the stage paths split the whole edge arm behind the uniform branch that follows Gaborish's last barrier).
    --skip FROM.. (no TO) reaches to the end of the kernel: the plain-division blocks that the compiler places behind s_endpgm.
  * --per-pixel THREADS/PIXELS scales the per-thread counts (default 512 threads per 62 x 30 output pixels).
"""
import argparse
import re
import sys
from collections import OrderedDict

CLASSES = OrderedDict([
    # the reference's f32 arithmetic (the division expansion included: v_div_*, v_rcp, v_fma)
    ("f32", re.compile(r"^v_(pk_)?(add|sub|subrev|mul|max|min|fma|fmac|mac|mad)_f32|^v_(rcp|div_scale|div_fmas|div_fixup)_f32")),
    # transfer-function pieces of the sinks (absent from the float-plane variant)
    ("f32-special", re.compile(r"^v_(exp|log|sqrt|rsq|ldexp|frexp_\w+|fract|floor|ceil|rndne|trunc|med3)_f32")),
    ("cvt", re.compile(r"^v_cvt_")),
    ("mov/sel/cmp", re.compile(r"^v_(mov|cndmask|cmp|cmpx|readlane|readfirstlane|writelane|accvgpr|swap|perm|bfi|mbcnt)")),
    ("int/addr", re.compile(r"^v_")),  # whatever is left: integer, shift, logic and address arithmetic
])
OTHER = OrderedDict([
    ("lds", re.compile(r"^ds_")),
    ("vmem", re.compile(r"^(global|buffer|flat|scratch)_")),
    ("salu", re.compile(r"^s_(?!waitcnt|nop|barrier|endpgm|cbranch|branch|setprio|sleep)")),
])


def kernel_lines(text, pattern):
    rx = re.compile(pattern)
    lines = text.splitlines()
    start = None
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if start is None and m and not m.group(1).startswith(".L") and rx.search(m.group(1)):
            start = i + 1
        elif start is not None and l.startswith(".Lfunc_end"):
            return lines[start:i]
    if start is None:
        sys.exit("no kernel matches %r" % pattern)
    return lines[start:]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", required=True, help="regular expression on the kernel's (mangled) symbol")
    ap.add_argument("--stages", default="", help="comma-separated names of the segments between barriers")
    ap.add_argument("--trip", action="append", default=[], metavar="LABEL=N")
    ap.add_argument("--default-trip", type=float, default=3.0)
    ap.add_argument("--skip", action="append", default=[], metavar="FROM..TO")
    ap.add_argument("--per-pixel", default="512/1860", help="threads/pixels, e.g. 512/1860")
    ap.add_argument("--loops", action="store_true", help="list the loops found and the weights used")
    ap.add_argument("--branches", action="store_true",
                    help="list barriers, workgroup-uniform branches (scc / vcc) and the labels they reach: what --stages and --skip are chosen from")
    a = ap.parse_args()

    body = kernel_lines(open(a.asm).read(), a.kernel)
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.L\w+):", l) or re.match(r"^; (%bb\.\d+):", l)
        if m:
            label_at[m.group(1)] = i
    weight = [1.0] * len(body)
    trips = dict((k, float(v)) for k, v in (t.split("=") for t in a.trip))
    last_back = OrderedDict()  # loop header -> its last back edge
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.L\w+)", l)
        # (the compiler marks loop headers in the label's comment; other backward branches only reach blocks placed out of line)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i and "Loop Header" in body[label_at[m.group(1)]]:
            last_back[m.group(1)] = i
    loops = []
    for lab, i in last_back.items():
        n = trips.get(lab, a.default_trip)
        loops.append((lab, label_at[lab], i, n))
        for j in range(label_at[lab], i + 1):
            weight[j] *= n
    for s in a.skip:
        lo, hi = s.split("..")
        # (an empty TO: to the end of the kernel's text -- the out-of-line blocks placed behind s_endpgm)
        for j in range(label_at[lo], label_at[hi] if hi else len(body)):
            weight[j] = 0.0
    if a.branches:
        for i, l in enumerate(body):
            t = l.strip()
            if t.startswith("s_barrier") or re.match(r"s_cbranch_(scc|vcc)", t) or re.match(r"^(\.L\w+):|^; (%bb\.\d+):", l) and i in label_at.values():
                if t.startswith(("s_", ".LBB")) or "Loop Header" in l:
                    print("%5d  %s" % (i, t.split(";")[0].strip()))
        return
    if a.loops:
        for lab, lo, hi, n in loops:
            print("loop %-12s lines %5d-%5d  x %g" % (lab, lo, hi, n))

    names = [s for s in a.stages.split(",") if s]
    table = OrderedDict()
    seg = 0
    cols = list(CLASSES) + list(OTHER)
    for i, l in enumerate(body):
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        mn = t.split()[0]
        if mn == "s_barrier":
            if weight[i] > 0:
                seg += 1
            continue
        name = names[seg] if seg < len(names) else "seg%d" % seg
        row = table.setdefault(name, OrderedDict((c, 0.0) for c in cols))
        for group in (CLASSES, OTHER):
            for c, rx in group.items():
                if rx.search(mn):
                    row[c] += weight[i]
                    break
            else:
                continue
            break

    num, den = (float(x) for x in a.per_pixel.split("/"))
    scale = num / den
    valu = list(CLASSES)
    print("| stage | " + " | ".join(valu) + " | VALU / thread | VALU / output px | " + " | ".join(OTHER) + " |")
    print("|---|" + "---:|" * (len(cols) + 2))
    tot = OrderedDict((c, 0.0) for c in cols)
    for name, row in table.items():
        v = sum(row[c] for c in valu)
        for c in cols:
            tot[c] += row[c]
        print("| %s | " % name + " | ".join("%g" % row[c] for c in valu) + " | %g | %.1f | " % (v, v * scale)
              + " | ".join("%g" % row[c] for c in OTHER) + " |")
    v = sum(tot[c] for c in valu)
    print("| **total** | " + " | ".join("%g" % tot[c] for c in valu) + " | %g | %.1f | " % (v, v * scale)
          + " | ".join("%g" % tot[c] for c in OTHER) + " |")
    print()
    print("per output pixel by class: " + ", ".join("%s %.1f" % (c, tot[c] * scale) for c in valu))


if __name__ == "__main__":
    main()
