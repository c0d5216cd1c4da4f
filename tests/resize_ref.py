"""A numpy model of the resized tensor exit's filter, written from the contract's formulas:

taps(L, O, filter): per axis, in float64 -- s = L / O, fs = max(s, 1), sup = r * fs (r = 1 triangle, 0.5 box); for output o:
c = (o + 0.5) * s, lo = max(0, floor(c - sup + 0.5)), hi = min(L, floor(c + sup + 0.5)); weight of j in [lo, hi) with
t = (j + 0.5 - c) / fs: triangle max(0, 1 - |t|), box 1 where -0.5 < t <= 0.5 else 0; divided by their sum (ascending j), rounded
to float32; trailing, then leading zero weights dropped, one tap kept at least. Returns a list of (first, float32 weights).

resample(plane, ytaps, xtaps): float32, every product and sum rounded separately, the vertical pass first, each sum sequential
in ascending index: V = wy[0] * S(y0), V = V + wy[k] * S(y0 + k); R = wx[0] * V(x0), R = R + wx[k] * V(x0 + k)."""
import math

import numpy as np

F = np.float32
TRIANGLE, BOX = 0, 1


def taps(L, O, filt):
    s = L / O
    fs = max(s, 1.0)
    sup = (0.5 if filt == BOX else 1.0) * fs
    out = []
    for o in range(O):
        c = (o + 0.5) * s
        lo = max(0, math.floor(c - sup + 0.5))
        hi = min(L, math.floor(c + sup + 0.5))
        w = []
        for j in range(lo, hi):
            t = ((j + 0.5) - c) / fs
            if filt == BOX:
                w.append(1.0 if -0.5 < t <= 0.5 else 0.0)
            else:
                w.append(max(0.0, 1.0 - abs(t)))
        total = 0.0
        for v in w:  # (sequential: numpy's sum is pairwise)
            total += v
        w = [F(v / total) for v in w]
        while len(w) > 1 and w[-1] == 0:
            w.pop()
        while len(w) > 1 and w[0] == 0:
            w.pop(0)
            lo += 1
        out.append((lo, np.array(w, F)))
    return out


def _pass(rows, tp):
    """rows: [L, ...] float32; the filter along axis 0 -> [O, ...]"""
    out = np.empty((len(tp),) + rows.shape[1:], F)
    for o, (first, w) in enumerate(tp):
        acc = w[0] * rows[first]
        for k in range(1, len(w)):
            acc = acc + w[k] * rows[first + k]
        out[o] = acc
    return out


def resample(plane, ytaps, xtaps, box=None):
    """plane: 2-D float32; box: (x0, y0, w, h) of the plane the taps are relative to (default: the whole plane)"""
    p = np.asarray(plane, F)
    if box is not None:
        x0, y0, bw, bh = box
        p = p[y0:y0 + bh, x0:x0 + bw]
    with np.errstate(all="ignore"):
        v = _pass(p, ytaps)
        return np.ascontiguousarray(_pass(np.ascontiguousarray(v.T), xtaps).T)
