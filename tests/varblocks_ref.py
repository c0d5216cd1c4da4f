"""The independent model of Frame.drawVarblocks (Frame.java:464-503), written from the Java semantics in numpy: float32 with
every product, sum and quotient rounded on its own, (float)Math.cos and (float)Math.cbrt as numpy's double-precision functions
cast back. It calls nothing of jxlatte_amd and walks the block list the way the reference does -- block by block, with no cell
map -- so it shares no structure with the kernel. The type sizes come from include/jxl_transform_types.h."""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _type_sizes():
    hdr = open(os.path.join(ROOT, "include", "jxl_transform_types.h")).read()
    rows = re.findall(r"\{(\d+), \d+, \d+, JXL_METHOD_\w+, (\d+), (\d+)\},", hdr)
    assert [int(r[0]) for r in rows] == list(range(27))
    return [(int(r[1]), int(r[2])) for r in rows]  # (pixelHeight, pixelWidth) by type


TYPE_SIZES = _type_sizes()
PHI_BAR = F(np.sqrt(np.float64(5.0)) * 0.5 - 0.5)  # MathHelper.PHI_BAR
PI = F(np.pi)                                      # (float)Math.PI


def _cos(x):
    return F(np.cos(np.float64(F(x))))


def factors(t):
    """(rFactor, gFactor, bFactor) of transform type t (Frame.java:476-479)"""
    hue = F(F(np.fmod(F(F(t) * PHI_BAR), F(1.0))) * F(2.0)) * PI
    r = F(F(_cos(hue) + F(0.5)) / F(1.5))
    g = F(F(_cos(F(hue - F(F(F(2.0) * PI) / F(3.0)))) + F(1.0)) / F(2.0))
    b = F(F(_cos(F(hue - F(F(F(4.0) * PI) / F(3.0)))) + F(1.0)) / F(2.0))
    return r, g, b


def light_root(r, g, b):
    """the float64 cube root Math.cbrt sees for float32 arrays r, g, b (before its cast back to float)"""
    with np.errstate(all="ignore"):
        light = (F(0.25) * (r + b)).astype(F) + (F(0.5) * g).astype(F)
        return np.cbrt(light.astype(np.float64))


def draw(planes, blocks):
    """planes: three float32 arrays of one shape; blocks: rows (cy, cx, type) in frame cells. Returns three new planes: the
    pixels of every block's extent that lie inside the planes redrawn, the others untouched"""
    out = [np.array(p, F, copy=True) for p in planes]
    h, w = out[0].shape
    for cy, cx, t in np.asarray(blocks, np.int64).reshape(-1, 3):
        ph, pw = TYPE_SIZES[t]
        y0, x0 = cy << 3, cx << 3
        y1, x1 = min(y0 + ph, h), min(x0 + pw, w)
        if y1 <= y0 or x1 <= x0:
            continue
        fac = factors(int(t))
        r, g, b = (out[c][y0:y1, x0:x1].copy() for c in range(3))
        with np.errstate(all="ignore"):
            light = (light_root(r, g, b).astype(F) * F(0.5)).astype(F) + F(0.25)
            new = [(F(fac[c] * F(0.5)) + ((F(0.5) * s).astype(F) / light).astype(F)).astype(F) for c, s in enumerate((r, g, b))]
        for c in range(3):
            new[c][0, :] = F(0)  # y == 0
            new[c][:, 0] = F(0)  # x == 0
            out[c][y0:y1, x0:x1] = new[c]
    return out
