"""Frames and boxes for the region tests (tests/test_region_cpu.py, tests/test_region_gpu.py), made with the VarDCT writer
(jxl_writer_vardct_cases.draw / fit, jxl_writer_vardct.encode) at the smallest sizes that show each thing:

  A        520 x 520, Gaborish and three EPF iterations (M = 7): 3 x 3 groups, the centre group has all eight neighbours and the last
           row and column of groups are 8 pixels
  A1, A2   the same with one and two iterations and no Gaborish (M = 2, 3)
  B, C     2312 x 40 and 40 x 2312: two LF groups side by side / on top of each other (M = 4)
  D        264 x 264 in two passes
  E        520 x 264 with the writer's NOISE_FIELD
  F1, F2   264 x 264 without XYB: with and without the YCbCr transform

What a region decode must read is computed here from the box, M and the geometry alone (expected_reads)."""
import functools

import numpy as np

import jxl_writer_vardct as V
import jxl_writer_vardct_cases as C

GROUP = 256
LF_GROUP = 2048
EPF_REACH = (0, 2, 3, 6)
TWO_LF_TYPES = (0, 1, 2, 3, 4, 7, 12, 14)


def _smooth_restoration(iters, gab):
    return dict(C._restoration(iters), gab=gab)


FRAMES = {
    "A": (lambda s: C.draw(s, 520, 520, allowed=C.MID_TYPES, **_smooth_restoration(3, True)), 501),
    "A1": (lambda s: C.draw(s, 520, 520, allowed=C.MID_TYPES, **_smooth_restoration(1, False)), 502),
    "A2": (lambda s: C.draw(s, 520, 520, allowed=C.MID_TYPES, **_smooth_restoration(2, False)), 503),
    "B": (lambda s: C.draw(s, 2312, 40, allowed=TWO_LF_TYPES, epf_iters=2, **C.SMOOTH), 504),
    "C": (lambda s: C.draw(s, 40, 2312, allowed=TWO_LF_TYPES, epf_iters=2, **C.SMOOTH), 505),
    "D": (lambda s: C.draw(s, 264, 264, allowed=C.MID_TYPES, pass_shifts=[2], amp=40, density=0.03), 506),
    "E": (lambda s: C.draw(s, 520, 264, allowed=C.MID_TYPES, density=0.03, **C.NOISE_FIELD), 507),
    "F1": (lambda s: C.draw(s, 264, 264, allowed=C.MID_TYPES, density=0.03, xyb=False, do_ycbcr=True), 508),
    "F2": (lambda s: C.draw(s, 264, 264, allowed=C.MID_TYPES, density=0.03, xyb=False), 509),
}


BOX_COUNT = dict(A=6, A1=6, A2=6, B=3, C=3, D=4, E=6, F1=4, F2=4)  # len(boxes(name)), known without building a frame


@functools.lru_cache(maxsize=None)
def source(name):
    fn, seed = FRAMES[name]
    return C.fit(fn, seed)


@functools.lru_cache(maxsize=None)
def encoded(name):
    return V.encode(source(name), None)


def size(name):
    src = source(name)
    return src["width"], src["height"]


def margin(name):
    """M from the settings the case chose: Gaborish reaches 1 pixel, the EPF 2, 3 or 6 for 1, 2 or 3 iterations"""
    src = source(name)
    return (1 if src.get("gab", True) else 0) + EPF_REACH[src.get("epf_iters", 0)]


def boxes(name):
    """the boxes (x0, y0, w, h) of a frame"""
    w, h = size(name)
    m = margin(name)
    if name in ("A", "A1", "A2"):
        out = [(256 + m, 256 + m, 256 - 2 * m, 256 - 2 * m), (256 + m - 1, 256 + m - 1, 256 - 2 * m + 1, 256 - 2 * m + 1), (0, 0, 8, 8),
               (519, 519, 1, 1), (518, 518, 2, 2), (0, 0, 520, 520)]
        if name == "A":
            assert out[:2] == [(263, 263, 242, 242), (262, 262, 243, 243)]
        return out
    if name == "B":
        return [(2048 + m, 0, 200, 40), (2048 + m - 1, 0, 200, 40), (1000, 4, 224, 30)]
    if name == "C":
        return [(0, 2048 + m, 40, 200), (0, 2048 + m - 1, 40, 200), (4, 1000, 30, 224)]
    if name == "E":  # the noise test's windows
        return [(0, 0, 20, 20), (250, 0, 12, 264), (500, 244, 20, 20), (255, 255, 2, 2), (0, 0, 520, 264), (519, 263, 1, 1)]
    return [(0, 0, 16, 16), (w // 2 - 20, h // 2 - 20, 40, 40), (250, 250, 14, 14), (0, 0, w, h)]


def expected_reads(frame_w, frame_h, box, m, padded=None):
    """(groups, LF groups) a region decode reads: the box grown by m, clipped to the padded frame, in 256-pixel groups (padding lies
    in the last real pixel's group), and the 2048-pixel LF groups that hold those groups"""
    pw, ph = padded or (-(-frame_w // 8) * 8, -(-frame_h // 8) * 8)
    x0, y0, w, h = box
    cols, rows = -(-frame_w // GROUP), -(-frame_h // GROUP)
    gx0, gy0 = max(0, x0 - m) // GROUP, max(0, y0 - m) // GROUP
    gx1, gy1 = min((min(pw, x0 + w + m) - 1) // GROUP, cols - 1), min((min(ph, y0 + h + m) - 1) // GROUP, rows - 1)
    return (gx1 - gx0 + 1) * (gy1 - gy0 + 1), ((gx1 >> 3) - (gx0 >> 3) + 1) * ((gy1 >> 3) - (gy0 >> 3) + 1)


def crop(planes, box):
    x0, y0, w, h = box
    return [np.ascontiguousarray(p[y0:y0 + h, x0:x0 + w]) for p in planes]
