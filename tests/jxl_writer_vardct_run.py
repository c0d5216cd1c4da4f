"""Running the cases of jxl_writer_vardct_cases.py through a decoder backend and holding the result to the model: shared by
test_jxl_writer_vardct_cpu.py (oracle backend) and test_jxl_writer_vardct_gpu.py (device backend). No oracle in any comparison."""
import numpy as np

import jxl_writer_vardct_cases as C
import vardct_ref64 as M
from jxlatte_amd import abi
from jxlatte_amd.decoder import JXLDecoder

IDCT, GAB, EPF, XYB = 1, 3, 7, 15  # vardct_ref64.decode's stage sets
CUTS = (("idct", IDCT, abi.STAGE_IDCT), ("gab", GAB, abi.STAGE_IDCT | abi.STAGE_GAB),
        ("epf", EPF, abi.STAGE_IDCT | abi.STAGE_GAB | abi.STAGE_EPF))


def k_idct(n):
    """test_vardct_ref64_cpu.k_idct: the roundings on the longest path of one sample of an n-point block"""
    return 3 + 2 + (2 * (n // 8) + 3) + 2 * n + 2


# The table of DESIGN section 3 by the class of the frame, extended by its own rules for a frame that comes from a codestream.
# Derived rows extend by their formula: the frame's LF planes are the LF stage's float32 results, not inputs, so IDCT and + Gaborish
# gain the LF stage's K (pixel_ref64: dequantisation and chroma from luma 5, smoothing 34 -- the table's "LF stage in a frame: LF
# smoothing + IDCT"). Measured rows are K = ceil(2 x the largest oracle-vs-model ratio) over the cases of the class, measured on
# the CPU (test_measured_rows_are_twice_the_largest_ratio): the rows the table had are kept as they are, FILLED names the ones these
# cases add -- + XYB at the classes it lacked, and the stage sets without Gaborish, which the table never ran (the inverse XYB cubes
# its input, so it triples the relative error of what it is given, and Gaborish is what smooths that error down).
K_LF = {True: 34, False: 5}
MEASURED = {("+ EPF", 8): 111, ("+ EPF", 32): 167, ("+ EPF", 64): 200, ("+ XYB", 32): 12, ("+ XYB", 64): 8,
            ("+ XYB", 8): 5, ("+ XYB", 16): 12, ("+ XYB", 128): 1, ("+ XYB", 256): 1,
            ("IDCT + EPF", 32): 98, ("IDCT (+ EPF) + XYB", 32): 34}
FILLED = (("+ XYB", 8), ("+ XYB", 16), ("+ XYB", 128), ("+ XYB", 256), ("IDCT + EPF", 32), ("IDCT (+ EPF) + XYB", 32))


def measured_row(src, stage):
    """the measured row of the table that holds `stage` of this frame, or None where the row is derived"""
    gab, epf, n = src.get("gab", True), src.get("epf_iters", 0) > 0, C.size_class(src)
    if stage == XYB:
        return ("+ XYB" if gab else "IDCT (+ EPF) + XYB", n)
    if stage == EPF and epf:
        return ("+ EPF" if gab else "IDCT + EPF", n)
    return None


def bound(name, stage):
    src = C.source(name)
    key = measured_row(src, stage)
    if key is not None:
        return MEASURED[key]
    g = src["lfgroups"][0]
    smoothed = not src.get("skip_smoothing", False) and min(np.asarray(g["hf_mul"]).shape) >= 3  # LFCoefficients.java:121, :133
    return k_idct(C.size_class(src)) + K_LF[smoothed] + (12 if stage != IDCT and src.get("gab", True) else 0)


def decode(data, backend, cuts=True, **switches):
    """-> dict: "idct" / "gab" / "epf" (the stage-masked runs of the frame's vardct call, padded planes; only with `cuts`), "xyb" (the
    trace cut after performColorTransforms, the frame's size), "image" (JXLImage), "stats" """
    dec = JXLDecoder(data, backend=backend, **switches)
    out = {}
    orig = backend.vardct

    def vardct(params, weights, woffs, lfgroups, groups, **kw):
        groups = list(groups)
        if cuts:
            want, xyb = params.stages, params.xyb
            plain = {k: v for k, v in kw.items() if k != "keep"}
            for stage, _, mask in CUTS:
                params.stages, params.xyb = mask, 0
                out[stage] = np.array(orig(params, weights, woffs, lfgroups, groups, **plain), copy=True)
            params.stages, params.xyb = want, xyb
        return orig(params, weights, woffs, lfgroups, groups, **kw)

    def trace(fi, stage, planes, fused):
        if stage == "xyb":
            out["xyb"] = np.stack([np.array(p, copy=True) for p in planes[:3]])
    backend.vardct = vardct
    dec.trace = trace
    try:
        out["image"] = dec.decode()
    finally:
        del backend.vardct
    out["stats"] = dec.stats
    return out


def ratio(got, name, stage, model=None):
    """the K `got` needs against the model of the case after `stage`, on the part of the padded planes `got` covers"""
    x, a = model if model is not None else C.expected(name, stage)
    got = np.asarray(got)
    h, w = got.shape[1:]
    return M.error_ratio(got, x[:, :h, :w], a[:, :h, :w])


def final_stage(name):
    """the stage set whose planes the trace cut after the colour transforms holds; None for a YCbCr frame (compared at "epf")"""
    src = C.source(name)
    if src.get("do_ycbcr", False):
        return None
    return XYB if src.get("xyb", True) else EPF
