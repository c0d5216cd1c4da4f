"""Running the cases of jxl_writer_vardct_cases.py through a decoder backend and holding the result to the model: shared by
test_jxl_writer_vardct_cpu.py (oracle backend) and test_jxl_writer_vardct_gpu.py (device backend). No oracle in any comparison."""
import numpy as np

import jxl_writer_vardct as V
import jxl_writer_vardct_cases as C
import vardct_ref64 as M
from jxlatte_amd import abi
from jxlatte_amd.decoder import JXLDecoder

IDCT, GAB, EPF, XYB = 1, 3, 7, 15  # vardct_ref64.decode's stage sets
TAIL = 31  # jxl_writer_vardct_cases.expected_image: upsampling, noise and the colour transforms after the EPF
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
# The rows of a frame's tail (stage set TAIL) are named after what runs between the EPF and the trace cut after the colour transforms:
# "+ upsample (+ XYB)", "+ noise + XYB" (an upsampled frame with noise is in this one), "+ YCbCr" (after invertSubsampling where
# the frame is subsampled); a frame that writes an opsin matrix of its own has "+ XYB, custom opsin" and leaves the rows of the
# default matrix as they were. These rows are not split by the size class of the frame's largest transform (their key has 0 in its
# place): what the tail adds to a sample's error does not depend on the transform that made the sample.
MEASURED = {("+ EPF", 8): 111, ("+ EPF", 32): 167, ("+ EPF", 64): 200, ("+ XYB", 32): 12, ("+ XYB", 64): 8,
            ("+ XYB", 8): 5, ("+ XYB", 16): 12, ("+ XYB", 128): 1, ("+ XYB", 256): 1,
            ("IDCT + EPF", 32): 98, ("IDCT (+ EPF) + XYB", 32): 34,
            ("+ upsample (+ XYB)", 0): 6, ("+ noise + XYB", 0): 4, ("+ YCbCr", 0): 9, ("+ XYB, custom opsin", 0): 5,
            ("+ EPF + XYB, custom opsin", 0): 4}
FILLED = (("+ XYB", 8), ("+ XYB", 16), ("+ XYB", 128), ("+ XYB", 256), ("IDCT + EPF", 32), ("IDCT (+ EPF) + XYB", 32),
          ("+ upsample (+ XYB)", 0), ("+ noise + XYB", 0), ("+ YCbCr", 0), ("+ XYB, custom opsin", 0), ("+ EPF + XYB, custom opsin", 0))
K_UPSAMPLE = 25  # an extra channel upsampled on its own: K["upsample"] of test_pixel_ref64_cpu.py


def measured_row(src, stage):
    """the measured row of the table that holds `stage` of this frame, or None where the row is derived"""
    gab, epf, n = src.get("gab", True), src.get("epf_iters", 0) > 0, C.size_class(src)
    if stage == TAIL:
        if src.get("noise") is not None:
            return ("+ noise + XYB", 0)
        if src.get("upsampling", 1) > 1:
            return ("+ upsample (+ XYB)", 0)
        if src.get("do_ycbcr", False):
            return ("+ YCbCr", 0)
        return ("+ EPF + XYB, custom opsin" if epf else "+ XYB, custom opsin", 0)
    if stage == XYB:
        return ("+ XYB" if gab else "IDCT (+ EPF) + XYB", n)
    if stage == EPF and epf:
        return ("+ EPF" if gab else "IDCT + EPF", n)
    return None


def bound(name, stage):
    return bound_of_source(C.source(name), stage)


def bound_of_source(src, stage):
    """the table's K of `stage` for a frame's SOURCE, whichever stream holds the frame"""
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
    x, a = model if model is not None else C.expected_image(name) if stage == TAIL else C.expected(name, stage)
    got = np.asarray(got)
    h, w = got.shape[1:]
    return M.error_ratio(got, x[:, :h, :w], a[:, :h, :w])


def final_stage(name):
    """the stage set whose planes the trace cut after the colour transforms holds: TAIL for a frame whose tail does more than the
    inverse XYB with the default matrix on planes of the frame's own size"""
    src = C.source(name)
    if src.get("do_ycbcr", False) or src.get("upsampling", 1) > 1 or src.get("noise") is not None or src.get("opsin") is not None:
        return TAIL
    return XYB if src.get("xyb", True) else EPF


# ---- packed samples of the alpha cases: PNGWriter and toTensor ------------------------------------------------------------------
def srgb_from_linear(x):
    """TransferFunction.TF_SRGB.fromLinear (color/TransferFunction.java:31-36) in float64"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x < 0.00313066844250063, x * 12.92, 1.055 * np.power(np.maximum(x, 0.0), 0.4166666666666667) - 0.055)


def sample_bounds(name, transfer):
    """(lo, hi), [H][W][4] integers: the 8-bit samples R, G, B, A that numpy packing makes of the case's expected planes -- a float
    sample v is (int)(v * 255 + 0.5) clamped to 0 .. 255 (ImageBuffer.castToInt0, ImageBuffer.java:129-145) -- taken at both ends
    of what the planes' bound lets v be: a colour is within K u (A + |model|) of its model (K: the bound of the cut after the colour
    transforms), which the sRGB curve stretches by no more than 12.92, and its float32 evaluation (fromLinearF, whose pow the JVM
    leaves 1 ulp open) adds 16 u (1 + |v|); an alpha sample that was not upsampled is exact. transfer: "srgb" (PNGWriter of an XYB
    image, whose planes are linear sRGB) or "linear" (toTensor(target="as-is")). lo == hi nearly everywhere."""
    src = C.source(name)
    ih, iw = V.image_size(src)
    x, a = C.expected_image(name)
    x, a = x[:, :ih, :iw], a[:, :ih, :iw]
    slack = bound(name, final_stage(name)) * M.U * (a + np.abs(x))
    if transfer == "srgb":
        v, slack = srgb_from_linear(x), 12.92 * slack
    else:
        v = x
    slack = slack + 16 * M.U * (1.0 + np.abs(v))
    planes = [(v[c], slack[c]) for c in range(3)]
    ex, ea = C.expected_extras(name)[0]
    planes.append((np.asarray(ex, np.float64), 0.0 if ea is None else K_UPSAMPLE * M.U * (ea + np.abs(ex)) + 16 * M.U))

    def pack(f):
        return np.clip(np.trunc(f * 255.0 + 0.5), 0, 255).astype(np.int64)
    return np.stack([pack(v - d) for v, d in planes], -1), np.stack([pack(v + d) for v, d in planes], -1)
