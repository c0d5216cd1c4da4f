"""Running the cases of jxl_writer_features_cases.py through a decoder backend and holding every frame to the model: shared by
test_jxl_writer_features_cpu.py (oracle backend) and test_jxl_writer_features_gpu.py (device backend). No oracle and no second decode
in any comparison.

Bounds, |float32 - model| <= K u (A + |model|), per frame and cut:

  * the "epf" cut of a VarDCT frame is held under the row jxl_writer_vardct_run gives the frame's class (derived, or its measured
    "+ EPF" rows, which are untouched); a reference slot filled before the colour transform holds that cut's planes, upsampled or not,
    under the same row -- or modularToFloat's 2 for a Modular XYB frame;
  * the cut after the colour transforms, the image, and a slot that is the canvas are held under the rows of MEASURED here, named
    after what runs between the EPF and that cut: K = ceil(2 x the largest oracle-vs-model ratio) over the row's cases, measured on
    the CPU against the oracle backend (test_measured_rows_are_twice_the_largest_ratio), never against the device. A spline row is
    large beside the others: an arc's position ends a float32 walk along the curve, and far from the arc a sample is the square of a
    difference of two erf values near 1, where spline_model64's companion -- the sum of |0.25 values sigma factor^2| -- does not grow
    with the cancellation."""
import numpy as np

import jxl_writer as W
import jxl_writer_features_cases as FC
import jxl_writer_lossy_cases as LC
import jxl_writer_vardct_run as R
import vardct_ref64 as M
from jxlatte_amd.decoder import JXLDecoder

HEADER = ("type", "encoding", "flags", "width", "height", "upsampling", "is_last", "num_patches", "has_splines", "has_noise",
          "save_as_reference", "save_before_ct")
# row: ceil(2 x the second figure, the largest ratio the CPU run printed)
MEASURED = {
    "+ EPF + splines + XYB": 53,  # 26.166
    "+ XYB": 7,  # 3.177
    "+ patches + XYB": 11,  # 5.318
    "+ patches + splines + XYB": 7,  # 3.124
    "+ patches + splines + noise + XYB": 3,  # 1.107
    "+ splines + XYB": 140,  # 69.539
    "+ splines + noise + XYB": 3,  # 1.293
    "+ upsample + patches + XYB": 3,  # 1.417
    "+ upsample + splines + XYB": 11,  # 5.121
    "Modular": 4,  # 1.954
    "Modular + splines": 7,  # 3.302
    "Modular + splines + noise": 2,  # 0.844
    "Modular + upsample + noise": 7,  # 3.098
}


def decode(data, backend, trace=True, **switches):
    """-> dict: frames -- per frame of the stream a dict: header (HEADER as the front-end hands it out), "epf" of a VarDCT frame (the
    stage-masked run of its vardct call without the inverse XYB, padded planes; only with `trace`), "xyb" (the trace cut after the
    colour transforms; only with `trace`) --, image, stats, reference (the four slots at the end of the decode)"""
    dec = JXLDecoder(data, backend=backend, **switches)
    out = dict(frames=[], vardct_calls=0)
    orig, real = backend.vardct, dec._next_frame
    mask = R.CUTS[2][2]

    def next_frame():
        fr = real()
        if fr is not None:
            out["frames"].append(dict(header={k: getattr(fr, k) for k in HEADER}))
        return fr

    def vardct(params, weights, woffs, lfgroups, groups, **kw):
        groups = list(groups)
        out["vardct_calls"] += 1
        if trace:
            want, xyb = params.stages, params.xyb
            params.stages, params.xyb = mask, 0
            out["frames"][-1]["epf"] = np.array(orig(params, weights, woffs, lfgroups, groups, **{k: v for k, v in kw.items() if k != "keep"}), copy=True)
            params.stages, params.xyb = want, xyb
        return orig(params, weights, woffs, lfgroups, groups, **kw)

    def listen(fi, stage, planes, fused):
        if stage == "xyb":
            out["frames"][fi]["xyb"] = np.stack([np.array(p, copy=True) for p in planes[:3]])
    backend.vardct, dec._next_frame = vardct, next_frame
    if trace:
        dec.trace = listen
    try:
        out["image"] = dec.decode()
        # the slots as host arrays: a slot of device_canvas is a plane set, released with the decoder
        out["reference"] = [None if r is None else [np.array(r.download(c) if dec._is_set(r) else r[c], copy=True) for c in range(3)]
                            for r in dec.reference]
    finally:
        del backend.vardct
        out["stats"] = dec.stats
    return out


K_SPLINE_STAGE = 392  # (195.978) measured as the rows above, on decoder.render_splines (test_the_spline_stage_alone_is_the_model)
STAGE_CASES = ("splines_40x40", "splines_up2_19x15_of_37x29", "patches_splines_noise_72x64")  # 40 x 40, 38 x 30 and 72 x 64
# 72 x 64, 40 x 40 from a VarDCT slot, 72 x 64 upsampled, and 72 x 64 with an alpha channel (BLEND and MULADD through their alpha)
PATCH_STAGE_CASES = ("patches_splines_noise_72x64", "patches_chain_40x40", "patches_up2", "patches_alpha_blend")


def spline_stage(name):
    """the spline stage of the case's last frame alone: (float32 planes in front of it -- the model's, rounded --, the splines as the
    front-end hands them out, base correlations, (model, companion) of the stage's result on those planes)"""
    fr, m = FC.case(name)["frames"][-1], FC.expected(name)["frames"][-1]
    corr = fr.get("corr") or {}
    bx, bb = np.float32(corr.get("base_x", 0.0)), np.float32(corr.get("base_b", 1.0))
    planes = np.ascontiguousarray(m["at"]["splines"][0], np.float32)
    sx, sa, und = FC.SM.render(fr["splines"], float(bx), float(bb), planes.shape[1], planes.shape[2])
    assert not und
    return planes, FC.frontend_splines(fr["splines"]), bx, bb, (planes.astype(np.float64) + sx, sa)


def patch_stage(name):
    """the patch stage of the case's last frame alone: (float32 planes in front of it -- three colours, and the alpha plane as the
    float plane blendBuffers' casts make of it --, the slots as lists of float32 planes, the positions and blend rows as
    decoder.patch_type_plan makes them, (model, companion), K).
    K is derived from the SOURCE: the largest number of applications that draw on one sample, times the roundings of one
    application -- one for a sum (blendAdd), twelve where the frame has an alpha channel: BLEND's ten (JXLCodestreamDecoder.java:374-375:
    five in the numerator, four in the denominator, the division) and two for the alpha it reads, which an earlier application
    has written with two roundings (:369-370)"""
    from jxlatte_amd import abi
    fr, m = FC.case(name)["frames"][-1], FC.expected(name)
    planes = np.ascontiguousarray(m["frames"][-1]["at"]["patches"][0], np.float32)
    n_chan = planes.shape[0]
    slots = [None if s is None else np.ascontiguousarray(s[0], np.float32) for s in m["slots"]]
    pos, rows = [], []
    drawn = np.zeros(planes.shape[1:], np.int64)
    for p in fr["patches"]:
        for (x, y), b in zip(p["positions"], p["blend"]):
            pos.append((y, x, p["height"], p["width"], p["ref"], p["y0"], p["x0"], len(rows)))
            row = [b[0]] * 3 + list(b[1:])
            assert len(row) == n_chan
            rows.append([[r["mode"], r.get("alpha", 0), int(r.get("clamp", False))] for r in row])
            if any(r["mode"] != 0 for r in row) and slots[p["ref"]] is not None:
                drawn[y:y + p["height"], x:x + p["width"]] += 1
    s64 = [None if s is None else (s.astype(np.float64), np.abs(s.astype(np.float64))) for s in slots]
    x, a, _ = FC.patch_stage(planes.astype(np.float64), np.abs(planes.astype(np.float64)), s64, fr["patches"])
    return planes, [None if s is None else [s[c].copy() for c in range(n_chan)] for s in slots], np.array(pos, abi.PATCH_POS_DTYPE), \
        np.array(rows, np.int32), (x, a - np.abs(x)), int(drawn.max()) * (12 if n_chan > 3 else 1)


def final_row(fr):
    """the measured row of the cut after the colour transforms of a frame"""
    parts = [k for k in ("patches", "splines") if fr.get(k)] + (["noise"] if fr.get("noise") is not None else [])
    if fr.get("upsampling", 1) > 1:
        parts.insert(0, "upsample")
    if FC.is_modular(fr):
        return "Modular" + "".join(" + " + k for k in parts)
    if fr.get("epf_iters", 0):
        parts.insert(0, "EPF")
    return "".join("+ " + k + " " for k in parts) + "+ XYB"


def epf_bound(fr):
    """jxl_writer_vardct_run.bound of the frame's class at the cut after the EPF"""
    return R.bound_of_source(fr, R.EPF)


def ratio(got, pair):
    x, a = pair
    got = np.asarray(got)
    h, w = got.shape[1:]
    if got.dtype != np.float32 or h > x.shape[1] or w > x.shape[2]:
        return np.inf
    return M.error_ratio(got, x[:got.shape[0], :h, :w], a[:got.shape[0], :h, :w])


def frame_ratios(name, out, models=None):
    """[(frame | slot, cut, ratio, K, row)] of one decode: the cuts of every frame that were listened to, the reference slots at the
    end, and the image"""
    c, rows = FC.case(name), []
    m = models or FC.expected(name)
    assert len(out["frames"]) == len(c["frames"])
    for i, (fr, got, fm) in enumerate(zip(c["frames"], out["frames"], m["frames"])):
        if "epf" in got:
            h, w = fm["epf"][0].shape[1:]
            rows.append((i, "epf", ratio(got["epf"][:, :h, :w], fm["epf"]), epf_bound(fr), "epf"))
        if "xyb" in got:
            r = final_row(fr)
            rows.append((i, "xyb", ratio(got["xyb"], fm["final"]), MEASURED.get(r), r))
    for s, slot in enumerate(m["slots"]):
        planes = out["reference"][s]
        assert (planes is None) == (slot is None), (name, s)
        if slot is None:
            continue
        src = [f for f in c["frames"] if f.get("save_as_reference", 0) == s and not f.get("is_last", f.get("type", 0) == W.REGULAR)][-1]
        if not src.get("save_before_ct", False):
            r = final_row(src)
            k = MEASURED.get(r)
        elif FC.is_modular(src):
            r, k = "modularToFloat", LC.K_TO_FLOAT
        else:
            r, k = "epf", epf_bound(src) if src.get("upsampling", 1) == 1 else None
        rows.append((s, "slot", ratio(np.stack([np.asarray(p) for p in planes[:3]]), slot), k, r))
    last = len(c["frames"]) - 1
    planes = out["image"].getBuffer()
    ih, iw = c["image"]["height"], c["image"]["width"]
    assert len(planes) == 3 + len(c["image"].get("extra", [])) and all(p.shape == (ih, iw) and p.dtype == np.float32 for p in planes), name
    r = final_row(c["frames"][last])
    rows.append((last, "image", ratio(np.stack(planes), m["image"]), MEASURED.get(r), r))
    return rows
