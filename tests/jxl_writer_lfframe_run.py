"""Running the cases of jxl_writer_lfframe_cases.py through a decoder backend and holding every frame to the model: shared by
test_jxl_writer_lfframe_cpu.py (oracle backend) and test_jxl_writer_lfframe_gpu.py (device backend). No oracle and no second decode
in any comparison.

Bounds, |float32 - model| <= K u (A + |model|), per frame and cut:

  * derived rows extend by their formula, as jxl_writer_vardct_run.bound does: IDCT is k_idct(n) + K_in, + Gaborish adds 12. K_in is
    the LF stage's K (5, or 34 with smoothing) for a frame with an LF stream of its own; for a frame that copies its LF out of an LF
    frame's planes it is the bound of that LF frame's LAST stage -- the stored planes are that stage's float32 results -- or 2 for
    integer planes, which are exact and cast on the way (modularToFloat's K). The consumer's companion is made of A_lf + |lf|
    (jxl_writer_lfframe_cases), so K_in u (A + |model|) holds what the copied error becomes;
  * a Modular XYB LF frame without an EPF is modularToFloat's 2, + 12 with Gaborish (jxl_writer_lossy_cases);
  * measured rows -- an EPF, and every cut after the colour transforms -- are K = ceil(2 x the largest oracle-vs-model ratio) over
    the cases of the row, measured on the CPU against the oracle backend (test_jxl_writer_lfframe_cpu.py holds MEASURED to that),
    never against the device. Every measured row of these cases is in MEASURED here, the "+ XYB" of the permuted frames too: a
    row of jxl_writer_vardct_run.MEASURED is twice the largest ratio of ITS cases, and a new draw of the class may pass it."""
import numpy as np

import jxl_writer_lfframe_cases as L
import jxl_writer_lossy_cases as LC
import jxl_writer_vardct_cases as VC
import jxl_writer_vardct_run as R
import vardct_ref64 as M
from jxlatte_amd.decoder import JXLDecoder

CUTS = R.CUTS
HEADER = ("type", "encoding", "flags", "lf_level", "width", "height", "padded_width", "padded_height", "upsampling", "is_last",
          "num_groups", "num_lf_groups", "has_noise", "do_ycbcr")
# (row, size class of the frame's largest transform | 0): ceil(2 x the second figure, the largest ratio the CPU run printed)
MEASURED = {
    ("+ XYB", 16): 6,  # 2.556
    ("+ XYB", 64): 17,  # 8.276
    ("LF frame + EPF", 8): 10,  # 4.621
    ("Modular LF frame + EPF", 0): 5,  # 2.268
    ("consumer + XYB", 16): 13,  # 6.388
    ("consumer + YCbCr", 0): 12,  # 5.513
    ("consumer + noise + XYB", 0): 1,  # 0.165
}


def decode(data, backend, cuts=True, trace=True, **switches):
    """-> dict: frames -- per frame of the stream a dict: header (HEADER as the front-end hands it out), and for a VarDCT frame
    "idct" / "gab" / "epf" (the stage-masked runs of its vardct call, padded planes; only with `cuts`), for a frame that reaches the
    colour transforms "xyb" (the trace cut after them; only with `trace`: a listener changes the route of device_frames) --,
    image, stats, lfBuffer, vardct_calls"""
    dec = JXLDecoder(data, backend=backend, **switches)
    out = dict(frames=[], vardct_calls=0)
    orig, real = backend.vardct, dec._next_frame

    def next_frame():
        fr = real()
        if fr is not None:
            out["frames"].append(dict(header={k: getattr(fr, k) for k in HEADER}))
        return fr

    def vardct(params, weights, woffs, lfgroups, groups, **kw):
        groups = list(groups)
        out["vardct_calls"] += 1
        if cuts:
            want, xyb = params.stages, params.xyb
            plain = {k: v for k, v in kw.items() if k != "keep"}
            for stage, _, mask in CUTS:
                params.stages, params.xyb = mask, 0
                out["frames"][-1][stage] = np.array(orig(params, weights, woffs, lfgroups, groups, **plain), copy=True)
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
    finally:
        del backend.vardct
        out["stats"], out["lfBuffer"] = dec.stats, dec.lfBuffer
    return out


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
def _lf_source(name, i):
    """the index of the frame whose stored planes frame i copies its LF from: the last LF frame of level lf_level + 1 before it"""
    frames = L.case(name)["frames"]
    want = frames[i].get("lf_level", 0) + 1
    return max(k for k in range(i) if frames[k].get("lf_level", 0) == want)


def row(name, i, cut):
    """the row of the table that bounds `cut` ("idct", "gab", "epf", "stored", "xyb") of frame i: a number where it is derived, the key
    of a measured row else, None where the planes are integers (bit for bit)"""
    fr = L.case(name)["frames"][i]
    if L.is_modular(fr):
        assert cut == "stored"
        rf = fr.get("restoration", {})
        if not L.case(name)["image"].get("xyb", False):
            return None
        if rf.get("epf_iters", 0):
            return ("Modular LF frame + EPF", 0)
        return LC.K_TO_FLOAT + (LC.K_GAB if rf.get("gab", False) else 0)
    n, epf, gab = VC.size_class(fr), fr.get("epf_iters", 0) > 0, fr.get("gab", True)
    lf_frame, consumer = fr.get("lf_level", 0) > 0, fr.get("use_lf_frame", False)
    if cut == "xyb":
        if not (lf_frame or consumer):
            return R.measured_row(fr, R.XYB if fr.get("xyb", True) else R.EPF)
        tail = "+ noise + XYB" if fr.get("noise") is not None else "+ YCbCr" if fr.get("do_ycbcr", False) else "+ XYB"
        return ("consumer " + tail, 0 if tail != "+ XYB" else n)
    if cut in ("epf", "stored") and epf:
        return ("consumer + EPF" if consumer else "LF frame + EPF" if lf_frame else "+ EPF", n)
    if consumer:
        k_in = bound(name, _lf_source(name, i), "stored") or LC.K_TO_FLOAT
    else:
        g = fr["lfgroups"][0]
        smoothed = not fr.get("skip_smoothing", False) and min(np.asarray(g["hf_mul"]).shape) >= 3  # LFCoefficients.java:121, :133
        k_in = R.K_LF[smoothed]
    return R.k_idct(n) + k_in + (12 if cut != "idct" and gab else 0)


def bound(name, i, cut):
    r = row(name, i, cut)
    return MEASURED[r] if isinstance(r, tuple) else r


def ratio(got, pair):
    """the K `got` needs against (model, companion) on the part of the padded planes `got` covers; integer planes: 0 or inf"""
    x, a = pair
    got = np.asarray(got)
    h, w = got.shape[1:]
    if a is None:
        return 0.0 if got.dtype == np.int32 and np.array_equal(got, np.asarray(x)[:, :h, :w]) else np.inf
    return M.error_ratio(got, x[:, :h, :w], a[:, :h, :w]) if got.dtype == np.float32 else np.inf


def frame_ratios(name, out, cuts=True, models=None):
    """[(frame, cut, ratio, K, row)] of one decode: every cut of every frame, what every LF frame left in lfBuffer, and the image"""
    c, rows = L.case(name), []
    models = models or L.models(name)
    assert len(out["frames"]) == len(c["frames"])
    for i, (fr, got, m) in enumerate(zip(c["frames"], out["frames"], models)):
        if cuts and not L.is_modular(fr):
            rows += [(i, cut, ratio(got[cut], m[cut]), bound(name, i, cut), row(name, i, cut)) for cut, _, _ in CUTS]
        if "xyb" in got and "final" in m:
            rows.append((i, "xyb", ratio(got["xyb"], m["final"]), bound(name, i, "xyb"), row(name, i, "xyb")))
    held = {}
    for i, (fr, m) in enumerate(zip(c["frames"], models)):  # the last LF frame of a level is what lfBuffer holds at the end
        if fr.get("lf_level", 0):
            held[fr["lf_level"] - 1] = (i, m)
    for slot, (i, m) in sorted(held.items()):
        planes = out["lfBuffer"][slot]
        assert planes is not None and len(planes) == 3, (name, slot)
        rows.append((i, "stored", ratio(np.stack([np.asarray(p) for p in planes]), m["stored"]), bound(name, i, "stored"), row(name, i, "stored")))
    last = len(c["frames"]) - 1
    if out.get("image") is not None:
        planes = out["image"].getBuffer()
        ih, iw = c["image"]["height"], c["image"]["width"]
        assert len(planes) == 3 and all(p.shape == (ih, iw) and p.dtype == np.float32 for p in planes), name
        rows.append((last, "image", ratio(np.stack(planes), models[last]["final"]), bound(name, last, "xyb"), row(name, last, "xyb")))
    return rows
