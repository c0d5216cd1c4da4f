"""Running the cases of jxl_writer_lossy_cases.py through a decoder backend and holding the result to the expectation: shared by
test_jxl_writer_lossy_cpu.py (oracle backend) and test_jxl_writer_lossy_gpu.py (device backend). No oracle in any comparison."""
import numpy as np

import jxl_writer as W
import jxl_writer_lossy_cases as C
from jxlatte_amd.decoder import JXLDecoder

CUTS = ("gab", "epf", "xyb")
FIELDS = ("do_ycbcr", "gab", "gab1", "gab2", "epf_iters", "epf_channel_scale", "epf_pass0_sigma", "epf_pass2_sigma", "epf_border_sad_mul",
          "epf_sigma_modular", "lf_dequant")


def decode(data, backend, trace=True, **switches):
    """-> dict: info (the image header), fields (FIELDS of the frame header as the front-end hands them out), mod / gab / epf / xyb (the
    planes at the decoder's trace cuts; only with `trace`: a listener changes the route of device_frames), image, stats"""
    dec = JXLDecoder(data, backend=backend, **switches)
    out = dict(info=dec.info)
    real = dec._next_frame

    def next_frame():
        fr = real()
        if fr is not None:
            out["fields"] = {k: (list(getattr(fr, k)) if hasattr(getattr(fr, k), "__len__") else getattr(fr, k)) for k in FIELDS}
        return fr
    dec._next_frame = next_frame
    if trace:
        def listen(fi, stage, planes, fused):
            if stage in CUTS + ("mod",):
                out[stage] = [np.array(p, copy=True) for p in planes]
        dec.trace = listen
    try:
        out["image"] = dec.decode()
        out["planes"] = out["image"].getBuffer()
    finally:
        out["stats"] = dec.stats
        out["close"] = dec.close
    return out


def fields_differ(name, out):
    """None, or the first header field that is not the SOURCE's"""
    want = C.header_fields(C.image(name))
    if int(out["info"].xyb_encoded) != want["xyb_encoded"]:
        return "xyb_encoded"
    for k in FIELDS:
        got, exp = out["fields"][k], want[k]
        same = [np.float32(a) == np.float32(b) for a, b in zip(got, exp)] if isinstance(exp, list) else [got == exp]
        if not all(same) or (isinstance(exp, list) and len(got) != len(exp)):
            return "%s: %r, not %r" % (k, got, exp)
    return None


def image_ratios(name, planes, m=None):
    """per plane of the decoded image: the K it needs against the expectation, 0.0 for an exact plane that is bit for bit the
    expected one and inf for one that is not (a wrong dtype or shape included)"""
    m = m or C.model(name)
    if len(planes) != len(m["image"]):
        return [np.inf]
    out = []
    for got, (x, a) in zip(planes, m["image"]):
        got = np.asarray(got)
        if got.shape != x.shape:
            out.append(np.inf)
        elif a is None:
            out.append(0.0 if got.dtype == x.dtype and np.array_equal(got, x) else np.inf)
        else:
            out.append(C.ratio(got, (x, a)) if got.dtype == np.float32 else np.inf)
    return out


def check(name, out, what, cuts=True):
    """every cut and the image within the case's bounds; returns {row: ratio} of the measured rows it met"""
    im = C.image(name)
    n_col = W.colour_planes(im, im["frames"][0])
    m = C.model(name)
    met = {}
    if cuts:
        assert len(out["mod"]) == len(m["mod"]), what
        for c, (got, exp) in enumerate(zip(out["mod"], m["mod"])):
            assert got.dtype == np.int32 and np.array_equal(got[:exp.shape[0], :exp.shape[1]], exp), "%s: channel %d of the stream" % (what, c)
        for cut in CUTS:
            x, a = m[cut]
            got = np.stack([np.asarray(p) for p in out[cut][:n_col]])
            if a is None:
                assert got.dtype == np.int32 and np.array_equal(got, x), "%s: integer planes at %s" % (what, cut)
                continue
            assert got.dtype == np.float32, (what, cut)
            r, k = C.ratio(got, (x, a)), C.bound(name, cut)
            print("%s %s: ratio %.3f of K = %d (%s)" % (what, cut, r, k, C.row(name, cut)))
            assert r <= k, "%s at %s: ratio %.3f > K = %d" % (what, cut, r, k)
            if isinstance(C.row(name, cut), str):
                met[C.row(name, cut)] = max(met.get(C.row(name, cut), 0.0), r)
    k = C.bound(name, "xyb")
    rs = image_ratios(name, out["planes"], m)
    print("%s image: ratios %s of K = %s" % (what, ["%.3f" % r for r in rs], k))
    assert len(out["planes"]) == len(m["image"]), what
    assert all(r <= (k or 0) for r in rs), "%s image: ratios %s > K = %s" % (what, rs, k)
    return met
