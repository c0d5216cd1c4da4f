"""Seeded Modular frames that are NOT lossless integer RGB -- frames of an XYB-encoded image, frames with Gaborish, the edge-preserving
filter under the header's epf_sigma_for_modular, do_ycbcr frames -- for tests/jxl_writer.py, and what a decoder must make of them,
computed from the SOURCE arrays alone: a fifth witness, shared by test_jxl_writer_lossy_cpu.py (oracle backend),
test_jxl_writer_lossy_gpu.py (device backend) and test_modular_restore_ref64_gpu.py (the stage entry points). Nothing here reads a
bitstream, and no expectation passes through jxlatte_amd's front-end, decoder or kernels.

The expectation is a composition of the float64 models the project already has, each carrying its magnitude companion A:
pixel_ref64.modular_to_float (Frame.java:430-455: the stream's channels are Y, X, B - Y; channel c lands in buffer cMap[c] scaled
by lf_dequant[cMap[c]]; B is scale * (channel 0 + channel 2) with Java's wrapping int sum) or the cast of integer colours by
float32(1) / float32(maxValue) (Frame.java:519, :579), vardct_ref64.gab, vardct_ref64.epf with the SCALAR float32(1) / float32(sigma)
(:573-575) on planes of the frame's own size (getPaddedFrameSize pads a VarDCT frame only, :924-941), vardct_ref64.xyb or .ycbcr.
A one-colour frame is the three-plane model on three copies of the plane with channel 0's Gaborish weights and the three channel
scales (:641-642, :660-661), plane 0 taken. A grey image with an XYB frame takes plane 1 of the inverse XYB
(JXLCodestreamDecoder.java:420). An integer alpha channel beside float colours is what tests/blend_ref.py makes of it on a float
canvas. `mut=` selects expectations that are WRONG on purpose (MUTATIONS: the CPU test shows that the bound tells each from a decode).

Bounds: |float32 - model| <= K u (A + |model|), u = 2^-24. The derived rows follow DESIGN section 3 (K_TO_FLOAT 2, K_GAB + 12).
K_MEASURED rows are K = ceil(2 x the largest oracle-vs-model ratio) over the cases of the row, measured on the CPU against the oracle
(test_jxl_writer_lossy_cpu.test_measured_rows_are_twice_the_largest_ratio holds the table to that), never against the device.

Sizes: 1x1, 2x9, 5x3, 7x8 (below 8 mirrorCoordinate reflects more than once), 13x21, 37x70 and 70x37 (70 crosses the 64-sample
column and the 4-row row of the restoration kernels' workgroups). Planes are a smooth field plus small noise, so that EPF weights
are neither all 0 nor all 1 (test_the_cases_themselves: a "filter" case changes at least 20 % of its samples, a "copy" case none)."""
import math

import numpy as np

import blend_ref as R
import jxl_writer as W
import jxl_writer_cases as WC
import pixel_ref64 as P
import vardct_ref64 as M

F, D = np.float32, np.float64
U = 2.0 ** -24
SIZES = ((1, 1), (2, 9), (5, 3), (7, 8), (13, 21), (37, 70), (70, 37))  # (height, width)
DEFAULT_OPSIN = (11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                 -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863)  # OpsinInverseMatrix.java:11-15
OPSIN_BIAS = -0.0037930732552754493  # :17-21
C_MAP = (1, 0, 2)  # Frame.java:42
MUTATIONS = ("c_map_identity", "b_without_y", "lf_dequant_c_in", "sigma_not_inverted", "padded_to_8", "one_colour_distance_once",
             "cast_by_power_of_two", "grey_plane_0", "cb_cr_exchanged")


def _h(v):
    return float(np.float16(v))


# ---- source planes ---------------------------------------------------------------------------------------------------------------
def _field(rng, h, w, mean, swing, noise):
    """a smooth field plus small noise, as integers"""
    y, x = np.mgrid[0:h, 0:w]
    px, py, ph = rng.uniform(4.0, 7.0), rng.uniform(3.0, 6.0), rng.uniform(0.0, 6.0)
    return np.rint(mean + swing * np.sin(x / px + ph) * np.cos(y / py) + rng.integers(-noise, noise + 1, (h, w))).astype(np.int64)


def xyb_planes(rng, h, w, x=(40, 6), b=(0, 8)):
    """Y, X, B - Y in stream order: about 0.4, 0.01 and +-0.03 after the default lf_dequant (1 / 512, 1 / 4096, 1 / 256). No plane of the
    frame crosses zero: a filter's rounding error is relative to the neighbourhood's magnitude, which the bound takes from the
    companion, and a plane whose samples cancel has none to speak of. x, b: (mean, swing) of the X and B - Y channels"""
    return [_field(rng, h, w, 200, 15, 2), _field(rng, h, w, x[0], x[1], 1), _field(rng, h, w, b[0], b[1], 1)]


def int_planes(rng, h, w, bits, n, centred=()):
    """a gentle field around half of the depth's range: neighbours differ by about 1 / 255 of it, where the EPF's weights lie between
    0 and 1. centred: the planes that hold a chroma channel, moved towards 0"""
    mx = (1 << bits) - 1
    out = []
    for c in range(n):
        y, x = np.mgrid[0:h, 0:w]
        f = 0.5 + 0.02 * np.sin(x / rng.uniform(4.0, 7.0) + rng.uniform(0.0, 6.0)) * np.cos(y / rng.uniform(3.0, 6.0)) + rng.uniform(-0.002, 0.002, (h, w))
        p = np.rint(f * mx).astype(np.int64)
        out.append(p - mx // 4 if c in centred else p)  # (about a quarter: no plane crosses zero, see xyb_planes)
    return out


def _rf(gab=False, epf=0, sigma=1.0, **kw):
    rf = dict(gab=gab, epf_iters=epf, **kw)
    if epf:
        rf["sigma_for_modular"] = sigma
    return rf


def _im(planes, rf, bits=8, xyb=False, grey=False, extra=(), **frame):
    h, w = planes[0].shape
    return dict(width=w, height=h, bits=bits, xyb=xyb, grey=grey, extra=list(extra), frames=[dict(planes=planes, restoration=rf, **frame)])


def _cases():
    """name -> (image, kind): "plain" (no filter), "filter" (a filter that runs), "copy" (an EPF whose inverse sigma is over the copy
    threshold 1 / 0.3, Frame.java:608, or a 1 x 1 frame, where every tap of either filter is the sample itself), "exact" (integer
    planes come back as they are)"""
    rng = np.random.default_rng(7500)
    out = {}
    for h, w in SIZES:
        combos = [(False, 0), (True, 0), (False, 1), (False, 2), (False, 3), (True, 2)] + ([(True, 3)] if (h, w) in ((13, 21), (70, 37)) else [])
        for k, (gab, it) in enumerate(combos):
            sigma = (1.0, 1.5, 2.0)[(k + h) % 3]  # all exact halves, none near the threshold: 1 / sigma <= 1 < 1 / 0.3
            out["xyb_%dx%d_gab%d_epf%d" % (h, w, gab, it)] = (_im(xyb_planes(rng, h, w), _rf(gab, it, sigma), xyb=True),
                                                                "plain" if not (gab or it) else "copy" if (h, w) == (1, 1) else "filter")
    for h, w, it in ((13, 21, 2), (5, 3, 3), (70, 37, 1)):  # sigma 0.25: inverse sigma 4 > 1 / 0.3, every pixel is copied
        out["xyb_%dx%d_epf%d_copied" % (h, w, it)] = (_im(xyb_planes(rng, h, w), _rf(False, it, 0.25), xyb=True), "copy")
    # custom restoration fields, every one an exact half and different per channel
    gw = [(_h(0.115), _h(0.061)), (_h(0.2), _h(0.01)), (_h(0.05), _h(0.1))]
    out["xyb_custom_gab_weights"] = (_im(xyb_planes(rng, 13, 21), _rf(True, 0, gab_weights=gw), xyb=True), "filter")
    out["xyb_custom_channel_scale"] = (_im(xyb_planes(rng, 13, 21), _rf(False, 2, 1.0, epf_channel_scale=[30.0, 7.0, 2.5]), xyb=True), "filter")
    out["xyb_custom_sigma_block"] = (_im(xyb_planes(rng, 13, 21), _rf(True, 3, 1.5, pass0=0.75, pass2=5.0, border_sad_mul=0.5), xyb=True), "filter")
    out["xyb_custom_everything"] = (_im(xyb_planes(rng, 37, 70), _rf(True, 3, 2.0, gab_weights=gw, epf_channel_scale=[30.0, 7.0, 2.5], pass0=0.75,
                                                                     pass2=5.0, border_sad_mul=0.5), xyb=True, lf_dequant=[0.0625, 0.125, 0.75]), "filter")
    # lf_dequant per channel: X 1 / 2048, Y 1 / 1024, B 3 / 512 -- none the default's, all three differ: lf_dequant[cOut] is not [cIn]
    out["xyb_custom_lf_dequant"] = (_im(xyb_planes(rng, 16, 16), _rf(True, 2, 1.0), xyb=True, lf_dequant=[0.0625, 0.125, 0.75]), "filter")
    out["xyb_custom_lf_dequant_plain"] = (_im(xyb_planes(rng, 5, 3), _rf(), xyb=True, lf_dequant=[0.0625, 0.125, 1.0]), "plain")
    # the wrapping sum: channel 0 + channel 2 leaves int32 on a third of the samples, in both directions (Frame.java:441)
    big = [rng.integers(-(1 << 31), 1 << 31, (9, 11)).astype(np.int64) for _ in range(3)]
    big[0].reshape(-1)[:4] = ((1 << 31) - 1, (1 << 31) - 1, -(1 << 31), -(1 << 31))
    big[2].reshape(-1)[:4] = (1, (1 << 31) - 1, -1, -(1 << 31))
    out["xyb_wrapping_sum"] = (_im(big, _rf(), xyb=True, predictor=0), "plain")
    # integer frames of an image that is not XYB: the result is float planes
    for name, bits, grey, h, w, gab, it in (("rgb8", 8, False, 9, 11, True, 2), ("rgb8", 8, False, 5, 3, False, 3), ("rgb16", 16, False, 9, 11, True, 0),
                                            ("rgb16", 16, False, 5, 3, True, 1), ("grey8", 8, True, 9, 11, True, 3), ("grey8", 8, True, 9, 11, False, 2),
                                            ("grey8", 8, True, 5, 3, True, 2), ("grey8", 8, True, 5, 3, True, 0)):
        out["%s_%dx%d_gab%d_epf%d" % (name, h, w, gab, it)] = (_im(int_planes(rng, h, w, bits, 1 if grey else 3), _rf(gab, it, 1.0), bits=bits, grey=grey),
                                                                 "filter")
    out["grey8_9x11_custom_channel_scale"] = (_im(int_planes(rng, 9, 11, 8, 1), _rf(True, 3, 1.0, epf_channel_scale=[30.0, 7.0, 2.5]), grey=True), "filter")
    out["rgb8_9x11_unfiltered"] = (_im(int_planes(rng, 9, 11, 8, 3), _rf()), "exact")
    out["grey8_5x3_unfiltered"] = (_im(int_planes(rng, 5, 3, 8, 1), _rf(), grey=True), "exact")
    # YCbCr: Cb, Y, Cr in stream order, the chroma planes centred on 0
    out["ycbcr_13x21"] = (_im(int_planes(rng, 13, 21, 8, 3, centred=(0, 2)), _rf(), ycbcr=True), "plain")
    out["ycbcr_13x21_gab1_epf2"] = (_im(int_planes(rng, 13, 21, 8, 3, centred=(0, 2)), _rf(True, 2, 1.0), ycbcr=True), "filter")
    out["grey_tagged_xyb_9x11_gab1_epf2"] = (_im(xyb_planes(rng, 9, 11), _rf(True, 2, 1.0), xyb=True, grey=True), "filter")
    alpha = WC._alpha_plane(rng, 13, 21).astype(np.int64)
    # (near grey, inside the sRGB gamut: its packed 8-bit samples are not the clamp's)
    out["xyb_alpha_13x21_gab1_epf2"] = (_im(xyb_planes(rng, 13, 21, x=(5, 2), b=(-40, 8)) + [alpha], _rf(True, 2, 1.0), xyb=True, extra=[dict(type="alpha", bits=8)]), "filter")
    return out


CASES = _cases()
NAMES = list(CASES)
_bytes = {}


def image(name):
    return CASES[name][0]


def kind(name):
    return CASES[name][1]


def encoded(name, variant=None):
    if (name, variant) not in _bytes:
        _bytes[name, variant] = W.encode(image(name), variant)
    return _bytes[name, variant]


# ---- what the headers say ---------------------------------------------------------------------------------------------------------
def header_fields(im):
    """the fields of the front-end's FrameInfo that these frames exercise, as the reference derives them from what the writer was given
    (RestorationFilter.java:14-25 for the defaults, which hold where the field is not in the stream; LFGlobal.java:22, :64)"""
    fr = im["frames"][0]
    rf = fr.get("restoration", {})
    it = rf.get("epf_iters", 0)
    gw = rf.get("gab_weights") if rf.get("gab", False) else None
    gw = gw or [(F(0.115169525), F(0.061248592))] * 3
    lfd = [F(1.0 / 4096.0), F(1.0 / 512.0), F(1.0 / 256.0)]
    if fr.get("lf_dequant") is not None:
        lfd = [F(F(v) * F(1.0 / 128.0)) for v in fr["lf_dequant"]]

    def epf(key, default):
        return F(rf[key]) if it and key in rf else F(default)
    return dict(xyb_encoded=int(bool(im.get("xyb", False))), do_ycbcr=int(bool(fr.get("ycbcr", False))), gab=int(bool(rf.get("gab", False))),
                gab1=[F(p[0]) for p in gw], gab2=[F(p[1]) for p in gw], epf_iters=it,
                epf_channel_scale=[F(v) for v in (it and rf.get("epf_channel_scale") or (40.0, 5.0, 3.5))],
                epf_pass0_sigma=epf("pass0", 0.9), epf_pass2_sigma=epf("pass2", 6.5), epf_border_sad_mul=epf("border_sad_mul", F(2) / F(3)),
                epf_sigma_modular=epf("sigma_for_modular", 1.0), lf_dequant=lfd)


# ---- the expectation ----------------------------------------------------------------------------------------------------------------
def _pad8(x, a):
    _, h, w = x.shape
    ph, pw = -(-h // 8) * 8, -(-w // 8) * 8
    return np.pad(x, ((0, 0), (0, ph - h), (0, pw - w))), np.pad(a, ((0, 0), (0, ph - h), (0, pw - w)))


def model(name_or_im, mut=None):
    """-> dict: mod (the stream's channels, integers), gab / epf / xyb: (planes [colours][H][W], companion) as the decoder's trace
    cuts hold the colour planes after Gaborish, after the EPF and after the colour transforms -- or (integer planes, None) where
    nothing has made them float -- and image: [(plane, companion | None)] per plane of the decoded image"""
    assert mut is None or mut in MUTATIONS
    im = image(name_or_im) if isinstance(name_or_im, str) else name_or_im
    fr = im["frames"][0]
    hf = header_fields(im)
    n_col = W.colour_planes(im, fr)
    src = [np.asarray(p, np.int64) for p in fr["planes"]]
    h, w = src[0].shape
    out = dict(mod=[p.copy() for p in src])
    filt = hf["gab"] or hf["epf_iters"] > 0
    xyb, ycbcr = bool(hf["xyb_encoded"]), bool(hf["do_ycbcr"])

    def cast():
        maxv = F(1 << im["bits"]) if mut == "cast_by_power_of_two" else F((1 << im["bits"]) - 1)
        pairs = [P.modular_to_float(src[c], None, F(1) / maxv) for c in range(n_col)]
        return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    if xyb:
        pairs = [None] * 3
        for c in range(3):
            c_out = c if mut == "c_map_identity" else C_MAP[c]
            scale = hf["lf_dequant"][c if mut == "lf_dequant_c_in" else c_out]
            second = src[2] if c == 2 and mut != "b_without_y" else None
            pairs[c_out] = P.modular_to_float(src[0] if second is not None else src[c], second, scale)
        x, a = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    elif hf["gab"]:
        x, a = cast()
    else:
        x = a = None  # integers so far: each filter casts where it starts (Frame.java:519, :579)
    one = n_col == 1

    def three(v):
        return np.repeat(v, 3, 0) if one else v
    if hf["gab"]:
        w1, w2 = [float(v) for v in hf["gab1"]], [float(v) for v in hf["gab2"]]
        if one:
            w1, w2 = [w1[0]] * 3, [w2[0]] * 3
        gx, ga = three(x), three(a)
        if mut == "padded_to_8":
            gx, ga = _pad8(gx, ga)
        gx, ga = M.gab(gx, ga, w1, w2)
        x, a = gx[:n_col, :h, :w], ga[:n_col, :h, :w]
    out["gab"] = (np.stack(src[:n_col]), None) if x is None else (x, a)
    if hf["epf_iters"] > 0:
        if x is None:
            x, a = cast()
        sigma =F(hf["epf_sigma_modular"]) if mut == "sigma_not_inverted" else F(F(1) / F(hf["epf_sigma_modular"]))  # Frame.java:573-575
        cs = [float(v) for v in hf["epf_channel_scale"]]
        if one and mut == "one_colour_distance_once":
            cs = [cs[0], 0.0, 0.0]
        ex, ea = three(x), three(a)
        if mut == "padded_to_8":
            ex, ea = _pad8(ex, ea)
        ex, ea = M.epf(ex, ea, hf["epf_iters"], float(sigma), cs, float(hf["epf_pass0_sigma"]), float(hf["epf_pass2_sigma"]),
                       float(hf["epf_border_sad_mul"]))
        x, a = ex[:n_col, :h, :w], ea[:n_col, :h, :w]
    out["epf"] = (np.stack(src[:n_col]), None) if x is None else (x, a)
    if xyb:
        bias = [F(OPSIN_BIAS)] * 3
        x, a = M.xyb(x, a, [F(v) for v in DEFAULT_OPSIN], bias, [F(np.cbrt(D(b))) for b in bias], 255.0)
    elif ycbcr:
        if x is None:
            x, a = cast()
        if mut == "cb_cr_exchanged":
            x, a = x[::-1], a[::-1]
        x, a = M.ycbcr(x, a)
    out["xyb"] = (np.stack(src[:n_col]), None) if x is None else (x, a)
    if x is None:
        planes = [(p.astype(np.int32), None) for p in src[:n_col]]
    elif xyb and im.get("grey", False):
        k = 0 if mut == "grey_plane_0" else 1
        planes = [(x[k], a[k])]
    else:
        planes = [(x[c], a[c]) for c in range(n_col)]
    for k, e in enumerate(im.get("extra", [])):
        p = np.asarray(src[n_col + k], np.int32)
        if x is None:
            planes.append((p, None))
            continue
        # the canvas is made in the colours' type (JXLCodestreamDecoder.java:640-643): the blend casts the integer plane
        n_img = len(planes)
        info, hdr = WC.header_objects(dict(width=w, height=h, bits=im["bits"], extra=[e]), dict(planes=[np.zeros((h, w), F)]))
        canvas = [R.Buf(np.zeros((h, w), F)) for _ in range(4)]
        R.blend_frame(info, hdr, canvas, [R.Buf(np.zeros((h, w), F)) for _ in range(3)] + [R.Buf(p)], [None] * 4)
        assert n_img in (1, 3)
        planes.append((canvas[3].a, None))
    out["image"] = planes
    return out


def changed_share(name):
    """the share of colour samples that the filters of the model change"""
    m = model(name)
    im = image(name)
    plain = dict(im, frames=[dict(im["frames"][0], restoration={})])
    before = model(plain)["epf"][0].astype(D)
    if model(plain)["epf"][1] is None:  # integer planes: the cast alone
        before = before * float(F(1) / F((1 << im["bits"]) - 1))
    after = m["epf"][0].astype(D)
    return float((np.abs(after - before) > 1e-9 * np.abs(before)).mean())  # (the model's own rounding is no change)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
K_TO_FLOAT, K_GAB = 2, 12  # modularToFloat; + Gaborish
# measured rows: ceil(2 x the largest oracle-vs-model ratio) over the row's cases (the second figure: that ratio)
K_MEASURED = {
    "+ EPF, three colours": (13, 6.273),
    "+ EPF, one colour": (6, 2.825),
    "+ XYB": (6, 2.965),
    "+ EPF + XYB": (13, 6.458),
    "+ YCbCr": (2, 0.956),
    "+ EPF + YCbCr": (4, 1.797),
}


def row(name, cut):
    """the row of the table that bounds `cut` ("gab", "epf", "xyb"; the image is "xyb") of the case: a number where it is derived, the
    name of a measured row else, None where the planes are integers (bit for bit)"""
    im = image(name)
    hf = header_fields(im)
    n_col = W.colour_planes(im, im["frames"][0])
    filt = hf["gab"] or hf["epf_iters"] > 0
    if not (hf["xyb_encoded"] or filt or (cut == "xyb" and hf["do_ycbcr"])):
        return None
    if cut == "gab" and not hf["xyb_encoded"] and not hf["gab"]:
        return None  # the EPF casts, not yet the cut before it
    if cut == "gab" or(cut == "epf" and not hf["epf_iters"]) or (cut == "xyb" and not hf["epf_iters"] and not hf["xyb_encoded"] and not hf["do_ycbcr"]):
        return K_TO_FLOAT + (K_GAB if hf["gab"] else 0)
    epf = "+ EPF" if hf["epf_iters"] else ""
    if cut == "epf" or not (hf["xyb_encoded"] or hf["do_ycbcr"]):
        return "+ EPF, one colour" if n_col == 1 else "+ EPF, three colours"
    return (epf + " " if epf else "") + ("+ XYB" if hf["xyb_encoded"] else "+ YCbCr")


def bound(name, cut):
    r = row(name, cut)
    return K_MEASURED[r][0] if isinstance(r, str) else r


def ratio(got, pair):
    """the K `got` needs against (model, companion); every sample counts"""
    x, a = pair
    got = np.asarray(got)
    assert got.shape == x.shape, (got.shape, x.shape)
    return M.error_ratio(got, x, a)


def packed_rgba(name):
    """(lo, hi), [H][W][4] of the 8-bit samples R, G, B, A that numpy packing makes of the XYB + alpha case's expected planes at both
    ends of the planes' bound, for toTensor(target="as-is") -- (int)(v * 255 + 0.5) clamped to 0 .. 255 (ImageBuffer.castToInt0) -- and,
    through the sRGB curve (whose slope is at most 12.92, its float32 evaluation adding 16 u (1 + |v|)), for PNGWriter"""
    def srgb_from_linear(x):  # TransferFunction.TF_SRGB.fromLinear (color/TransferFunction.java:31-36) in float64
        with np.errstate(invalid="ignore"):
            return np.where(x < 0.00313066844250063, x * 12.92, 1.055 * np.power(np.maximum(x, 0.0), 0.4166666666666667) - 0.055)
    planes = model(name)["image"]
    k = bound(name, "xyb")

    def ends(transfer):
        lo, hi = [], []
        for x, a in planes[:3]:
            slack = k * U * (a + np.abs(x))
            v = x
            if transfer == "srgb":
                v, slack = srgb_from_linear(x), 12.92 * slack
            slack = slack + 16 * U * (1.0 + np.abs(v))
            lo.append(v - slack), hi.append(v + slack)
        al = np.asarray(planes[3][0], D)
        pack = lambda f: np.clip(np.trunc(f * 255.0 + 0.5), 0, 255).astype(np.int64)  # noqa: E731
        return np.stack([pack(v) for v in lo + [al]], -1), np.stack([pack(v) for v in hi + [al]], -1)
    return ends


assert math.isclose(M.COPY_THRESHOLD, 1 / 0.3, rel_tol=1e-6)
