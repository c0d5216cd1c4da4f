"""Seeded VarDCT cases for tests/jxl_writer_vardct.py at the smallest sizes where the code can go wrong: each gives the SOURCE dict the
writer takes, and what a decoder must make of it, computed from the SOURCE alone -- never through jxlatte_amd:

  * the frame dict of vardct_ref64.frame_inputs is built from the SOURCE arrays (model_frame);
  * the parameters come from the header values the case chose, by the reference's own expressions (params_of, lines cited);
  * the LF planes are pixel_ref64.lf_stage on the source LF integers;
  * the weights are quant_weights_ref.tables on the source parameter sets.

Conditions, checked here when a case is built: no cell's inverse sigma is within 1e-5 of the EPF's copy threshold
(vardct_ref64.epf_undecided_cells is empty), and no entry of a case's quant tables is in the "either neighbour" set of
quant_weights_ref; a draw that violates one is made again with the next seed. The cases of the frame's tail (TAIL_CASES) have two
more, checked on the model alone (tail_model): of an upsampled frame's outputs some are clamped to their window and most are not
(between 0.5 % and 50 %), and the inputs of a noisy frame's noise strength, 3 (Y +- X), lie under 0, at or over 7 and between them in
at least five of the LUT's seven segments -- the two clamps a strength has: the LUT holds ten-bit values below 1, so clampAsc of the
interpolated strength itself (Frame.java:825-826) can never act. Observed: clamped outputs
up2_19x15_of_37x29 3.7 %, up4_ragged 1.2 %, up8_40x40 1.3 %, up2_custom_weights 3.1 %, noise_up2 8.6 %, noise_up2_of_271x39 3.9 %,
opsin_custom_up2 0.7 %, alpha_up2 1.6 %; noise inputs under 0 / at or over 7 of 2 x the samples: noise_40x40 1988 / 16 of 3200, noise_264x264 68470 / 3 of
139392, noise_up2 10876 / 1044 and noise_up2_of_271x39 9839 / 2 of 21760, noise_corr 2327 / 9 of 3200, all seven segments in each.

The reference has no group_size_shift for a VarDCT frame (FrameHeader.java:121): groups are 256 x 256 and LF groups 2048 x 2048, so the
multi-group case is 264 x 264 (2 x 2 groups) and the case of two LF groups 2056 x 16."""
import functools
import math
import types

import numpy as np

import jxl_writer as W
import jxl_writer_vardct as V
import pixel_ref64 as P
import quant_weights_ref as Q
import vardct_ref64 as M
from jxlatte_amd import upweights

F = np.float32
I64 = np.int64


def _f16(v):
    return float(np.float16(v))


# ---- the parameters a decoder derives from the headers ------------------------------------------------------------------------
DEFAULT_OPSIN = (11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                 -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863)  # OpsinInverseMatrix.java:11-15


def params_of(src):
    """jxl_vardct_params as the reference computes them from the fields the case wrote"""
    ph, pw = V.padded_size(src)
    xyb = src.get("xyb", True)
    gs = F(F(65536.0) / F(src["global_scale"]))  # HFCoefficients.java:270
    xqm, bqm = (src.get("xqm", 3), src.get("bqm", 2)) if xyb else (2, 2)  # FrameHeader.java:126-137
    scale_factor = [F(gs * F(math.pow(0.8, xqm - 2.0))), gs, F(gs * F(math.pow(0.8, bqm - 2.0)))]  # :271-275
    lfd = [F(1.0 / 4096.0), F(1.0 / 512.0), F(1.0 / 256.0)]  # LFGlobal.java:22
    if src.get("lf_dequant") is not None:
        lfd = [F(F(v) * F(1.0 / 128.0)) for v in src["lf_dequant"]]  # :64
    scaled_dequant = [F(F(F(1 << 16) * lfd[i]) / F(src["global_scale"] * src["quant_lf"])) for i in range(3)]  # :71
    c = src.get("corr") or dict(colour_factor=84, base_x=0.0, base_b=1.0, x_factor_lf=128, b_factor_lf=128)  # LFChannelCorrelation.java:23-29
    # RestorationFilter.java:14-25, :70-78; the EPF's fields are in the stream only where it has an iteration (:57, :63, :69)
    epf = src.get("epf_iters", 0) > 0
    gw = src.get("gab_weights") or ([F(0.115169525)] * 3, [F(0.061248592)] * 3)
    sg = epf and src.get("sigma") or (F(0.46), F(0.9), F(6.5), F(F(2) / F(3)))
    lut = epf and src.get("sharp_lut") or [F(F(i) / F(7)) for i in range(8)]
    lut = [F(F(v) * F(sg[0])) for v in lut]  # :77-78
    cs = epf and src.get("channel_scale") or [40.0, 5.0, 3.5]
    o = src.get("opsin") or {}  # OpsinInverseMatrix.java:54-75: the custom fields are halves, taken as they are
    bias = [F(v) for v in o.get("opsin_bias", [-0.0037930732552754493] * 3)]  # :17-21
    return types.SimpleNamespace(
        width=pw, height=ph, scale_factor=scale_factor,
        quant_bias=[F(v) for v in o.get("quant_bias", (0.945349926692846, 0.9299455010825141, 0.9500648966626564))],  # :23-25
        quant_bias_numerator=F(o.get("quant_bias_numerator", 0.145)), base_corr_x=F(c["base_x"]), base_corr_b=F(c["base_b"]), color_factor=c["colour_factor"],
        gab=int(src.get("gab", True)), gab_w1=[F(v) for v in gw[0]], gab_w2=[F(v) for v in gw[1]], epf_iters=src.get("epf_iters", 0),
        global_scale_f=gs, epf_sharp_lut=lut, epf_channel_scale=[F(v) for v in cs], epf_pass0_sigma_scale=F(sg[1]),
        epf_pass2_sigma_scale=F(sg[2]), epf_border_sad_mul=F(sg[3]), xyb=int(xyb),
        # :11-15; getMatrix (:94-100) multiplies by the identity for sRGB / D65 (ColorManagement.java:139-140)
        opsin_matrix=[F(v) for v in o.get("matrix", DEFAULT_OPSIN)],
        # bakeCbrtBias (:81-84): the float of the double cube root; ToneMapping.java:15, :28
        opsin_bias=bias, cbrt_opsin_bias=[F(np.cbrt(np.float64(b))) for b in bias], intensity_target=F(src.get("intensity_target", 255.0)),
        jpeg_upsampling_y=list(src.get("shift_y", [0] * 3)), jpeg_upsampling_x=list(src.get("shift_x", [0] * 3)),
        scaled_dequant=scaled_dequant, x_factor_lf=c["x_factor_lf"], b_factor_lf=c["b_factor_lf"])


def quant_params(src):
    q = src.get("quant")
    d = Q.default_params()
    return d if q is None else [d[i] if p["mode"] == 0 else p for i, p in enumerate(q)]  # HFGlobal.java:222-224


def lf_planes(src, g, p, extra_precision=None):
    """LFCoefficients.java:64-100 on the source integers"""
    ep = g.get("extra_precision", 0) if extra_precision is None else extra_precision
    q = [np.asarray(a, I64) for a in g["lf_quant"]]
    if any(p.jpeg_upsampling_y) or any(p.jpeg_upsampling_x):  # :78: no chroma from luma; :33-34: no smoothing
        return [q[i].astype(np.float64) * (float(p.scaled_dequant[i]) / (1 << ep)) for i in range(3)]  # :68-73
    x, _, gap = P.lf_stage(np.stack(q), p.scaled_dequant, ep, p.x_factor_lf, p.b_factor_lf, not src.get("skip_smoothing", False),
                           float(p.base_corr_x), float(p.base_corr_b), p.color_factor)
    g["_gap"] = gap
    return [x[0], x[1], x[2]]


def model_frame(src, weights=None, extra_precision=None, params=None):
    """the dict vardct_ref64.frame_inputs takes"""
    p = params or params_of(src)
    geo = V.geometry(src)
    groups = []
    for i, g in enumerate(src["lfgroups"]):
        blocks = sorted(g["blocks"])
        sel = np.zeros(np.asarray(g["hf_mul"]).shape, I64)
        for y, x, t in blocks:
            sel[y:y + V.cells(t)[0], x:x + V.cells(t)[1]] = t
        groups.append(dict(lfg_y=i // geo["lcols"], lfg_x=i % geo["lcols"], dct_select=sel, hf_mul=np.asarray(g["hf_mul"]),
                           sharpness=np.asarray(g["sharpness"]), x_from_y=np.asarray(g["x_from_y"]), b_from_y=np.asarray(g["b_from_y"]),
                           lf=lf_planes(src, g, p, extra_precision), block_yx=np.array([(y, x) for y, x, _ in blocks], I64)))
    shifts = list(src.get("pass_shifts", [])) + [0]
    coeff = [sum(np.asarray(src["coeff_passes"][k][c], I64) << shifts[k] for k in range(len(shifts))) for c in range(3)]
    if weights is None:
        t = Q.tables(quant_params(src))
        weights = (t.w, t.offs)
    return dict(params=p, lfgroups=groups, coeff=coeff, weights=weights[0], woffs=weights[1])


def size_class(src):
    return max(max(V.TYPES[t][3:5]) for g in src["lfgroups"] for _, _, t in g["blocks"])


# ---- drawing a SOURCE ----------------------------------------------------------------------------------------------------------
SMALL_TYPES = tuple(range(18))
MID_TYPES = tuple(range(21))


def tiling(rng, ch, cw, allowed, first=None):
    """a complete tiling of ch x cw cells: at each free cell in raster order, a random allowed type that fits there without crossing
    a 256-pixel group edge, DCT8 where nothing else does. first: types to place first, one after the other"""
    sel = -np.ones((ch, cw), I64)
    out, queue = [], list(first or [])
    for y in range(ch):
        for x in range(cw):
            if sel[y, x] >= 0:
                continue
            cand = [queue[0]] if queue else list(rng.permutation(allowed)[:4])
            t = 0
            for k in cand:
                bh, bw = V.cells(int(k))
                if y + bh <= ch and x + bw <= cw and (y % 32) + bh <= 32 and (x % 32) + bw <= 32 and (sel[y:y + bh, x:x + bw] < 0).all():
                    t = int(k)
                    if queue:
                        queue.pop(0)
                    break
            bh, bw = V.cells(t)
            sel[y:y + bh, x:x + bw] = t
            out.append((y, x, t))
    return out


def hf_clusters(rng, n, k=4):
    """every context's cluster by a seeded draw; the last k make sure every cluster exists"""
    m = rng.integers(0, k, n)
    m[-k:] = np.arange(k)
    cfg = [W.CONFIGS[i] for i in rng.permutation(len(W.CONFIGS))[:k]]
    return m.tolist(), cfg


def draw(seed, width, height, allowed=SMALL_TYPES, first=None, density=0.08, amp=6, mul_max=9, lf_amp=60, dense=False, split=None,
         **opt):
    """one SOURCE. density: share of the HF positions of a block that hold a coefficient; split(rng, coeff, shifts) -> per-pass arrays"""
    rng = np.random.default_rng(seed)
    src = dict(width=width, height=height, global_scale=int(rng.integers(1500, 6000)), quant_lf=int(rng.integers(8, 40)),
               epf_iters=0, gab=True)
    src.update(opt)
    geo = V.geometry(src)
    sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
    coeff = [np.zeros((geo["ph"] >> sy[c], geo["pw"] >> sx[c]), I64) for c in range(3)]
    groups = []
    for i in range(geo["num_lf_groups"]):
        y0, x0 = (i // geo["lcols"]) << 8, (i % geo["lcols"]) << 8
        ch, cw = min(256, (geo["ph"] >> 3) - y0), min(256, (geo["pw"] >> 3) - x0)
        blocks = tiling(rng, ch, cw, allowed, first)
        hf = np.zeros((ch, cw), I64)
        for y, x, t in blocks:
            bh, bw = V.cells(t)
            hf[y:y + bh, x:x + bw] = rng.integers(1, mul_max + 1)
            for c in range(3):
                if (y >> sy[c]) << sy[c] != y or (x >> sx[c]) << sx[c] != x:
                    continue
                ph, pw = V.TYPES[t][3], V.TYPES[t][4]
                n = ph * pw
                k = n - bh * bw if dense else max(1, int(rng.binomial(n, density)))
                blk = np.zeros(n, I64)
                where = rng.choice(n, size=min(k, n), replace=False)
                mag = np.where(rng.random(where.size) < 0.5, 1, rng.integers(1, amp + 1, where.size))
                blk[where] = mag * rng.choice([-1, 1], where.size)
                blk = blk.reshape(ph, pw)
                if dense:
                    blk[blk == 0] = 1
                blk[:bh, :bw] = 0  # the LLF corner is not coded (HFCoefficients.java:305-306)
                blk[(np.abs(blk) > 0).cumsum().reshape(ph, pw) > 63 * bh * bw] = 0  # :254: at most 63 non-zeros per 8 x 8
                cy, cx = ((y0 + y) >> sy[c]) << 3, ((x0 + x) >> sx[c]) << 3
                coeff[c][cy:cy + ph, cx:cx + pw] = blk
        th, tw = (ch + 7) // 8, (cw + 7) // 8
        groups.append(dict(extra_precision=int(opt.get("extra_precision", rng.integers(0, 4))),
                           lf_quant=[rng.integers(-lf_amp, lf_amp + 1, (ch >> sy[c], cw >> sx[c])) for c in range(3)], blocks=blocks,
                           hf_mul=hf, sharpness=rng.integers(0, 8, (ch, cw)), x_from_y=rng.integers(-40, 41, (th, tw)),
                           b_from_y=rng.integers(-40, 41, (th, tw))))
    src.pop("extra_precision", None)
    src["lfgroups"] = groups
    shifts = list(src.get("pass_shifts", [])) + [0]
    if len(shifts) == 1:
        src["coeff_passes"] = [coeff]
    else:  # coefficient = sum_p value_p << shift_p: the high bits to the first pass, the remainders after it
        passes, rest = [], coeff
        for s in shifts:
            passes.append([r >> s for r in rest])  # (an arithmetic shift: the remainder stays non-negative)
            rest = [r - ((r >> s) << s) for r in rest]
        assert all((r == 0).all() for r in rest)
        src["coeff_passes"] = passes
    presets = src.get("num_presets", 1)
    if presets > 1:
        src["presets"] = [[int(v) for v in rng.integers(0, presets, geo["num_groups"])] for _ in shifts]
        src["presets"][0][:presets] = list(range(presets))
    clusters = V.block_ctx_of(src)[1]
    src["hf_clusters"] = [hf_clusters(rng, 495 * presets * clusters, int(rng.integers(4, 9))) for _ in shifts]
    src["tree_clusters"] = ([0, 1], [W.CONFIGS[i] for i in rng.permutation(8)[:2]])
    src["tree"] = src.get("tree", dict(property=0, value=int(rng.integers(0, 3)), predictors=(int(rng.choice([1, 2, 4, 5])), int(rng.choice([3, 5, 13])))))
    return src


def conditions(src):
    """the two conditions of the module's docstring; returns the reason a draw is unfit, or None"""
    p = params_of(src)
    if p.epf_iters > 0:
        for g in src["lfgroups"]:
            sig = M.epf_sigma(g["hf_mul"], g["sharpness"], float(p.global_scale_f), [float(v) for v in p.epf_sharp_lut])
            if M.epf_undecided_cells(sig).any():
                return "an inverse sigma at the EPF's copy threshold"
    if src.get("quant") is not None and Q.tables(quant_params(src)).near.any():
        return "a quant weight whose distance sits on a band index"
    if src.get("upsampling", 1) > 1 or src.get("noise") is not None:
        t = tail_model(src)
        if src.get("upsampling", 1) > 1 and not 0.005 <= t["clamped"] <= 0.5:
            return "%.2f %% of the upsampled outputs clamped" % (100 * t["clamped"])
        if src.get("noise") is not None and not (t["below"] > 0 and t["above"] > 0 and len(t["segments"]) >= 5):
            return "the noise strength's inputs miss a clamp or reach %d LUT segments" % len(t["segments"])
    return None


# ---- the frame's tail: upsampling, noise, the colour transforms (JXLCodestreamDecoder.java:628-637) ---------------------------
EPF_STAGES = 7  # vardct_ref64.decode: the inverse transforms, Gaborish and the EPF
NOISE_SEED0 = 1 << 32  # (visibleFrames << 32) | invisibleFrames at the image's first, visible frame (:622-629)


def frame_bounds(src):
    """(height, width) of the frame's bounds: the coded size rounded up to the subsampling factors (FrameHeader.java:196-199)"""
    my, mx = max(src.get("shift_y", [0] * 3)), max(src.get("shift_x", [0] * 3))
    return -(-src["height"] // (1 << my)) << my, -(-src["width"] // (1 << mx)) << mx


def packed_up_weights(src, k, default=False):
    """the 15 / 55 / 210 coefficients of factor k: the case's own where it wrote some (ImageHeader.java:268-293), else the defaults"""
    up = src.get("up_weights") or {}
    return np.asarray(upweights.DEFAULT_UP[k] if default or k not in up else up[k], F)


def upsample_model(x, a, k, packed):
    """pixel_ref64.upsample per plane. The companion of the weighted sum is the same sum of the input's companion under the absolute
    weights; the clamp hands out one of the window's samples instead, so the window's largest companion is held too (the clamp is
    continuous, not linear: an output moves by no more than the sum or the window's extremes do)"""
    wt = P.up_weights(k, packed)
    outs, mags, clamped = [], [], []
    for c in range(len(x)):
        o, _, cl = P.upsample(x[c], k, wt)
        _, lin, _ = P.upsample(a[c], k, wt)
        top = P._windows(np.asarray(a[c], np.float64)).max(axis=(0, 1))
        outs.append(o)
        mags.append(np.maximum(lin, np.repeat(np.repeat(top, k, 0), k, 1)))
        clamped.append(cl)
    return np.stack(outs), np.stack(mags), np.stack(clamped)


def tail_model(src, seed0=NOISE_SEED0, noise_group_dim=V.GROUP_DIM, exchange_cb_cr=False, default_up_weights=False, params=None,
               model=None, upsample_padded=False):
    """what a decoder must make of the SOURCE after performColorTransforms, on the frame's upsampled bounds (the crop to the image
    is the blend's): the model after the EPF cropped to the frame's bounds, Frame.upsample, initializeNoise at the upsampled size
    with the frame counters' seed and synthesizeNoise, invertXYB, the YCbCr loop; the magnitude companion through every step. The
    keyword arguments make the WRONG expectations of test_jxl_writer_vardct_cpu.py. Returns a dict: x, a, and the figures the
    cases' conditions read (clamped: the share of clamped upsampled outputs; below / above: how many inputs of noise_strength lie
    under 0 / at or over 7 / 3; segments: the LUT segments the others reach)"""
    p = params or params_of(src)
    if model is None:
        model = M.decode(model_frame(src, params=p), EPF_STAGES)[:2]
    h, w = frame_bounds(src)
    x, a = model[0], model[1]
    if not upsample_padded:  # the window is mirrored at the frame's bounds: the padding of the last blocks is never read
        x, a = x[:, :h, :w], a[:, :h, :w]
    out = {}
    k = src.get("upsampling", 1)
    if k > 1:
        x, a, cl = upsample_model(x, a, k, packed_up_weights(src, k, default_up_weights))
        x, a, cl = x[:, :h * k, :w * k], a[:, :h * k, :w * k], cl[:, :h * k, :w * k]
        out["clamped"] = float(cl.mean())
    if src.get("noise") is not None:
        lut = np.asarray(src["noise"], np.float64) / 1024.0  # LFGlobal.java:58
        nz, na, _ = P.noise_init(x.shape[1], x.shape[2], seed0, noise_group_dim)
        y, _, raw = P.noise_add(x, nz, lut, p.base_corr_x, p.base_corr_b)
        _, mag, _ = P.noise_add(x, na, lut, p.base_corr_x, p.base_corr_b)  # (the high-pass's own companion for |noise|)
        v = 3.0 * np.stack([x[1] + x[0], x[1] - x[0]])  # Frame.java:801-804
        out.update(below=int((v < 0).sum()), above=int((v >= 7.0).sum()),
                   segments=sorted(set(np.floor(v[(v >= 0) & (v < 7.0)]).astype(int).tolist())))
        x, a = y, mag + a  # the strength is continuous in the planes, not linear: the input's companion is added, not dropped
    if p.xyb:
        x, a = M.xyb(x, a, p.opsin_matrix, p.opsin_bias, p.cbrt_opsin_bias, float(p.intensity_target))
    if src.get("do_ycbcr", False):
        if exchange_cb_cr:
            x, a = x[::-1], a[::-1]
        x, a = M.ycbcr(x, a)
    out.update(x=x, a=a)
    return out


def extra_model(src, e):
    """one extra channel of the frame as the blend puts it on the image's float canvas: castToFloat with the channel's depth
    (tests/blend_ref.py, the reference's ImageBuffer.castToFloat), upsampled first by the model where ec_upsampling > 1
    (Frame.java:226-228 casts there). Returns (plane of the image's size, companion | None where the plane is exact)"""
    import blend_ref as B
    import jxl_writer_cases as WC
    ih, iw = V.image_size(src)
    k, bits = e.get("upsampling", 1), e.get("bits", 8)
    buf = B.Buf(np.asarray(e["plane"], np.int32))
    mag = None
    if k > 1:
        buf.cast_to_float(bits)
        x, mag, _ = P.upsample(buf.a, k, P.up_weights(k, packed_up_weights(src, k)))
        buf, mag = B.Buf(x.astype(F)), mag[:ih, :iw]
        model = x[:ih, :iw]
    im = dict(width=iw, height=ih, bits=8, extra=[dict(type="alpha", bits=bits, alpha_associated=e.get("alpha_associated", False))])
    fh, fw = buf.a.shape
    info, hdr = WC.header_objects(im, dict(planes=[np.zeros((fh, fw), F)]))
    hdr.upsampling = 1  # (the planes are past Frame.upsample: the blend reads them at their own size)
    canvas = [B.Buf(np.zeros((ih, iw), F)) for _ in range(4)]
    B.blend_frame(info, hdr, canvas, [B.Buf(np.zeros((fh, fw), F)) for _ in range(3)] + [buf], [None] * 4)
    return (canvas[3].a, None) if k == 1 else (model, mag)


def fit(make, seed):
    for k in range(20):
        src = make(seed + 1000 * k)
        if conditions(src) is None:
            return src
    raise AssertionError("no fit draw")


# ---- quant parameter sets the stream can hold (F16 values) -------------------------------------------------------------------------
def quant_set(rng, mode_of, bands_of):
    def args(n):
        kind = rng.integers(0, 3, n)
        return [_f16(0.0 if k == 0 else rng.uniform(0.05, 2.0) if k == 1 else -rng.uniform(0.05, 3.0)) for k in kind]

    def dct(n):
        return [[64.0 * _f16(rng.uniform(2.0, 60.0))] + args(n - 1) for _ in range(3)]

    def big(k):
        return [[64.0 * _f16(rng.uniform(1.0, 50.0)) for _ in range(k)] for _ in range(3)]
    out = []
    for i in range(17):
        mode, n = mode_of(i), bands_of(i)
        assert mode == 0 or Q.legal(i, mode)
        q = dict(mode=mode, dct=None, par=None, p44=None, denominator=1.0)
        if mode == 1:
            q["par"] = big(3)
        elif mode == 2:
            q["par"] = big(6)
        elif mode == 3:
            q["par"], q["dct"] = big(2), dct(n)
        elif mode == 4:
            q["par"], q["dct"] = [[_f16(rng.uniform(0.5, 3.0))] for _ in range(3)], dct(n)
        elif mode == 5:
            q["par"] = [r + a for r, a in zip(big(6), [args(3) for _ in range(3)])]
            q["dct"], q["p44"] = dct(n), dct(1 + (n + 3) % 16)
        elif mode == 6:
            q["dct"] = dct(n)
        elif mode == 7:
            mh, mw = Q.MATRIX[i]
            q["denominator"] = _f16(rng.uniform(0.0005, 0.004))
            # (1 / weight: a RAW table is used as it stands, HFGlobal.java:408-416, so small numbers make usual weights)
            q["par"] = [rng.integers(1, 40, mh * mw).tolist() for _ in range(3)]
        out.append(q)
    return out


def quant_case(s):
    """set s of eight: together they put every mode on every index validateIndex allows, library defaults (mode 0) in between"""
    def make(seed):
        rng = np.random.default_rng(seed)
        def mode_of(i):
            if i in Q.SMALL:
                return (s + i) % 8
            return (0, 6, 7)[(s + i) % 3]
        quant = quant_set(rng, mode_of, lambda i: 1 + (5 * s + 3 * i) % 16)
        stream = 1 + 3 * 1 + 16  # a RAW table's stream index (HFGlobal.java:265) decides the tree's leaf
        raw = [i for i in range(17) if quant[i]["mode"] == 7]
        tree = dict(property=1, value=(3 + raw[len(raw) // 2] if raw else stream), predictors=(4, 5))
        return draw(seed, 72, 64, allowed=MID_TYPES if s % 2 else SMALL_TYPES, quant=quant, tree=tree, mul_max=4)
    return functools.partial(fit, make, 7000 + s)


def lf_rough(seed):
    """extra_precision 3 and an LF field whose smoothing gap lies in all three regimes (the construction of pixel_ref64_cases: the
    integers of +-2000 under the default dequantisers; the gap goes with (65536 / (global_scale quant_lf)) ** 2 >> extra_precision,
    and global_scale is searched around the value that construction's multipliers give)"""
    for gs in (221, 200, 250, 180, 280, 160, 320, 140, 360):
        src = draw(seed, 96, 88, lf_amp=2000, extra_precision=3, global_scale=gs, quant_lf=16)
        model_frame(src)
        shares = P.lf_regimes(src["lfgroups"][0]["_gap"])
        if min(shares) >= 0.10:
            src["_lf_regimes"] = shares
            return src
    raise AssertionError("no scale puts a tenth of the cells into each regime")


def block_ctx_case(seed):
    rng = np.random.default_rng(seed)
    b = dict(lf_thresholds=[[-10, 12], [0], [-20]], qf_thresholds=[3, 6])  # hf_mul is drawn from 1..9, the LF from +-60
    n = 39 * 3 * 3 * 2 * 2
    cm = rng.integers(0, 6, n)
    cm[:6] = np.arange(6)
    b["cluster_map"] = cm.tolist()
    return draw(seed, 48, 40, block_ctx=b)


def shared_order(seed):
    """an explicit order on order id 4, which DCT16_8 (vertical) and DCT8_16 share, and on id 0; a different permutation per channel"""
    rng = np.random.default_rng(seed)
    orders = {}
    for oid in (0, 4):
        n = len(V.natural_order(oid))
        perms = []
        for c in range(3):
            p = np.arange(n)
            k = n // 64
            p[k:k + 24] = k + rng.permutation(24)
            perms.append(p.tolist())
        orders[oid] = perms
    return draw(seed, 48, 48, allowed=(0, 6, 7), first=[6, 7, 0], orders=[orders],
                order_clusters=([0, 1, 2, 3, 0, 1, 2, 3], list(W.CONFIGS[2:6])), density=0.3)


# what lets the EPF filter instead of giving every neighbour the weight 0: few coefficients of magnitude 1 and an almost flat LF
# field (the weight is 1 - distance / sigma, and the distance counts five pixels of three channels)
SMOOTH = dict(lf_amp=2, amp=1, density=0.02)


def _restoration(iters):
    return dict(gab=False, epf_iters=iters, sharp_lut=[_f16(v) for v in (0.0, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0)],
                channel_scale=[_f16(30.0), _f16(6.0), _f16(3.0)], sigma=(_f16(0.75), _f16(0.8), _f16(6.0), _f16(0.7)), **SMOOTH)


def corr_case(seed):
    return draw(seed, 136, 136, allowed=MID_TYPES, corr=dict(colour_factor=100, base_x=_f16(0.05), base_b=_f16(0.9), x_factor_lf=140,
                                                              b_factor_lf=100))


def _sub(name):
    sy, sx = dict(s420=([1, 0, 1], [1, 0, 1]), s422=([0, 0, 0], [1, 0, 1]), s440=([1, 0, 1], [0, 0, 0]))[name]
    # (8 x 8 types only: a larger block of a subsampled channel would cover its aligned neighbours' samples)
    return dict(xyb=False, do_ycbcr=True, shift_y=sy, shift_x=sx, skip_smoothing=True, allowed=(0, 1, 2, 3, 12, 13, 14, 15, 16, 17))


def _case(fn, *a, **kw):
    return functools.partial(fit, lambda seed: fn(seed, *a, **kw))


# ---- the cases of the frame's tail -----------------------------------------------------------------------------------------------
RAGGED_TYPES = MID_TYPES[:18] + (4, 5, 6, 7, 8, 9, 10, 11)
# a noise LUT (ten-bit integers, LFGlobal.java:58) with rising and falling segments that touches both ends of its range
NOISE_LUT = (0, 300, 1023, 640, 900, 120, 0, 512)
# what puts the inputs of the noise strength, 3 (Y +- X), on both sides of [0, 7): LF integers of +-600 at a dequantiser of 1 / 187
NOISE_FIELD = dict(lf_amp=600, global_scale=1500, quant_lf=16, noise=list(NOISE_LUT))


def up_weights_case(seed):
    """fifteen coefficients that are not the default ones: each default moved by up to a fifth of itself, as an exact half"""
    rng = np.random.default_rng(seed)
    packed = [_f16(float(v) * (1.0 + rng.uniform(-0.2, 0.2))) for v in upweights.DEFAULT_UP[2]]
    return draw(seed, 40, 40, upsampling=2, up_weights={2: packed})


def _opsin(rng):
    """OpsinInverseMatrix.java:61-73: a matrix near the default one, biases and quantisation biases of their usual size, all halves"""
    return dict(matrix=[_f16(v * (1.0 + rng.uniform(-0.1, 0.1))) for v in DEFAULT_OPSIN],
                opsin_bias=[_f16(v) for v in (-0.0045, -0.003, -0.0036)], quant_bias=[_f16(v) for v in (0.9, 0.85, 0.97)],
                quant_bias_numerator=_f16(0.2))


def opsin_case(seed, **kw):
    return draw(seed, 40, 40, opsin=_opsin(np.random.default_rng(seed)), **kw)


def alpha_case(seed, width, height, k=1, **kw):
    """an alpha channel of eight bits with 0 and 255 in it, of the frame's size; k: the factor of the colours and of the alpha"""
    rng = np.random.default_rng(seed)
    plane = rng.integers(0, 256, (height, width))
    plane.reshape(-1)[rng.choice(plane.size, 2, replace=False)] = (0, 255)
    return draw(seed, width, height, extra=[dict(bits=8, alpha_associated=False, plane=plane, upsampling=k)], upsampling=k, **kw)


TAIL_CASES = {
    "up2_19x15_of_37x29": (_case(draw, 19, 15, upsampling=2, image_width=37, image_height=29), 31),
    "up4_ragged": (_case(draw, 67, 83, allowed=RAGGED_TYPES, upsampling=4), 32),
    "up8_40x40": (_case(draw, 40, 40, upsampling=8), 33),
    "up2_custom_weights": (functools.partial(fit, up_weights_case), 34),
    "noise_40x40": (_case(draw, 40, 40, **NOISE_FIELD), 35),
    "noise_264x264": (_case(draw, 264, 264, allowed=MID_TYPES, density=0.03, **NOISE_FIELD), 36),
    "noise_up2": (_case(draw, 136, 20, upsampling=2, **NOISE_FIELD), 37),
    # (not in the list the cases were asked for: noise is initialised at the upsampled frame's size, 272 x 40, which the image crops)
    "noise_up2_of_271x39": (_case(draw, 136, 20, upsampling=2, image_width=271, image_height=39, **NOISE_FIELD), 46),
    "noise_corr": (_case(draw, 40, 40, corr=dict(colour_factor=100, base_x=_f16(0.05), base_b=_f16(0.9), x_factor_lf=140,
                                                  b_factor_lf=100), **NOISE_FIELD), 38),
    "ycbcr_444": (_case(draw, 40, 40, xyb=False, do_ycbcr=True), 39),
    "opsin_custom": (functools.partial(fit, functools.partial(opsin_case, intensity_target=1000.0)), 40),
    "opsin_custom_epf2": (functools.partial(fit, functools.partial(opsin_case, epf_iters=2, **SMOOTH)), 41),
    "opsin_custom_up2": (functools.partial(fit, functools.partial(opsin_case, upsampling=2)), 42),
    "alpha_40x40": (functools.partial(fit, functools.partial(alpha_case, width=40, height=40)), 43),
    # (the tree splits on the stream index between the second and the third group's Modular stream: 18 + 3 + group)
    "alpha_264x264": (functools.partial(fit, functools.partial(alpha_case, width=264, height=264, allowed=MID_TYPES, density=0.03,
                                                               tree=dict(property=1, value=22, predictors=(4, 5)))), 44),
    "alpha_up2": (functools.partial(fit, functools.partial(alpha_case, width=40, height=40, k=2)), 45),
}


CASES = {
    "one_dct8": (_case(draw, 8, 8, allowed=(0,), dense=True), 11),
    "ragged_67x83": (_case(draw, 67, 83, allowed=MID_TYPES[:18] + (4, 5, 6, 7, 8, 9, 10, 11)), 12),
    "groups_264x264": (_case(draw, 264, 264, allowed=MID_TYPES, num_presets=2, density=0.03), 13),
    "two_lf_groups_2056x16": (_case(draw, 2056, 16, allowed=(0, 1, 2, 3, 4, 7, 12, 14), density=0.03), 14),
    "passes_2": (_case(draw, 40, 32, pass_shifts=[2], amp=40, density=0.2), 15),
    "passes_3": (_case(draw, 40, 32, pass_shifts=[3, 1], downsample=[4], last_pass=[0], amp=80, density=0.2), 16),
    "block_ctx": (functools.partial(fit, block_ctx_case), 17),
    "shared_order": (functools.partial(fit, shared_order), 18),
    "lf_rough": (lf_rough, 19),
    "corr": (functools.partial(fit, corr_case), 20),
    "xqm0_bqm7": (_case(draw, 32, 24, xqm=0, bqm=7), 21),
    "gab_custom": (_case(draw, 40, 40, gab_weights=([_f16(0.1), _f16(0.12), _f16(0.09)], [_f16(0.05), _f16(0.07), _f16(0.04)])), 22),
    "epf0": (_case(draw, 40, 40, **_restoration(0)), 23),
    "epf1": (_case(draw, 40, 40, **_restoration(1)), 24),
    "epf2_default": (_case(draw, 40, 40, epf_iters=2, **SMOOTH), 25),
    "epf3": (_case(draw, 40, 40, **_restoration(3)), 26),
    "rgb": (_case(draw, 24, 24, xyb=False), 27),
    "s420": (_case(draw, 40, 24, **_sub("s420")), 28),
    "s422": (_case(draw, 40, 24, **_sub("s422")), 29),
    "s440": (_case(draw, 40, 24, **_sub("s440")), 30),
}
for _t in range(27):  # each type alone in a frame of its own pixel size
    CASES["type_%02d" % _t] = (_case(draw, V.TYPES[_t][4], V.TYPES[_t][3], allowed=(_t,), first=[_t],
                                     density=0.3 if _t < 18 else 0.002), 100 + _t)
QUANT_CASES = tuple("quant_%d" % _s for _s in range(8))
for _s in range(8):
    CASES["quant_%d" % _s] = (quant_case(_s), 0)
OLD_CASES = tuple(sorted(CASES))  # the cases whose bytes tests/golden/jxl_writer_vardct_sha256.json records
CASES.update(TAIL_CASES)

_built = {}


def source(name):
    if name not in _built:
        fn, seed = CASES[name]
        _built[name] = fn(seed) if seed else fn()
    return _built[name]


_bytes = {}


def encoded(name, variant=None):
    if (name, variant) not in _bytes:
        _bytes[name, variant] = V.encode(source(name), variant)
    return _bytes[name, variant]


@functools.lru_cache(maxsize=None)
def expected(name, stages):
    """the model's planes of the padded frame after `stages` (vardct_ref64.decode: 1 IDCT, +2 Gaborish, +4 EPF, +8 XYB), with the
    magnitude companion"""
    x, a, undecided = M.decode(model_frame(source(name)), stages)
    assert not undecided.any()
    return x, a


# the cases the writer variants are shown on (every one of them exercises the variant's branch)
VARIANT_CASES = {
    "predicted_rounded_down": ("ragged_67x83", "groups_264x264"),
    "block_ctx_channel_not_exchanged": ("one_dct8", "ragged_67x83", "block_ctx"),
    "prev_inverted": ("one_dct8", "ragged_67x83", "passes_2"),
    "nonzero_ctx_without_4": ("ragged_67x83", "groups_264x264"),
    "vertical_not_flipped": ("type_06", "type_08", "type_10", "shared_order"),
    "shift_on_token": ("passes_2", "passes_3"),
    "lf_buffer_order": ("one_dct8", "lf_rough", "s420"),
    "block_info_rows_exchanged": ("ragged_67x83", "type_05"),
    "raw_stream_index_off_by_one": QUANT_CASES,
    "noise_lut_after_lf_dequant": ("noise_40x40", "noise_up2", "noise_up2_of_271x39", "noise_corr"),
    "extra_group_stream_index_off_by_one": ("alpha_264x264",),
}


@functools.lru_cache(maxsize=None)
def expected_image(name):
    """tail_model of the case: the planes after the colour transforms on the frame's upsampled bounds, with their companion"""
    t = tail_model(source(name), model=expected(name, EPF_STAGES))
    return t["x"], t["a"]


def expected_extras(name):
    """[(plane of the image's size, companion | None)] of the case's extra channels"""
    src = source(name)
    return [extra_model(src, e) for e in src.get("extra", [])]

