"""A float64 model of the reference's VarDCT pixel path, restated for the tests (no test in here): dequantisation, chroma from
luma, LLF, the inverse transform of all 27 types, invertSubsampling, Gaborish, the EPF sigma map, the EPF and the inverse XYB.

It is a second witness next to oracle/ (float32, loops, a line-by-line restatement): written from the reference's Java, in
matrices and whole-array numpy, and importing nothing of this project. The one table without a closed form, the AFV basis, is
read from include/jxl_tables.h (tests/test_vardct_ref64_cpu.py compares it with the reference's source text).

Every linear result comes with its MAGNITUDE COMPANION A: the same computation with every input and every matrix entry replaced
by its absolute value (A = |S| |x| for a transform, summed through chroma from luma and LLF, carried through the filters with their
own weights). Float32 rounding error is proportional to it, so the tests bound |float32 result - model| by K u A, u = 2^-24.

`mut=` selects deliberately WRONG variants of the model (the mutation table of the CPU tests: the tolerance must tell each of them
from the oracle); production comparisons pass none. Citations are file:line of the reference (java/com/traneptora/jxlatte/...)."""
import math
import os
import re

import numpy as np

D = np.float64
U = 2.0 ** -24  # unit roundoff of float32

# (name, type, parameterIndex, orderID, transformMethod, pixelHeight, pixelWidth): frame/vardct/TransformType.java:10-36
METHOD_DCT, METHOD_DCT2, METHOD_DCT4, METHOD_HORNUSS, METHOD_DCT8_4, METHOD_DCT4_8, METHOD_AFV = range(7)  # :47-53
TYPES = [
    ("DCT8", 0, 0, 0, 0, 8, 8), ("HORNUSS", 1, 1, 1, 3, 8, 8), ("DCT2", 2, 2, 1, 1, 8, 8), ("DCT4", 3, 3, 1, 2, 8, 8),
    ("DCT16", 4, 4, 2, 0, 16, 16), ("DCT32", 5, 5, 3, 0, 32, 32), ("DCT16_8", 6, 6, 4, 0, 16, 8), ("DCT8_16", 7, 6, 4, 0, 8, 16),
    ("DCT32_8", 8, 7, 5, 0, 32, 8), ("DCT8_32", 9, 7, 5, 0, 8, 32), ("DCT32_16", 10, 8, 6, 0, 32, 16),
    ("DCT16_32", 11, 8, 6, 0, 16, 32), ("DCT4_8", 12, 9, 1, 5, 8, 8), ("DCT8_4", 13, 9, 1, 4, 8, 8), ("AFV0", 14, 10, 1, 6, 8, 8),
    ("AFV1", 15, 10, 1, 6, 8, 8), ("AFV2", 16, 10, 1, 6, 8, 8), ("AFV3", 17, 10, 1, 6, 8, 8), ("DCT64", 18, 11, 7, 0, 64, 64),
    ("DCT64_32", 19, 12, 8, 0, 64, 32), ("DCT32_64", 20, 12, 8, 0, 32, 64), ("DCT128", 21, 13, 9, 0, 128, 128),
    ("DCT128_64", 22, 14, 10, 0, 128, 64), ("DCT64_128", 23, 14, 10, 0, 64, 128), ("DCT256", 24, 15, 11, 0, 256, 256),
    ("DCT256_128", 25, 16, 12, 0, 256, 128), ("DCT128_256", 26, 16, 12, 0, 128, 256),
]
NAME = [t[0] for t in TYPES]
BY_NAME = {t[0]: t[1] for t in TYPES}

MUTATIONS = ("no_weight_flip", "afv_flip_swapped", "afv_not_transposed", "dct84_48_exchanged", "hornuss_centre_00",
             "llf_scale_one", "cfl_origin_tile", "quant_bias_channel", "epf_no_border_mul", "epf_iter0_5tap", "gab_w_exchanged",
             "xyb_bias_sign")


def _mut(mut, name):
    if mut is not None and mut not in MUTATIONS:
        raise KeyError(mut)
    return mut == name


def pixel_size(t):
    """TransformType.java:113-114"""
    return TYPES[t][5], TYPES[t][6]


def dct_select_size(t):
    """:152-153"""
    return TYPES[t][5] >> 3, TYPES[t][6] >> 3


def param_index(t):
    return TYPES[t][2]


def method(t):
    return TYPES[t][4]


def matrix_size(t):
    """:154-155"""
    return min(pixel_size(t)), max(pixel_size(t))


def flip(t):
    """TransformType.flip() (:129-131)"""
    h, w = pixel_size(t)
    return h > w or (method(t) == METHOD_DCT and h == w)


def _tables():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "jxl_tables.h")).read()
    a, b = hdr.index("JXL_AFV_BASIS_INIT"), hdr.index("JXL_LLF_SCALE_INIT")
    hexf = r"-?0x[0-9a-f.]+p[-+]\d+"
    afv = np.array([float.fromhex(v) for v in re.findall(hexf, hdr[a:b])], D).reshape(16, 16)
    return afv, np.array([float.fromhex(v) for v in re.findall(hexf, hdr[b:])], D)


AFV_BASIS, _LLF_SCALE_TABLE = _tables()  # PassGroup.java:19-58 as float32 values; only the AFV table is used from the header
# LLFScale.java:7-19 has a closed form: 1 / (cos(pi i / 512) cos(pi i / 256) cos(pi i / 128)), rounded to float
LLF_SCALE = np.array([1.0 / (math.cos(math.pi * i / 512) * math.cos(math.pi * i / 256) * math.cos(math.pi * i / 128))
                      for i in range(32)], D).astype(np.float32).astype(D)


def llf_scale(t, mut=None):
    """TransformType.java:158-165 with LLFScale.scaleF (LLFScale.java:21-23)"""
    ch, cw = dct_select_size(t)
    yll, xll = (ch - 1).bit_length(), (cw - 1).bit_length()  # MathHelper.ceilLog2
    f32 = np.float32
    s = (LLF_SCALE[np.arange(ch) << (5 - yll)].astype(f32)[:, None] * LLF_SCALE[np.arange(cw) << (5 - xll)].astype(f32)[None, :]).astype(D)
    if _mut(mut, "llf_scale_one") and s.size > 1:
        s[-1, -1] = 1.0
    return s


def synthesis(n):
    """S[k][j] = the weight of coefficient j in sample k of MathHelper.inverseDCTHorizontal (MathHelper.java:68-78) with the
    table of :20-29: 1 for j = 0, sqrt2 cos(pi j (k + 1/2) / n) else. S^T S = n I."""
    k, j = np.arange(n, dtype=D)[:, None], np.arange(n, dtype=D)[None, :]
    s = math.sqrt(2.0) * np.cos(math.pi * j * (k + 0.5) / n)
    s[:, 0] = 1.0
    return s


def analysis(n):
    """forwardDCTHorizontal (:80-94): the transpose of synthesis(n) over n"""
    return synthesis(n).T / n


def idct2d(x, transposed=False, a=None):
    """MathHelper.inverseDCT2D (:96-122) of a height x width array of coefficients (a batch in the leading axes): sample (y, x) =
    sum c[u][v] S_h[y][u] S_w[x][v]; `transposed` delivers the width x height transpose. Returns (samples, companion)."""
    x = np.asarray(x, D)
    sh, sw = synthesis(x.shape[-2]), synthesis(x.shape[-1])
    out = sh @ x @ sw.T
    mag = np.abs(sh) @ (np.abs(x) if a is None else a) @ np.abs(sw).T
    if transposed:
        return np.swapaxes(out, -1, -2), np.swapaxes(mag, -1, -2)
    return out, mag


def fdct2d(x, a=None):
    """MathHelper.forwardDCT2D (:124-136)"""
    x = np.asarray(x, D)
    dh, dw = analysis(x.shape[-2]), analysis(x.shape[-1])
    return dh @ x @ dw.T, np.abs(dh) @ (np.abs(x) if a is None else a) @ np.abs(dw).T


# ---- the nine special 8x8 types as dense 64 x 64 matrices ---------------------------------------------------------------------
def _aux_dct2(c, s):
    """PassGroup.auxDCT2 (PassGroup.java:149-168) on a batch [..., 8, 8]: the s x s corner's quadrants butterflied and interleaved"""
    n = s // 2
    c00, c01, c10, c11 = c[..., :n, :n], c[..., :n, n:s], c[..., n:s, :n], c[..., n:s, n:s]
    r = c.copy()
    r[..., 0:s:2, 0:s:2] = c00 + c01 + c10 + c11
    r[..., 0:s:2, 1:s:2] = c00 + c01 - c10 - c11
    r[..., 1:s:2, 0:s:2] = c00 - c01 + c10 - c11
    r[..., 1:s:2, 1:s:2] = c00 - c01 - c10 + c11
    return r


def _special_apply(t, c, mut=None):
    """the inverse transform of a special type on a batch of 8 x 8 coefficient blocks (PassGroup.java:88-147, 234-325)"""
    m = method(t)
    if _mut(mut, "dct84_48_exchanged") and m in (METHOD_DCT8_4, METHOD_DCT4_8):
        m = METHOD_DCT8_4 + METHOD_DCT4_8 - m
    s4, s8 = synthesis(4), synthesis(8)
    out = np.zeros_like(c)
    if m == METHOD_DCT2:  # :273-277
        return _aux_dct2(_aux_dct2(_aux_dct2(c, 2), 4), 8)
    if m in (METHOD_HORNUSS, METHOD_DCT4):
        lf = _aux_dct2(c, 2)
        for y in range(2):
            for x in range(2):
                sub = c[..., y::2, x::2].copy()  # [iy][ix] = coeffs[y + 2 iy][x + 2 ix]
                if m == METHOD_DCT4:  # :306-324: transposed 4 x 4 IDCT
                    sub[..., 0, 0] = lf[..., y, x]
                    out[..., 4 * y:4 * y + 4, 4 * x:4 * x + 4] = s4 @ np.swapaxes(sub, -1, -2) @ s4.T
                    continue
                # :278-305
                residual = sub.sum(axis=(-1, -2)) - sub[..., 0, 0]
                centre = lf[..., y, x] - residual * 0.0625
                blk = sub + centre[..., None, None]
                if not _mut(mut, "hornuss_centre_00"):
                    blk[..., 0, 0] = sub[..., 1, 1] + centre  # :300-301
                    blk[..., 1, 1] = centre
                else:
                    blk[..., 0, 0] = centre
                out[..., 4 * y:4 * y + 4, 4 * x:4 * x + 4] = blk
        return out
    if m in (METHOD_DCT8_4, METHOD_DCT4_8):  # :234-269
        c0, c1 = c[..., 0, 0], c[..., 1, 0]
        for k, lf in enumerate((c0 + c1, c0 - c1)):
            sub = c[..., k::2, :].copy()  # 4 x 8: rows k, k + 2, ...
            sub[..., 0, 0] = lf
            if m == METHOD_DCT8_4:  # transposed: 8 rows of 4, side by side
                out[..., :, 4 * k:4 * k + 4] = s8 @ np.swapaxes(sub, -1, -2) @ s4.T
            else:
                out[..., 4 * k:4 * k + 4, :] = s4 @ sub @ s8.T
        return out
    if m == METHOD_AFV:  # invertAFV (:88-147)
        fy, fx = (1 if t in (16, 17) else 0), (1 if t in (15, 17) else 0)  # :97-98
        if _mut(mut, "afv_flip_swapped"):
            fy, fx = fx, fy
        c00, c10, c01 = c[..., 0, 0], c[..., 1, 0], c[..., 0, 1]
        a = c[..., 0::2, 0::2].copy()
        a[..., 0, 0] = (c00 + c10 + c01) * 4.0
        s = (a.reshape(a.shape[:-2] + (16,)) @ AFV_BASIS).reshape(a.shape)  # :100-110
        s = s[..., ::-1, :] if fy else s
        s = s[..., :, ::-1] if fx else s
        out[..., 4 * fy:4 * fy + 4, 4 * fx:4 * fx + 4] = s
        b = c[..., 0::2, 1::2].copy()
        b[..., 0, 0] = c00 + c10 - c01  # :119
        p = s4 @ b @ s4.T
        x0 = 0 if fx else 4
        out[..., 4 * fy:4 * fy + 4, x0:x0 + 4] = p if _mut(mut, "afv_not_transposed") else np.swapaxes(p, -1, -2)  # :128-133
        d = c[..., 1::2, :].copy()
        d[..., 0, 0] = c00 - c10
        y0 = 0 if fy else 4
        out[..., y0:y0 + 4, :] = s4 @ d @ s8.T  # :140-146
        return out
    raise KeyError(t)


def special_matrix(t, mut=None):
    """S[64][64]: pixel (row-major) x coefficient (row-major, position (0, 0) holding the LF sample) of a special 8 x 8 type"""
    return _special_apply(t, np.eye(64, dtype=D).reshape(64, 8, 8), mut).reshape(64, 64).T.copy()


def inverse_blocks(t, c, a, mut=None):
    """all blocks [n][h][w] of type t: dequantised coefficients -> pixels, with the companion"""
    if method(t) == METHOD_DCT:  # PassGroup.java:230-233
        return idct2d(c, False, a)
    s = special_matrix(t, mut)
    n = c.shape[0]
    return (c.reshape(n, 64) @ s.T).reshape(n, 8, 8), (a.reshape(n, 64) @ np.abs(s).T).reshape(n, 8, 8)


# ---- frame level ------------------------------------------------------------------------------------------------------------
def params_dict(p):
    """a jxl_vardct_params-like object (attribute access) as plain float64 / int values"""
    g = lambda n: getattr(p, n)
    v3 = lambda n: [float(x) for x in g(n)]
    return dict(width=int(g("width")), height=int(g("height")), scale_factor=v3("scale_factor"), quant_bias=v3("quant_bias"),
                quant_bias_numerator=float(g("quant_bias_numerator")), base_corr_x=float(g("base_corr_x")),
                base_corr_b=float(g("base_corr_b")), color_factor=int(g("color_factor")), gab=int(g("gab")), gab_w1=v3("gab_w1"),
                gab_w2=v3("gab_w2"), epf_iters=int(g("epf_iters")), global_scale_f=float(g("global_scale_f")),
                epf_sharp_lut=v3("epf_sharp_lut"), epf_channel_scale=v3("epf_channel_scale"),
                epf_pass0_sigma_scale=float(g("epf_pass0_sigma_scale")), epf_pass2_sigma_scale=float(g("epf_pass2_sigma_scale")),
                epf_border_sad_mul=float(g("epf_border_sad_mul")), xyb=int(g("xyb")), opsin_matrix=v3("opsin_matrix"),
                opsin_bias=v3("opsin_bias"), cbrt_opsin_bias=v3("cbrt_opsin_bias"), intensity_target=float(g("intensity_target")),
                sy=[int(x) for x in g("jpeg_upsampling_y")], sx=[int(x) for x in g("jpeg_upsampling_x")])


def frame_inputs(frame):
    """the boundary inputs of one frame (the dict layout of the synthetic frames: per-LF-group side info of 256 x 256 cells)
    as frame-level arrays; blocks = (y, x, type) in cells, in the reference's visiting order (LF groups in order, each one's
    blockList in order: HFCoefficients.java:74-76)"""
    p = params_dict(frame["params"])
    H, W = p["height"], p["width"]
    bh, bw = H // 8, W // 8
    sel = np.zeros((bh, bw), np.int64)
    hf = np.zeros((bh, bw), np.int64)
    sharp = np.zeros((bh, bw), np.int64)
    xfy = np.zeros(((bh + 7) // 8, (bw + 7) // 8), np.int64)
    bfy = np.zeros_like(xfy)
    lf = [np.zeros((bh >> p["sy"][c], bw >> p["sx"][c]), D) for c in range(3)]
    blocks = []
    for g in frame["lfgroups"]:
        y0, x0 = g["lfg_y"] * 256, g["lfg_x"] * 256
        ch, cw = np.asarray(g["dct_select"]).shape
        sel[y0:y0 + ch, x0:x0 + cw] = g["dct_select"]
        hf[y0:y0 + ch, x0:x0 + cw] = g["hf_mul"]
        sharp[y0:y0 + ch, x0:x0 + cw] = g["sharpness"]
        th, tw = np.asarray(g["x_from_y"]).shape
        xfy[y0 // 8:y0 // 8 + th, x0 // 8:x0 // 8 + tw] = g["x_from_y"]
        bfy[y0 // 8:y0 // 8 + th, x0 // 8:x0 // 8 + tw] = g["b_from_y"]
        for c in range(3):
            a = np.asarray(g["lf"][c], D)
            lf[c][y0 >> p["sy"][c]:(y0 >> p["sy"][c]) + a.shape[0], x0 >> p["sx"][c]:(x0 >> p["sx"][c]) + a.shape[1]] = a
        for by, bx in np.asarray(g["block_yx"]).reshape(-1, 2).tolist():
            blocks.append((y0 + by, x0 + bx, int(sel[y0 + by, x0 + bx])))
    coeff = []
    for c in range(3):  # channel c fills the first (H >> sy) (W >> sx) samples of its plane
        h, w = H >> p["sy"][c], W >> p["sx"][c]
        coeff.append(np.asarray(frame["coeff"][c]).reshape(-1)[:h * w].reshape(h, w).astype(np.int64))
    woffs = np.asarray(frame["woffs"]).astype(np.int64)
    wts = np.asarray(frame["weights"], D)
    return dict(p=p, coeff=coeff, blocks=blocks, hf_mul=hf, sharpness=sharp, x_from_y=xfy, b_from_y=bfy, lf=lf, weights=wts,
                woffs=woffs)


def weight_table(weights, woffs, t, c, mut=None):
    """HFGlobal.weights[parameterIndex][c] seen through the index swap of HFCoefficients.java:312-314: [y][x] of the block"""
    mh, mw = matrix_size(t)
    o = int(woffs[param_index(t) * 3 + c])
    w = weights[o:o + mh * mw].reshape(mh, mw)
    if _mut(mut, "no_weight_flip") and mh == mw:  # (on a tall block the unswapped index leaves the table: squares only)
        return w
    return w.T if flip(t) else w


def cfl_factor_maps(inp, mut=None):
    """HFCoefficients.chromaFromLuma (:146-192) as per-pixel factor planes. The factor of a 64 x 64 tile is computed, and cached,
    when the pixel at the tile's origin is visited (:177-181); every other pixel reads the cache (:183-184), which holds 0 until
    then. The visiting order is block by block, rows then columns inside a block, so a pixel gets its tile's factor iff it is
    visited no earlier than the tile's origin pixel."""
    p = inp["p"]
    H, W = p["height"], p["width"]
    order = np.zeros((H // 8, W // 8), np.int64)
    oy = np.zeros_like(order)
    ox = np.zeros_like(order)
    for i, (by, bx, t) in enumerate(inp["blocks"]):
        ch, cw = dct_select_size(t)
        order[by:by + ch, bx:bx + cw], oy[by:by + ch, bx:bx + cw], ox[by:by + ch, bx:bx + cw] = i, by, bx
    up = lambda m: np.repeat(np.repeat(m, 8, 0), 8, 1)
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    when = (up(order) << 16) + ((yy - up(oy) * 8) << 8) + (xx - up(ox) * 8)
    ty, tx = yy >> 6, xx >> 6
    if _mut(mut, "cfl_origin_tile"):  # the tile of the block's origin, for the whole block
        ty, tx = np.broadcast_to(up(oy) >> 3, (H, W)), np.broadcast_to(up(ox) >> 3, (H, W))
        seen = np.ones((H, W), bool)
    else:
        seen = when >= when[ty << 6, tx << 6]
    kx = p["base_corr_x"] + inp["x_from_y"][ty, tx] / float(p["color_factor"])  # :178-179
    kb = p["base_corr_b"] + inp["b_from_y"][ty, tx] / float(p["color_factor"])
    return np.where(seen, kx, 0.0), np.where(seen, kb, 0.0)


def idct_stage(inp, mut=None):
    """HFCoefficients.bakeDequantizedCoeffs (:140-144, 146-229, 267-319), PassGroup.invertVarDCT (PassGroup.java:203-331) and
    Frame.invertSubsampling (Frame.java:681-723): returns (planes [3][H][W], companion)."""
    p = inp["p"]
    H, W = p["height"], p["width"]
    sy, sx = p["sy"], p["sx"]
    subsampled = any(sy) or any(sx)
    out = [np.zeros((H >> sy[c], W >> sx[c]), D) for c in range(3)]
    mag = [np.zeros((H >> sy[c], W >> sx[c]), D) for c in range(3)]
    if not subsampled:
        kx, kb = cfl_factor_maps(inp, mut)
    by_type = {}
    for by, bx, t in inp["blocks"]:
        by_type.setdefault(t, []).append((by, bx))
    for t, pos in sorted(by_type.items()):
        ph, pw = pixel_size(t)
        ch, cw = dct_select_size(t)
        pos = np.array(pos, np.int64)
        mul = inp["hf_mul"][pos[:, 0], pos[:, 1]].astype(D)  # hfMultiplier at the block's origin (:299)
        hfmask = ~((np.arange(ph)[:, None] < ch) & (np.arange(pw)[None, :] < cw))  # :305-306
        scale = llf_scale(t, mut)
        dq, am, rows, cols = [None] * 3, [None] * 3, [None] * 3, [None] * 3
        for c in (1, 0, 2):
            keep = ((pos[:, 0] >> sy[c]) << sy[c] == pos[:, 0]) & ((pos[:, 1] >> sx[c]) << sx[c] == pos[:, 1])  # :292-297
            cy, cx = pos[keep, 0] >> sy[c], pos[keep, 1] >> sx[c]
            rows[c] = (cy * 8)[:, None, None] + np.arange(ph)[None, :, None]
            cols[c] = (cx * 8)[:, None, None] + np.arange(pw)[None, None, :]
            q = inp["coeff"][c][rows[c], cols[c]].astype(D)
            qb = p["quant_bias"][(c + 1) % 3 if _mut(mut, "quant_bias_channel") else c]
            with np.errstate(divide="ignore", invalid="ignore"):
                quant = np.where(np.abs(q) < 2, np.sign(q) * qb, q - p["quant_bias_numerator"] / q)  # :310-311
            w = weight_table(inp["weights"], inp["woffs"], t, c, mut)
            dq[c] = quant * (p["scale_factor"][c] / mul[keep])[:, None, None] * w[None] * hfmask[None]  # :299, :314
            am[c] = np.abs(dq[c])
            if not subsampled and c != 1:  # :186-188
                k = (kx if c == 0 else kb)[rows[c], cols[c]]
                dq[c] = dq[c] + k * dq[1]
                am[c] = am[c] + np.abs(k) * am[1]
        for c in range(3):
            keep = ((pos[:, 0] >> sy[c]) << sy[c] == pos[:, 0]) & ((pos[:, 1] >> sx[c]) << sx[c] == pos[:, 1])
            # the LF cells of the block on the channel's own grid (:214-220)
            ly = (pos[keep, 0] >> sy[c])[:, None, None] + np.arange(ch)[None, :, None]
            lx = (pos[keep, 1] >> sx[c])[:, None, None] + np.arange(cw)[None, None, :]
            llf, llfa = fdct2d(inp["lf"][c][ly, lx])
            dq[c][:, :ch, :cw] = llf * scale  # :221-226
            am[c][:, :ch, :cw] = llfa * scale
            px, pa = inverse_blocks(t, dq[c], am[c], mut)
            out[c][rows[c], cols[c]] = px
            mag[c][rows[c], cols[c]] = pa
    for c in range(3):
        out[c], mag[c] = invert_subsampling(out[c], mag[c], sx[c], sy[c])
    return np.stack(out), np.stack(mag)


def invert_subsampling(x, a, x_shift, y_shift):
    """Frame.invertSubsampling (Frame.java:681-723): horizontal doublings, then vertical ones; 3/4 and 1/4 of the clamped neighbours"""
    for axis, n in ((1, x_shift), (0, y_shift)):
        for _ in range(n):
            def double(v):
                v = np.moveaxis(v, axis, 0)
                prev, nxt = np.concatenate([v[:1], v[:-1]]), np.concatenate([v[1:], v[-1:]])
                r = np.empty((2 * v.shape[0],) + v.shape[1:], D)
                r[0::2], r[1::2] = 0.75 * v + 0.25 * prev, 0.75 * v + 0.25 * nxt
                return np.moveaxis(r, 0, axis)
            x, a = double(x), double(a)
    return x, a


def gab(x, a, w1, w2, mut=None):
    """Frame.performGabConvolution (Frame.java:505-542) of planes [C][H][W]; borders clamp (:526-534)"""
    if _mut(mut, "gab_w_exchanged"):
        w1, w2 = w2, w1
    outs = []
    for src, absw in ((np.asarray(x, D), False), (np.asarray(a, D), True)):
        res = np.empty_like(src)
        for c in range(src.shape[0]):
            mult = 1.0 / (1.0 + 4.0 * (w1[c] + w2[c]))
            k = np.array([[w2[c], w1[c], w2[c]], [w1[c], 1.0, w1[c]], [w2[c], w1[c], w2[c]]], D) * mult
            k = np.abs(k) if absw else k
            e = np.pad(src[c], 1, mode="edge")
            h, w = src[c].shape
            res[c] = sum(k[dy, dx] * e[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
        outs.append(res)
    return outs[0], outs[1]


COPY_THRESHOLD = float(np.float32(1.0) / np.float32(0.3))  # the float constant 1f/0.3f of Frame.java:608


def epf_sigma(hf_mul, sharpness, global_scale_f, sharp_lut):
    """the inverseSigma map of Frame.java:553-571 (one value per 8 x 8 cell)"""
    lut = np.asarray(sharp_lut, D)[np.asarray(sharpness)]
    with np.errstate(divide="ignore"):
        return 1.0 / (global_scale_f * lut / np.asarray(hf_mul, D))


def epf_undecided_cells(inv_sigma, rel=1e-5):
    """cells whose inverse sigma lies within `rel` of the copy threshold: float32 and float64 may decide differently there"""
    s = np.asarray(inv_sigma, D)
    with np.errstate(invalid="ignore"):
        return np.abs(s - COPY_THRESHOLD) <= rel * COPY_THRESHOLD


def _mirror_index(n, pad):
    """MathHelper.mirrorCoordinate (MathHelper.java:323-329) of -pad .. n + pad - 1"""
    m = np.mod(np.arange(-pad, n + pad), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


_CROSS = [(0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)]  # Frame.java:44-48 (y, x)
_DOUBLE_CROSS = _CROSS + [(-1, 1), (1, 1), (1, -1), (-1, -1), (0, -2), (0, 2), (2, 0), (-2, 0)]  # :50-55


def epf(x, a, iterations, inv_sigma, channel_scale, pass0_scale, pass2_scale, border_sad_mul, mut=None):
    """Frame.performEdgePreservingFilter (Frame.java:544-679) of three planes with a per-cell inverse sigma (scalar: Modular).
    The companion is carried with the filter's own weights."""
    x, a = np.asarray(x, D).copy(), np.asarray(a, D).copy()
    _, H, W = x.shape
    step = float(np.float32(1.65)) * 4.0 * (1.0 - float(np.float32(math.sqrt(0.5))))  # :545
    s = np.asarray(inv_sigma, D)
    if s.ndim == 2:
        s = np.repeat(np.repeat(s, 8, 0), 8, 1)[:H, :W]  # :605
    else:
        s = np.full((H, W), float(s))
    with np.errstate(invalid="ignore"):
        copied = np.isnan(s) | (s > COPY_THRESHOLD)  # :608
    s_ok = np.where(copied, 0.0, s)
    my, mx = np.arange(H)[:, None] & 7, np.arange(W)[None, :] & 7
    border = (my == 0) | (my == 7) | (mx == 0) | (mx == 7)  # :672-675
    bmul = np.where(border, 1.0 if _mut(mut, "epf_no_border_mul") else border_sad_mul, 1.0)
    iy, ix = _mirror_index(H, 3), _mirror_index(W, 3)
    win = lambda p, dy, dx, m=0: p[..., 3 + dy - m:3 + dy + H + m, 3 + dx - m:3 + dx + W + m]
    cs = np.asarray(channel_scale, D)[:, None, None]
    for i in range(3 if iterations > 0 else 0):  # epfIterations == 0: never called (:460)
        if i == 0 and iterations < 3:  # :584-587
            continue
        if i == 2 and iterations < 2:
            break
        sigma_scale = step * (pass0_scale if i == 0 else pass2_scale if i == 2 else 1.0)  # :592-598
        taps = _DOUBLE_CROSS if (i == 0 and not _mut(mut, "epf_iter0_5tap")) else _CROSS  # :599
        px, pa = x[:, iy][:, :, ix], a[:, iy][:, :, ix]
        sw, sx_, sa = np.zeros((H, W), D), np.zeros_like(x), np.zeros_like(a)
        for dy, dx in taps:
            if i == 2:  # epfDistance2 (:657-669)
                dist = (np.abs(win(px, 0, 0) - win(px, dy, dx)) * cs).sum(0)
            else:  # epfDistance1 (:638-655): the five-point cross around both pixels
                diff = (np.abs(win(px, 0, 0, 1) - win(px, dy, dx, 1)) * cs).sum(0)  # one pixel of margin
                dist = sum(diff[1 + ky:1 + ky + H, 1 + kx:1 + kx + W] for ky, kx in _CROSS)
            wgt = np.maximum(0.0, 1.0 - dist * bmul * sigma_scale * s_ok)  # epfWeight (:671-679)
            sw += wgt
            sx_ += wgt * win(px, dy, dx)
            sa += wgt * win(pa, dy, dx)
        x, a = np.where(copied, x, sx_ / sw), np.where(copied, a, sa / sw)  # :609-611, :625-626
    return x, a


def xyb(x, a, matrix, opsin_bias, cbrt_opsin_bias, intensity_target, mut=None):
    """OpsinInverseMatrix.invertXYB (color/OpsinInverseMatrix.java:105-142)"""
    x, a = np.asarray(x, D), np.asarray(a, D)
    m = np.asarray(matrix, D).reshape(3, 3) * (255.0 / intensity_target)
    ob = np.asarray(opsin_bias, D)
    cob = -np.asarray(cbrt_opsin_bias, D)
    if _mut(mut, "xyb_bias_sign"):
        cob = -cob
    g = np.stack([x[1] + x[0] + cob[0], x[1] - x[0] + cob[1], x[2] + cob[2]])
    ga = np.stack([a[1] + a[0] + abs(cob[0]), a[1] + a[0] + abs(cob[1]), a[2] + abs(cob[2])])
    mix = g * g * g + ob[:, None, None]
    mixa = ga * ga * ga + np.abs(ob)[:, None, None]
    return np.einsum("ij,jhw->ihw", m, mix), np.einsum("ij,jhw->ihw", np.abs(m), mixa)


YCBCR_OFFSET = 0.50196078431372549019  # the float literals of JXLCodestreamDecoder.java:275-279
YCBCR_R_CR, YCBCR_G_CB, YCBCR_G_CR, YCBCR_B_CB = 1.402, 0.34413628620102214650, 0.71413628620102214650, 1.772


def ycbcr(x, a):
    """the YCbCr loop of JXLCodestreamDecoder.performColorTransforms (JXLCodestreamDecoder.java:270-281): plane 0 is Cb, plane 1 Y,
    plane 2 Cr; the result is R, G, B. The reference runs it over getPaddedFrameSize() of the frame's bounds (:271), a region that
    holds the bounds, on buffers of at least that size; it works sample by sample, so on planes cropped to the bounds it is the
    whole plane."""
    x, a = np.asarray(x, D), np.asarray(a, D)
    off, r_cr, g_cb, g_cr, b_cb = (float(np.float32(v)) for v in (YCBCR_OFFSET, YCBCR_R_CR, YCBCR_G_CB, YCBCR_G_CR, YCBCR_B_CB))
    yh, ya = x[1] + off, a[1] + off
    out = np.stack([yh + r_cr * x[2], yh - g_cb * x[0] - g_cr * x[2], yh + b_cb * x[0]])
    mag = np.stack([ya + r_cr * a[2], ya + g_cb * a[0] + g_cr * a[2], ya + b_cb * a[0]])
    return out, mag


def decode(frame, stages, mut=None):
    """the stages of one frame as the reference runs them (Frame.java:455-463: inverse transforms, invertSubsampling, Gaborish,
    EPF; JXLCodestreamDecoder: invertXYB). stages: 2 adds Gaborish, 4 the EPF, 8 the inverse XYB to the inverse transforms.
    Returns (planes, companion, undecided): `undecided` marks the pixels of cells whose copy decision float32 may take differently."""
    inp = frame_inputs(frame) if "p" not in frame else frame
    p = inp["p"]
    x, a = idct_stage(inp, mut)
    undecided = np.zeros(x.shape[1:], bool)
    if stages & 2 and p["gab"]:
        x, a = gab(x, a, p["gab_w1"], p["gab_w2"], mut)
    if stages & 4 and p["epf_iters"] > 0:
        sig = epf_sigma(inp["hf_mul"], inp["sharpness"], p["global_scale_f"], p["epf_sharp_lut"])
        undecided = np.repeat(np.repeat(epf_undecided_cells(sig), 8, 0), 8, 1)
        x, a = epf(x, a, p["epf_iters"], sig, p["epf_channel_scale"], p["epf_pass0_sigma_scale"], p["epf_pass2_sigma_scale"],
                   p["epf_border_sad_mul"], mut)
    if stages & 8 and p["xyb"]:
        x, a = xyb(x, a, p["opsin_matrix"], p["opsin_bias"], p["cbrt_opsin_bias"], p["intensity_target"], mut)
    return x, a, undecided


def error_ratio(got, model, companion, mask=None):
    """the largest |got - model| / (u (A + |model|)) over the (unmasked) samples: the K a result needs. A sample where the bound is
    0 must be exact (ratio inf otherwise); NaN in either counts as inf."""
    got, model, companion = np.asarray(got, D), np.asarray(model, D), np.asarray(companion, D)
    err = np.abs(got - model)
    bound = U * (companion + np.abs(model))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    if mask is not None:
        r = np.where(mask, 0.0, r)
    return float(r.max()) if r.size else 0.0
