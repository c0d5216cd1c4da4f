"""JXLDecoder / JXLImage / PNGWriter: the reference's user-facing API (J/JXLDecoder.java, J/JXLCodestreamDecoder.java,
J/JXLImage.java, J/io/PNGWriter.java) on top of the C++ bitstream front-end (jxlatte_amd.frontend, row f2) and the
device library (jxlatte_amd._lib / host, the hot path).

    from jxlatte_amd.decoder import JXLDecoder, PNGWriter
    image = JXLDecoder("in.jxl").decode()
    PNGWriter(image).write(open("out.png", "wb"))

Every pixel operation goes through a *backend* object. The product backend is DeviceBackend (HIP kernels through the
C-ABI); it fails loudly without a GPU. Tests construct the decoder with the oracle-backed backend from
oracle/pybackend.py to exercise this host logic on CPU-only machines -- the product package never imports it.
"""
import ctypes as C
import math
import struct
import zlib

import numpy as np

from . import abi, frontend, hfglobal

F = np.float32

# ---- FrameFlags / ColorFlags constants (J/frame/FrameFlags.java, J/color/ColorFlags.java) ------------------------
REGULAR_FRAME, LF_FRAME, REFERENCE_ONLY, SKIP_PROGRESSIVE = 0, 1, 2, 3
VARDCT, MODULAR = 0, 1
FLAG_NOISE, FLAG_PATCHES, FLAG_SPLINES, FLAG_USE_LF_FRAME, FLAG_SKIP_ADAPTIVE_LF = 1, 2, 16, 32, 128
CE_RGB, CE_GRAY, CE_XYB = 0, 1, 2
TF_BT709, TF_UNKNOWN, TF_LINEAR, TF_SRGB, TF_PQ, TF_DCI, TF_HLG = [(1 << 24) + v for v in (1, 2, 8, 13, 16, 17, 18)]
PRI_SRGB = np.array([0.639998686, 0.330010138, 0.300003784, 0.600003357, 0.150002046, 0.059997204], F)
PRI_BT2100 = np.array([0.708, 0.292, 0.170, 0.797, 0.131, 0.046], F)
PRI_P3 = np.array([0.680, 0.320, 0.265, 0.690, 0.150, 0.060], F)
WP_D65 = np.array([0.3127, 0.3290], F)
WP_D50 = np.array([0.34567, 0.34567], F)
PEAK_DETECT_AUTO, PEAK_DETECT_ON, PEAK_DETECT_OFF = -1, 1, 0


class InvalidBitstreamException(IOError):
    pass


class UnsupportedOperationException(RuntimeError):
    pass


# ---- colour management (J/color/ColorManagement.java, J/util/MathHelper.java matrix helpers), float32 ------------
def _xy_matches(a, b):
    return abs(F(a[0]) - F(b[0])) + abs(F(a[1]) - F(b[1])) < 1e-4


def _prim_matches(a, b):
    return all(_xy_matches(a[2 * i:2 * i + 2], b[2 * i:2 * i + 2]) for i in range(3))


def _mat_mul(left, right):
    """MathHelper.matrixMultiply: result[y] = left[y] . right with the row-vector accumulation order of :257-269"""
    if left is None:
        return right
    if right is None:
        return left
    out = np.zeros((3, 3), F)
    for y in range(3):
        for k in range(3):
            for x in range(3):
                out[y, x] = F(out[y, x] + F(left[y, k] * right[k, x]))
    return out


def _mat_vec(m, v):
    out = np.zeros(3, F)
    for y in range(3):
        for x in range(3):
            out[y] = F(out[y] + F(m[y, x] * v[x]))
    return out


def _invert3(m):
    """MathHelper.invertMatrix3x3 (:296-322)"""
    det = F(0)
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        det = F(det + F(F(F(m[c, 0] * m[c1, 1]) * m[c2, 2]) - F(F(m[c, 0] * m[c1, 2]) * m[c2, 1])))
    if det == 0:
        return None
    inv_det = F(F(1) / det)
    out = np.zeros((3, 3), F)
    for x in range(3):
        for y in range(3):
            x1, x2, y1, y2 = (x + 1) % 3, (x + 2) % 3, (y + 1) % 3, (y + 2) % 3
            out[y, x] = F(F(F(m[x1, y1] * m[x2, y2]) - F(m[x2, y1] * m[x1, y2])) * inv_det)
    return out


_BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]], F)
_BRADFORD_INV = _invert3(_BRADFORD)


def _xyz(xy):
    if xy[0] < 0 or xy[0] > 1 or xy[1] <= 0 or xy[1] > 1:
        raise ValueError("chromaticity out of range")
    inv_y = F(F(1) / F(xy[1]))
    return np.array([F(F(xy[0]) * inv_y), F(1), F(F(F(F(1) - F(xy[0])) - F(xy[1])) * inv_y)], F)


def _adapt_white_point(target, current):
    target = WP_D50 if target is None else target
    current = WP_D50 if current is None else current
    lms_c = _mat_vec(_BRADFORD, _xyz(current))
    lms_t = _mat_vec(_BRADFORD, _xyz(target))
    if np.any(np.abs(lms_c) < 1e-8):
        raise ValueError("degenerate white point")
    a = np.zeros((3, 3), F)
    for i in range(3):
        a[i, i] = F(lms_t[i] / lms_c[i])
    return _mat_mul(_mat_mul(_BRADFORD_INV, a), _BRADFORD)


def _primaries_to_xyz(prim, wp):
    wp = WP_D50 if wp is None else wp
    pm = np.stack([_xyz(prim[0:2]), _xyz(prim[2:4]), _xyz(prim[4:6])]).T.astype(F).copy()
    xyz = _mat_vec(_invert3(pm), _xyz(wp))
    return _mat_mul(pm, np.diag(xyz).astype(F))


def get_conversion_matrix(target_prim, target_wp, current_prim, current_wp):
    """ColorManagement.getConversionMatrix (:141-151)"""
    if _prim_matches(target_prim, current_prim) and _xy_matches(target_wp, current_wp):
        return np.eye(3, dtype=F)
    wpc = None if _xy_matches(target_wp, current_wp) else _adapt_white_point(target_wp, current_wp)
    forward = _primaries_to_xyz(current_prim, current_wp)
    reverse = _invert3(_primaries_to_xyz(target_prim, target_wp))
    return _mat_mul(_mat_mul(reverse, wpc), forward)


def _to_linear(buf, tf):
    """TransferFunction.toLinearF for the transfer functions an un-XYB image can be tagged with (host side)"""
    b = buf.astype(F)
    if tf == TF_LINEAR:
        return b
    if tf == TF_SRGB:
        hi = np.power((b * F(0.9478672985781991) + F(0.052132701)).astype(np.float64), 2.4).astype(F)
        return np.where(b < F(0.0404482362771082), b * F(0.07739938080495357), hi).astype(F)
    d = b.astype(np.float64)
    if tf == TF_BT709:
        hi = np.power((d + 0.0992968268094429403) * 0.90967241568627260377, 2.2222222222222222222)
        return np.where(d < 0.081242858298635133011, d * 0.22222222222222222222, hi).astype(F)
    if tf == TF_PQ:
        e = np.power(d, 0.012683313515655965121)
        return np.power((e - 0.8359375) / (18.8515625 + 18.6875 * e), 6.2725880551301684533).astype(F)
    if tf == TF_HLG:
        raise UnsupportedOperationException("Not yet implemented")  # ColorManagement.java:164
    gamma = 3846154 if tf == TF_DCI else tf
    if gamma < (1 << 24):
        return np.power(d, 1e7 / gamma).astype(F)  # GammaTransferFunction
    raise ValueError("Invalid transfer function")


def _tf_selector(tf):
    """ColorManagement.getTransferFunction (:149-170) as the device library's (JXL_TF_*, gamma)"""
    named = {TF_LINEAR: abi.TF_LINEAR, TF_SRGB: abi.TF_SRGB, TF_BT709: abi.TF_BT709, TF_PQ: abi.TF_PQ}
    if tf in named:
        return named[tf], 0
    if tf == TF_HLG:
        raise UnsupportedOperationException("Not yet implemented")  # ColorManagement.java:161-162
    gamma = 3846154 if tf == TF_DCI else tf
    if 0 < gamma < (1 << 24):
        return abi.TF_GAMMA, gamma  # GammaTransferFunction
    raise ValueError("Invalid transfer function")


# ---- splines (J/frame/features/spline/Spline.java): host-side feature, as in the reference ------------------------------
_SQRT_H = F(math.sqrt(0.5))
_SQRT_F = F(math.sqrt(0.125))


def _erf(z):
    """MathHelper.erf (MathHelper.java:40-66), vectorised float32 with the reference's operation order"""
    z = z.astype(F)
    az = np.abs(z)
    t = (F(1) / (az * F(0.5) + F(1))).astype(F)
    u = t * F(0.17087277) - F(0.82215223)
    for cst, sign in ((1.48851587, 1), (1.13520398, -1), (0.27886807, 1), (0.18628806, -1), (0.09678418, 1), (0.37409196, 1),
                      (1.00002368, 1)):
        u = (t * u + F(cst)).astype(F) if sign > 0 else (t * u - F(cst)).astype(F)
    u = (t * u - F(1.26551223)).astype(F)
    big = (F(1) - t * np.exp((-(z * z) + u).astype(np.float64)).astype(F)).astype(F)
    t2 = (F(1) / (az * F(0.47047) + F(1))).astype(F)
    u2 = (t2 * ((t2 * ((t2 * F(0.7478556) - F(0.0958798)).astype(F)) + F(0.3480242)).astype(F))).astype(F)
    small = (F(1) - u2 * np.exp((-(z * z)).astype(np.float64)).astype(F)).astype(F)
    a = np.where(az > F(1e-4), big, small).astype(F)
    return np.where(z < 0, -a, a).astype(F)


def _spline_knots(control):
    """Spline.upsampleControlPoints (Spline.java:27-87): the knots as two lists of float32 (y, x). Repeated control points
    divide by a zero t[k + 1] - t[k]: their NaN / inf knots are kept as the float operations give them"""
    cp = [(int(y), int(x)) for y, x in control]
    if len(cp) == 1:
        uy, ux = [F(cp[0][0])], [F(cp[0][1])]
    else:
        def i32(v):  # Point arithmetic is Java int arithmetic: it wraps (Spline.java:37-43)
            return ((v + 2**31) % 2**32) - 2**31
        ext = [(i32(cp[0][0] * 2 - cp[1][0]), i32(cp[0][1] * 2 - cp[1][1]))] + cp + \
              [(i32(cp[-1][0] * 2 - cp[-2][0]), i32(cp[-1][1] * 2 - cp[-2][1]))]
        n = 16 * (len(ext) - 3) + 1
        uy, ux = [F(0)] * n, [F(0)] * n
        for i in range(len(ext) - 3):
            pY = [F(ext[i + k][0]) for k in range(4)]
            pX = [F(ext[i + k][1]) for k in range(4)]
            uy[i << 4], ux[i << 4] = pY[1], pX[1]
            t = [F(0)] * 4
            dY, dX = [F(0)] * 3, [F(0)] * 3
            for k in range(3):
                dY[k], dX[k] = F(pY[k + 1] - pY[k]), F(pX[k + 1] - pX[k])
                t[k + 1] = F(t[k] + F(math.pow(float(F(F(dY[k] * dY[k]) + F(dX[k] * dX[k]))), 0.25)))
            for step in range(1, 16):
                knot = F(t[1] + F(F(F(0.0625) * F(step)) * F(t[2] - t[1])))
                aY, aX = [F(0)] * 3, [F(0)] * 3
                with np.errstate(all="ignore"):
                    for k in range(3):
                        f = F(F(knot - t[k]) / F(t[k + 1] - t[k]))
                        aY[k], aX[k] = F(F(dY[k] * f) + pY[k]), F(F(dX[k] * f) + pX[k])
                    bY, bX = [F(0)] * 2, [F(0)] * 2
                    for k in range(2):
                        f = F(F(knot - t[k]) / F(t[k + 2] - t[k]))
                        bY[k], bX[k] = F(F(F(aY[k + 1] - aY[k]) * f) + aY[k]), F(F(F(aX[k + 1] - aX[k]) * f) + aX[k])
                    f = F(F(knot - t[1]) / F(t[2] - t[1]))
                    uy[i * 16 + step] = F(F(F(bY[1] - bY[0]) * f) + bY[0])
                    ux[i * 16 + step] = F(F(F(bX[1] - bX[0]) * f) + bX[0])
        uy[-1], ux[-1] = F(cp[-1][0]), F(cp[-1][1])
    return uy, ux


def _spline_arcs(control):
    """Spline.upsampleControlPoints + computeIntermediarySamples(1.0f): list of (y, x, arcLength)"""
    uy, ux = _spline_knots(control)
    rd = F(1.0)
    cy, cx = uy[0], ux[0]
    nxt = 0
    arcs = [(cy, cx, rd)]
    while nxt < len(uy):
        py, px = cy, cx
        acc = F(0)
        while True:
            if nxt >= len(uy):
                arcs.append((py, px, acc))
                break
            ny, nx = uy[nxt], ux[nxt]
            dy, dx = F(ny - py), F(nx - px)
            to_next = F(math.sqrt(float(F(F(dy * dy) + F(dx * dx)))))
            if F(acc + to_next) >= rd:
                f = F(F(rd - acc) / to_next)
                cy, cx = F(F(dy * f) + py), F(F(dx * f) + px)
                arcs.append((cy, cx, rd))
                break
            acc = F(acc + to_next)
            py, px = ny, nx
            nxt += 1
    return arcs


def _fourier_ict(coeffs, t):
    total = F(_SQRT_H * coeffs[0])
    for i in range(1, 32):
        total = F(total + F(coeffs[i] * F(math.cos(i * (math.pi / 32.0) * (float(t) + 0.5)))))
    return total


def spline_arc_table(splines, base_corr_x, base_corr_b, width, height):
    """the per-arc half of Frame.renderSplines + Spline.renderSpline (Spline.java:155-179): the arcs that draw, in the
    reference's order, as tuples (y, x, sigma, inv_sigma, values[3], (x0, x1, y0, y1)) of float32 / int. The reference never
    stores the spline index (Spline.java:22-24), so every spline is drawn with the coefficients of spline 0;
    `MathHelper.max(float...)` returns the minimum (MathHelper.java:190-195). Both restated as they are. The library's
    jxl_spline_arcs is the same table with mul[c] = (0.25f * values[c]) * sigma."""
    table = []
    if not splines:
        return table
    s0 = splines[0]
    qa = F(F(s0["quant_adjust"]) / F(8))
    inv_qa = F(F(1) / F(F(1) + qa)) if qa >= 0 else F(F(1) - qa)
    adj = [F(F(0.005939697) * inv_qa), F(F(0.106066017) * inv_qa), F(F(0.098994949) * inv_qa), F(F(0.47135738) * inv_qa)]
    cY = [F(F(v) * adj[1]) for v in s0["coeff"][1]]
    cX = [F(F(F(v) * adj[0]) + F(F(base_corr_x) * cY[i])) for i, v in enumerate(s0["coeff"][0])]
    cB = [F(F(F(v) * adj[2]) + F(F(base_corr_b) * cY[i])) for i, v in enumerate(s0["coeff"][2])]
    cS = [F(F(v) * adj[3]) for v in s0["coeff"][3]]
    for sp in splines:
        arcs = _spline_arcs(sp["control"])
        rd = F(1.0)
        arc_len = F(F(F(len(arcs)) - F(2)) * rd + arcs[-1][2])
        if arc_len <= 0:
            continue
        for i, (ay, ax, alen) in enumerate(arcs):
            with np.errstate(all="ignore"):
                prog = min(F(1.0), F(F(F(i) * rd) / arc_len))
                t = F(F(31) * prog)
                vals = [F(_fourier_ict(c, t) * alen) for c in (cX, cY, cB)]
                sigma = _fourier_ict(cS, t)
                inv_sigma = F(F(1) / sigma)
                max_color = min(F(0.01), vals[0], vals[1], vals[2])  # MathHelper.max(float...) is a minimum
                md = F(math.sqrt(float(F(F(F(-2) * sigma) * sigma * F(F(F(math.log(0.1)) * F(3)) - max_color))))) \
                    if F(F(F(-2) * sigma) * sigma * F(F(F(math.log(0.1)) * F(3)) - max_color)) >= 0 else F(np.nan)
            if not np.isfinite(md):
                continue  # (int)(NaN + 0.5f) == 0 for both bounds of an empty-ish box; nothing sensible to draw

            def rnd(v):
                return int(np.trunc(np.clip(F(v + F(0.5)), -2**31, 2**31 - 1)))
            xb, xe = max(0, rnd(F(ax - md))), min(width - 1, rnd(F(ax + md)))
            yb, ye = max(0, rnd(F(ay - md))), min(height - 1, rnd(F(ay + md)))
            if xb > xe or yb > ye:
                continue
            table.append((ay, ax, sigma, inv_sigma, vals, (xb, xe, yb, ye)))
    return table


def render_splines(buffers, splines, base_corr_x, base_corr_b, width, height):
    """Frame.renderSplines + Spline.renderSpline (Spline.java:157-201) on the host: the arcs of spline_arc_table drawn in
    order, each over its box (:180-197)"""
    for ay, ax, sigma, inv_sigma, vals, (xb, xe, yb, ye) in spline_arc_table(splines, base_corr_x, base_corr_b, width, height):
        ys = np.arange(yb, ye + 1, dtype=F)[:, None]
        xs = np.arange(xb, xe + 1, dtype=F)[None, :]
        dy, dx = (ys - ay).astype(F), (xs - ax).astype(F)
        dist = np.sqrt(((dy * dy).astype(F) + (dx * dx).astype(F)).astype(np.float64)).astype(F)
        with np.errstate(all="ignore"):
            fac = _erf(((F(0.5) * dist).astype(F) + _SQRT_F).astype(F) * inv_sigma)
            fac = (fac - _erf(((F(0.5) * dist).astype(F) - _SQRT_F).astype(F) * inv_sigma)).astype(F)
            for c in range(3):
                extra = ((((F(0.25) * vals[c]) * sigma).astype(F) * fac).astype(F) * fac).astype(F)
                buffers[c][yb:ye + 1, xb:xe + 1] = (buffers[c][yb:ye + 1, xb:xe + 1] + extra).astype(F)


# ---- backends -------------------------------------------------------------------------------------------------
def lf_from_lf_frame(lf_buffer, lfg_y, lfg_x, cells_h, cells_w, jpeg_up_y, jpeg_up_x, bits_per_sample):
    """LFCoefficients.java:44-57 (USE_LF_FRAME): the dequantised LF of LF group (lfg_y, lfg_x) is a copy out of the planes a
    preceding LF frame left in lfBuffer[] -- rows pY .. pY + size, columns from pX, with pY = lfg_y << 8, pX = lfg_x << 8 for
    every channel (the reference does not shift the origin of a subsampled channel; kept) -- after ImageBuffer.castToFloat
    (integer planes: v * (1f / maxValue)). Returns three float32 planes in X, Y, B order, each exactly the size the LF group
    entry of the device expects: the planes travel as bare pointers, and a numpy slice that runs past the stored planes comes
    back short without a word. The reference's System.arraycopy (:53) throws there; so does this -- a consuming frame whose LF
    groups reach beyond the LF frame's planes (a crop larger than the image, say) is an invalid bitstream."""
    py, px = lfg_y << 8, lfg_x << 8
    out = []
    for c in range(3):
        b = lf_buffer[c]
        h, w = cells_h >> jpeg_up_y[c], cells_w >> jpeg_up_x[c]
        win = b[py:py + h, px:px + w]
        if win.shape != (h, w):
            raise InvalidBitstreamException("LF frame too small: LF group (%d, %d) needs %d x %d cells at (%d, %d) of stored planes of %d x %d"
                                            % (lfg_y, lfg_x, w, h, px, py, b.shape[1], b.shape[0]))
        if win.dtype != np.float32:
            win = (win.astype(np.float32) * (F(1) / F((1 << bits_per_sample) - 1))).astype(np.float32)
        out.append(np.ascontiguousarray(win, np.float32))
    return out


def put_group_sparse(hf, pass_, grp, sp):
    """one (pass, group) of frontend.Frontend.coeffs_sparse -> host.Frame.putGroupSparseEntries. A call carries ONE entry form:
    when only some channels came back wide (a value outside int16), the narrow lists are widened"""
    wide = any(w for _, w, _ in sp)
    ents = []
    for e, w, _ in sp:
        if wide and not w:
            t = np.empty(2 * e.size, np.uint32)
            t[0::2] = e & 0xffff
            t[1::2] = (e >> 16).astype(np.uint16).view(np.int16).astype(np.int32).view(np.uint32)
            e = t
        ents.append(e)
    hf.putGroupSparseEntries(pass_, grp, ents, wide)


def feed_frame(hf, lfgroups, groups, sparse):
    """one VarDCT frame's inputs into a host.Frame: the LF groups, then every (pass, group) of `groups`, dense planes or the
    entry lists of Frontend.coeffs_sparse. Returns the frame"""
    for g in lfgroups:
        hf.setLFGroup(g)
        if g.get("lf_quant") is not None:
            hf.setLFGroupQuant(g["lfg_y"], g["lfg_x"], g["lf_quant"], g["scaled_dequant"], g["extra_precision"], g["x_factor_lf"],
                               g["b_factor_lf"], g["adaptive_smoothing"])
    for pass_, grp, q in groups:
        if sparse:
            put_group_sparse(hf, pass_, grp, q)
        else:
            hf.putGroup(pass_, grp, q)
    return hf


# ---- the type plan of the patch stage (JXLCodestreamDecoder.blendBuffers' casts, :433-465) ------------------------
class PatchPlan:
    """what JXLDecoder._patches would do to the TYPES of the planes, without touching a sample (patch_type_plan)"""

    def __init__(self):
        self.calls = []       # one dict per backend.blend call, in order: i, j, d, slot, mode, pmode, below, canvas / frame_alpha /
                              # ref_alpha (dtype, or None where the call passes None)
        self.segments = []    # dicts: first, last (call indices, inclusive), frame (dtype per channel), ref {slot: [dtype or None]}
        self.frame_types = None  # after the stage
        self.ref_types = {}      # slot -> [dtype, or None for a plane still absent]; only the slots some applied patch names
        self.created = set()     # (slot, channel): reference planes blendBuffers creates as zeros (:441-442, :449-451)
        self.gather = True       # False: a below mode (5, 7) reads the frame away from the pixel it writes (see jxl_patch_bins)
        self.pos = None          # the positions in stage order, abi.PATCH_POS_DTYPE (the absent-slot ones included)
        self.blend = None        # [n_pos][colours + num_extra][3]: one blend row per position, one entry per channel


def _patch_upsampling_mismatch(info, fr, mode, c):
    """computePatches' check of an extra channel's upsampling against the frame's (:243-247). fr: the frame record, looked at
    for an extra channel with a mode above 3 only"""
    return mode > 3 and c > 0 and fr.upsampling > 1 and (fr.ec_upsampling[c - 1] << info.ec_dim_shift[c - 1]) != fr.upsampling


def patch_type_plan(info, patches, frame_buffers, reference, frame_colors, fr=None):
    """Simulates JXLDecoder._patches / _blend_buffers(patch=True) over the whole list of patches (the dicts of Frontend.patch) on
    the dtypes and shapes of `frame_buffers` and `reference` alone. blendBuffers casts planes to float as a side effect, decided
    on the RAW patch mode compared with the frame blend constants; the casts persist in the frame's buffers and in the reference
    slot. A cast of a plane no earlier application of the running segment handed to backend.blend commutes with those
    applications and is hoisted to the segment's entry; a cast of a plane one of them used closes the segment. So a segment is a
    maximal run of applications during which every plane they use keeps its type, and its entry types are the types after its
    last application. Raises what _patches would raise by itself, before anything runs: the InvalidBitstreamExceptions of
    computePatches and of blendBuffers' switch (raw mode 1, "Illegal blend mode") in stage order (and the IndexError /
    AttributeError of a malformed list). fr: the frame record (upsampling, ec_upsampling) for the check of :243-247; None: the
    frame is not upsampled."""
    colors = 1 if info.colour_space == CE_GRAY else 3
    if colors != frame_colors:
        raise ValueError("the patch plan covers frames with the image's colour count")
    has_extra = info.num_extra > 0
    plan = PatchPlan()
    ft = [b.dtype for b in frame_buffers]
    fshape = frame_buffers[0].shape
    rt = plan.ref_types
    f32 = np.dtype(np.float32)
    used, first = {}, 0  # plane key -> dtype it was used with in the running segment
    pos, rows = [], []

    def close(last):
        plan.segments.append(dict(first=first, last=last, frame=list(ft), ref={k: list(v) for k, v in rt.items()}))

    for i, p in enumerate(patches):
        for j in range(p["positions"].shape[0]):
            pos.append((int(p["positions"][j, 0]), int(p["positions"][j, 1]), p["h"], p["w"], p["ref"], p["y0"], p["x0"], len(rows)))
            row = np.asarray(p["blend"][j], np.int32).reshape(1 + info.num_extra, 3)
            rows.append(row[[0] * colors + list(range(1, 1 + info.num_extra))])  # per channel d (:239)
        if p["ref"] > 3:
            raise InvalidBitstreamException("Patch out of range")
        ref = reference[p["ref"]]
        if ref is None:
            continue
        slot = p["ref"]
        if p["y0"] + p["h"] > ref[0].shape[0] or p["x0"] + p["w"] > ref[0].shape[1]:
            raise InvalidBitstreamException("Patch too large")
        if slot not in rt:
            rt[slot] = [None if b is None else b.dtype for b in ref]
        r = rt[slot]
        for j in range(p["positions"].shape[0]):
            y0, x0 = int(p["positions"][j, 0]), int(p["positions"][j, 1])
            if y0 < 0 or x0 < 0 or p["h"] + y0 > fshape[0] or p["w"] + x0 > fshape[1]:
                raise InvalidBitstreamException("Patch size out of bounds")
            for d in range(colors + info.num_extra):
                c = 0 if d < colors else d - colors + 1
                mode, alpha, clamp = (int(v) for v in p["blend"][j, c])
                if mode == 0:
                    continue
                if fr is not None and _patch_upsampling_mismatch(info, fr, mode, c):
                    raise InvalidBitstreamException("Alpha channel upsampling mismatch during patches")
                if mode == 1:  # -> BLEND_REPLACE, for which the switch of :493-512 has no case
                    raise InvalidBitstreamException("Illegal blend mode")
                # -- _blend_buffers(d, ..., patch=True): the canvas is the frame plane itself
                ex = d - colors
                is_alpha = ex >= 0 and info.ec_type[ex] == 0
                premult = has_extra and bool(info.ec_alpha_associated[alpha])  # noqa: F841  (an IndexError is the host path's)
                canvas_dt = ft[d]  # the local `canvas` / `frame_buffer`: an alpha cast below does not reach it
                if r[d] is None:
                    r[d] = canvas_dt
                    plan.created.add((slot, d))
                a_ref, a_frame = colors + alpha, frame_colors + alpha
                pmode, below = {5: (abi.BLEND_BLEND, True), 6: (abi.BLEND_MULADD, False), 7: (abi.BLEND_MULADD, True)}.get(mode, (mode - 1, False))
                if has_extra and mode in (abi.BLEND_BLEND, abi.BLEND_MULADD):
                    if mode == abi.BLEND_BLEND:
                        if r[a_ref] is None:
                            plan.created.add((slot, a_ref))
                        r[a_ref] = f32
                    ft[a_frame] = f32
                fa = ra = None
                if has_extra:
                    ra, fa = r[a_ref], ft[a_frame]
                should_cast = mode == abi.BLEND_MULT or (mode == abi.BLEND_BLEND and has_extra) or \
                    (mode == abi.BLEND_MULADD and has_extra and not is_alpha)
                if should_cast or r[d] != canvas_dt:
                    canvas_dt = r[d] = f32
                ft[d] = canvas_dt  # canvas_list[idx] = backend.blend(...): the result has the canvas' type
                if below and (p["y0"] != y0 or p["x0"] != x0 or tuple(ref[0].shape) != tuple(fshape)):
                    plan.gather = False
                call = dict(i=i, j=j, d=d, slot=slot, mode=mode, pmode=pmode, below=below, canvas=canvas_dt,
                            frame_alpha=fa if fa == f32 else None, ref_alpha=ra if ra == f32 else None, pos=len(pos) - p["positions"].shape[0] + j)
                k = len(plan.calls)
                now = {}
                if call["frame_alpha"] is not None:
                    now[("f", a_frame)] = f32
                if call["ref_alpha"] is not None:
                    now[("r", slot, a_ref)] = f32
                now.update({("f", d): canvas_dt, ("r", slot, d): r[d]})  # (last: the call leaves its result, of the canvas' type, in plane d)
                types = lambda key: ft[key[1]] if key[0] == "f" else rt[key[1]][key[2]]  # noqa: E731
                if any(types(key) != dt for key, dt in used.items()):
                    # (the segment's entry types are those BEFORE this application's casts of the planes it used: they are in `used`)
                    seg_f, seg_r = list(ft), {s_: list(v) for s_, v in rt.items()}
                    for key, dt in used.items():
                        if key[0] == "f":
                            seg_f[key[1]] = dt
                        else:
                            seg_r[key[1]][key[2]] = dt
                    plan.segments.append(dict(first=first, last=k - 1, frame=seg_f, ref=seg_r))
                    used, first = {}, k
                used.update(now)
                plan.calls.append(call)
    if plan.calls:
        close(len(plan.calls) - 1)
    plan.frame_types = list(ft)
    plan.pos = np.array(pos, abi.PATCH_POS_DTYPE) if pos else np.zeros(0, abi.PATCH_POS_DTYPE)
    plan.blend = np.stack(rows) if rows else np.zeros((0, colors + info.num_extra, 3), np.int32)
    return plan


class BlendPlan:
    """what one blendFrame does to the TYPES of the planes, and the one launch that replays it (blend_type_plan)"""

    def __init__(self):
        self.verdict = "device"   # or "land: <reason>"
        self.rect = None          # (h, w, canvas_y, canvas_x, frame_y, frame_x, ref_y, ref_x); None: the rectangle is empty
        self.casts = []           # whole-plane castToFloat calls to make before the launch: ("c" | "f" | "r", plane, depth), in order
        self.chans = []           # per canvas channel: (frame_plane, mode, flags, frame_alpha, ref_alpha) of jxl_canvas_blend_chan
        self.source = None        # the reference slot the blend functions read, or None: every channel is a copy
        self.aliased = False      # that slot IS the canvas
        self.ref_zero = False     # that slot is empty: the functions read fresh zero planes (ref_types tells their types)
        self.canvas_types = self.frame_types = self.ref_types = None  # after the call (ref_types: None without a source)


def blend_type_plan(info, fr, canvas_types, frame_types, ref_types):
    """JXLCodestreamDecoder.blendFrame + blendBuffers (:415-537) replayed on the plane TYPES alone, channel by channel in canvas
    order: the casts of :433-436 and :446-465 become whole-plane casts in front of ONE launch, the rest the per-channel
    descriptor of jxl_canvas_blend. canvas_types / frame_types: one numpy dtype per plane. ref_types: per reference slot
    None (empty), the string "canvas" (the slot is the canvas object itself) or a list of dtypes (None: an absent plane).
    The verdict is "land: <reason>" where one launch behind hoisted casts would not give the reference's samples:
      - more than 16 planes; one-colour images; a frame whose colour count is not the image's;
      - channels that blend from different reference slots (the descriptor names one reference set), a slot with another
        plane count or an absent plane;
      - blendMulAdd's copy of the alpha channel (:390) out of a reference that is the canvas, at another offset;
      - a plane that one channel's function reads or writes as int32 and a LATER channel of the same call casts to float (the
        hoisted cast would turn the earlier int sum into a float sum).
    Raises nothing and touches no sample."""
    f32, i32 = np.dtype(np.float32), np.dtype(np.int32)
    plan = BlendPlan()

    def land(reason):
        plan.verdict = "land: " + reason
        return plan

    colors = 1 if info.colour_space == CE_GRAY else 3
    n = len(canvas_types)
    if n > abi.CANVAS_MAX_PLANES or len(frame_types) > abi.CANVAS_MAX_PLANES:
        return land("more than 16 planes")
    if colors != 3:
        return land("one-colour image")
    frame_colors = len(frame_types) - info.num_extra
    if frame_colors != colors or n != colors + info.num_extra:
        return land("the frame's colour count is not the image's")
    ih, iw = info.height, info.width
    py, px = min(max(fr.y0, 0), ih), min(max(fr.x0, 0), iw)       # Point.inBounds
    fy, fx = py - fr.y0, px - fr.x0
    ly, lx = fr.y0 + fr.height * fr.upsampling, fr.x0 + fr.width * fr.upsampling  # bounds after Frame.upsample()
    bh, bw = min(ly, ih) - py, min(lx, iw) - px
    ct, ft = [np.dtype(t) for t in canvas_types], [np.dtype(t) for t in frame_types]
    plan.canvas_types, plan.frame_types = ct, ft
    if bh <= 0 or bw <= 0:
        return plan
    plan.rect = (bh, bw, py, px, fy, fx, py, px)
    has_extra = info.num_extra > 0
    infos = []
    for c in range(n):
        if c >= colors:
            e = c - colors
            infos.append((fr.ec_blend_mode[e], fr.ec_blend_alpha[e], bool(fr.ec_blend_clamp[e]), fr.ec_blend_source[e]))
        else:
            infos.append((fr.blend_mode, fr.blend_alpha, bool(fr.blend_clamp), fr.blend_source))
    is_copy = [m == abi.BLEND_REPLACE or (ref_types[src] is None and m == abi.BLEND_ADD) for m, _, _, src in infos]  # :437
    sources = sorted({src for (m, _, _, src), cp in zip(infos, is_copy) if not cp})
    if len(sources) > 1:
        return land("channels blend from different reference slots")
    rt = None
    if sources:
        plan.source = sources[0]
        ref = ref_types[plan.source]
        if ref is None:
            plan.ref_zero, rt = True, [None] * n
        elif isinstance(ref, str):
            plan.aliased, rt = True, ct  # one object: a cast of either is a cast of both
        else:
            if len(ref) != n:
                return land("the reference slot has another plane count")
            rt = [None if t is None else np.dtype(t) for t in ref]
    plan.ref_types = rt
    int_used = set()  # (set, plane) an earlier channel of this call has read or written as int32

    def key(which):
        return "c" if which == "r" and plan.aliased else which

    def cast(which, plane, depth):
        types = {"c": ct, "f": ft, "r": rt}[which]
        if types[plane] == f32:
            return True
        if (key(which), plane) in int_used:
            return False
        types[plane] = f32
        if not (which == "r" and plan.ref_zero):  # (fresh zero planes are made with the type they end with)
            plan.casts.append((key(which), plane, depth))
        return True

    hazard = "a plane is read as int32 by one channel and cast to float by a later one"
    for idx, ((mode, alpha, clamp, _), cp) in enumerate(zip(infos, is_copy)):
        ex = idx - colors
        is_alpha = ex >= 0 and info.ec_type[ex] == 0
        premult = has_extra and bool(info.ec_alpha_associated[alpha])
        depth = info.bits_per_sample if idx < colors else info.ec_bits[ex]
        flags = (abi.BLEND_FLAG_IS_ALPHA if is_alpha else 0) | (abi.BLEND_FLAG_HAS_EXTRA if has_extra else 0) | \
            (abi.BLEND_FLAG_CLAMP if clamp else 0) | (abi.BLEND_FLAG_PREMULT if premult else 0)
        a_ref, a_frame = (colors + alpha, frame_colors + alpha) if has_extra else (0, 0)
        if ct[idx] != ft[idx]:  # :433-436
            if not (cast("f", idx, depth) and cast("c", idx, depth)):
                return land(hazard)
        if cp:
            if ft[idx] == i32:
                int_used.update({("f", idx), ("c", idx)})
            plan.chans.append((idx, abi.BLEND_REPLACE, flags, a_frame, a_ref))
            continue
        if rt[idx] is None:  # :441-442
            if not plan.ref_zero:
                return land("the reference slot lacks a plane")
            rt[idx] = ct[idx]
        if has_extra and mode in (abi.BLEND_BLEND, abi.BLEND_MULADD):  # :446-456
            a_depth = info.ec_bits[alpha]
            if mode == abi.BLEND_BLEND:
                if rt[a_ref] is None:
                    if not plan.ref_zero:
                        return land("the reference slot lacks a plane")
                    rt[a_ref] = f32
                if not cast("r", a_ref, a_depth):
                    return land(hazard)
            if not cast("f", a_frame, a_depth):
                return land(hazard)
        should_cast = mode == abi.BLEND_MULT or (mode == abi.BLEND_BLEND and has_extra) or \
            (mode == abi.BLEND_MULADD and has_extra and not is_alpha)
        if should_cast or rt[idx] != ft[idx]:  # :457-465
            if not (cast("f", idx, depth) and cast("c", idx, depth) and cast("r", idx, depth)):
                return land(hazard)
        if plan.aliased and mode == abi.BLEND_MULADD and has_extra and is_alpha and (fy, fx) != (py, px):
            # :390 copies ref at frameOffset: rows of the canvas onto other rows of itself, which no lane-owns-its-pixel launch replays
            return land("the alpha channel is copied from another place of the canvas itself")
        if ct[idx] != ft[idx] or rt[idx] != ft[idx]:
            # (an alpha channel that names itself: :455 casts the frame plane behind the comparison of :433 -- the reference's
            # copy then throws; the calls without the switch keep their own answer)
            return land("the planes of a channel differ in type")
        if ft[idx] == i32:  # the copy of :390 or the int sum of :287-301 (a float function on int planes cannot be reached)
            int_used.update({("f", idx), ("c", idx), (key("r"), idx)})
        plan.chans.append((idx, mode, flags, a_frame, a_ref))
    if plan.ref_zero:
        plan.ref_types = [f32 if t is None else t for t in rt]
    return plan


class ToneMap:
    """HDR -> SDR on the device (csrc/tone_map_ops.h has the operator): the BT.2408 luminance curve from the content's
    peak to a display of targetNits, then -- gamut -- the least desaturation that brings a pixel into [0, 1].
    sourceNits: the content's mastering peak (default: the image's intensity target). unitNits: the nits of a linear 1.0 (default:
    the intensity target for an XYB-encoded image; else 10000 for an image tagged PQ, else the intensity target)."""

    def __init__(self, targetNits=203.0, sourceNits=None, unitNits=None, gamut=True):
        for name, v in (("targetNits", targetNits), ("sourceNits", sourceNits), ("unitNits", unitNits)):
            if v is None and name != "targetNits":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
                raise ValueError("ToneMap: %s is a finite, positive number of nits" % name)
        if sourceNits is not None and sourceNits > 10000:
            raise ValueError("ToneMap: sourceNits is at most 10000")
        self.targetNits = float(targetNits)
        self.sourceNits = None if sourceNits is None else float(sourceNits)
        self.unitNits = None if unitNits is None else float(unitNits)
        self.gamut = bool(gamut)

    def resolve(self, image):
        """(unitNits, sourceNits, targetNits, gamut) for `image`: the defaults filled in from its header"""
        target = float(image.info.intensity_target)
        source = target if self.sourceNits is None else self.sourceNits
        if self.unitNits is not None:
            unit = self.unitNits
        else:
            unit = target if image.info.xyb_encoded else 10000.0 if image.taggedTransfer == TF_PQ else target
        return (unit, source, self.targetNits, self.gamut)

    def __repr__(self):
        return "ToneMap(targetNits=%r, sourceNits=%r, unitNits=%r, gamut=%r)" % (self.targetNits, self.sourceNits, self.unitNits, self.gamut)


def _tone_map_check(toneMap, backend, transfer=None):
    """what every toneMap= entry refuses before any call"""
    if not isinstance(toneMap, ToneMap):
        raise ValueError("toneMap: a ToneMap")
    if not hasattr(backend, "set_tone_map"):
        raise ValueError("toneMap needs the device path")
    if transfer == TF_PQ:
        raise ValueError("toneMap: the output is SDR; a linear, sRGB, BT.709 or gamma target")


class _ToneMapArmed:
    """the backend's colour passes tone-map while this is open: armed on entry, always cleared on exit"""

    def __init__(self, backend, primaries, whitePoint, resolved):
        self.backend = backend
        unit, source, target, gamut = resolved
        self.args = ([float(v) for v in _primaries_to_xyz(primaries, whitePoint)[1]], unit, source, target, gamut)

    def __enter__(self):
        self.backend.set_tone_map(*self.args)
        return self

    def __exit__(self, *exc):
        self.backend.set_tone_map(None)
        return False


class DeviceBackend:
    """the product backend: HIP kernels through the C-ABI (jxlatte_amd._lib / host). No CPU fallback."""

    def __init__(self, device=0):
        from . import _lib, host
        self.host = host
        self.ctx = _lib.Context(device)
        self.palette_log = []

    def close(self):
        self.ctx.close()

    resident = True  # vardct(keep=(h, w)) / keep_planes(planes) hand back host.ResidentPlanes

    def keep_planes(self, planes):
        return self.host.ResidentPlanes.upload(self.ctx, planes)

    def vardct(self, params, weights, woffs, lfgroups, groups, keep=None, sparse=False):
        """sparse: `groups` yields the entry lists of Frontend.coeffs_sparse, fed through jxl_vardct_put_group_sparse.
        keep: (h, w), or (y, x, h, w) for a window that does not begin at the origin (jxl_planes_from_frame_at)"""
        fr = feed_frame(self.host.Frame(self.ctx, params, weights, woffs), lfgroups, groups, sparse)
        if keep is not None:  # the planes stay on the device for the stages after decodeFrame: host.ResidentPlanes
            return fr.keepPlanes(*keep)
        return fr.decodeFrame()

    def lf_image(self, groups, cells, bcx, bcb, color_factor, xyb, keep=False):
        """a frame's LF image as the picture at 1:8 in one launch (host.lfImage): jxl_planes_from_lf where the planes stay (keep:
        host.ResidentPlanes come back), jxl_stage_lf_image otherwise"""
        return self.host.lfImage(self.ctx, groups, cells, bcx, bcb, color_factor, xyb, keep=keep)

    def gab(self, planes, w1, w2):
        return self.host.performGabConvolution(self.ctx, planes, w1, w2)

    def epf(self, planes, iters, inv_sigma, sigma_modular, rf):
        return self.host.performEdgePreservingFilter(self.ctx, planes, iters, inv_sigma, invModularSigma=sigma_modular,
                                                     epfChannelScale=rf["channel_scale"], epfPass0SigmaScale=rf["pass0"],
                                                     epfPass2SigmaScale=rf["pass2"], epfBorderSadMul=rf["border_sad_mul"])

    def xyb(self, planes, matrix, opsin_bias, cbrt_bias, intensity_target):
        return self.host.OpsinInverseMatrix(matrix, opsin_bias, cbrt_bias).invertXYB(self.ctx, planes, intensity_target)

    def ycbcr(self, planes):
        return self.host.performColorTransformsYCbCr(self.ctx, planes)

    def squeeze(self, ins, steps, shapes):
        ms = self.host.ModularStream(self.ctx, ins, steps)
        out = ms.applyTransforms()
        assert [o.shape for o in out] == list(shapes)
        return out

    def rct(self, a, b, c, rct_type):
        return self.host.rct(self.ctx, np.stack([a, b, c]), rct_type)

    def palette(self, index, palette, pred, num_c, nb_colors, nb_deltas, d_pred, bit_depth):
        """one frame-level Palette transform (jxl_stage_palette); what it took is appended to self.palette_log"""
        out = self.host.inversePalette(self.ctx, index, palette, num_c, nb_colors, nb_deltas, d_pred, bit_depth, pred=pred)
        launches, deltas = self.host.lastPalette(self.ctx)
        self.__dict__.setdefault("palette_log", []).append(dict(num_c=int(num_c), nb_colors=int(nb_colors), delta_pixels=deltas, launches=launches))
        return out

    def modular_to_float(self, a, b, scale):
        return self.host.modularToFloat(self.ctx, a, b, scale)

    def chroma_upsample(self, plane, xs, ys):
        return self.host.invertSubsampling(self.ctx, plane, xs, ys)

    def upsample(self, plane, k, weights):
        return self.host.performUpsampling(self.ctx, plane, k, weights)

    def splines(self, planes, splines, bcx, bcb):
        return self.host.renderSplines(self.ctx, planes, splines, bcx, bcb)

    def patches(self, frame, ref, pos, blend, n_color, ec_is_alpha, ec_alpha_associated):
        return self.host.computePatches(self.ctx, frame, ref, pos, blend, n_color, ec_is_alpha, ec_alpha_associated)

    def noise_init(self, h, w, seed0, group_dim, colors):
        return self.host.initializeNoise(self.ctx, h, w, seed0, group_dim, colors)

    def noise_add(self, planes, noise, lut, bcx, bcb):
        return self.host.synthesizeNoise(self.ctx, planes, noise, lut, bcx, bcb)

    def noise_window(self, planes, group_dim, seed0, lut, bcx, bcb, frame_h, frame_w, y0, x0):
        """initializeNoise + synthesizeNoise of a frame_h x frame_w frame on `planes`, its window at (y0, x0) (host.noiseWindow)"""
        return self.host.noiseWindow(self.ctx, planes, group_dim, seed0, lut, bcx, bcb, frame_h, frame_w, y0, x0)

    def blend(self, mode, canvas, frame, ref, rect, **kw):
        return self.host.blend(self.ctx, mode, canvas, frame, ref, rect, **kw)

    def orient(self, plane, orientation):
        return self.host.transposeBuffer(self.ctx, plane, orientation)

    def transfer(self, plane, tf):
        code = {TF_PQ: abi.TRANSFER_PQ, TF_SRGB: abi.TRANSFER_SRGB}[tf]
        return self.host.transfer(self.ctx, plane, code, 0)

    def color_convert(self, planes, **params):
        """JXLImage.transform's sample chain as one pass (host.colorConvert; the keywords are host.colorParams')"""
        return self.host.colorConvert(self.ctx, planes, **params)

    def color_peak(self, planes, **params):
        return self.host.determinePeak(self.ctx, planes, **params)

    def set_tone_map(self, lum, unitNits=None, sourceNits=None, targetNits=None, gamut=True):
        """arm the HDR -> SDR stage of this backend's colour passes (host.setToneMap), or clear it (lum None)"""
        self.host.setToneMap(self.ctx, None if lum is None else self.host.toneMapParams(lum, unitNits, sourceNits, targetNits, gamut))

    def png_samples(self, planes, alpha, **params):
        """PNGWriter's samples in one pass (host.pngSamples; the keywords are host.pngParams')"""
        return self.host.pngSamples(self.ctx, planes, alpha, **params)

    def tensor_samples(self, planes, alpha, out_ptr, **params):
        """the image as a device tensor in one pass (host.tensorSamples; the keywords are host.tensorParams')"""
        return self.host.tensorSamples(self.ctx, planes, alpha, out_ptr, **params)

    def tensor_resized(self, planes, alpha, out_ptr, size, box, resample, **params):
        """the image resampled to a device tensor in one pass (host.tensorResized)"""
        return self.host.tensorResized(self.ctx, planes, alpha, out_ptr, size, box, resample, **params)

    def tensor_resized_batch(self, items, out_ptr):
        """N images resampled into one batch tensor in one launch (host.tensorResizedBatch). items: per image the keywords of
        host.tensorBatchItem; out_ptr: the DEVICE address of the batch"""
        return self.host.tensorResizedBatch(self.ctx, [self.host.tensorBatchItem(**it) for it in items], out_ptr)

    def tensor_device(self):
        """the torch device of the memory tensor_samples writes"""
        return "cuda:%d" % self.ctx.device

    def varblocks(self, planes, blocks, cells):
        """Frame.drawVarblocks in one pass (host.varblocks)"""
        return self.host.varblocks(self.ctx, planes, blocks, cells)

    def pfm_samples(self, planes, tagged):
        """PFMWriter's samples in one pass (host.pfmSamples)"""
        return self.host.pfmSamples(self.ctx, planes, tagged)

    def pack(self, planes, bit_depth, alpha, premultiplied, tagged, big_endian):
        return self.host.packSamples(self.ctx, planes, bit_depth, alpha=alpha, premultiplied=premultiplied, taggedDepth=tagged,
                                     bigEndian=big_endian)


# ---- JXLImage (J/JXLImage.java) ---------------------------------------------------------------------------------
class JXLImage:
    def __init__(self, buffer, info, backend, resident=None, planeSet=None):
        """planeSet: a device plane set (host.DeviceCanvas) holding EVERY plane of the image, colours and extra channels, each of
        its own type; `buffer` is then a list of None: JXLDecoder(device_image=True). The set is the image's own (sets do not
        share the resident planes' single-owner rule): `buffer` / getBuffer() download the typed planes on first use and keep
        the host arrays, the writers read the set; close() or deletion releases it.
        resident: the backend's resident planes (host.ResidentPlanes) holding the three colour planes, whose places in
        `buffer` are None: JXLDecoder(device_output=True). They are the image's until the backend decodes another frame;
        `buffer` / getBuffer() download them on first use and keep the host arrays; once another frame has taken the planes,
        a first use raises IllegalStateException instead (ResidentPlanes.live)."""
        self.info = info
        self.backend = backend
        self.resident = resident
        self.planeSet = planeSet
        self.buffer = buffer  # list of 2-D arrays (int32 or float32), colour channels first
        self.height, self.width = planeSet.shape if planeSet is not None else buffer[0].shape if resident is None else resident.shape
        self.colorEncoding = info.colour_space
        alphas = [i for i in range(info.num_extra) if info.ec_type[i] == 0]
        self.alphaIndex = alphas[0] if alphas else -1
        self.primariesXY = np.array(info.prim_xy, F)
        self.whiteXY = np.array(info.white_xy, F)
        self.taggedTransfer = info.transfer
        self.transfer_ = TF_LINEAR if info.xyb_encoded else info.transfer
        self.alphaIsPremultiplied = self.alphaIndex >= 0 and bool(info.ec_alpha_associated[self.alphaIndex])
        colors = self.getColorChannelCount()
        self.bitDepths = [info.bits_per_sample if c < colors else info.ec_bits[c - colors] for c in range(len(buffer))]
        self.has_icc = bool(info.use_icc) and not info.xyb_encoded

    resident = None
    planeSet = None
    region = None  # JXLDecoder(region=): the box of the whole image that this image is

    def setLive(self):
        """the image's planes are in a device plane set that has not been released"""
        return self.planeSet is not None and self.planeSet.id is not None

    def close(self):
        """release the image's plane set (the host arrays, once downloaded, stay)"""
        ps, self.planeSet = self.planeSet, None
        if ps is not None:
            ps.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def buffer(self):
        if self.planeSet is not None and self._buffer and self._buffer[0] is None:
            for c in range(len(self._buffer)):  # the typed planes: bit for bit the default decoder's arrays
                self._buffer[c] = self.planeSet.download(c)
        if self.resident is not None and self._buffer[0] is None:
            self.resident._need_live()  # (a later frame of the backend has taken the planes: an error, not its pixels)
            planes = self.resident.download()
            for c in range(3):
                self._buffer[c] = planes[c]
        return self._buffer

    @buffer.setter
    def buffer(self, planes):
        self._buffer = planes

    def onDevice(self):
        """the colour planes are the backend's resident planes (and nothing has replaced them on this image)"""
        return self.resident is not None or self.planeSet is not None

    # -- where the samples are, for the writers' one-pass kernels: the three operations below and nobody else ask ---------
    def _home(self, colors, one_type=False):
        """"set": the live plane set comes first; else "resident": the resident planes, if the host arrays were never
        downloaded (planes a later decode took then raise IllegalStateException) or the planes are still live; else "host".
        one_type: a set whose colour planes differ in type is passed over (jxl_color_params states one type for a pass)"""
        if self.setLive() and not (one_type and len({self.planeSet.types[c] for c in range(colors)}) != 1):
            return "set"
        if self.resident is not None and (self._buffer[0] is None or self.resident.live()):
            return "resident"
        return "host"

    def _plan_planes(self, colors):
        """_color_plan's `planes` for a writer: stand-ins (shape and dtype, never read) while the samples are on the device,
        None for the host arrays"""
        home = self._home(colors, True)
        if home == "set":
            return self.planeSet._stand_ins(colors)
        return [np.broadcast_to(F(0), (self.height, self.width))] * 3 if home == "resident" else None

    def _peak(self, planes, **front):
        """determinePeak of the front stages, where the colour planes are: (peak, bytes sent up)"""
        home = self._home(len(planes), True)
        if home == "set":
            return self.planeSet.colorPeak(nColor=len(planes), **front), 0
        if home == "resident":
            return self.resident.colorPeak(**front), 0
        up = sum(a.nbytes for a in planes) if front.get("matrix") is not None else planes[min(1, len(planes) - 1)].nbytes
        return self.backend.color_peak(planes, **front), up

    def _png_samples(self, planes, **kw):
        """PNGWriter's samples in one pass (pngParams' keywords): (samples, bytes sent up). A set is read where it is, alpha
        included; beside the resident planes only the alpha plane goes up; the host arrays `planes` go up whole"""
        colors, a = len(planes), self.alphaIndex
        home = self._home(colors, True)
        if home == "set":
            return self.planeSet.pngSamples(nColor=colors, alphaPlane=colors + a if a >= 0 else None, **kw), 0
        alpha = np.ascontiguousarray(self.extraChannel(a)) if a >= 0 else None
        up = alpha.nbytes if alpha is not None else 0
        if home == "resident":
            return self.resident.pngSamples(alpha, **kw), up
        planes = [np.ascontiguousarray(p) for p in planes]
        return self.backend.png_samples(planes, alpha, **kw), up + sum(p.nbytes for p in planes)

    def _tensor_samples(self, planes, out_ptr, resize=None, **kw):
        """the image as a device tensor in one pass (tensorParams' keywords), written to the device address out_ptr: the bytes
        sent up, by _png_samples' rule. Nothing comes down from any home. resize: None, or (size, box, resample) -- the
        resampled pass (tensorResized) from the same home"""
        colors, a = len(planes), self.alphaIndex
        home = self._home(colors, True)
        if home == "set":
            ap = colors + a if a >= 0 else None
            if resize is None:
                self.planeSet.tensorSamples(out_ptr, nColor=colors, alphaPlane=ap, **kw)
            else:
                self.planeSet.tensorResized(out_ptr, *resize, nColor=colors, alphaPlane=ap, **kw)
            return 0
        alpha = np.ascontiguousarray(self.extraChannel(a)) if a >= 0 else None
        up = alpha.nbytes if alpha is not None and (kw.get("writeAlpha") or kw.get("premultiplied")) else 0
        if home == "resident":
            if resize is None:
                self.resident.tensorSamples(out_ptr, alpha, **kw)
            else:
                self.resident.tensorResized(out_ptr, *resize, alpha=alpha, **kw)
            return up
        planes = [np.ascontiguousarray(p) for p in planes]
        if resize is None:
            self.backend.tensor_samples(planes, alpha, out_ptr, **kw)
        else:
            self.backend.tensor_resized(planes, alpha, out_ptr, *resize, **kw)
        return up + sum(p.nbytes for p in planes)

    _TENSOR_TARGETS = ("srgb", "pq", "linear", "as-is")

    def toTensor(self, dtype=None, layout="CHW", target="srgb", peakDetect=PEAK_DETECT_AUTO, alpha="drop", mean=None, std=None, out=None,
                 size=None, box=None, resample="triangle", toneMap=None):
        """The image as a torch tensor on the backend's device, (C, H, W) or (H, W, C), in ONE device pass from wherever its planes
        are -- no sample crosses the bus downwards.
        dtype: torch.uint8, float16, bfloat16 or float32 (the default). target: "srgb" (PNGWriter's non-HDR target: sRGB
        primaries, D65, the sRGB curve), "pq" (its HDR target: BT.2100 primaries, PQ), "linear" (sRGB primaries, D65, linear) or
        "as-is" (no colour stage; integer planes cast with their depth); an image with an ICC profile is taken as it is whatever
        is asked, as PNGWriter takes it. A grey image that has to be tone-mapped yields three channels: the shape tells.
        alpha: "drop" or "append" (the last channel); a premultiplied image's colours are divided either way.
        mean / std: per output channel, float dtypes only: (v - mean) * (float32(1) / float32(std)).
        out: a contiguous tensor of the result's shape and dtype on that device -- batch[i] of a batch of equal-sized images is
        one -- filled in place and returned; the current torch stream is synchronised first. tensor_bus_bytes = (bytes up, 0).
        size = (h, w): the tensor's size; the image (or `box`) is resampled to it in the same pass -- behind the colour stages'
        linear intermediate where the plan has one, before the output curve -- with resample "triangle" (bilinear with the
        support scaled to the ratio: antialiased) or "box". box = (x0, y0, w, h) in whole source pixels: alone it is a crop
        (an identity-ratio resample: an exact copy). With both left out the pass and its bytes are the unresized ones; images
        of any size then fill one batch through out=batch[i]. Peak detection stays the whole image's.
        toneMap: a ToneMap -- HDR to SDR per source pixel behind the primaries matrix, in place of peak detection (which is not
        consulted); a resample then filters tone-mapped linear light. Three colour channels, of a grey image too. Targets "srgb"
        and "linear"; ValueError for "pq", "as-is" and an image with an ICC profile."""
        import torch
        be = self.backend
        if toneMap is not None:
            _tone_map_check(toneMap, be)
            if target in ("pq", "as-is") or self.has_icc:
                raise ValueError("toneMap: the output is SDR in known primaries; target srgb or linear, and no ICC profile")
        if not hasattr(be, "tensor_samples"):
            raise TypeError("toTensor needs a backend with tensor_samples")
        if (size is not None or box is not None) and not hasattr(be, "tensor_resized"):
            raise TypeError("toTensor(size=, box=) needs a backend with tensor_resized")
        resize, dtype, name, channels, mean, inv_std = self._tensor_request(torch, dtype, layout, target, alpha, mean, std, size, box, resample,
                                                                             toneMap is not None)
        oh, ow = (self.height, self.width) if resize is None else resize[0]
        shape = (channels, oh, ow) if layout == "CHW" else (oh, ow, channels)
        device = torch.device(be.tensor_device())
        if out is not None:
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
                raise ValueError("out: a contiguous %s tensor of shape %s on %s" % (name, shape, device))
        planes, kw, up = self._tensor_plan(target, peakDetect, alpha, name, layout, mean, inv_std, toneMap)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=device)
        elif device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()  # what the caller queued on its tensor is done before the library writes
        if toneMap is None:
            sent = self._tensor_samples(planes, out.data_ptr(), resize=resize, **kw)
        else:
            with _ToneMapArmed(be, self._tensor_target(target)[0], WP_D65, toneMap.resolve(self)):
                sent = self._tensor_samples(planes, out.data_ptr(), resize=resize, **kw)
        self.tensor_bus_bytes = (up + sent, 0)
        return out

    def _tensor_request(self, torch, dtype, layout, target, alpha, mean, std, size, box, resample, toneMapped=False):
        """toTensor's arguments checked against the image, before any call: (resize, dtype, its name, channels, mean, inv_std);
        resize: None, or (size, box, resample)"""
        resize = None
        if size is not None or box is not None:
            if resample not in ("triangle", "box"):
                raise ValueError("resample: triangle or box")
            try:
                bx = (0, 0, self.width, self.height) if box is None else tuple(int(v) for v in box)
                sz = (bx[3], bx[2]) if size is None else tuple(int(v) for v in size)
            except (TypeError, ValueError, IndexError):
                raise ValueError("size: (height, width); box: (x0, y0, width, height)")
            if len(bx) != 4 or len(sz) != 2 or (box is not None and bx != tuple(box)) or (size is not None and sz != tuple(size)):
                raise ValueError("size: (height, width); box: (x0, y0, width, height), whole numbers")
            if bx[0] < 0 or bx[1] < 0 or bx[2] <= 0 or bx[3] <= 0 or bx[0] + bx[2] > self.width or bx[1] + bx[3] > self.height:
                raise ValueError("box: (x0, y0, width, height) inside the %d x %d image" % (self.width, self.height))
            if sz[0] <= 0 or sz[1] <= 0:
                raise ValueError("size: (height, width), both positive")
            resize = (sz, bx, resample)
        elif resample not in ("triangle", "box"):
            raise ValueError("resample: triangle or box")
        if dtype is None:
            dtype = torch.float32
        names = {torch.uint8: "uint8", torch.float16: "float16", torch.bfloat16: "bfloat16", torch.float32: "float32"}
        if dtype not in names:
            raise ValueError("dtype: torch.uint8, float16, bfloat16 or float32")
        if layout not in ("CHW", "HWC"):
            raise ValueError("layout: CHW or HWC")
        if target not in self._TENSOR_TARGETS:
            raise ValueError("target: one of %s" % (self._TENSOR_TARGETS,))
        if alpha not in ("drop", "append"):
            raise ValueError("alpha: drop or append")
        if alpha == "append" and self.alphaIndex < 0:
            raise ValueError("the image has no alpha channel to append")
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        if mean is not None and dtype == torch.uint8:
            raise ValueError("normalisation is for the float dtypes")
        colors = self.getColorChannelCount()
        primaries, _, as_is = self._tensor_target(target)
        tone_map = not as_is and not (_prim_matches(primaries, self.primariesXY) and _xy_matches(WP_D65, self.whiteXY))
        channels = (3 if (colors == 3 or tone_map or toneMapped) else 1) + (alpha == "append")
        inv_std = None
        if mean is not None:
            mean, std = [float(v) for v in mean], [float(v) for v in std]
            if len(mean) != channels or len(std) != channels:
                raise ValueError("mean and std have one entry per output channel (%d)" % channels)
            with np.errstate(all="ignore"):
                inv_std = [F(1) / F(s) for s in std]
            if not all(np.isfinite(v) for v in inv_std):
                raise ValueError("std: 1 / std is not finite")
        return resize, dtype, names[dtype], channels, mean, inv_std

    def _tensor_target(self, target):
        """(primaries, transfer, as_is) of a toTensor target"""
        as_is = target == "as-is" or self.has_icc
        primaries, tf = {"srgb": (PRI_SRGB, TF_SRGB), "pq": (PRI_BT2100, TF_PQ), "linear": (PRI_SRGB, TF_LINEAR)}.get(target, (None, None))
        return primaries, tf, as_is

    def _tensor_plan(self, target, peakDetect, alpha, dtype_name, layout, mean, inv_std, toneMap=None):
        """the colour plan of a checked toTensor request, with at most one _peak call: (planes, _tensor_samples' keywords, bytes
        the peak sent up)"""
        colors = self.getColorChannelCount()
        primaries, tf, as_is = self._tensor_target(target)
        up = 0
        planes = self._plan_planes(colors)  # (stand-ins while the samples are on the device)

        def peak_of(pl, **front):
            nonlocal up
            peak, sent = self._peak(pl, **front)
            up += sent
            return peak
        plan = None if as_is else self._color_plan(primaries, WP_D65, tf, peakDetect, peak_of, planes=planes, toneMap=toneMap)
        if plan is not None:
            planes, params = plan[0], plan[1]
        else:  # the image as it is: every colour stage off; integer planes are cast with their depth's maximum
            if planes is None:
                planes = [self.buffer[c] for c in range(colors)]
                if len({a.dtype for a in planes}) != 1:
                    planes = [self._as_float(c) for c in range(colors)]
            params = dict(inMax=[(1 << self.bitDepths[c]) - 1 for c in range(colors)])
        has_alpha = self.alphaIndex >= 0
        kw = dict(premultiplied=self.isAlphaPremultiplied() and has_alpha, writeAlpha=alpha == "append", dtype=dtype_name, layout=layout,
                  alphaDepth=self.getTaggedBitDepth(colors + self.alphaIndex) if has_alpha else None, colorDepth=self.getTaggedBitDepth(0),
                  mean=mean, invStd=inv_std, **params)
        return planes, kw, up

    def _tensor_batch_item(self, planes, resize, **kw):
        """this image as one item of Backend.tensor_resized_batch, from the home _tensor_samples would read: (item, bytes that
        go up). item: the keywords of host.tensorBatchItem"""
        colors, a = len(planes), self.alphaIndex
        size, box, resample = resize
        home = self._home(colors, True)
        if home == "set":
            return dict(size=size, box=box, resample=resample, canvas=self.planeSet, nColor=colors, alphaPlane=colors + a if a >= 0 else None, **kw), 0
        alpha = np.ascontiguousarray(self.extraChannel(a)) if a >= 0 else None
        up = alpha.nbytes if alpha is not None and (kw.get("writeAlpha") or kw.get("premultiplied")) else 0
        if home == "resident":
            return dict(size=size, box=box, resample=resample, resident=self.resident, alpha=alpha, **kw), up
        planes = [np.ascontiguousarray(p) for p in planes]
        return dict(size=size, box=box, resample=resample, planes=planes, alpha=alpha, **kw), up + sum(p.nbytes for p in planes)

    def _pfm_samples(self, tagged):
        """PFMWriter's samples in one pass: (samples, bytes sent up). A set's planes, int32 or float, as they are"""
        colors = len(tagged)
        home = self._home(colors)
        if home == "set":
            return self.planeSet.pfmSamples(nColor=colors, taggedDepths=tagged), 0
        if home == "resident":
            return self.resident.pfmSamples(), 0
        planes = [np.ascontiguousarray(a) for a in self.getBuffer(False)[:colors]]
        return self.backend.pfm_samples(planes, tagged), sum(a.nbytes for a in planes)

    def _clone(self, buffer=None):
        im = JXLImage.__new__(JXLImage)
        im.__dict__.update(self.__dict__)
        im.buffer = list(self.buffer if buffer is None else buffer)
        im.bitDepths = list(self.bitDepths)
        im.resident = None  # a clone lives on the host
        im.planeSet = None
        return im

    def getWidth(self):
        return self.width

    def getHeight(self):
        return self.height

    def getColorChannelCount(self):
        return 1 if self.colorEncoding == CE_GRAY else 3

    def getAlphaIndex(self):
        return self.alphaIndex

    def hasAlpha(self):
        return self.alphaIndex >= 0

    def isAlphaPremultiplied(self):
        return self.alphaIsPremultiplied

    def getTaggedBitDepth(self, c):
        return self.bitDepths[c]

    def extraChannel(self, i):
        """extra channel i (a host array), without touching the colour planes"""
        return (self.buffer if self.planeSet is not None else self._buffer)[self.getColorChannelCount() + i]

    def getBuffer(self, copy=True):
        return [b.copy() for b in self.buffer] if copy else self.buffer

    def isHDR(self):
        if self.taggedTransfer in (TF_PQ, TF_HLG, TF_LINEAR):
            return True
        prim = np.array(self.info.prim_xy, F)
        return not _prim_matches(prim, PRI_SRGB) and not _prim_matches(prim, PRI_P3)

    def _as_float(self, c, with_depth=True):
        b = self.buffer[c]
        if b.dtype == np.float32:
            return b
        mx = ((1 << self.bitDepths[c]) - 1) if with_depth else self.bitDepths[c]
        return (b.astype(F) * F(F(1) / F(mx))).astype(F)  # ImageBuffer.castToFloat0

    def linearize(self):
        if self.transfer_ == TF_LINEAR:
            return self
        im = self._clone()
        for c in range(self.getColorChannelCount()):
            im.buffer[c] = _to_linear(self._as_float(c), self.transfer_)
        im.transfer_ = TF_LINEAR
        return im

    def _determine_peak(self):
        im = self.linearize()
        c = 0 if im.colorEncoding == CE_GRAY else 1
        # MathHelper.max(float...) returns the MINIMUM of each row (MathHelper.java:190-195); the
        # reference then takes the maximum over rows. Restated as is.
        b = im._as_float(c)
        if im.buffer[c].dtype == np.int32:
            return F(im.buffer[c].max(axis=1).max()) / F((1 << im.bitDepths[c]) - 1)
        return F(b.min(axis=1).max())

    def transfer(self, transfer, peakDetect):
        """JXLImage.transfer(int, int) (:263-286)"""
        if transfer == self.transfer_:
            return self
        im = self.linearize()
        if self.taggedTransfer == TF_PQ and peakDetect in (PEAK_DETECT_AUTO, PEAK_DETECT_ON):
            to_pq = transfer in (TF_PQ, TF_LINEAR)
            from_pq = self.transfer_ in (TF_PQ, TF_LINEAR)
            if from_pq and not to_pq:
                scale = F(F(1) / im._determine_peak())
                if scale > 1.0 or peakDetect == PEAK_DETECT_ON:
                    im = im._clone()
                    for c in range(im.getColorChannelCount()):
                        im.buffer[c] = (im._as_float(c) * scale).astype(F)
        if im is self:
            im = self._clone()
        for c in range(im.getColorChannelCount()):
            # transferInPlace casts int planes with the bit depth itself as max value (JXLImage.java:248); float planes
            # (every XYB image) are unaffected by that
            src = im._as_float(c, with_depth=False)
            if transfer in (TF_PQ, TF_SRGB):
                im.buffer[c] = self.backend.transfer(src, transfer)  # device: TransferFunction.fromLinearF
            elif transfer == TF_LINEAR:
                im.buffer[c] = src
            else:
                raise UnsupportedOperationException("output transfer function %d" % (transfer - (1 << 24)))
        im.transfer_ = transfer
        return im

    def fillColor(self):
        if self.colorEncoding != CE_GRAY:
            return self
        im = self._clone([self.buffer[0].copy(), self.buffer[0].copy()] + list(self.buffer))
        im.bitDepths = [self.bitDepths[0]] * 2 + list(self.bitDepths)
        im.colorEncoding = CE_RGB
        return im

    def toneMapLinear(self, primaries, whitePoint):
        if _prim_matches(self.primariesXY, primaries) and _xy_matches(self.whiteXY, whitePoint):
            return self
        m = get_conversion_matrix(primaries, whitePoint, self.primariesXY, self.whiteXY)
        src = [self._as_float(c) for c in range(3)]
        im = self._clone()
        for r in range(3):  # MathHelper.matrixMutliply3InPlace: (m0*a + m1*b) + m2*c
            im.buffer[r] = ((m[r, 0] * src[0] + m[r, 1] * src[1]).astype(F) + m[r, 2] * src[2]).astype(F)
        im.primariesXY, im.whiteXY = np.array(primaries, F), np.array(whitePoint, F)
        return im

    def _color_plan(self, primaries, whitePoint, transfer, peakDetect, peak_of, planes=None, toneMap=None):
        """the decisions of transform / linearize / fillColor / toneMapLinear / transfer (JXLImage.java:114-141, 185-193, 260-286)
        for a backend that does the sample work in one pass: None when the image is returned as it is, else (planes, params,
        tone_map), params being the keywords of host.colorParams for those planes. peak_of(planes, **front) is asked for
        determinePeak of the front stages, at most once, where transfer() would take it. planes: stand-ins for colour planes
        that are not on the host (their dtype is what is looked at). toneMap: a ToneMap is armed around the pass -- there is
        always a pass then, through linear light, and peak_of is not asked."""
        tone_map = not (_prim_matches(primaries, self.primariesXY) and _xy_matches(whitePoint, self.whiteXY))
        if not tone_map and transfer == self.transfer_ and toneMap is None:
            return None
        tf_in, gamma_in = _tf_selector(self.transfer_)
        tf_out, gamma_out = _tf_selector(transfer)
        colors = self.getColorChannelCount()
        depth_max = [(1 << self.bitDepths[c]) - 1 for c in range(colors)]
        if planes is None:
            planes = [self.buffer[c] for c in range(colors)]
        if len({p.dtype for p in planes}) != 1:  # mixed int / float colour planes: the first cast, done here
            cast_max = depth_max if (self.transfer_ != TF_LINEAR or tone_map) else None
            planes = [self._as_float(c) if cast_max else self._as_float(c, with_depth=False) for c in range(colors)]
        front = dict(tfIn=tf_in, gammaIn=gamma_in)
        if tone_map:
            front["matrix"] = get_conversion_matrix(primaries, whitePoint, self.primariesXY, self.whiteXY)
        if toneMap is not None:
            return planes, dict(inMax=depth_max, tfOut=tf_out, gammaOut=gamma_out, **front), tone_map
        if tone_map and transfer == TF_LINEAR:  # transfer() of the tone-mapped, linear image returns it as it is (:270-271)
            return planes, dict(inMax=depth_max, **front), tone_map
        scale = None
        if self.taggedTransfer == TF_PQ and peakDetect in (PEAK_DETECT_AUTO, PEAK_DETECT_ON):
            to_pq = transfer in (TF_PQ, TF_LINEAR)
            from_pq = tone_map or self.transfer_ in (TF_PQ, TF_LINEAR)  # the tone-mapped image is linear
            if from_pq and not to_pq:
                s = F(F(1) / peak_of(planes, inMax=depth_max, **front))
                if s > 1.0 or peakDetect == PEAK_DETECT_ON:
                    scale = s
        # the first stage that touches the samples casts them: linearize, toneMapLinear and the scale with the depth's
        # maximum, transferInPlace with the depth itself (:248)
        first_max = depth_max if (self.transfer_ != TF_LINEAR or tone_map or scale is not None) else [self.bitDepths[c] for c in range(colors)]
        return planes, dict(inMax=first_max, scale=scale, tfOut=tf_out, gammaOut=gamma_out, **front), tone_map

    def _transform_device(self, primaries, whitePoint, transfer, peakDetect, toneMap=None):
        """transform() with the samples on the device: the decisions are _color_plan's, the sample work is at most one
        color_peak and one color_convert call of the backend. Same metadata as the host path; float samples within the 1 ulp
        of the double-pow curves (include/jxlatte_amd.h)."""
        plan = self._color_plan(primaries, whitePoint, transfer, peakDetect, self.backend.color_peak, toneMap=toneMap)
        if plan is None:
            return self
        planes, params, tone_map = plan
        colors = self.getColorChannelCount()
        if toneMap is None:
            out = self.backend.color_convert(planes, **params)
        else:
            with _ToneMapArmed(self.backend, primaries, whitePoint, toneMap.resolve(self)):
                out = self.backend.color_convert(planes, **params)
        im = self._clone()
        if tone_map or toneMap is not None:  # three planes
            if colors == 1:  # fillColor
                im.buffer = list(out) + list(self.buffer[1:])
                im.bitDepths = [self.bitDepths[0]] * 2 + list(self.bitDepths)
                im.colorEncoding = CE_RGB
            else:
                im.buffer[:3] = out
            if tone_map:
                im.primariesXY, im.whiteXY = np.array(primaries, F), np.array(whitePoint, F)
        else:
            im.buffer[:colors] = out
        im.transfer_ = transfer
        return im

    def transform(self, primaries, whitePoint, transfer, peakDetect=PEAK_DETECT_AUTO, device=False, toneMap=None):
        """JXLImage.transform (:186-193). device: the whole chain as one pass of a backend that has color_convert -- which also
        serves the BT.709, DCI and gamma targets; else on the host, one plane and one stage at a time.
        toneMap: a ToneMap -- HDR to SDR in the same pass, behind the primaries matrix and in place of peak detection; the
        device path only, and not towards PQ. The result has three colour planes."""
        if toneMap is not None:
            if not device or not hasattr(self.backend, "color_convert"):
                raise ValueError("toneMap needs the device path")
            _tone_map_check(toneMap, self.backend, transfer)
            return self._transform_device(primaries, whitePoint, transfer, peakDetect, toneMap)
        if device and hasattr(self.backend, "color_convert"):
            return self._transform_device(primaries, whitePoint, transfer, peakDetect)
        if _prim_matches(primaries, self.primariesXY) and _xy_matches(whitePoint, self.whiteXY):
            return self.transfer(transfer, peakDetect)
        return self.linearize().fillColor().toneMapLinear(primaries, whitePoint).transfer(transfer, peakDetect)


def toTensorBatch(images, size, boxes=None, dtype=None, layout="CHW", target="srgb", peakDetect=PEAK_DETECT_AUTO, alpha="drop", mean=None,
                  std=None, out=None, resample="triangle", toneMap=None):
    """N decoded images as ONE torch tensor on their backend's device, (N, C, h, w) or (N, h, w, C), in ONE launch: image i is
    resampled to `size` = (h, w) exactly as images[i].toTensor(size=size, box=boxes[i], ...) resamples it -- bit for bit -- from
    wherever its planes are (a plane set, the resident planes, host arrays), each with the colour plan toTensor builds for it
    (at most one peak detection per image). boxes: None, or per image None or (x0, y0, w, h). The other arguments are
    toTensor's, one value for the batch. All images are on one backend and their plans give one channel count (a grey image
    does not join colour ones); ValueError before any call otherwise, and for everything toTensor raises.
    out: a contiguous tensor of the batch's shape and dtype on that device -- a slice batch[a:a + N] of a larger batch is one --
    filled in place and returned; the current torch stream is synchronised first. Each image's tensor_bus_bytes is set as
    toTensor sets it; the batch's total is the returned tensor's bus_bytes = (bytes up, 0).
    toneMap: toTensor's, one value for the batch: its per-image defaults must resolve to the same numbers for every image
    (ValueError naming two images that differ otherwise)."""
    import torch
    images = list(images)
    if not images:
        raise ValueError("toTensorBatch: no image")
    if any(not isinstance(im, JXLImage) for im in images):
        raise ValueError("toTensorBatch: JXLImage objects")
    be = images[0].backend
    if any(im.backend is not be for im in images):
        raise ValueError("toTensorBatch: the images are on different backends")
    if not hasattr(be, "tensor_resized_batch"):
        raise TypeError("toTensorBatch needs a backend with tensor_resized_batch")
    resolved = None
    if toneMap is not None:
        _tone_map_check(toneMap, be)
        if target in ("pq", "as-is") or any(im.has_icc for im in images):
            raise ValueError("toneMap: the output is SDR in known primaries; target srgb or linear, and no ICC profile")
        each = [toneMap.resolve(im) for im in images]
        for i, r in enumerate(each):
            if r != each[0]:
                raise ValueError("toTensorBatch: toneMap resolves differently for image 0 %r and image %d %r" % (each[0], i, r))
        resolved = each[0]
    if size is None:
        raise ValueError("size: (height, width)")
    boxes = [None] * len(images) if boxes is None else list(boxes)
    if len(boxes) != len(images):
        raise ValueError("boxes: one box (or None) per image")
    reqs = [im._tensor_request(torch, dtype, layout, target, alpha, mean, std, size, bx, resample, toneMap is not None) for im, bx in zip(images, boxes)]
    resize0, dtype, name, channels, _, _ = reqs[0]
    if any(r[3] != channels for r in reqs):
        raise ValueError("toTensorBatch: the images give different channel counts (%s)" % sorted({r[3] for r in reqs}))
    (oh, ow), n = resize0[0], len(images)
    shape = (n, channels, oh, ow) if layout == "CHW" else (n, oh, ow, channels)
    device = torch.device(be.tensor_device())
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
            raise ValueError("out: a contiguous %s tensor of shape %s on %s" % (name, shape, device))
    items, sent = [], []
    for im, req in zip(images, reqs):
        planes, kw, up = im._tensor_plan(target, peakDetect, alpha, name, layout, req[4], req[5], toneMap)
        item, more = im._tensor_batch_item(planes, req[0], **kw)
        items.append(item)
        sent.append(up + more)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    elif device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()  # what the caller queued on its tensor is done before the library writes
    if resolved is None:
        be.tensor_resized_batch(items, out.data_ptr())
    else:
        with _ToneMapArmed(be, images[0]._tensor_target(target)[0], WP_D65, resolved):
            be.tensor_resized_batch(items, out.data_ptr())
    for im, b in zip(images, sent):
        im.tensor_bus_bytes = (b, 0)
    out.bus_bytes = (sum(sent), 0)
    return out


# ---- a frame's channels between decodeFrame and the blend ---------------------------------------------------------
def _to_float(a, depth):
    """ImageBuffer.castToFloat (ImageBuffer.java:112-127): a float plane stays as it is"""
    if a.dtype == np.float32:
        return a
    return (a.astype(F) * F(F(1) / F((1 << depth) - 1))).astype(F)


class FramePlanes:
    """One frame's planes from decodeFrame to the blend (JXLCodestreamDecoder.java:628-655), wherever they are:
      host  the host list. The extra channels live there; the colours too while they are on the host (None while not)
      rp    the backend's resident planes (host.ResidentPlanes) while the three colours are on the device, else None
      set   the ready-made plane set (host.DeviceCanvas) of a device_frames frame: every plane, extras included; else None
      moves each real crossing of the colours, "h2d" / "d2h", in order: stats[k]["plane_moves"]
    The five sample stages run on the resident planes where the backend keeps planes resident and the frame has three
    colours (`resident`; row f4), else through the backend's stage calls on the host arrays; the caller does not know which.
    Every device stage works on float samples (Frame.java:221, :806; JXLCodestreamDecoder.java:262): _to_float. The stages
    after the upsampling read planes 0..2 whatever the colour count, as they always have."""

    def __init__(self, backend, info, host, colors, rp=None, fset=None):
        self.be, self.info, self.host, self.colors, self.rp, self.set = backend, info, host, colors, rp, fset
        self.resident = bool(getattr(backend, "resident", False)) and colors == 3
        self.moves = []
        self.away = False  # device_patch_sets: the colours of `set` are in the resident planes (rp) or, after a host stage, in `host`

    @property
    def shape(self):
        return self.set.shape if self.set is not None else self.rp.shape if self.rp is not None else self.host[0].shape

    @property
    def dtypes(self):
        """one per plane, as the blend will see them"""
        if self.set is not None:
            return self.set.dtypes
        return [np.dtype(np.float32) if self.rp is not None and c < 3 else b.dtype for c, b in enumerate(self.host)]

    def _floats(self):
        return np.stack([_to_float(self.host[c], self.info.bits_per_sample) for c in range(3)])

    def _put(self, planes):
        for c in range(3):
            self.host[c] = np.ascontiguousarray(planes[c])

    def to_device(self):
        """the colours as the backend's resident planes (idempotent); returns them"""
        if self.rp is None:
            self.rp = self.be.keep_planes(self._floats())
            self.moves.append("h2d")
        return self.rp

    def to_host(self, log="d2h"):
        """the colours as host arrays (idempotent); returns the host list"""
        if self.rp is not None:
            self._put(self.rp.download())
            self.rp = None
            if log:
                self.moves.append(log)
        return self.host

    def snapshot(self, log):
        """every plane as a host array while the colours stay where they are: a copy of resident colours comes down, logged
        as `log`"""
        if self.rp is None:
            return self.host if self.set is None else self.land()
        planes = self.rp.download()
        self.moves.append(log)
        return list(planes) + (self.host[3:] if self.set is None else [self.set.download(c) for c in range(3, len(self.set))])

    def land(self):
        """every plane as a host array, for a blend on the host after all (stats[k]["canvas"] tells; no move of the tail)"""
        if self.set is not None:
            self.settle()
            return [self.set.download(c) for c in range(len(self.set))]
        return self.to_host(log=None)

    def blend_set(self):
        """a plane set of this frame for jxl_canvas_blend: the ready-made one, the resident colours with the extras uploaded
        beside them (the colours cross no bus), or the host arrays uploaded"""
        if self.set is not None:
            self.settle()
            return self.set
        canvas, ctx = self.be.host.DeviceCanvas, self.be.ctx
        if self.rp is None:
            return canvas.fromArrays(ctx, self.host)
        fset = canvas.fromPlanes(ctx, [b.dtype for b in self.host[3:]])
        for i, b in enumerate(self.host[3:]):
            fset.upload(3 + i, b)
        return fset

    def one_size(self):
        """(the planes of a ready-made set are those of one launch: one size by construction)"""
        shape = tuple(self.shape)
        return self.set is not None or all(tuple(b.shape) == shape for b in self.host[3 if self.rp is not None else 0:])

    # -- device_patch_sets: the frame's planes become a set at the patch stage ------------------------------------------------
    def adopt_set(self):
        """every plane of the frame in ONE set from here on, which blend_set() hands to the blend. From a host list every
        plane goes up once; from resident colours only the extra channels do, and the colours stay where they are until
        settle() copies them into the set (`away`). Returns the set"""
        canvas, ctx = self.be.host.DeviceCanvas, self.be.ctx
        if self.set is not None:  # a ready-made set (device_frames with device_chains): it is the one; nothing goes up
            return self.set
        if self.rp is None:
            self.set = canvas.fromArrays(ctx, self.host)
        else:
            self.set = canvas.create(ctx, [np.dtype(np.float32)] * 3 + [b.dtype for b in self.host[3:]], *self.shape)
            for i, b in enumerate(self.host[3:]):
                self.set.upload(3 + i, b)
            self.away = True
        return self.set

    def leave_for_host(self):
        """a ready-made set comes down for good: every plane a host array, as a frame that never was a set has them"""
        self.host = [self.set.download(c) for c in range(len(self.set))]
        self.set.release()
        self.set = None

    def visit_planes(self):
        """the colours of an adopted set into the resident planes for the stages that follow the patches; integer colours are
        cast in the set before they leave it (every device stage works on float samples)"""
        if not self.away:
            ints = [(self.set, c, self.info.bits_per_sample) for c in range(3) if self.set.dtypes[c] != np.float32]
            if ints:
                self.be.host.canvas_cast_planes(self.be.ctx, ints)
            self.leave_set()
            self.away = True

    def settle(self):
        """the colours back into the adopted set, before the set is read as a whole"""
        if self.away:
            self.rejoin_set()
            self.away = False

    # -- device_frames: the colours of the ready-made set visit the resident planes for the stages -----------------------
    def leave_set(self):
        self.rp = self.set.toPlanes()

    def rejoin_set(self):
        if self.rp is not None:
            self.set.takePlanes()
            self.rp = None
        else:  # the last stage was a host stage (splines without device_splines): its planes go up into the set
            for c in range(3):
                self.set.upload(c, self.host[c])
            self.moves.append("h2d")

    # -- the sample stages (JXLCodestreamDecoder.java:628-637) --------------------------------------------------------------
    def upsample(self, fr, weights):
        """Frame.upsample (Frame.java:217-260): every channel by its own factor; weights(k) gives the kernel"""
        info = self.info
        for c in range(len(self.host)):
            k = fr.upsampling if c < self.colors else fr.ec_upsampling[c - self.colors]
            if k > 1 and not (self.resident and c < 3):
                depth = info.bits_per_sample if c < self.colors else info.ec_bits[c - self.colors]
                self.host[c] = self.be.upsample(_to_float(self.host[c], depth), k, weights(k))
        if self.resident and fr.upsampling > 1:
            self.to_device().upsample(fr.upsampling, weights(fr.upsampling))

    def splines(self, fr, splines, on_device):
        """Frame.renderSplines: in the backend with `on_device` (no silent return to the host render), else render_splines"""
        if on_device and self.resident:
            return self.to_device().splines(splines, fr.base_corr_x, fr.base_corr_b)
        host = self.to_host()
        for c in range(3):
            host[c] = _to_float(host[c], self.info.bits_per_sample).copy()
        if on_device:  # the stage entry
            self._put(self.be.splines(np.stack(host[:3]), splines, fr.base_corr_x, fr.base_corr_b))
        else:
            render_splines(host, splines, fr.base_corr_x, fr.base_corr_b, host[0].shape[1], host[0].shape[0])

    def noise(self, fr, seed0, at=None):
        """initializeNoise + synthesizeNoise (Frame.java:748-831). initializeNoise depends on the frame counters and the size
        only: its place before the patches in the reference is moot. at: (frame_h, frame_w, y0, x0) when the planes are that
        window of the frame: the whole frame's noise restricted to it (ResidentPlanes.noiseAt / backend.noise_window; a backend
        without `noise_window` is an error)"""
        lut = np.array(fr.noise, F)
        if at is not None:
            if self.resident:
                return self.to_device().noiseAt(fr.group_dim, seed0, lut, fr.base_corr_x, fr.base_corr_b, *at)
            if not hasattr(self.be, "noise_window"):
                raise RuntimeError("noise on a region needs a backend with `noise_window`")
            return self._put(self.be.noise_window(self._floats(), fr.group_dim, seed0, lut, fr.base_corr_x, fr.base_corr_b, *at))
        if self.resident:
            return self.to_device().noise(fr.group_dim, seed0, lut, fr.base_corr_x, fr.base_corr_b)
        h, w = self.host[0].shape
        noise = self.be.noise_init(h, w, seed0, fr.group_dim, self.colors)
        self._put(self.be.noise_add(self._floats(), noise, lut, fr.base_corr_x, fr.base_corr_b))

    def invert_xyb(self, matrix, opsin_bias, cbrt_bias, intensity_target):
        if self.resident:
            return self.to_device().invertXYB(matrix, opsin_bias, cbrt_bias, intensity_target)
        self._put(self.be.xyb(self._floats(), matrix, opsin_bias, cbrt_bias, intensity_target))

    def ycbcr(self):
        if self.resident:
            return self.to_device().ycbcr()
        self._put(self.be.ycbcr(self._floats()))

    def varblocks(self, blocks, cells):
        """Frame.drawVarblocks in one device pass, where the colours are; returns stats[k]["varblocks"]"""
        if self.rp is not None:
            self.rp.varblocks(blocks, cells)
            return "device planes"
        self._put(self.be.varblocks(self._floats(), blocks, cells))
        return "host planes"


# ---- JXLDecoder (J/JXLDecoder.java + J/JXLCodestreamDecoder.java) ---------------------------------------------
def _tt_dims():
    return [(t[5] >> 3, t[6] >> 3) for t in abi.TRANSFORM_TYPES]


class JXLDecoder:
    # the switches' defaults (a decoder made with JXLDecoder.__new__ -- tests, tools, load_vardct_frame -- has them too)
    sparse_coeffs = device_splines = device_patches = device_output = device_canvas = False
    draw_varblocks = device_palette = device_image = device_frames = device_patch_sets = device_chains = False
    downsample = 1
    region = None
    trace = None  # test hook: see _trace
    _patch_sets = False  # device_patch_sets acts on the frame in hand (_canvas_route)

    def __init__(self, source, backend=None, sparse_coeffs=False, device_splines=False, device_patches=False, device_output=False,
                 device_canvas=False, draw_varblocks=False, device_palette=False, device_image=False, device_frames=False,
                 device_patch_sets=False, device_chains=False, downsample=1, region=None):
        """sparse_coeffs: hand the HF coefficients to the backend as lists of non-zero entries (jxf_get_coeffs_sparse ->
        jxl_vardct_put_group_sparse), not as dense planes; same pixels.
        device_splines: Frame.renderSplines runs in the backend (jxl_planes_splines on the resident planes, jxl_stage_splines
        otherwise) instead of render_splines on the host; the samples agree except where a (float)Math.exp falls on the other
        side of a float rounding boundary (include/jxlatte_amd.h). A backend without `splines` is an error.
        device_patches: computePatches runs in the backend as one launch per segment of patch_type_plan (jxl_planes_patches on
        the resident planes, jxl_stage_patches otherwise) instead of one backend.blend per (position, channel); the same bits.
        Grey images and frames whose colour count is not the image's keep the blend calls; stats[-1]["patches"] tells. A backend
        without `patches` is an error.
        device_output: a frame that IS the image -- a regular last frame of three float colour planes at the origin, of the
        image's size after upsampling, blended with REPLACE, the first to reach the canvas, lf_level 0 -- leaves its colour
        planes on the device when they are there after performColorTransforms, and decode() returns a JXLImage that carries
        them (JXLImage.resident; getBuffer() downloads on first use, the same bits). A VarDCT frame without a stage after
        decodeFrame qualifies too. The extra channels are blended and oriented on the host as ever; the orientation of the
        colour planes is ResidentPlanes.orient. Every other frame takes the usual path. stats[-1]["output"] tells which:
        "device" or "host".
        device_canvas: the canvas and the reference frames saved after the colour transform live on the device as plane sets
        (host.DeviceCanvas) and blendFrame is one launch per frame (jxl_canvas_blend) behind the whole-plane casts of
        blend_type_plan; a frame's resident colour planes reach the blend without touching the host. decode() ends with the
        canvas' colour planes as the image's resident planes when they are float (else it downloads them); getBuffer() gives
        the default decoder's arrays either way. Where blend_type_plan says "land", and before a frame with patches, every set
        comes down into host lists (aliases stay aliases) and the image goes on as without the switch. stats[-1]["canvas"]:
        "device", "host" (the switch is off) or "landed: <reason>". device_output's single-frame path takes precedence. A backend
        without a context is an error.
        draw_varblocks: JXLOptions.renderVarblocks -- every VarDCT frame that reaches performColorTransforms (invisible frames
        too) gets Frame.drawVarblocks right after it (JXLCodestreamDecoder.java:638-639): each varblock tinted by its transform
        type, its top row and left column black, after the saveBeforeCT reference is taken and before the blend. One device pass:
        ResidentPlanes.varblocks where the colour planes are on the device at that point (device_output, device_canvas),
        backend.varblocks on the host planes otherwise; there is no host restatement, and a backend without `varblocks` is an
        error. Modular frames are left alone. stats[k]["varblocks"] then says "device planes" or "host planes" (the type
        histogram it holds without the switch moves to stats[k]["varblock_types"]). A frame of several LF groups whose group
        size is not 256 raises UnsupportedOperationException: the reference's hard-coded << 11 leaves the frame there.
        device_palette: the Palette transforms of the frame-level Modular stream (ModularStream.java:327-378) run in the backend
        (backend.palette: jxl_stage_palette, one call per transform) instead of the front-end's loop; the same samples. The
        palettes of the per-group sub-streams stay in the front-end, and so does a palette with predictor 6 whose weighted
        predictor's plane was not kept. stats[k]["palette"] lists, per transform in the order they were undone, dict(num_c,
        nb_colors, delta_pixels, launches); it is [] for a frame without one. A backend without `palette` is an error.
        device_image: the decoded JXLImage is backed by a device plane set (JXLImage.planeSet), colours and extra channels,
        whatever their types, where one of two routes leads there; PNGWriter / PFMWriter(deviceSamples=True) read the set, so only
        the file's samples come down. Route "modular frame": a Modular frame that is the whole image (_modular_frame_route lists
        the conditions) is decoded with the front-end's frame-level transforms deferred; the encoded channels go up once
        (jxl_modular_begin), the plan runs, and jxl_canvas_from_modular makes the set -- nothing comes down. Route "canvas": with
        device_canvas, the canvas set at the end of decode() becomes the image's (cloned while the animation continues).
        Every other frame runs jxf_apply_transforms with the usual hooks and goes on exactly as without the switch.
        stats[k]["image"]: "device set (modular frame)", "device set (canvas)" or "host: <reason>". device_output's direct path
        is unchanged and comes first for the frames it covers. A backend without a context is an error.
        device_frames: with device_canvas, while the canvas is a plane set, a Modular frame reaches the blend as a plane set made
        from the Modular context, not through the host. The front-end decodes every frame with its frame-level transforms
        deferred (as device_image does); for a frame that frame_set_rule accepts -- a chain that is one plan, three int32 colour
        planes, no patches, restoration filter, YCbCr or XYB, extra channels upsampled as the colours are, no `trace` listener;
        position, blend modes, reference slots, noise and splines are free -- the encoded channels go up once, the plan runs,
        and the frame's set is jxl_canvas_from_modular (int32 colours where no stage follows, float colours at 1f / maxValue
        where noise or splines do) or jxl_canvas_from_modular_up (upsampling 2, 4, 8: every plane cast with its own depth and
        upsampled in one launch). Noise and splines run on the resident planes between jxl_canvas_to_planes and
        jxl_canvas_take_planes; splines without device_splines still bring the three colour planes down and up
        (stats[k]["plane_moves"]). The extra channels never move. The same bits as without the switch. Every other frame runs
        jxf_apply_transforms with the usual hooks and goes on as ever. stats[k]["frame"]: "device set (modular)", "host: <the
        first condition that failed>" or "host: device_frames is off". device_image's "modular frame" route and device_output's
        direct path come first for the frames they cover.
        device_patch_sets: with device_canvas and device_patches, while the canvas is a plane set, on a three-colour image, a
        frame with patches whose colour count is the image's (patch_sets_rule) no longer lands the canvas: at the patch stage
        its planes become a plane set (from a host list every plane goes up once; from resident colours only the extra
        channels do), and computePatches runs per segment of patch_type_plan as one jxl_canvas_cast_planes call for the hoisted
        casts and one jxl_canvas_patches call, the reference slots read where they are -- a slot that is a plane set (the
        canvas itself included: one set, one set of tags) keeps its casts; a slot that is a host list (saved before the colour
        transform) keeps them in the list and goes up as a temporary set. The stages after the patches run on the resident
        planes and the blend reads the frame's set: nothing goes up again. The same bits. stats[k]["patches"]["path"] is
        "plane sets" and stats[k]["canvas"] stays "device"; what still lands says why there: a below mode that reads the
        frame off its own pixel, frame planes of different sizes, a slot with another plane count, more than 16 planes.
        device_chains: acts only together with device_image or device_frames. The plan those two make of a frame's frame-level
        chain is built from the whole transform list (jxl_modular_begin_chain): any chain of RCT, Palette and Squeeze
        transforms is one plan -- a Palette reads its palette from the device copy of channel 0, a run of consecutive Palettes
        is one launch -- except a Palette with nb_deltas > 0 and d_pred 6 ("a Palette with weighted-predictor deltas": that
        plane exists only inside the front-end's decode). With device_frames a frame with patches is accepted too where
        patch_sets_rule holds for it: the set made from the Modular context goes through the patch stage as it is (nothing
        goes up again) and the blend reads it; what _patches_sets refuses lands the canvas with its reason, as without the
        switch. The same bits. stats[k]["chain"], only with the switch: dict(kinds, runs) for a frame whose chain ran as a
        plan -- runs: dict(fused, steps, redone), the launches of its Palette runs as one launch each, as single steps, and
        the runs that ran again because a pixel needed its neighbours.
        downsample: 1 (the image) or 8: the image at 1:8 from the LF image of its VarDCT frame, without reading one HF section. The
        front-end stops after the LF coefficients (jxf_set_lf_only), and ONE backend.lf_image call turns every LF group's integers
        into three planes of ceil(h / 8) x ceil(w / 8) samples: the LF stage per LF group (dequantisation, LF chroma-from-luma,
        adaptive smoothing) and the inverse XYB. YCbCr, the orientation and everything a JXLImage offers follow on an image of that
        size; with device_output the planes are the image's resident planes and nothing comes down. This is a faithful thumbnail
        -- the full decode box-averaged 8 x 8, up to what Gaborish, the EPF and the low frequencies of large varblocks add -- not the
        reference's pixels. preview_rule lists what a frame needs; one that does not qualify raises
        UnsupportedOperationException("downsample=8: <reason>") before any HF section is read, and the caller decodes in full.
        Noise is left out (zero-mean grain). stats[k]["preview"] is "lf image (1:8)", with ", noise left out" where there was
        some. Refused together with draw_varblocks, device_canvas, device_frames or a `trace` listener. A backend without
        `lf_image` is an error.
        region: None (the image) or a box (x0, y0, w, h) in the coordinates of the image as delivered (after the orientation):
        decode() returns a JXLImage of h x w pixels whose planes are the full decode's planes[y0:y0 + h, x0:x0 + w] bit for bit,
        and the front-end reads only the sections the box needs (jxf_set_region): the groups that the box, mapped into the frame
        (region_in_frame) and grown by the restoration filters' reach M, touches, and the LF groups that hold them. Those LF
        groups, renumbered from their corner, go through backend.vardct as a frame of their own -- the groups that were not read
        are never sent and count as zero -- and the box is cut out of its result: jxl_planes_from_frame_at where the planes stay
        on the device, a slice otherwise. The tail runs on box-sized planes; noise, the one stage that depends on where a pixel
        lies in the frame, through jxl_planes_noise_at / jxl_stage_noise_window. With device_output the planes are the image's
        resident planes. region_rule lists what a frame needs; one that does not qualify raises
        UnsupportedOperationException("region: <reason>") before backend.vardct is called. A single-section frame is read whole
        and cropped. stats[k]["region"]: dict(box, frame_box, margin, groups_read, groups_total, lf_groups_read, lf_groups_total,
        section_bytes_read, section_bytes_total, subframe (x, y, w, h), path: "groups" or "whole frame (single section)"). An
        empty box or one that is not inside the image is a ValueError. Refused together with downsample=8, draw_varblocks,
        device_canvas, device_frames, device_image or a `trace` listener."""
        if region is not None:
            try:
                box = tuple(region)
                ok = len(box) == 4 and all(int(v) == v for v in box)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("region must be four integers (x0, y0, w, h), not %r" % (region,))
            region = tuple(int(v) for v in box)
            for name, on in (("downsample=8", downsample == 8), ("draw_varblocks", draw_varblocks), ("device_canvas", device_canvas),
                             ("device_frames", device_frames), ("device_image", device_image)):
                if on:
                    raise ValueError("region cannot be combined with " + name)
        self.region = region
        if downsample not in (1, 8):
            raise ValueError("downsample must be 1 or 8, not %r" % (downsample,))
        self.downsample = int(downsample)
        if self.downsample == 8:
            for name, on in (("draw_varblocks", draw_varblocks), ("device_canvas", device_canvas), ("device_frames", device_frames)):
                if on:
                    raise ValueError("downsample=8 cannot be combined with " + name)
        self.device_chains = bool(device_chains)
        self.device_patch_sets = bool(device_patch_sets)
        self.device_frames = bool(device_frames)
        self.device_image = bool(device_image)
        self.device_palette = bool(device_palette)
        self.draw_varblocks = bool(draw_varblocks)
        self.device_output = bool(device_output)
        self.device_canvas = bool(device_canvas)
        self._landed = None   # why the canvas is (back) on the host for the rest of this image
        self._dead_sets = []  # plane sets of the last blend, released once the next call has no use for them
        self._patch_sets = False  # device_patch_sets acts on the frame in hand (_canvas_route)
        self.sparse_coeffs = bool(sparse_coeffs)
        self.device_splines = bool(device_splines)
        self.device_patches = bool(device_patches)
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
        else:
            with open(source, "rb") as f:
                data = f.read()
        self.backend = backend if backend is not None else DeviceBackend()
        try:
            self.fe = frontend.Frontend(data)
        except frontend.FrontendError as e:
            raise self._map(e)
        self.info = self.fe.image
        if self.region is not None:
            self.region_in_frame(self.info, self.region)  # (a ValueError before any frame is read)
        self.reference = [None] * 4
        self.lfBuffer = [None] * 5
        self.canvas = None
        self.visibleFrames = 0
        self.invisibleFrames = 0
        self.frames_decoded = 0
        self.stats = []  # per frame: dict(encoding, size, groups, types histogram...) for reporting

    def close(self):
        """release the plane sets of device_canvas (the context frees what is left of them when it is destroyed)"""
        self._release_dead()
        sets = {id(s_): s_ for s_ in [self.canvas] + list(self.reference) if self._is_set(s_)}
        for s_ in sets.values():
            s_.release()
        if self._is_set(self.canvas):
            self.canvas = None
        self.reference = [None if self._is_set(r) else r for r in self.reference]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _map(e):
        if e.status == -3:
            return UnsupportedOperationException(str(e))
        if e.status == -2:
            return InvalidBitstreamException(str(e))
        return e

    def getImageHeader(self):
        return self.info

    def _trace(self, stage, planes, fused):
        """test hook (tests/test_jvm_pin.py): `self.trace(frame_index, stage, planes, fused)` at the cut points where the pin-on-arrival
        harness makes the reference dump its planes; None (the default): nothing"""
        if self.trace is not None:
            self.trace(self.frames_decoded - 1, stage, planes, fused)

    # -- frame-level pieces ---------------------------------------------------------------------------------------
    def _colors(self, fr):
        return 3 if (self.info.xyb_encoded or fr.encoding == VARDCT) else (1 if self.info.colour_space == CE_GRAY else 3)

    def _opsin(self):
        """OpsinInverseMatrix.getMatrix(bundle.prim, bundle.white) (JXLCodestreamDecoder.java:592-595)"""
        info = self.info
        conv = get_conversion_matrix(np.array(info.prim_xy, F), np.array(info.white_xy, F), PRI_SRGB, WP_D65)
        m = _mat_mul(conv, np.array(info.opsin_matrix, F).reshape(3, 3))
        bias = np.array(info.opsin_bias, F)
        cbrt = np.array([F(np.cbrt(np.float64(b))) for b in bias], F)
        return m.reshape(-1), bias, cbrt

    def _weights(self, fr):
        if fr.quant_all_default:
            return hfglobal.default_weights()
        params = []
        for i in range(17):
            q = self.fe.quant_params(i)
            if q["mode"] == 0:
                params.append(hfglobal.DEFAULT_PARAMS[i])
            else:
                params.append(dict(mode=q["mode"], denominator=q["denominator"],
                                   dct=None if q["dct"] is None else [list(r) for r in q["dct"]],
                                   par=None if q["par"] is None else [list(r) for r in q["par"]],
                                   p44=None if q["p44"] is None else [list(r) for r in q["p44"]]))
        return hfglobal.generate_weights(params)

    def _vardct_frame(self, fr, fuse_xyb, keep=None, sub=None):
        p, weights, woffs, lfgroups, groups, hist = self._vardct_inputs(fr, fuse_xyb, sub)
        self.stats[-1]["varblocks"] = {abi.TT_NAME[t]: int(n) for t, n in enumerate(hist) if n}
        self._varblock_list = self._gather_varblocks(fr, lfgroups) if self.draw_varblocks else None
        sparse = self.sparse_coeffs
        kw = dict(sparse=True) if sparse else {}
        if keep is not None:
            return self.backend.vardct(p, weights, woffs, lfgroups, groups(sparse), keep=keep, **kw)
        planes = self.backend.vardct(p, weights, woffs, lfgroups, groups(sparse), **kw)
        return [np.ascontiguousarray(planes[c]) for c in range(3)]

    @staticmethod
    def _gather_varblocks(fr, lfgroups):
        """the frame's block list as Frame.drawVarblocks walks it (Frame.java:468-481): (cy, cx, type) in frame cells, and the
        cell grid they live on. The LF group's offset is the reference's << 11 pixels = << 8 cells"""
        if len(lfgroups) > 1 and fr.group_dim != 256:
            raise UnsupportedOperationException("draw_varblocks: several LF groups with group_dim %d (the reference's LF-group "
                                                "pitch of 2048 pixels holds for 256 only)" % fr.group_dim)
        rows, cells_h, cells_w = [], 1, 1
        for g in lfgroups:
            oy, ox = g["lfg_y"] << 8, g["lfg_x"] << 8
            yx, sel = g["block_yx"], np.asarray(g["dct_select"])
            rows.append(np.stack([yx[:, 0] + oy, yx[:, 1] + ox, sel[yx[:, 0], yx[:, 1]]], axis=1).astype(np.int32))
            cells_h, cells_w = max(cells_h, oy + sel.shape[0]), max(cells_w, ox + sel.shape[1])
        return np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 3), np.int32), (cells_h, cells_w)

    def _up_weights(self, k):
        info = self.info
        idx = {2: 0, 4: 1, 8: 2}[k]
        if info.custom_up[idx]:
            packed = self.fe.up_weights(idx)
        else:
            from .upweights import DEFAULT_UP
            packed = DEFAULT_UP[k]
        from . import host
        return host.getUpWeights(k, packed)

    def _chained_tail(self, fr, planes, save, xyb_done, keep=False, upsampled=False, adopted=False, noise_at=None):
        """Frame.upsample .. performColorTransforms (JXLCodestreamDecoder.java:628-637), the one statement of that order, for
        every backend: upsample, the saveBeforeCT reference, patches, splines, noise, inverse XYB, YCbCr. `planes`
        (FramePlanes) runs each sample stage where the samples can be and moves the colours between host and device only
        where the next stage lives on the other side; the saveBeforeCT reference and the patches' blend calls are host stages
        (as in the reference).
        keep: colours that are on the device at the end stay there. upsampled: the planes are already past Frame.upsample
        (_modular_frame_set). adopted: the planes are a ready-made set that the patch stage takes as it is (device_chains).
        noise_at: (frame_h, frame_w, y0, x0) when the planes are that window of the frame and not the frame (region)."""
        info = self.info
        if not upsampled:
            planes.upsample(fr, self._up_weights)
        dev_patches = self.device_patches and bool(fr.num_patches)
        if save and fr.save_before_ct:
            if dev_patches and planes.rp is not None:  # a copy comes down, the planes stay
                self.reference[fr.save_as_reference] = planes.snapshot("d2h")[:3] + [b.copy() for b in planes.host[3:]]
            else:
                self.reference[fr.save_as_reference] = [b.copy() for b in planes.to_host()]
        if fr.num_patches:
            on_sets = self._patch_sets
            if on_sets:
                why = self._patches_sets(fr, planes)
                if why is not None:  # nothing has been touched: everything lands and the stage runs as without the switch
                    self._land(why)
                    self.stats[-1]["canvas"] = "landed: " + why
                    on_sets = False
                    if adopted:
                        planes.leave_for_host()
            if not on_sets and not (dev_patches and planes.colors == 3 and info.colour_space != CE_GRAY and self._patches_device(fr, planes)):
                self._patches(fr, planes.to_host(), planes.colors)
                self.stats[-1].setdefault("patches", dict(path="blend calls"))
        adopted = planes.set is not None and (adopted or not upsampled)  # (device_patch_sets: the frame's set is the patch stage's)
        if adopted and (fr.has_splines or fr.has_noise or (info.xyb_encoded and not xyb_done) or fr.do_ycbcr):
            planes.visit_planes()
        if fr.has_splines:
            planes.splines(fr, self.fe.splines(), self.device_splines)
        if fr.has_noise:
            planes.noise(fr, (self.visibleFrames << 32) | self.invisibleFrames, at=noise_at)
        if info.xyb_encoded and not xyb_done:
            planes.invert_xyb(*self._opsin(), info.intensity_target)
        if fr.do_ycbcr:
            planes.ycbcr()
        if not keep:
            planes.to_host()
        if planes.resident:
            self.stats[-1]["plane_moves"] = planes.moves

    @staticmethod
    def _subframe(fr, plan):
        """region: the LF-group rectangle of a region plan (Frontend.region_plan) as a frame of its own: dict(x, y, w, h: its
        place in the padded frame -- the origin is a multiple of the LF-group size --, lf: [(index in the frame, lfg_y, lfg_x)
        in the sub-frame], groups: [(index in the frame, index in the sub-frame's own group grid)] of the groups that were read)"""
        gd = fr.group_dim
        lfd = gd << 3
        ox, oy = plan["lf_group_x0"] * lfd, plan["lf_group_y0"] * lfd
        w = min(fr.padded_width, (plan["lf_group_x0"] + plan["lf_group_w"]) * lfd) - ox
        h = min(fr.padded_height, (plan["lf_group_y0"] + plan["lf_group_h"]) * lfd) - oy
        lf = [((plan["lf_group_y0"] + y) * fr.lf_group_cols + plan["lf_group_x0"] + x, y, x)
              for y in range(plan["lf_group_h"]) for x in range(plan["lf_group_w"])]
        cols = (w + gd - 1) // gd
        groups = [(gy * fr.group_cols + gx, (gy - (plan["lf_group_y0"] << 3)) * cols + gx - (plan["lf_group_x0"] << 3))
                  for gy in range(plan["group_y0"], plan["group_y0"] + plan["group_h"])
                  for gx in range(plan["group_x0"], plan["group_x0"] + plan["group_w"])]
        return dict(x=ox, y=oy, w=w, h=h, lf=lf, groups=groups)

    def _vardct_inputs(self, fr, fuse_xyb, sub=None):
        """the boundary tensors of one VarDCT frame: (jxl_vardct_params, weights, offsets, LF groups, group iterator). sub: a
        sub-frame of whole LF groups (_subframe) in the frame's place: its size, its LF groups and the groups that were read,
        both numbered in the sub-frame's own grids"""
        info, fe = self.info, self.fe
        p = abi.VarDCTParams()
        for c in range(3):
            p.jpeg_upsampling_y[c], p.jpeg_upsampling_x[c] = fr.jpeg_up_y[c], fr.jpeg_up_x[c]
        p.width, p.height = (fr.padded_width, fr.padded_height) if sub is None else (sub["w"], sub["h"])
        stages = abi.STAGE_IDCT | abi.STAGE_GAB | abi.STAGE_EPF | (abi.STAGE_XYB if fuse_xyb else 0)
        p.stages = stages
        gs = F(F(65536.0) / F(fr.global_scale))  # HFCoefficients.java:270-275
        sf = [F(gs * F(math.pow(0.8, fr.xqm - 2.0))), gs, F(gs * F(math.pow(0.8, fr.bqm - 2.0)))]
        for c in range(3):
            p.scale_factor[c] = sf[c]
            p.quant_bias[c] = info.quant_bias[c]
            p.gab_w1[c], p.gab_w2[c] = fr.gab1[c], fr.gab2[c]
            p.epf_channel_scale[c] = fr.epf_channel_scale[c]
        p.quant_bias_numerator = info.quant_bias_numerator
        p.base_corr_x, p.base_corr_b, p.color_factor = fr.base_corr_x, fr.base_corr_b, fr.colour_factor
        p.gab, p.epf_iters = fr.gab, fr.epf_iters
        p.global_scale_f = gs
        for i in range(8):
            p.epf_sharp_lut[i] = fr.epf_sharp_lut[i]
        p.epf_pass0_sigma_scale, p.epf_pass2_sigma_scale = fr.epf_pass0_sigma, fr.epf_pass2_sigma
        p.epf_border_sad_mul = fr.epf_border_sad_mul
        m, bias, cbrt = self._opsin()
        p.xyb = 1 if fuse_xyb else 0
        for i in range(9):
            p.opsin_matrix[i] = m[i]
        for c in range(3):
            p.opsin_bias[c], p.cbrt_opsin_bias[c] = bias[c], cbrt[c]
        p.intensity_target = info.intensity_target
        p.transfer, p.out_format = abi.TRANSFER_NONE, abi.OUT_F32
        weights, woffs = self._weights(fr)
        adaptive = (fr.flags & (FLAG_SKIP_ADAPTIVE_LF | FLAG_USE_LF_FRAME)) == 0
        lfgroups, hist = [], np.zeros(27, np.int64)
        lf_list = [(i, i // fr.lf_group_cols, i % fr.lf_group_cols) for i in range(fr.num_lf_groups)] if sub is None else sub["lf"]
        for i, lfg_y, lfg_x in lf_list:
            g = fe.lfgroup(i)
            g.update(lfg_y=lfg_y, lfg_x=lfg_x, lf=None,
                     scaled_dequant=list(fr.scaled_dequant), x_factor_lf=fr.x_factor_lf, b_factor_lf=fr.b_factor_lf,
                     adaptive_smoothing=adaptive)
            if fr.flags & FLAG_USE_LF_FRAME:
                g["lf"] = lf_from_lf_frame(self.lfBuffer[fr.lf_level], i // fr.lf_group_cols, i % fr.lf_group_cols, g["cells_h"],
                                           g["cells_w"], list(fr.jpeg_up_y), list(fr.jpeg_up_x), info.bits_per_sample)
                g["lf_quant"] = None
            g["block_yx"] = np.ascontiguousarray(g["block_yx"], np.int32)
            sel = g["dct_select"][g["block_yx"][:, 0], g["block_yx"][:, 1]]
            hist += np.bincount(sel, minlength=27)[:27]
            lfgroups.append(g)

        group_list = [(g, g) for g in range(fr.num_groups)] if sub is None else sub["groups"]

        def groups(sparse=False):
            for pass_ in range(fr.num_passes):
                for grp, as_ in group_list:
                    yield pass_, as_, fe.coeffs_sparse(pass_, grp) if sparse else fe.coeffs(pass_, grp)
        return p, weights, woffs, lfgroups, groups, hist

    def _modular_buffers(self, fr, buffers, colors):
        """modular channels -> frame buffers (Frame.decodeFrame :430-455)"""
        info, fe = self.info, self.fe
        n_mod = fr.num_modular_channels
        chans = [fe.modular_channel(i)[0] for i in range(n_mod)]
        self._trace("mod", chans, False)  # ModularStream.getDecodedBuffer after applyTransforms (Frame.java:427-428)
        c_map = (1, 0, 2)
        for c in range(n_mod):
            is_mod_color = fr.encoding == MODULAR and c < colors
            is_mod_xyb = bool(info.xyb_encoded) and is_mod_color
            c_out = (c_map[c] if is_mod_xyb else c) + len(buffers) - n_mod
            h, w = fr.height, fr.width
            src = chans[c][:h, :w]
            scale = fr.lf_dequant[c_out] if is_mod_xyb else 1.0
            if is_mod_xyb and c == 2:
                val = self.backend.modular_to_float(np.ascontiguousarray(chans[0][:h, :w]), np.ascontiguousarray(src), scale)
            elif buffers[c_out].dtype == np.float32:
                val = self.backend.modular_to_float(np.ascontiguousarray(src), None, scale)
            else:
                val = src
            buffers[c_out][:h, :w] = val

    # -- the canvas on the device (device_canvas) -----------------------------------------------------------------
    def _is_set(self, obj):
        return hasattr(obj, "canvasShape")  # host.DeviceCanvas (the decoder imports no binding at module level)

    def _release_dead(self):
        for s_ in self._dead_sets:
            s_.release()
        self._dead_sets = []

    def _land(self, reason):
        """every plane set comes down: self.canvas and each self.reference[k] that is a set become host lists -- ONE list per
        set, so the aliases stay aliases -- and the sets are released. The canvas is not taken up again within this image."""
        if self._landed is None:
            self._landed = reason
        self._release_dead()
        done = {}
        def host_list(s_):
            if id(s_) not in done:
                done[id(s_)] = ([s_.download(i) for i in range(len(s_))], s_)
            return done[id(s_)][0]
        if self._is_set(self.canvas):
            self.canvas = host_list(self.canvas)
        for k in range(4):
            if self._is_set(self.reference[k]):
                self.reference[k] = host_list(self.reference[k])
        for _, s_ in done.values():
            s_.release()

    def _count_frame(self, fr):
        """the frame counters initializeNoise's seed is made of (JXLCodestreamDecoder.java:620-627); returns whether the frame is
        saved as a reference"""
        visible = fr.type in (REGULAR_FRAME, SKIP_PROGRESSIVE) and (fr.duration != 0 or fr.is_last)
        if visible:
            self.visibleFrames += 1
            self.invisibleFrames = 0
        else:
            self.invisibleFrames += 1
        return (fr.save_as_reference != 0 or fr.duration == 0) and not fr.is_last and fr.type != LF_FRAME

    def _frame_done(self, fr, save, bus0):
        """the end of a frame's turn (:656-658): the canvas into its reference slot, the frame's bus traffic into the stats;
        returns whether decode() has its image"""
        if save and not fr.save_before_ct:
            self.reference[fr.save_as_reference] = self.canvas
        self._bus_since(bus0)
        return fr.is_last or fr.duration != 0

    def _blend_bus(self):
        """host._bus: what the blend path has moved so far, (bytes up, bytes down)"""
        return tuple(getattr(getattr(self.backend, "ctx", None), "blend_bus", (0, 0)))

    def _bus_since(self, bus0):
        bus1 = self._blend_bus()
        self.stats[-1]["blend_bus"] = (bus1[0] - bus0[0], bus1[1] - bus0[1])  # bytes up, bytes down: patches and blendFrame

    def _canvas_frame(self, fr, planes):
        """one frame onto the canvas set (:640-655): the set is made when the first frame reaches it, copied when a reference
        slot shares it, and blended in one launch -- or everything lands and the host blends"""
        info, be = self.info, self.backend
        if not self._is_set(self.canvas):  # :640-643: every plane of the type of the frame's first buffer
            self.canvas = be.host.DeviceCanvas.create(be.ctx, [planes.dtypes[0]] * len(self.canvas), info.height, info.width)
        why = None
        if fr.type in (REGULAR_FRAME, SKIP_PROGRESSIVE):
            if any(self.reference[i] is self.canvas and i != fr.save_as_reference for i in range(4)):
                self.canvas = self.canvas.clone()  # :645-653
            why = self._blend_frame_device(fr, planes)
        # landing: the frame's planes come down, then the sets, and this frame is blended as without the switch (the
        # copy-on-write above has been made already, on the device)
        buffers = planes.land() if why is not None else None
        if planes.set is not None and not any(s_ is planes.set for s_ in self._dead_sets):
            planes.set.release()
        if why is not None:
            self._land(why)
            self.stats[-1]["canvas"] = "landed: " + why
            self._blend_frame(fr, buffers, planes.colors)

    def _blend_frame_device(self, fr, planes):
        """blendFrame on the plane sets: the type plan, the frame's planes into a set (FramePlanes.blend_set), the hoisted
        casts, one launch. Returns None, or the reason to land (nothing has been touched then)."""
        host, ctx = self.backend.host, self.backend.ctx
        info, cv = self.info, self.canvas
        refs = self.reference
        ref_types = [None if r is None else "canvas" if r is cv else r.dtypes if self._is_set(r) else
                     [None if b is None else b.dtype for b in r] for r in refs]
        plan = blend_type_plan(info, fr, cv.dtypes, planes.dtypes, ref_types)
        if plan.verdict != "device":
            return plan.verdict[len("land: "):]
        if plan.rect is None:
            return None
        if not planes.one_size():
            return "the frame's planes differ in size"
        self._release_dead()
        fset = planes.blend_set()
        self._dead_sets.append(fset)
        ref = None
        if plan.source is not None:
            slot = refs[plan.source]
            if plan.ref_zero:
                ref = host.DeviceCanvas.create(ctx, plan.ref_types, info.height, info.width)
                self._dead_sets.append(ref)
            elif plan.aliased:
                ref = cv
            elif self._is_set(slot):
                ref = slot
            else:  # a host list (saved before the colour transform): its casts persist in the list, as today; then it goes up
                for which, plane, depth in plan.casts:
                    if which == "r":
                        slot[plane] = self._to_float(slot[plane], depth)
                ref = host.DeviceCanvas.fromArrays(ctx, slot)
                self._dead_sets.append(ref)
        for which, plane, depth in plan.casts:
            target = {"c": cv, "f": fset, "r": ref}[which]
            target.cast(plane, depth)  # (nothing happens to the float planes of an uploaded list)
        host.canvas_blend(cv, fset, ref, plan.rect, plan.chans)
        return None

    def _blend_frame(self, fr, frame_buffers, colors_frame, first=0):
        """JXLCodestreamDecoder.blendFrame + blendBuffers (:424-537). first: the first canvas channel to blend (the colour
        planes of a device_output frame are not on the canvas)"""
        info = self.info
        ih, iw = info.height, info.width
        colors = 1 if info.colour_space == CE_GRAY else 3
        py, px = min(max(fr.y0, 0), ih), min(max(fr.x0, 0), iw)       # Point.inBounds
        fy, fx = py - fr.y0, px - fr.x0
        ly, lx = fr.y0 + fr.height * fr.upsampling, fr.x0 + fr.width * fr.upsampling  # bounds after Frame.upsample()
        bh, bw = min(ly, ih) - py, min(lx, iw) - px
        if bh <= 0 or bw <= 0:
            return
        has_extra = info.num_extra > 0
        for c in range(first, len(self.canvas)):
            if c >= colors:
                e = c - colors
                mode, alpha_ch, clamp, source = fr.ec_blend_mode[e], fr.ec_blend_alpha[e], fr.ec_blend_clamp[e], fr.ec_blend_source[e]
            else:
                mode, alpha_ch, clamp, source = fr.blend_mode, fr.blend_alpha, fr.blend_clamp, fr.blend_source
            ref_buffers = self.reference[source]
            self._blend_buffers(c, frame_buffers, ref_buffers, (py, px), (fy, fx), (py, px), (bh, bw), colors_frame,
                                mode, alpha_ch, bool(clamp), patch=False, canvas_list=self.canvas)

    def _depth_of(self, idx):
        colors = 1 if self.info.colour_space == CE_GRAY else 3
        return self.info.bits_per_sample if idx < colors else self.info.ec_bits[idx - colors]

    _to_float = staticmethod(_to_float)

    def _blend_buffers(self, idx, frame_buffers, ref_buffers, patch_start, frame_off, ref_off, size, frame_colors, mode,
                       alpha_channel, clamp, patch, canvas_list):
        info = self.info
        colors = 1 if info.colour_space == CE_GRAY else 3
        fb_idx = (1 if idx == 0 else idx + 2) if colors != frame_colors else idx
        ex = idx - colors
        is_extra = ex >= 0
        has_extra = info.num_extra > 0
        is_alpha = is_extra and info.ec_type[ex] == 0
        premult = has_extra and bool(info.ec_alpha_associated[alpha_channel])
        depth = self._depth_of(idx)
        canvas = canvas_list[idx]
        frame_buffer = frame_buffers[fb_idx]
        if canvas.dtype != frame_buffer.dtype:
            frame_buffer = frame_buffers[fb_idx] = self._to_float(frame_buffer, depth)
            canvas = canvas_list[idx] = self._to_float(canvas, depth)
        rect = (size[0], size[1], patch_start[0], patch_start[1], frame_off[0], frame_off[1], ref_off[0], ref_off[1])
        if mode == abi.BLEND_REPLACE and not patch or (ref_buffers is None and mode == abi.BLEND_ADD and not patch):
            canvas_list[idx] = self.backend.blend(abi.BLEND_REPLACE, canvas, frame_buffer, None, rect)
            return
        if ref_buffers is None:
            if patch:
                return
            ref_buffers = [None] * len(canvas_list)
        if ref_buffers[idx] is None:
            ref_buffers[idx] = np.zeros(canvas.shape, canvas.dtype)
        ref_alpha = frame_alpha = None
        a_idx_ref, a_idx_frame = colors + alpha_channel, frame_colors + alpha_channel
        pmode = mode
        if patch:  # Patch blend modes 0..7 -> frame blend modes (JXLCodestreamDecoder.java:478-494)
            if mode == 0:
                return
            pmode, below = {5: (abi.BLEND_BLEND, True), 6: (abi.BLEND_MULADD, False), 7: (abi.BLEND_MULADD, True)}.get(mode, (mode - 1, False))
        else:
            below = False
        if has_extra and mode in (abi.BLEND_BLEND, abi.BLEND_MULADD):
            a_depth = info.ec_bits[alpha_channel]
            if mode == abi.BLEND_BLEND:
                if ref_buffers[a_idx_ref] is None:
                    ref_buffers[a_idx_ref] = np.zeros(canvas.shape, F)
                ref_buffers[a_idx_ref] = self._to_float(ref_buffers[a_idx_ref], a_depth)
            frame_buffers[a_idx_frame] = self._to_float(frame_buffers[a_idx_frame], a_depth)
            if not patch:
                # :455 casts the very object :420 named when this channel is that alpha, so :461 sees a float frame plane. (Under
                # computePatches the canvas is that object too, :248; patch_type_plan and the calls here still keep the array they
                # took before the cast -- DESIGN.md section 3, open.)
                frame_buffer = frame_buffers[fb_idx]
        if has_extra:
            ref_alpha = ref_buffers[a_idx_ref]
            frame_alpha = frame_buffers[a_idx_frame]
        should_cast = mode == abi.BLEND_MULT or (mode == abi.BLEND_BLEND and has_extra) or \
            (mode == abi.BLEND_MULADD and has_extra and not is_alpha)
        ref_buffer = ref_buffers[idx]
        if should_cast or ref_buffer.dtype != frame_buffer.dtype:
            frame_buffer = frame_buffers[fb_idx] = self._to_float(frame_buffer, depth)
            canvas = canvas_list[idx] = self._to_float(canvas, depth)
            ref_buffer = ref_buffers[idx] = self._to_float(ref_buffer, depth)
        if patch and pmode == abi.BLEND_REPLACE:  # raw mode 1: the switch of :493-512 has no case for it, behind the casts
            raise InvalidBitstreamException("Illegal blend mode")
        old_buffer, new_buffer = (ref_buffer, frame_buffer) if below else (frame_buffer, ref_buffer)
        fa = frame_alpha if (frame_alpha is not None and frame_alpha.dtype == np.float32) else None
        ra = ref_alpha if (ref_alpha is not None and ref_alpha.dtype == np.float32) else None
        kw = dict(refAlpha=ra, isAlpha=is_alpha, hasExtra=has_extra, clamp=clamp, premult=premult)
        if patch and below and tuple(ref_off) != tuple(patch_start):
            canvas_list[idx] = self._blend_live(pmode, canvas, old_buffer, rect, fa, a_idx_frame == fb_idx, kw)
            return
        canvas_list[idx] = self.backend.blend(pmode, canvas, old_buffer, new_buffer, rect, frameAlpha=fa, **kw)

    def _blend_live(self, pmode, canvas, frame, rect, frame_alpha, alpha_is_canvas, kw):
        """A below patch mode away from its own pixel: the blend function's `ref` is the frame plane, which in the reference IS
        the canvas, read at patch.bounds.origin while the position's rectangle is written; where the two overlap, later pixels
        of its loops read what earlier ones stored. backend.blend takes canvas and `ref` as two arrays, so the rectangle goes
        through it in pieces no pixel of which reads a pixel of the same piece, in raster order, each piece reading the canvas
        the pieces before it left: whole when the reads lie ahead of the writes, in bands of as many rows as the shift when
        they lie in earlier rows, in column strips of the shift's width when they lie earlier in the same rows."""
        h, w, py, px, fy, fx, ry, rx = rect
        dy, dx = ry - py, rx - px
        if dy > 0 or (dy == 0 and dx > 0) or h <= 0 or w <= 0:
            pieces = [(0, 0, h, w)]
        elif dy < 0:
            pieces = [(y, 0, min(-dy, h - y), w) for y in range(0, h, -dy)]
        else:
            pieces = [(0, x, h, min(-dx, w - x)) for x in range(0, w, -dx)]
        for y, x, ph, pw in pieces:
            fa = canvas if (alpha_is_canvas and frame_alpha is not None) else frame_alpha
            canvas = self.backend.blend(pmode, canvas, frame, canvas, (ph, pw, py + y, px + x, fy + y, fx + x, ry + y, rx + x),
                                        frameAlpha=fa, **kw)
        return canvas

    def _patches(self, fr, frame_buffers, frame_colors):
        """JXLCodestreamDecoder.computePatches (:204-254)"""
        info = self.info
        colors = 1 if info.colour_space == CE_GRAY else 3
        for i in range(fr.num_patches):
            p = self.fe.patch(i)
            if p["ref"] > 3:
                raise InvalidBitstreamException("Patch out of range")
            ref = self.reference[p["ref"]]
            if ref is None:
                continue
            if p["y0"] + p["h"] > ref[0].shape[0] or p["x0"] + p["w"] > ref[0].shape[1]:
                raise InvalidBitstreamException("Patch too large")
            for j in range(p["positions"].shape[0]):
                y0, x0 = int(p["positions"][j, 0]), int(p["positions"][j, 1])
                if y0 < 0 or x0 < 0 or p["h"] + y0 > frame_buffers[0].shape[0] or p["w"] + x0 > frame_buffers[0].shape[1]:
                    raise InvalidBitstreamException("Patch size out of bounds")
                for d in range(colors + info.num_extra):
                    c = 0 if d < colors else d - colors + 1
                    mode, alpha, clamp = (int(v) for v in p["blend"][j, c])
                    if mode == 0:
                        continue
                    if _patch_upsampling_mismatch(info, fr, mode, c):
                        raise InvalidBitstreamException("Alpha channel upsampling mismatch during patches")
                    self._blend_buffers(d, frame_buffers, ref, (y0, x0), (y0, x0), (p["y0"], p["x0"]), (p["h"], p["w"]),
                                        frame_colors, mode, alpha, bool(clamp), patch=True, canvas_list=frame_buffers)

    def _patches_device(self, fr, planes):
        """computePatches as one backend call per segment of patch_type_plan on `planes` (FramePlanes). Where its colours can be
        resident, a segment whose colour planes are float runs on them (jxl_planes_patches) and one whose colour planes are
        integer on the host arrays (jxl_stage_patches); where they cannot, the stage entry only. Leaves the planes and
        self.reference[...] as _patches would: values, dtypes, absent reference planes replaced by zero planes. False (nothing
        touched): the plan holds an application the in-place launch cannot replay; the caller runs _patches."""
        info, be = self.info, self.backend
        f32 = np.dtype(np.float32)
        colors, buffers, shape = planes.colors, planes.host, planes.shape
        n_chan = colors + info.num_extra
        typed = [np.broadcast_to(np.zeros((), t), shape) for t in planes.dtypes[:n_chan]]  # (the plan reads dtype and shape only)
        plan = patch_type_plan(info, [self.fe.patch(i) for i in range(fr.num_patches)], typed, self.reference, colors, fr)
        st = self.stats[-1]["patches"] = dict(path="none", positions=len(plan.pos), applications=len(plan.calls), segments=len(plan.segments))
        if not plan.calls:
            return True
        if not plan.gather:
            st["path"] = "blend calls (a below mode reads the frame off its own pixel)"
            return False
        is_alpha = [t == 0 for t in info.ec_type[:info.num_extra]]
        assoc = [bool(v) for v in info.ec_alpha_associated[:info.num_extra]]
        ref_shapes = [None if self.reference[k] is None else tuple(self.reference[k][0].shape) for k in range(4)]
        call_pos = np.array([c["pos"] for c in plan.calls]), np.array([c["d"] for c in plan.calls])

        def seg_blend(seg):  # the blend rows with the modes of the applications outside the segment set to 0
            if len(plan.segments) == 1:
                return plan.blend
            b = plan.blend.copy()
            b[:, :, 0] = 0
            sl = slice(seg["first"], seg["last"] + 1)
            b[call_pos[0][sl], call_pos[1][sl], 0] = plan.blend[call_pos[0][sl], call_pos[1][sl], 0]
            return b

        def code(dt):
            return -1 if dt is None else 0 if dt == f32 else 1
        if len(plan.segments) > 1:  # every segment is checked before the first one runs (a single one: the entry does it)
            from . import host as _host
            for seg in plan.segments:
                rtypes = [[-1] * n_chan if k not in seg["ref"] or self.reference[k] is None else
                          [-1 if (k, n) in plan.created or self.reference[k][n] is None else code(seg["ref"][k][n]) for n in range(n_chan)]
                          for k in range(4)]
                _host.patch_bins(plan.pos, seg_blend(seg), colors, is_alpha, assoc, shape[0], shape[1],
                                             [code(t) for t in seg["frame"]], ref_shapes, rtypes)
        paths = set()
        for seg in plan.segments:
            # blendBuffers' casts, hoisted to the segment's entry (the reference's ImageBuffer.castToFloat: _to_float)
            resident = planes.resident and all(seg["frame"][c] == f32 for c in range(3))
            if not resident:
                planes.to_host()
            for n in range(n_chan):
                if planes.rp is not None and n < 3:
                    continue
                if buffers[n].dtype != seg["frame"][n]:
                    if seg["frame"][n] != f32:
                        raise ValueError("blend: this mode works on float samples")  # (blendBlend on an int alpha plane that is its own alpha)
                    buffers[n] = self._to_float(buffers[n], self._depth_of(n))
                buffers[n] = np.ascontiguousarray(buffers[n])
            for k, types in seg["ref"].items():
                lst = self.reference[k]
                for n in range(n_chan):
                    if lst[n] is not None and types[n] == f32 and lst[n].dtype != f32:
                        lst[n] = self._to_float(lst[n], self._depth_of(n))
            ref = [self.reference[k] if k in seg["ref"] else None for k in range(4)]
            blend = seg_blend(seg)
            if resident:
                planes.to_device().patches(buffers[3:], ref, plan.pos, blend, is_alpha, assoc)
                paths.add("resident planes")
            else:
                be.patches(buffers, ref, plan.pos, blend, colors, is_alpha, assoc)
                paths.add("stage entry")
        st["path"] = " + ".join(sorted(paths))
        # what the casts and `new ImageBuffer`s of blendBuffers leave behind in planes no application used
        for n in range(n_chan):
            if not (planes.rp is not None and n < 3) and buffers[n].dtype != plan.frame_types[n]:
                buffers[n] = self._to_float(buffers[n], self._depth_of(n))
        for k, types in plan.ref_types.items():
            lst = self.reference[k]
            for n in range(n_chan):
                if lst[n] is None and types[n] is not None:
                    lst[n] = np.zeros(shape, types[n])
                elif lst[n] is not None and lst[n].dtype != types[n]:
                    lst[n] = self._to_float(lst[n], self._depth_of(n))
        return True

    def _patches_sets(self, fr, planes):
        """device_patch_sets: computePatches on plane sets. patch_type_plan, handed the sets' dtypes, says which casts and
        which segments; per segment the hoisted casts of the frame's and the slots' planes are ONE jxl_canvas_cast_planes call
        and the applications ONE jxl_canvas_patches call. The frame's planes become a set here (FramePlanes.adopt_set). Leaves
        the planes, self.reference[...] and the canvas' tags as _patches would leave them. Returns None, or -- with nothing
        touched -- the reason why the canvas lands and the stage runs as without the switch."""
        info, be = self.info, self.backend
        host, ctx = be.host, be.ctx
        f32 = np.dtype(np.float32)
        colors, shape = planes.colors, tuple(planes.shape)
        n_chan = colors + info.num_extra
        refs = self.reference
        if n_chan > abi.CANVAS_MAX_PLANES:
            return "more than 16 planes"
        if not planes.one_size():
            return "the frame's planes differ in size"
        if any(r is not None and len(r) != n_chan for r in refs):
            return "a reference slot with another plane count"
        # the plan reads dtypes and shapes only: stand-ins for everything that is on the device
        typed = [np.broadcast_to(np.zeros((), t), shape) for t in planes.dtypes[:n_chan]]
        view = [r._stand_ins(len(r)) if self._is_set(r) else r for r in refs]
        plan = patch_type_plan(info, [self.fe.patch(i) for i in range(fr.num_patches)], typed, view, colors, fr)
        if not plan.gather:
            return "a below mode reads the frame off its own pixel"
        self.stats[-1]["patches"] = dict(path="plane sets", positions=len(plan.pos), applications=len(plan.calls), segments=len(plan.segments))
        if not plan.calls:
            return None
        is_alpha = [t == 0 for t in info.ec_type[:info.num_extra]]
        assoc = [bool(v) for v in info.ec_alpha_associated[:info.num_extra]]
        call_pos = np.array([c["pos"] for c in plan.calls]), np.array([c["d"] for c in plan.calls])

        def seg_blend(seg):  # the blend rows with the modes of the applications outside the segment set to 0
            if len(plan.segments) == 1:
                return plan.blend
            b = plan.blend.copy()
            b[:, :, 0] = 0
            sl = slice(seg["first"], seg["last"] + 1)
            b[call_pos[0][sl], call_pos[1][sl], 0] = plan.blend[call_pos[0][sl], call_pos[1][sl], 0]
            return b
        resident = planes.rp is not None
        used = sorted(plan.ref_types)  # the slots some applied patch names
        if len(plan.segments) > 1:  # every segment is checked before the first one runs (a single one: the entry does it)
            for seg in plan.segments:
                fs = abi.CanvasShape()
                fs.n, fs.h, fs.w = n_chan, shape[0], shape[1]
                for n in range(n_chan):
                    fs.types[n] = host._plane_code(seg["frame"][n])
                rs = [None] * 4
                for k in (k for k in used if k in seg["ref"]):
                    rs[k] = abi.CanvasShape()
                    rs[k].n, rs[k].h, rs[k].w = n_chan, view[k][0].shape[0], view[k][0].shape[1]
                    for n in range(n_chan):  # (a plane still absent reads as zeros of whatever type: the frame plane's)
                        rs[k].types[n] = host._plane_code(seg["ref"][k][n] if seg["ref"][k][n] is not None else seg["frame"][n])
                host.canvas_patches_check(plan.pos, seg_blend(seg), colors, is_alpha, assoc, fs, rs, colorsResident=resident)
        fset = planes.adopt_set()
        # the slots as sets: a slot that is a set (the canvas itself included) is read where it is; a host list goes up as a
        # temporary set for this frame, its absent planes as zeros of the type their first use gives them
        slot_set, temp = {}, []
        try:
            for k in used:
                r = refs[k]
                if self._is_set(r):
                    slot_set[k] = r
                    continue
                same = next((j for j in slot_set if refs[j] is r), None)
                if same is not None:
                    slot_set[k] = slot_set[same]
                    continue
                first_type = []
                for n in range(n_chan):
                    seen = [seg["ref"][k][n] for seg in plan.segments if k in seg["ref"] and seg["ref"][k][n] is not None]
                    first_type.append(r[n].dtype if r[n] is not None and tuple(r[n].shape) == tuple(r[0].shape) else seen[0] if seen else f32)
                ts = host.DeviceCanvas.create(ctx, first_type, *r[0].shape)
                temp.append(ts)
                for n in range(n_chan):  # (an all-zero plane of another size -- one a frame before created at ITS size -- reads as zeros)
                    if r[n] is not None and tuple(r[n].shape) == tuple(r[0].shape):
                        ts.upload(n, r[n])
                    elif r[n] is not None and r[n].any():
                        raise ValueError("planes of one reference slot differ in size")
                slot_set[k] = ts

            def casts_to(frame_types, ref_types):
                """the planes whose tags differ from the given types, each once (aliased slots are one set)"""
                items, named = [], set()
                for n in range(n_chan):
                    if not (resident and n < 3) and fset.dtypes[n] != frame_types[n]:
                        if frame_types[n] != f32:
                            raise ValueError("blend: this mode works on float samples")
                        items.append((fset, n, self._depth_of(n)))
                for k, types in ref_types.items():
                    s_ = slot_set.get(k)
                    for n in range(n_chan):
                        if s_ is not None and types[n] == f32 and s_.dtypes[n] != f32 and (id(s_), n) not in named:
                            named.add((id(s_), n))
                            items.append((s_, n, self._depth_of(n)))
                return items
            for seg in plan.segments:
                items = casts_to(seg["frame"], seg["ref"])
                if items:
                    host.canvas_cast_planes(ctx, items)
                host.canvas_patches(fset, [slot_set.get(k) if k in seg["ref"] else None for k in range(4)], plan.pos, seg_blend(seg),
                                    colors, is_alpha, assoc, colorsResident=resident)
            # what the casts and `new ImageBuffer`s of blendBuffers leave behind in planes no application used
            items = casts_to(plan.frame_types, plan.ref_types)
            if items:
                host.canvas_cast_planes(ctx, items)
        finally:
            self._release_dead()
            self._dead_sets.extend(temp)  # (released once the stream has passed the launches that read them)
        for k in used:  # a host list keeps its casts and its new planes in the list
            lst, types = refs[k], plan.ref_types[k]
            if self._is_set(lst):
                continue
            for n in range(n_chan):
                if lst[n] is None and types[n] is not None:
                    lst[n] = np.zeros(shape, types[n])
                elif lst[n] is not None and lst[n].dtype != types[n]:
                    lst[n] = self._to_float(lst[n], self._depth_of(n))
        return None

    # -- the image as a device plane set (device_image) -----------------------------------------------------------
    @staticmethod
    def _one_plan_chain_rule(fr, kinds, chain=None):
        """what device_image's "modular frame" route and device_frames ask of the frame-level stream: a Modular frame whose
        chain is one plan of the Modular context. None, or the condition that fails. chain: with device_chains the transform
        list itself (frontend.transforms()), else None"""
        if fr.encoding != MODULAR:
            return "not a Modular frame"
        R, P, S = frontend.TRANSFORM_RCT, frontend.TRANSFORM_PALETTE, frontend.TRANSFORM_SQUEEZE
        if chain is not None:  # jxl_modular_begin_chain: every chain but one
            if any(t["kind"] == P and t["nb_deltas"] > 0 and t["d_pred"] == 6 for t in chain):
                return "a Palette with weighted-predictor deltas"
            return None
        if P in kinds:
            return "a Palette in the frame-level chain"
        if kinds not in ([], [R], [S], [R, S]):
            return "a frame-level chain that is not one plan ([], [RCT], [Squeeze] or [RCT, Squeeze])"
        return None

    @staticmethod
    def _int_rgb_planes_rule(info, fr, colors, colors_img):
        """the other half the two routes share: three int32 colour planes that reach the blend as decodeFrame leaves them, in a
        set. None, or the condition that fails"""
        if fr.gab or fr.epf_iters > 0 or fr.do_ycbcr:
            return "a restoration filter or YCbCr"
        if info.xyb_encoded:
            return "an XYB image"
        if info.exp_bits != 0 or colors != 3 or colors_img != 3:
            return "colour planes that are not three int32 planes"
        if 3 + info.num_extra > abi.CANVAS_MAX_PLANES or fr.num_modular_channels < 1:
            return "more planes than a set holds"
        return None

    def _modular_frame_route(self, fr, colors, colors_img):
        """None when the frame qualifies for device_image's "modular frame" route, else the first condition that fails. The
        chain is looked at first after the encoding: it is what tells the committed images apart."""
        info = self.info
        chain = self.fe.transforms() if fr.encoding == MODULAR else []
        why = self._one_plan_chain_rule(fr, [t["kind"] for t in chain], chain if self.device_chains else None)
        if why is not None:
            return why
        if fr.type != REGULAR_FRAME or not fr.is_last or fr.lf_level != 0:
            return "not a regular last frame"
        if self._is_set(self.canvas) or self.canvas[0] is not None or fr.x0 != 0 or fr.y0 != 0:
            return "not the first frame on the canvas, at its origin"
        if fr.upsampling != 1 or any(fr.ec_upsampling[i] != 1 for i in range(info.num_extra)) or \
                fr.width != info.width or fr.height != info.height:
            return "upsampled, or not of the image's size"
        if fr.blend_mode != abi.BLEND_REPLACE or any(fr.ec_blend_mode[i] != abi.BLEND_REPLACE for i in range(info.num_extra)):
            return "a blend mode other than REPLACE"
        if fr.num_patches or fr.has_splines or fr.has_noise:
            return "patches, splines or noise"
        return self._int_rgb_planes_rule(info, fr, colors, colors_img)

    @staticmethod
    def frame_set_rule(info, fr, kinds, traced=False, chain=None, patch_sets=False):
        """device_frames: None when the header fields say that a frame can reach the resident canvas as a plane set made from
        the Modular context (_modular_frame_set), else the first condition that fails. info: the image header; fr: the frame
        header; kinds: the kinds of the frame-level transform chain in bitstream order; traced: a `trace` listener is set.
        Position, blend modes, is_last, the reference slots, noise and splines are free. With device_chains, chain: the
        transform list itself, and patch_sets: patch_sets_rule holds for the frame -- its patches then run on the set."""
        why = JXLDecoder._one_plan_chain_rule(fr, kinds, chain)
        if why is not None:
            return why
        if fr.type not in (REGULAR_FRAME, SKIP_PROGRESSIVE) or fr.lf_level != 0:
            return "not a regular or skip-progressive frame of LF level 0"
        if fr.num_patches and not (chain is not None and patch_sets):
            return "patches"
        colors_img = 1 if info.colour_space == CE_GRAY else 3
        colors = 3 if info.xyb_encoded else colors_img  # (_colors of a Modular frame)
        why = JXLDecoder._int_rgb_planes_rule(info, fr, colors, colors_img)
        if why is not None:
            return why
        save = (fr.save_as_reference != 0 or fr.duration == 0) and not fr.is_last
        if save and fr.save_before_ct:
            return "saved before the colour transform"
        if any(fr.ec_upsampling[i] != fr.upsampling for i in range(info.num_extra)):
            return "an extra channel whose upsampling is not the colours'"
        if fr.upsampling not in (1, 2, 4, 8):
            return "an upsampling factor other than 1, 2, 4 or 8"
        if traced:
            return "a trace listener is set"
        return None

    def _frame_set_route(self, fr, direct):
        """device_frames: whether the frame reaches the canvas as a plane set; stats[k]["frame"] says "device set (modular)"
        or "host: <why not>". The switch acts only while the canvas is a device set; the header's part is frame_set_rule"""
        if not self.device_frames:
            why = "device_frames is off"
        elif not self.device_canvas:
            why = "device_canvas is off"
        elif direct:
            why = "device_output's direct path"
        elif self._landed is not None:
            why = "the canvas has landed (%s)" % self._landed
        else:
            chain = self.fe.transforms() if fr.encoding == MODULAR else []
            colors_img = 1 if self.info.colour_space == CE_GRAY else 3
            patch_sets = self.device_chains and bool(fr.num_patches) and self.patch_sets_rule(
                self.device_patch_sets, self.device_canvas, self.device_patches, True, colors_img, self._colors(fr)) is None
            why = self.frame_set_rule(self.info, fr, [t["kind"] for t in chain], self.trace is not None,
                                      chain if self.device_chains else None, patch_sets)
            self._patch_sets = why is None and patch_sets  # (the patch stage of _chained_tail looks here)
        self.stats[-1]["frame"] = "device set (modular)" if why is None else "host: " + why
        return why is None

    def _direct_frame(self, fr, colors):
        """device_output: this frame is the image (the conditions of __init__'s docstring that the header settles)"""
        info = self.info
        return self.device_output and getattr(self.backend, "resident", False) and colors == 3 and info.colour_space != CE_GRAY and \
            fr.type == REGULAR_FRAME and bool(fr.is_last) and fr.lf_level == 0 and not self._is_set(self.canvas) and \
            self.canvas[0] is None and fr.y0 == 0 and fr.x0 == 0 and fr.width * fr.upsampling == info.width and \
            fr.height * fr.upsampling == info.height and fr.blend_mode == abi.BLEND_REPLACE

    @staticmethod
    def patch_sets_rule(device_patch_sets, device_canvas, device_patches, canvas_on_device, colors_image, colors_frame):
        """device_patch_sets: None when the switch acts on a frame with patches -- the frame does not land the canvas and its
        patches run on plane sets (_patches_sets) -- else the first condition that failed. canvas_on_device: nothing has landed
        the canvas so far; colors_image / colors_frame: the colour counts of the image and of the frame"""
        if not device_patch_sets:
            return "device_patch_sets is off"
        if not device_canvas:
            return "device_canvas is off"
        if not device_patches:
            return "device_patches is off"
        if not canvas_on_device:
            return "the canvas has landed"
        if colors_image != 3:
            return "one-colour image"
        if colors_frame != colors_image:
            return "a frame of another colour count"
        return None

    def _canvas_route(self, fr, direct):
        """device_canvas: whether this frame meets the canvas as a plane set. The canvas lives in one from the first frame that
        reaches it until something lands it; stats[k]["canvas"] tells. device_output's direct frame never sees a canvas"""
        on = self.device_canvas and not direct
        if on and self._landed is None and self.info.colour_space == CE_GRAY:
            self._landed = "one-colour image"
        if on and self._landed is None and len(self.canvas) > abi.CANVAS_MAX_PLANES:
            self._landed = "more than 16 planes"  # (no set holds them: jxl_canvas_create would refuse before blend_type_plan is asked)
        self._patch_sets = False
        if on and fr.num_patches and fr.type != LF_FRAME:
            # blendBuffers casts a patch's reference in place: no set stays up, unless the patches run on the sets themselves
            colors_img = 1 if self.info.colour_space == CE_GRAY else 3
            self._patch_sets = self.patch_sets_rule(self.device_patch_sets, self.device_canvas, self.device_patches,
                                                    self._landed is None, colors_img, self._colors(fr)) is None
            if not self._patch_sets:
                self._land("a frame with patches")
        self.stats[-1]["canvas"] = "host" if not on else "device" if self._landed is None else "landed: " + self._landed
        return on and self._landed is None

    def _modular_plan_run(self):
        """the frame-level stream's pending chain as ONE plan of the Modular context: the encoded channels go up once, from the
        front-end's own buffers (jxl_modular_begin), and the plan is queued. Returns the host.ModularStream"""
        info, be, fe = self.info, self.backend, self.fe
        host = be.host
        chans = [fe.modular_channel(i, copy=False)[0] for i in range(fe.modular_channel_count())]
        steps, rct_type, rct_begin = [], -1, 0
        for t in fe.transforms():
            if t["kind"] == frontend.TRANSFORM_SQUEEZE:
                steps = t["steps"]
            else:
                rct_type, rct_begin = t["rct_type"], t["begin_c"]
        if self.device_chains:  # the whole list, whatever it holds (jxl_modular_begin_chain)
            ms = host.ModularStream(be.ctx, chans, transforms=fe.transforms(), bitDepth=info.bits_per_sample)
        else:
            ms = host.ModularStream(be.ctx, chans, steps, rctType=rct_type, rctBegin=rct_begin)
        ms.run()
        host._bus(be.ctx, up=sum(c.nbytes for c in ms.channels))
        n = 3 + info.num_extra
        if be.ctx.lib.jxl_modular_out_count(be.ctx.h) != n:
            raise InvalidBitstreamException("the frame-level stream does not hold the frame's %d channels" % n)
        if self.device_chains:
            self._chain_plan = ms  # (_chain_stats reads the plan's counters once something has read its outputs)
        return ms

    def _chain_stats(self):
        """device_chains: stats[k]["chain"] of the frame whose plan _modular_plan_run queued, once its set has been made"""
        ms, self._chain_plan = getattr(self, "_chain_plan", None), None
        if ms is not None:
            fused, steps, redone = self.backend.host.lastPaletteRun(self.backend.ctx)
            self.stats[-1]["chain"] = dict(kinds=[t["kind"] for t in ms.transforms], runs=dict(fused=fused, steps=steps, redone=redone))

    def _modular_frame_set(self, fr, save):
        """device_frames: the frame's planes after Frame.upsample .. performColorTransforms (JXLCodestreamDecoder.java:628-637)
        as a plane set made from the Modular context, with the types the default path's buffers have at the blend"""
        info, be = self.info, self.backend
        host = be.host
        self._modular_plan_run()
        f32, k = np.dtype(np.float32), fr.upsampling
        on_sets = bool(fr.num_patches)  # device_chains: the patch stage takes the set as it is, the stages behind it visit the planes
        tail = bool(fr.has_noise or fr.has_splines) and not on_sets

        def inv_max(depth):  # ImageBuffer.castToFloat's factor (ImageBuffer.java:112-127), as _to_float forms it
            return float(F(F(1) / F((1 << depth) - 1)))
        if k > 1:  # Frame.performUpsampling casts every plane with its own depth first (Frame.java:226-228); a float plane stays
            desc = [(c, -1, f32, inv_max(info.bits_per_sample)) for c in range(3)]
            desc += [(3 + i, -1, f32, 1.0 if info.ec_exp_bits[i] != 0 else inv_max(info.ec_bits[i])) for i in range(info.num_extra)]
            fset = host.DeviceCanvas.fromModularUp(be.ctx, fr.height, fr.width, desc, k, self._up_weights(k))
        else:
            # the colour planes are float exactly where the default path's are: every device stage casts them (Frame.java:796)
            desc = [(c, -1, f32, inv_max(info.bits_per_sample)) if tail else (c, -1, np.int32, 1.0) for c in range(3)]
            desc += [(3 + i, -1, f32 if info.ec_exp_bits[i] != 0 else np.int32, 1.0) for i in range(info.num_extra)]
            fset = host.DeviceCanvas.fromModular(be.ctx, fr.height, fr.width, desc)
        self._chain_stats()
        planes = FramePlanes(be, info, [None] * 3, 3, fset=fset)
        self.stats[-1]["plane_moves"] = planes.moves
        if on_sets:  # the patches on the set, then the stages as behind any adopted set; a refusal has landed everything
            try:
                self._chained_tail(fr, planes, save, True, keep=True, upsampled=True, adopted=True)
            except Exception:
                if planes.set is not None:
                    planes.set.release()
                raise
        elif tail:  # noise and splines run on the resident planes between jxl_canvas_to_planes and jxl_canvas_take_planes
            try:
                planes.leave_set()
                self._chained_tail(fr, planes, save, True, keep=True, upsampled=True)
                planes.rejoin_set()
            except Exception:
                fset.release()
                raise
        return planes

    def _modular_frame_image(self, fr, bus0):
        """device_image, route "modular frame": the encoded channels up once, one plan, one set; nothing comes down"""
        info, be = self.info, self.backend
        host = be.host
        self.visibleFrames += 1
        self.invisibleFrames = 0
        ms = self._modular_plan_run()
        n = 3 + info.num_extra
        if self.trace is not None:  # a listener wants the samples: copies come down, the result stays
            self._trace("mod", ms.getDecodedBuffer(), False)
        planes = [(c, -1, np.int32, 1.0) for c in range(3)]
        planes += [(3 + i, -1, np.float32 if info.ec_exp_bits[i] != 0 else np.int32, 1.0) for i in range(info.num_extra)]
        cv = host.DeviceCanvas.fromModular(be.ctx, fr.height, fr.width, planes)
        self._chain_stats()
        if self.trace is not None:
            self._trace("xyb", [cv.download(c) for c in range(n)], False)
        if info.orientation != 1:
            cv.orient(info.orientation)
        self.stats[-1].update(image="device set (modular frame)", output="device", canvas="host",
                              frame="host: device_image's modular frame route" if self.device_frames else "host: device_frames is off")
        self._bus_since(bus0)
        if self.device_palette:
            self.stats[-1]["palette"] = []
        return JXLImage([None] * n, info, be, planeSet=cv)

    # -- the decode loop (JXLCodestreamDecoder.decode :546-677) ----------------------------------------------------
    def _check_switches(self):
        be = self.backend
        if self.device_palette and not hasattr(be, "palette"):
            raise RuntimeError("device_palette needs a backend with `palette`")
        if self.device_image and not hasattr(be, "ctx"):
            raise RuntimeError("device_image needs a backend with a device context")
        if self.device_canvas and not hasattr(be, "ctx"):
            raise RuntimeError("device_canvas needs a backend with a device context")
        if self.region is not None and self.trace is not None:
            raise ValueError("region cannot be combined with a trace listener")
        if self.downsample == 8:
            if self.trace is not None:
                raise ValueError("downsample=8 cannot be combined with a trace listener")
            if not hasattr(be, "lf_image"):
                raise RuntimeError("downsample=8 needs a backend with `lf_image`")

    def _hooks(self):
        be = self.backend
        return be.squeeze, be.rct, be.palette if self.device_palette else None

    def _next_frame(self):
        """the next frame header from the front-end, with a fresh stats row; None at the end of the stream. With device_image
        or device_frames the frame-level transforms wait until the route is known (_pending_transforms)"""
        if self.device_palette and hasattr(self.backend, "palette_log"):
            del self.backend.palette_log[:]
        try:
            if self.device_image or self.device_frames:
                self.fe.set_defer_transforms(True)
            fr = self.fe.next_frame(*self._hooks())
        except frontend.FrontendError as e:
            raise self._map(e)
        if fr is not None:
            self.frames_decoded += 1
            self.stats.append(dict(encoding="vardct" if fr.encoding == VARDCT else "modular", width=fr.width, height=fr.height,
                                   groups=fr.num_groups, passes=fr.num_passes, output="host"))
        return fr

    def _pending_transforms(self, fr, frame_set):
        """a frame that makes no plan of its deferred transforms runs them through the usual hooks and goes on exactly as
        without the switches; then what every frame's header owes: the palette log, the LF level"""
        if (self.device_image or self.device_frames) and not frame_set:
            try:
                self.fe.apply_transforms(*self._hooks())
            except frontend.FrontendError as e:
                raise self._map(e)
        if self.device_palette:
            self.stats[-1]["palette"] = [dict(e) for e in getattr(self.backend, "palette_log", [])]
        if fr.flags & FLAG_USE_LF_FRAME and self.lfBuffer[fr.lf_level] is None:
            raise InvalidBitstreamException("LF Level too large")  # JXLCodestreamDecoder.java:613-614

    def _host_frame(self, fr, colors, keep):
        """Frame.decodeFrame and what follows it on the padded planes: the VarDCT call or the Modular channels, the Modular
        frame's Gab / EPF, the LF-frame bookkeeping, the crop to the frame's bounds. keep: the colours of a VarDCT frame stay on
        the device for the caller's sake (device_output, device_canvas). Returns (FramePlanes, whether XYB has been inverted)"""
        info, be = self.info, self.backend
        resident = getattr(be, "resident", False) and colors == 3  # row f4: the stages after decodeFrame chained on the device
        simple = fr.upsampling == 1 and not fr.num_patches and not fr.has_splines and not fr.has_noise and \
            not (fr.save_before_ct and not fr.is_last)
        buffers = []
        for c in range(colors + info.num_extra):
            if c < colors:
                is_float = bool(info.xyb_encoded) or fr.encoding == VARDCT or info.exp_bits != 0
            else:
                is_float = info.ec_exp_bits[c - colors] != 0
            buffers.append(None if c < 3 and fr.encoding == VARDCT else np.zeros((fr.padded_height, fr.padded_width), F if is_float else np.int32))
        xyb_done, rp = False, None
        if fr.encoding == VARDCT:
            # an LF frame's buffers are read back as XYB LF coefficients (LFCoefficients.java:44-57) and are stored
            # BEFORE performColorTransforms (JXLCodestreamDecoder.java:615-617): never fuse the inverse XYB into them
            xyb_done = bool(info.xyb_encoded) and simple and fr.lf_level == 0 and fr.type != LF_FRAME
            # frames with stages between decodeFrame and the colour transform keep their colour planes on the device
            # through those stages (row f4); LF frames / lfBuffer consumers need the padded planes on the host
            if (not simple or keep) and resident and fr.lf_level == 0 and fr.type != LF_FRAME:
                rp = self._vardct_frame(fr, xyb_done, keep=(fr.height, fr.width))  # (fused XYB: simple frames only)
            else:
                buffers[:3] = self._vardct_frame(fr, xyb_done)
        self._modular_buffers(fr, buffers, colors)
        # (trace: the cut points of integration/jvm_pin/StageDump.java. For a VarDCT frame the colour planes in `buffers` are
        # already the fused kernel's result, or None while they are on the device -- `fused` tells the listener to take the
        # stages of planes 0..2 elsewhere)
        fused = fr.encoding == VARDCT
        self._trace("idct", buffers, fused)
        self._trace("sub", buffers, fused)  # Frame.invertSubsampling: VarDCT colour planes only (inside the backend call)

        def colour_planes_to_float():
            # Frame.performGabConvolution / performEdgePreservingFilter cast integer colour planes to float first
            # (Frame.java:519: ImageBuffer.castToFloat = v * (1f / maxValue)); one-colour frames keep one plane (the backends
            # feed the three-channel kernels three copies: Frame.java:642,661 read channel 0 in all three rounds)
            for c in range(colors):
                if buffers[c].dtype != np.float32:
                    maxv = (1 << info.bits_per_sample) - 1
                    buffers[c] = be.modular_to_float(np.ascontiguousarray(buffers[c], np.int32), None, float(F(1) / F(maxv)))
            return np.stack(buffers[:colors])
        if fr.encoding == MODULAR and fr.gab:
            planes = be.gab(colour_planes_to_float(), list(fr.gab1), list(fr.gab2))
            buffers[:colors] = [np.ascontiguousarray(planes[c]) for c in range(colors)]
        self._trace("gab", buffers, fused)
        if fr.encoding == MODULAR and fr.epf_iters > 0:
            sigma = F(F(1) / F(fr.epf_sigma_modular))  # Frame.java:573-575
            planes = be.epf(colour_planes_to_float(), fr.epf_iters, None, float(sigma),
                            dict(channel_scale=list(fr.epf_channel_scale), pass0=fr.epf_pass0_sigma,
                                 pass2=fr.epf_pass2_sigma, border_sad_mul=fr.epf_border_sad_mul))
            buffers[:colors] = [np.ascontiguousarray(planes[c]) for c in range(colors)]
        self._trace("epf", buffers, fused)
        if fr.lf_level > 0:  # JXLCodestreamDecoder.java:616-617: the frame's buffers as they stand after decodeFrame
            self.lfBuffer[fr.lf_level - 1] = [np.array(b, copy=True) for b in buffers]
        # crop to the frame bounds: everything after the restoration filters works on header.bounds
        buffers = [b if b is None else np.ascontiguousarray(b[:fr.height, :fr.width]) for b in buffers]
        return FramePlanes(be, info, buffers, colors, rp=rp), xyb_done

    def _after_colour_transforms(self, fr, planes):
        """JXLCodestreamDecoder.java:637-639: the trace cut of the frame's buffers after performColorTransforms, then
        Frame.drawVarblocks with draw_varblocks"""
        if self.trace is not None:  # a listener wants the samples: a copy comes down, the planes stay
            self._trace("xyb", planes.snapshot("trace"), False)
        if fr.encoding == VARDCT and self.draw_varblocks:
            st = self.stats[-1]
            st["varblock_types"] = st["varblocks"]
            st["varblocks"] = planes.varblocks(*self._varblock_list)

    def _direct_image(self, fr, planes):
        """device_output: the frame replaces the whole canvas: its resident colour planes are the image's; the extra channels
        take the usual way"""
        info, be = self.info, self.backend
        self.stats[-1]["output"] = "device"
        for c in range(3, len(self.canvas)):
            self.canvas[c] = np.zeros((info.height, info.width), F)
        self._blend_frame(fr, planes.host, planes.colors, first=3)
        if info.orientation != 1:
            planes.rp.orient(info.orientation)
        extras = [be.orient(np.ascontiguousarray(b), info.orientation) if info.orientation != 1 else b for b in self.canvas[3:]]
        return JXLImage([None] * 3 + extras, info, be, resident=planes.rp)

    def _host_canvas_frame(self, fr, planes):
        """one frame onto the host canvas (:640-655)"""
        buffers = planes.to_host()
        if self.canvas[0] is None:
            for c in range(len(self.canvas)):
                self.canvas[c] = np.zeros((self.info.height, self.info.width), buffers[0].dtype)
        if fr.type in (REGULAR_FRAME, SKIP_PROGRESSIVE):
            if any(self.reference[i] is self.canvas and i != fr.save_as_reference for i in range(4)):
                self.canvas = [b.copy() for b in self.canvas]
            self._blend_frame(fr, buffers, planes.colors)

    def _canvas_image(self, last):
        """the canvas as decode()'s JXLImage, after the frame `last`: oriented host arrays, or, from a canvas set, the set as
        the image's (device_image), its float colours as the image's resident planes, or its planes downloaded"""
        info, be, o = self.info, self.backend, self.info.orientation
        if not self._is_set(self.canvas):
            return JXLImage([be.orient(np.ascontiguousarray(b), o) if o != 1 else b for b in self.canvas], info, be)
        self._release_dead()
        cv = self.canvas
        if self.device_image:
            # route "canvas": the set becomes the image's, whatever its plane types -- handed over when the image ends
            # here, cloned while the animation continues (the canvas lives on for its next frame)
            if last.is_last:
                ps = cv
                self.reference = [None if r is cv else r for r in self.reference]
                self.canvas = None
            else:
                ps = cv.clone()
            if o != 1:
                ps.orient(o)
            self.stats[-1].update(image="device set (canvas)", output="device")
            return JXLImage([None] * len(ps), info, be, planeSet=ps)
        if all(t == np.float32 for t in cv.dtypes[:3]):
            # the canvas' colour planes become the image's resident planes; the set lives on for the next animation frame
            rp = cv.toPlanes()
            if o != 1:
                rp.orient(o)
            extras = [cv.download(c) for c in range(3, len(cv))]
            self.stats[-1]["output"] = "device"
            return JXLImage([None] * 3 + [be.orient(b, o) if o != 1 else b for b in extras], info, be, resident=rp)
        planes = [cv.download(c) for c in range(len(cv))]
        return JXLImage([be.orient(b, o) if o != 1 else b for b in planes], info, be)

    @staticmethod
    def preview_rule(info, fr):
        """downsample=8: None when the headers say that the frame's LF image is the image at 1:8, else the first condition that
        fails. info: the image header; fr: the frame header, or None to ask only what the image header settles, which decode()
        does before it lets the front-end read the frame -- so that condition comes first here too. A frame qualifies when the
        image has no extra channels and the frame is VarDCT; regular, of LF level 0, with LF coefficients of its own; the image's
        only frame (last, at the origin, of the image's size); not upsampled; not chroma-subsampled; without patches and splines.
        Noise and YCbCr without subsampling are accepted."""
        if info.num_extra:
            return "the image has extra channels"
        if fr is None:
            return None
        if fr.encoding != VARDCT:
            return "not a VarDCT frame"
        if fr.type != REGULAR_FRAME or fr.lf_level != 0 or fr.flags & FLAG_USE_LF_FRAME:
            return "not a regular frame of LF level 0 with LF coefficients of its own"
        if not fr.is_last or fr.x0 != 0 or fr.y0 != 0 or fr.width * fr.upsampling != info.width or fr.height * fr.upsampling != info.height:
            return "not the image's only frame"
        if fr.upsampling != 1:
            return "the frame is upsampled"
        if any(fr.jpeg_up_y[c] or fr.jpeg_up_x[c] for c in range(3)):
            return "chroma subsampling"
        if fr.num_patches or fr.flags & FLAG_PATCHES:
            return "patches"
        if fr.has_splines or fr.flags & FLAG_SPLINES:
            return "splines"
        return None

    def _preview_image(self):
        """downsample=8: the image's one VarDCT frame as its LF image (preview_rule), one backend.lf_image call"""
        info, be = self.info, self.backend
        why = self.preview_rule(info, None)
        if why is not None:
            raise UnsupportedOperationException("downsample=8: " + why)
        try:
            self.fe.set_lf_only(True)
        except frontend.FrontendError as e:
            raise self._map(e)
        fr = self._next_frame()
        if fr is None:
            return None
        why = self.preview_rule(info, fr)
        if why is not None:
            raise UnsupportedOperationException("downsample=8: " + why)
        self._count_frame(fr)
        adaptive = (fr.flags & (FLAG_SKIP_ADAPTIVE_LF | FLAG_USE_LF_FRAME)) == 0
        groups = []
        for i in range(fr.num_lf_groups):
            g = self.fe.lfgroup(i)
            groups.append(dict(lfg_y=i // fr.lf_group_cols, lfg_x=i % fr.lf_group_cols, lf_quant=g["lf_quant"],
                               extra_precision=g["extra_precision"], scaled_dequant=list(fr.scaled_dequant),
                               x_factor_lf=fr.x_factor_lf, b_factor_lf=fr.b_factor_lf, adaptive_smoothing=adaptive))
        cells = ((fr.height + 7) >> 3, (fr.width + 7) >> 3)
        xyb = (*self._opsin(), info.intensity_target) if info.xyb_encoded else None
        grey = info.colour_space == CE_GRAY  # (the canvas of a grey image takes the frame's plane 1: _blend_buffers)
        keep = self.device_output and getattr(be, "resident", False) and not grey
        planes = be.lf_image(groups, cells, fr.base_corr_x, fr.base_corr_b, fr.colour_factor, xyb, keep=keep)
        o = info.orientation
        st = self.stats[-1]
        st["preview"] = "lf image (1:8)" + (", noise left out" if fr.has_noise else "")
        st["output"] = "device" if keep else "host"
        if keep:
            if fr.do_ycbcr:
                planes.ycbcr()
            if o != 1:
                planes.orient(o)
            return JXLImage([None] * 3, info, be, resident=planes)
        if fr.do_ycbcr:
            planes = be.ycbcr(planes)
        planes = [np.ascontiguousarray(planes[c]) for c in ((1,) if grey else range(3))]
        return JXLImage([be.orient(b, o) if o != 1 else b for b in planes], info, be)

    @staticmethod
    def region_in_frame(info, region):
        """region: the box (x0, y0, w, h) of the image as delivered -> the box (x0, y0, w, h) of the frame's coded pixels that
        JXLCodestreamDecoder.transposeBuffer (the orientation) turns into it. A pure function of the image header. ValueError
        for an empty box or one that is not inside the image"""
        x0, y0, w, h = region
        H, W, o = info.height, info.width, info.orientation
        dh, dw = (W, H) if o > 4 else (H, W)
        if w <= 0 or h <= 0:
            raise ValueError("region %r is empty" % (tuple(region),))
        if x0 < 0 or y0 < 0 or x0 + w > dw or y0 + h > dh:
            raise ValueError("region %r is not inside the %d x %d image" % (tuple(region), dw, dh))
        return {1: (x0, y0, w, h), 2: (W - x0 - w, y0, w, h), 3: (W - x0 - w, H - y0 - h, w, h), 4: (x0, H - y0 - h, w, h),
                5: (y0, x0, h, w), 6: (y0, H - x0 - w, h, w), 7: (W - y0 - h, H - x0 - w, h, w), 8: (W - y0 - h, x0, h, w)}[o]

    @staticmethod
    def region_rule(info, fr):
        """region: None when the headers say that the image is one VarDCT frame whose stages all have a small, known reach, else
        the first condition that fails. fr None: only what the image header settles (asked before the frame is read). Noise,
        YCbCr and any opsin matrix qualify"""
        if info.num_extra:
            return "the image has extra channels"
        if fr is None:
            return None
        if fr.encoding != VARDCT:
            return "not a VarDCT frame"
        if fr.type != REGULAR_FRAME or fr.lf_level != 0 or fr.flags & FLAG_USE_LF_FRAME:
            return "not a regular frame of LF level 0 with LF coefficients of its own"
        if not fr.is_last or fr.x0 != 0 or fr.y0 != 0 or fr.width * fr.upsampling != info.width or \
                fr.height * fr.upsampling != info.height or fr.blend_mode != abi.BLEND_REPLACE:
            return "not the image's only frame"
        if fr.upsampling != 1:
            return "the frame is upsampled"
        if any(fr.jpeg_up_y[c] or fr.jpeg_up_x[c] for c in range(3)):
            return "chroma subsampling"
        if fr.num_patches or fr.flags & FLAG_PATCHES:
            return "patches"
        if fr.has_splines or fr.flags & FLAG_SPLINES:
            return "splines"
        return None

    def _region_image(self):
        """region: the box of the image's one VarDCT frame (region_rule) from the sections it needs: the front-end's selection,
        the selected LF groups as a sub-frame through backend.vardct, the box cut out of its result, the tail on the box"""
        info, be = self.info, self.backend
        why = self.region_rule(info, None)
        if why is not None:
            raise UnsupportedOperationException("region: " + why)
        fx, fy, fw, fh = frame_box = self.region_in_frame(info, self.region)
        try:
            self.fe.set_region(frame_box)
        except frontend.FrontendError as e:
            raise self._map(e)
        fr = self._next_frame()
        if fr is None:
            return None
        why = self.region_rule(info, fr)
        if why is not None:
            raise UnsupportedOperationException("region: " + why)
        self._count_frame(fr)
        plan = self.fe.region_plan()
        sub = self._subframe(fr, plan)
        st = self.stats[-1]
        st["region"] = dict(box=tuple(self.region), frame_box=frame_box, margin=plan["margin"],
                            groups_read=plan["groups_read"], groups_total=plan["groups_total"],
                            lf_groups_read=plan["lf_groups_read"], lf_groups_total=plan["lf_groups_total"],
                            section_bytes_read=plan["section_bytes_read"], section_bytes_total=plan["section_bytes_total"],
                            subframe=(sub["x"], sub["y"], sub["w"], sub["h"]),
                            path="groups" if plan["applied"] else "whole frame (single section)")
        grey = info.colour_space == CE_GRAY  # (the canvas of a grey image takes the frame's plane 1: _blend_buffers)
        resident = bool(getattr(be, "resident", False))
        keep = self.device_output and resident and not grey
        xyb_done = bool(info.xyb_encoded) and not fr.has_noise  # (the inverse XYB is fused where no stage comes before it)
        wy, wx = fy - sub["y"], fx - sub["x"]
        if resident:
            rp = self._vardct_frame(fr, xyb_done, keep=(wy, wx, fh, fw), sub=sub)
            planes = FramePlanes(be, info, [None] * 3, 3, rp=rp)
        else:
            full = self._vardct_frame(fr, xyb_done, sub=sub)
            planes = FramePlanes(be, info, [np.ascontiguousarray(b[wy:wy + fh, wx:wx + fw]) for b in full], 3)
        self._chained_tail(fr, planes, False, xyb_done, keep=keep, noise_at=(fr.height, fr.width, fy, fx))
        o = info.orientation
        st["output"] = "device" if keep else "host"
        if keep:
            if o != 1:
                planes.rp.orient(o)
            image = JXLImage([None] * 3, info, be, resident=planes.rp)
        else:
            host = [planes.host[1]] if grey else planes.host[:3]
            image = JXLImage([be.orient(np.ascontiguousarray(b), o) if o != 1 else b for b in host], info, be)
        image.region = tuple(self.region)
        return image

    def decode(self):
        """JXLCodestreamDecoder.decode (:546-677): frames until one completes an image; None at the end of the stream"""
        colors_img = 1 if self.info.colour_space == CE_GRAY else 3
        self._check_switches()
        if self.downsample == 8:
            return self._preview_image()
        if self.region is not None:
            return self._region_image()
        if self.canvas is None:
            self.canvas = [None] * (colors_img + self.info.num_extra)
        last = planes = None
        while True:
            fr = self._next_frame()                                   # 1. the next frame
            if fr is None:
                break
            last, bus0, colors = fr, self._blend_bus(), self._colors(fr)
            why = self._modular_frame_route(fr, colors, colors_img) if self.device_image else "device_image is off"
            if why is None:                                           # 2. which route
                return self._modular_frame_image(fr, bus0)
            self.stats[-1]["image"] = "host: " + why
            direct = self._direct_frame(fr, colors)
            frame_set = self._frame_set_route(fr, direct)
            self._pending_transforms(fr, frame_set)
            if frame_set:                                             # 3. the frame's planes, 4. the tail
                self.stats[-1]["canvas"] = "device"  # (the canvas is a set or becomes one now: _frame_set_route has looked)
                save = self._count_frame(fr)
                planes = self._modular_frame_set(fr, save)
                on_set = self._landed is None  # (device_chains: the patch stage of a frame with patches may have landed the canvas)
            else:
                planes = None  # (the last frame's arrays go right before this frame's are made: the allocator hands their memory on)
                on_set = self._canvas_route(fr, direct)
                planes, xyb_done = self._host_frame(fr, colors, keep=direct or on_set)
                if fr.type == LF_FRAME:
                    continue
                save = self._count_frame(fr)
                self._chained_tail(fr, planes, save, xyb_done, keep=direct or on_set)
                on_set = on_set and self._landed is None  # (device_patch_sets: the patch stage may have landed the canvas)
                self._after_colour_transforms(fr, planes)
            if direct and planes.rp is not None:                      # 5. the canvas
                return self._direct_image(fr, planes)
            if on_set:
                self._canvas_frame(fr, planes)
            else:
                self._host_canvas_frame(fr, planes)
            if self._frame_done(fr, save, bus0):                      # 6. done?
                break
        return None if last is None else self._canvas_image(last)


# ---- PNGWriter (J/io/PNGWriter.java) ---------------------------------------------------------------------------
class PNGWriter:
    def __init__(self, image, bitDepth=-1, hdr=False, peakDetect=PEAK_DETECT_AUTO, deflateLevel=6, deviceColor=False, deviceSamples=False,
                 toneMap=None):
        """deviceColor: JXLImage.transform(..., device=True).
        deviceSamples: the colour management and the packing in ONE device pass (backend.png_samples, or
        ResidentPlanes.pngSamples when the image's colour planes are on the device: JXLDecoder(device_output=True)), after at
        most one peak call; the same samples as deviceColor gives, byte for byte. bus_bytes = (bytes up, bytes down) of the
        sample planes. A backend without png_samples is an error.
        toneMap: a ToneMap -- HDR to SDR inside the device colour pass (deviceColor or deviceSamples), in place of peak
        detection; not with hdr, and not for an image with an ICC profile."""
        if toneMap is not None:
            if not (deviceColor or deviceSamples):
                raise ValueError("toneMap needs the device path")
            _tone_map_check(toneMap, image.backend, TF_PQ if hdr else None)
            if image.has_icc:
                raise ValueError("toneMap: an image with an ICC profile is written as it is")
        if bitDepth <= 0:
            bitDepth = 16 if (hdr or image.info.bits_per_sample > 8) else 8
        if bitDepth not in (8, 16):
            raise ValueError("PNG only supports 8 and 16")
        self.hdr = hdr
        gray = image.colorEncoding == CE_GRAY
        primaries = PRI_BT2100 if hdr else PRI_SRGB
        tf = TF_PQ if hdr else TF_SRGB
        self.has_icc = image.has_icc
        self.bus_bytes = None
        if deviceSamples and self._device_samples(image, bitDepth, primaries, tf, peakDetect, deflateLevel, toneMap):
            return
        if not image.has_icc:
            image = image.transform(primaries, WP_D65, tf, peakDetect, device=deviceColor or deviceSamples, toneMap=toneMap)
        self._layout(image, bitDepth, 1 if gray else 3, deflateLevel)
        planes = image.getBuffer(False)
        color = [np.ascontiguousarray(planes[c]) for c in range(self.colorChannels)]
        alpha = np.ascontiguousarray(planes[self.colorChannels + self.alphaIndex]) if self.alphaIndex >= 0 else None
        tagged = [image.getTaggedBitDepth(c) for c in range(self.colorChannels)]
        if alpha is not None:
            tagged.append(image.getTaggedBitDepth(self.colorChannels + self.alphaIndex))
        tagged += [bitDepth] * (4 - len(tagged))
        # PNGWriter.java:79-111 + the writeIDAT sample order: one device pass
        self.samples = image.backend.pack(color, bitDepth, alpha, image.isAlphaPremultiplied() and alpha is not None, tagged, True)

    def _layout(self, image, bitDepth, colors, deflateLevel):
        self.bitDepth, self.colorChannels, self.deflateLevel = bitDepth, colors, deflateLevel
        self.width, self.height = image.getWidth(), image.getHeight()
        self.alphaIndex = image.getAlphaIndex()
        self.colorMode = (4 if self.alphaIndex >= 0 else 0) if colors == 1 else (6 if self.alphaIndex >= 0 else 2)

    def _device_samples(self, image, bitDepth, primaries, tf, peakDetect, deflateLevel, toneMap=None):
        """the constructor with deviceSamples. False (nothing done): a grey image that is tone-mapped -- PNGWriter then takes
        plane 0 and plane 1 + alphaIndex of the three-plane result for its grey layout, which the one-pass kernel has no
        output for; the constructor runs the device passes one by one (deviceColor) and bus_bytes stays None."""
        be = image.backend
        if not hasattr(be, "png_samples"):
            raise TypeError("deviceSamples needs a backend with png_samples")
        colors = image.getColorChannelCount()
        up = 0
        planes = image._plan_planes(colors)  # (stand-ins while the samples are on the device)

        def peak_of(pl, **front):
            nonlocal up
            peak, sent = image._peak(pl, **front)
            up += sent
            return peak
        if colors == 1 and not image.has_icc and (toneMap is not None or not (_prim_matches(primaries, image.primariesXY) and _xy_matches(WP_D65, image.whiteXY))):
            return False  # (before the plan is made: the peak, if one is needed, is then taken once, by transform())
        plan = None if image.has_icc else image._color_plan(primaries, WP_D65, tf, peakDetect, peak_of, planes=planes, toneMap=toneMap)
        if plan is not None:
            planes, params = plan[0], plan[1]
        else:  # the image as it is: every colour stage off; integer planes are cast with their depth's maximum (PNGWriter's coercion)
            if planes is None:
                planes = [image.buffer[c] for c in range(colors)]
                if len({a.dtype for a in planes}) != 1:
                    planes = [image._as_float(c) for c in range(colors)]
            params = dict(inMax=[(1 << image.bitDepths[c]) - 1 for c in range(colors)])
        self._layout(image, bitDepth, colors, deflateLevel)
        has_alpha = self.alphaIndex >= 0
        kw = dict(premultiplied=image.isAlphaPremultiplied() and has_alpha, bitDepth=bitDepth, bigEndian=True,
                  alphaDepth=image.getTaggedBitDepth(colors + self.alphaIndex) if has_alpha else None,
                  colorDepth=image.getTaggedBitDepth(0), **params)
        if toneMap is None:
            self.samples, sent = image._png_samples(planes, **kw)
        else:
            with _ToneMapArmed(be, primaries, WP_D65, toneMap.resolve(image)):
                self.samples, sent = image._png_samples(planes, **kw)
        self.bus_bytes = (up + sent, self.samples.nbytes)
        return True

    @staticmethod
    def _chunk(tag, payload):
        body = tag + payload
        return struct.pack(">I", len(payload)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)

    def write(self, out):
        out.write(b"\x89PNG\r\n\x1a\n")
        out.write(self._chunk(b"IHDR", struct.pack(">IIBBBBB", self.width, self.height, self.bitDepth, self.colorMode, 0, 0, 0)))
        if not self.has_icc and not self.hdr:
            out.write(self._chunk(b"sRGB", b"\x01"))
        if self.hdr:
            out.write(self._chunk(b"cICP", bytes([9, 16, 0, 1])))  # BT.2100 PQ full range (the reference embeds an ICC profile)
        rows = self.samples.reshape(self.height, -1).view(np.uint8)
        raw = np.concatenate([np.zeros((self.height, 1), np.uint8), rows], axis=1).tobytes()  # filter type 0 per row
        out.write(self._chunk(b"IDAT", zlib.compress(raw, self.deflateLevel)))
        out.write(self._chunk(b"IEND", b""))


# ---- PFMWriter (J/io/PFMWriter.java) ---------------------------------------------------------------------------
class PFMWriter:
    def __init__(self, image, deviceSamples=False):
        """The image's own samples as a PFM: no colour transform, no peak scale, no transfer function (PFMWriter.java:30).
        deviceSamples: cast, floatToIntBits, byte order, interleaving and the row flip in ONE device pass
        (ResidentPlanes.pfmSamples when the image's colour planes are on the device: JXLDecoder(device_output=True); else
        backend.pfm_samples on the host arrays); the same bytes as the default path. bus_bytes = (bytes up, bytes down) of
        the sample planes. A backend without pfm_samples is an error."""
        self.width, self.height = image.getWidth(), image.getHeight()
        self.gray = image.colorEncoding == CE_GRAY
        colors = 1 if self.gray else 3
        tagged = [image.getTaggedBitDepth(c) for c in range(colors)]
        self.bus_bytes = None
        if deviceSamples:
            if not hasattr(image.backend, "pfm_samples"):
                raise TypeError("deviceSamples needs a backend with pfm_samples")
            self.samples, up = image._pfm_samples(tagged)
            self.bus_bytes = (up, self.samples.nbytes)
            return
        words = []
        for c, b in enumerate(image.getBuffer(False)[:colors]):
            if b.dtype != np.float32:  # ImageBuffer.castToFloat(depth): Java int arithmetic, shift counts modulo 32
                maxv = ~((-1 << (tagged[c] & 31)) & 0xffffffff) & 0xffffffff
                if maxv < 1:
                    raise ValueError("invalid Max Value")
                b = b.astype(F) * F(F(1) / F(maxv))
            w = np.ascontiguousarray(b, F).view(np.uint32)
            words.append(np.where(np.isnan(b), np.uint32(0x7fc00000), w))  # Float.floatToIntBits
        # bottom to top, channels interleaved, DataOutputStream.writeFloat's byte order
        rows = np.ascontiguousarray(np.stack(words, axis=-1)[::-1])
        self.samples = rows.astype(">u4").view(np.uint8).reshape(self.height, self.width, colors, 4)

    def write(self, out):
        out.write(("%s\n%d %d\n1.0\n" % ("Pf" if self.gray else "PF", self.width, self.height)).encode("ascii"))
        out.write(self.samples.tobytes())


def load_vardct_frame(source, ctx, transfer=abi.TRANSFER_NONE, out_format=abi.OUT_F32, sparse=False):
    """Parse the first frame of a VarDCT .jxl file with the front-end and stage it in a host.Frame on `ctx` (inputs
    resident, nothing run yet): the real-bitstream workload of bench.py. Returns (host.Frame, stats dict).
    sparse: the coefficients go through the sparse feed (jxl_vardct_put_group_sparse). The frame tail is not run here, so
    JXLDecoder's `device_splines` has no counterpart: this is the only load_* helper, and it stops before the splines."""
    from . import host
    if isinstance(source, (bytes, bytearray)):
        data = bytes(source)
    else:
        with open(source, "rb") as f:
            data = f.read()
    dec = JXLDecoder.__new__(JXLDecoder)
    dec.fe = frontend.Frontend(data)
    dec.info = dec.fe.image
    dec.backend = None
    dec.sparse_coeffs = bool(sparse)
    fr = dec.fe.next_frame(None, None)
    if fr is None or fr.encoding != VARDCT:
        raise ValueError("first frame is not a VarDCT frame")
    p, weights, woffs, lfgroups, groups, hist = dec._vardct_inputs(fr, bool(dec.info.xyb_encoded))
    if transfer != abi.TRANSFER_NONE or out_format != abi.OUT_F32:
        p.stages |= abi.STAGE_OUT
        p.transfer, p.out_format = transfer, out_format
    hf = feed_frame(host.Frame(ctx, p, weights, woffs), lfgroups, groups(sparse), sparse)
    stats = dict(width=fr.width, height=fr.height, padded_width=fr.padded_width, padded_height=fr.padded_height, groups=fr.num_groups,
                 passes=fr.num_passes, epf_iters=fr.epf_iters, gab=fr.gab,
                 varblocks={abi.TT_NAME[t]: int(n) for t, n in enumerate(hist) if n})
    return hf, stats
