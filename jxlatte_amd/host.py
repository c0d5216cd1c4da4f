"""Host-side mirror of the reference's interface for the transform stage, on top of the C-ABI.

Names, argument meaning and error behaviour follow the Java classes the path lives in
(J/ = java/com/traneptora/jxlatte/): `MathHelper.inverseDCT2D`, `Frame.performGabConvolution`,
`Frame.performEdgePreservingFilter`, `OpsinInverseMatrix.invertXYB`, `PassGroup.invertVarDCT`
(through `Frame.decodePassGroups`), `ModularStream.applyTransforms`,
`ModularChannel.inverse{Horizontal,Vertical}Squeeze`, `JXLImage.transfer`. numpy planes stand in for
the Java `float[][]` / `int[][]` row arrays. Every call runs on the GPU through libjxlatte_amd.so;
nothing here computes pixels on the CPU.
"""
import ctypes as C

import numpy as np

from . import abi
from ._lib import Context, IllegalStateException, check  # noqa: F401  (re-export)


def _p3(planes, ctype):
    arr = (C.POINTER(ctype) * 3)()
    for c in range(3):
        arr[c] = abi.ptr(planes[c], ctype)
    return arr


def _planes(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError("expected planes of shape (3, H, W)")
    return a


class MathHelper:
    """J/util/MathHelper.java"""

    @staticmethod
    def inverseDCT2D(ctx, src, transposed=False):
        src = np.ascontiguousarray(src, np.float32)
        h, w = src.shape
        dst = np.empty((w, h) if transposed else (h, w), np.float32)
        ctx.call("jxl_stage_idct2d", abi.fptr(src), abi.fptr(dst), h, w, 1 if transposed else 0)
        return dst

    @staticmethod
    def forwardDCT2D(ctx, src):
        src = np.ascontiguousarray(src, np.float32)
        h, w = src.shape
        dst = np.empty((h, w), np.float32)
        ctx.call("jxl_stage_fdct2d", abi.fptr(src), abi.fptr(dst), h, w)
        return dst


class OpsinInverseMatrix:
    """J/color/OpsinInverseMatrix.java"""

    def __init__(self, matrix, opsin_bias, cbrt_opsin_bias):
        self.matrix = [float(v) for v in matrix]
        self.opsinBias = [float(v) for v in opsin_bias]
        self.cbrtOpsinBias = [float(v) for v in cbrt_opsin_bias]

    def invertXYB(self, ctx, buffer, intensityTarget):
        if len(buffer) < 3:
            raise ValueError("Can only XYB on 3 channels")  # OpsinInverseMatrix.java:106-107
        out = np.array(buffer, np.float32, order="C", copy=True)
        ctx.call("jxl_stage_xyb", _p3(out, C.c_float), out[0].size, abi.f9(*self.matrix), abi.f3(*self.opsinBias),
                 abi.f3(*self.cbrtOpsinBias), C.c_float(intensityTarget))
        return out


class LFCoefficients:
    """device part of J/frame/vardct/LFCoefficients.java (row f1): dequant, LF chroma-from-luma, adaptiveSmooth"""

    @staticmethod
    def dequantLFCoeff(ctx, lfQuant, scaledDequant, extraPrecision=0, xFactorLF=128, bFactorLF=128, adaptiveSmoothing=True,
                       baseCorrelationX=0.0, baseCorrelationB=1.0, colorFactor=84):
        """lfQuant: int32 [3][H][W] in X,Y,B order (lfQuant[cMap[i]]). Returns float32 [3][H][W]."""
        q = np.ascontiguousarray(lfQuant, np.int32)
        d = abi.make_lfquant_desc(q, scaledDequant, extraPrecision, xFactorLF, bFactorLF, adaptiveSmoothing)
        out = np.empty(q.shape, np.float32)
        ctx.call("jxl_stage_lf_dequant", C.byref(d), C.c_float(baseCorrelationX), C.c_float(baseCorrelationB), colorFactor,
                 _p3(out, C.c_float))
        return out


def lfImage(ctx, groups, cells, baseCorrelationX=0.0, baseCorrelationB=1.0, colorFactor=84, xyb=None, keep=False):
    """The LF image of a VarDCT frame as the picture at 1:8, one launch (jxl_stage_lf_image; keep: jxl_planes_from_lf). groups: the
    frame's LF groups as abi.make_lf_image_desc takes them; cells: (ceil(h / 8), ceil(w / 8)); xyb: None or (matrix, opsinBias,
    cbrtOpsinBias, intensityTarget) for the inverse XYB behind the LF stage. Returns float32 [3][cells_h][cells_w], or with keep the
    context's ResidentPlanes holding them (nothing comes down)."""
    d, alive = abi.make_lf_image_desc(groups, cells, baseCorrelationX, baseCorrelationB, colorFactor, xyb)
    if keep:
        ctx.call("jxl_planes_from_lf", C.byref(d))
        return ResidentPlanes(ctx)
    out = np.empty((3, int(cells[0]), int(cells[1])), np.float32)
    ctx.call("jxl_stage_lf_image", C.byref(d), _p3(out, C.c_float))
    return out


def performColorTransformsYCbCr(ctx, buffer):
    """YCbCr branch of JXLCodestreamDecoder.performColorTransforms (:270-281)"""
    out = np.array(buffer, np.float32, order="C", copy=True)
    ctx.call("jxl_stage_ycbcr", _p3(out, C.c_float), out[0].size)
    return out


def _one_colour(buffer):
    """A frame with ONE colour channel (Frame.getColorChannelCount, Frame.java:874-877: grey, not XYB, Modular). The reference's
    EPF distance still runs its channel loop three times but reads channel 0 every time (`i = colors == 1 ? 0 : c`,
    Frame.java:642,661): three copies of the plane through the three-channel kernels are that sum, term for term."""
    a = np.ascontiguousarray(buffer, np.float32)
    return a.ndim == 3 and a.shape[0] == 1


def performGabConvolution(ctx, buffer, gab1Weights, gab2Weights):
    """Frame.performGabConvolution (Frame.java:505-542)"""
    if _one_colour(buffer):  # channel 0 with ITS weights; the copies keep the kernels' three-plane interface
        a = np.ascontiguousarray(buffer, np.float32)
        return performGabConvolution(ctx, np.repeat(a, 3, axis=0), [gab1Weights[0]] * 3, [gab2Weights[0]] * 3)[:1]
    buf = _planes(buffer, np.float32)
    out = np.empty_like(buf)
    ctx.call("jxl_stage_gab", _p3(buf, C.c_float), _p3(out, C.c_float), buf.shape[1], buf.shape[2],
             abi.f3(*gab1Weights), abi.f3(*gab2Weights))
    return out


def epfInverseSigma(ctx, hfMultiplier, sharpness, globalScaleF, epfSharpLut):
    """inverse-sigma map of Frame.performEdgePreservingFilter (Frame.java:552-571); raises
    InvalidBitstreamException for sharpness outside 0..7 (:565-566)."""
    hf = np.ascontiguousarray(hfMultiplier, np.int32)
    sh = np.ascontiguousarray(sharpness, np.int32)
    out = np.empty(hf.shape, np.float32)
    ctx.call("jxl_stage_epf_sigma", abi.iptr(hf), abi.iptr(sh), hf.shape[0], hf.shape[1], C.c_float(globalScaleF),
             abi.f8(*epfSharpLut), abi.fptr(out))
    return out


def performEdgePreservingFilter(ctx, buffer, epfIterations, inverseSigma=None, invModularSigma=0.0,
                                epfChannelScale=(40.0, 5.0, 3.5), epfPass0SigmaScale=0.9, epfPass2SigmaScale=6.5,
                                epfBorderSadMul=2.0 / 3.0):
    """Frame.performEdgePreservingFilter iteration loop (Frame.java:583-635)"""
    if _one_colour(buffer):
        a = np.ascontiguousarray(buffer, np.float32)
        return performEdgePreservingFilter(ctx, np.repeat(a, 3, axis=0), epfIterations, inverseSigma, invModularSigma, epfChannelScale,
                                           epfPass0SigmaScale, epfPass2SigmaScale, epfBorderSadMul)[:1]
    buf = _planes(buffer, np.float32)
    out = np.empty_like(buf)
    sig = None
    if inverseSigma is not None:
        inverseSigma = np.ascontiguousarray(inverseSigma, np.float32)
        sig = abi.fptr(inverseSigma)
    ctx.call("jxl_stage_epf", _p3(buf, C.c_float), _p3(out, C.c_float), buf.shape[1], buf.shape[2], epfIterations, sig,
             C.c_float(invModularSigma), abi.f3(*epfChannelScale), C.c_float(epfPass0SigmaScale),
             C.c_float(epfPass2SigmaScale), C.c_float(epfBorderSadMul))
    return out


def restoreFused(ctx, buffer, params, hfMultiplier=None, sharpness=None):
    """Gaborish -> EPF -> XYB of Frame.java:505-679 + OpsinInverseMatrix.invertXYB as the frame path's ONE fused launch, on planes of
    any size >= 8 x 8 (float planes out); params: abi.VarDCTParams (gab, epf_*, xyb, opsin_* ... are read)"""
    buf = _planes(buffer, np.float32)
    out = np.empty_like(buf)
    hf = sh = None
    if hfMultiplier is not None:
        hfMultiplier = np.ascontiguousarray(hfMultiplier, np.int32)
        sharpness = np.ascontiguousarray(sharpness, np.int32)
        cells = ((buf.shape[1] + 7) // 8, (buf.shape[2] + 7) // 8)
        if hfMultiplier.shape != cells or sharpness.shape != cells:
            raise ValueError("expected cell maps of shape %r" % (cells,))
        hf, sh = abi.iptr(hfMultiplier), abi.iptr(sharpness)
    ctx.call("jxl_stage_restore_fused", _p3(buf, C.c_float), _p3(out, C.c_float), buf.shape[1], buf.shape[2], hf, sh, C.byref(params))
    return out


def transfer(ctx, x, tf, maxValue=0):
    """JXLImage.transferInPlace (+ ImageBuffer.castToIntWithMax when maxValue > 0)"""
    x = np.ascontiguousarray(x, np.float32)
    if maxValue > 0:
        out = np.empty(x.shape, np.int32)
        ctx.call("jxl_stage_transfer", abi.fptr(x), x.size, tf, maxValue, None, abi.iptr(out))
    else:
        out = np.empty(x.shape, np.float32)
        ctx.call("jxl_stage_transfer", abi.fptr(x), x.size, tf, 0, abi.fptr(out), None)
    return out


def colorParams(planes, tfIn=abi.TF_LINEAR, gammaIn=0, inMax=None, scale=None, matrix=None, tfOut=abi.TF_LINEAR, gammaOut=0,
                maxValue=0):
    """jxl_color_params for a list of 1 or 3 equally shaped planes, all int32 (cast with inMax[c]) or all float32"""
    if len(planes) not in (1, 3) or len({(p.shape, p.dtype) for p in planes}) != 1 or planes[0].dtype not in (np.int32, np.float32):
        raise ValueError("expected 1 or 3 int32 or float32 planes of one shape")
    p = abi.ColorParams()
    p.n_planes = len(planes)
    p.in_is_int = 1 if planes[0].dtype == np.int32 else 0
    for c, v in enumerate(inMax if inMax is not None else ()):
        p.in_max[c] = int(v)
    p.tf_in, p.gamma_in, p.tf_out, p.gamma_out, p.max_value = int(tfIn), int(gammaIn), int(tfOut), int(gammaOut), int(maxValue)
    if scale is not None:
        p.use_scale, p.scale = 1, float(scale)
    if matrix is not None:
        p.use_matrix = 1
        p.matrix = abi.f9(*[float(v) for v in np.asarray(matrix, np.float32).reshape(-1)])
    return p


def toneMapParams(lum, unitNits, sourceNits, targetNits, gamut=True):
    """jxl_tone_map: the luminance weights of the primaries the samples are in behind the matrix stage, the nits of a linear 1.0,
    the content's mastering peak, the display's peak, and whether the gamut step runs"""
    t = abi.ToneMapParams()
    t.lum = (C.c_float * 3)(*[float(v) for v in lum])
    t.unit_nits, t.source_nits, t.target_nits, t.gamut = float(unitNits), float(sourceNits), float(targetNits), int(bool(gamut))
    return t


def setToneMap(ctx, tm):
    """arm (tm: a jxl_tone_map of toneMapParams) or clear (None) the HDR -> SDR stage of the context's colour passes
    (jxl_ctx_set_tone_map): while armed colorConvert, pngSamples, tensorSamples, tensorResized and tensorResizedBatch, from every
    home, apply it behind the matrix and write three colour channels; a scale is refused"""
    ctx.call("jxl_ctx_set_tone_map", None if tm is None else C.byref(tm))


def _pv(planes):
    arr = (C.c_void_p * 3)()
    for c, a in enumerate(planes):
        arr[c] = a.ctypes.data
    return arr


def colorConvert(ctx, planes, **params):
    """JXLImage.transform's sample chain in one device pass (jxl_stage_color_convert): cast, toLinearF, grey -> RGB, matrix,
    peak scale, fromLinearF, castToInt0, each one optional (colorParams). Returns the list of output planes: three when a
    matrix is given, three planes come in or the context's tone mapping is armed (setToneMap), else one; int32 when maxValue > 0, else float32."""
    planes = [np.ascontiguousarray(a) for a in planes]
    p = colorParams(planes, **params)
    n_out = 3 if (len(planes) == 3 or p.use_matrix or ctx.toneMapArmed()) else 1
    out = [np.empty(planes[0].shape, np.int32 if p.max_value > 0 else np.float32) for _ in range(n_out)]
    ctx.call("jxl_stage_color_convert", _pv(planes), planes[0].size, C.byref(p), _pv(out))
    return out


def determinePeak(ctx, planes, **params):
    """JXLImage.determinePeak of what the cast, toLinearF and matrix stages of colorParams make of the 2-D planes
    (jxl_stage_color_peak): the float the reference computes, as numpy.float32"""
    planes = [np.ascontiguousarray(a) for a in planes]
    p = colorParams(planes, **params)
    h, w = planes[0].shape
    peak = C.c_float(0)
    ctx.call("jxl_stage_color_peak", _pv(planes), h, w, C.byref(p), C.byref(peak))
    return np.float32(peak.value)


def pngParams(planes, shape, alpha=None, premultiplied=False, bitDepth=8, bigEndian=False, alphaDepth=None, colorDepth=None, **color):
    """jxl_png_params: colorParams(planes, **color) (maxValue stays 0) plus PNGWriter's arguments. alpha: the alpha plane (its
    dtype tells int32 from float32) or None; alphaDepth / colorDepth: the tagged depths (default: bitDepth)"""
    p = abi.PngParams()
    p.color = colorParams(planes, **color)
    p.height, p.width = int(shape[0]), int(shape[1])
    p.has_alpha, p.premultiplied = int(alpha is not None), int(bool(premultiplied))
    p.bit_depth, p.big_endian = int(bitDepth), int(bool(bigEndian))
    p.alpha_is_int = int(alpha is not None and alpha.dtype == np.int32)
    p.alpha_tagged_depth = int(bitDepth if alphaDepth is None else alphaDepth)
    p.color_tagged_depth = int(bitDepth if colorDepth is None else colorDepth)
    return p


def _png_out(ctx, p, shape):
    nch = (3 if (p.color.n_planes == 3 or p.color.use_matrix or ctx.toneMapArmed()) else 1) + p.has_alpha
    return np.empty((shape[0], shape[1], nch), np.uint8 if p.bit_depth == 8 else np.uint16)


def _png_alpha(alpha, shape):
    if alpha is None:
        return None
    a = np.ascontiguousarray(alpha)
    if a.dtype not in (np.int32, np.float32) or a.shape != tuple(shape):
        raise TypeError("the alpha plane must be int32 or float32 of the colour planes' shape")
    return a


def pngSamples(ctx, planes, alpha=None, **params):
    """PNGWriter's samples of 1 or 3 colour planes (2-D, all int32 or all float32) and an optional alpha plane in one device
    pass (jxl_stage_png_samples): colorConvert(planes, maxValue=0, ...) followed by packSamples, byte for byte, without the
    float planes in between. params: pngParams' keywords. Returns [h][w][channels] uint8 / uint16."""
    planes = [np.ascontiguousarray(a) for a in planes]
    shape = planes[0].shape
    a = _png_alpha(alpha, shape)
    p = pngParams(planes, shape, alpha=a, **params)
    out = _png_out(ctx, p, shape)
    ctx.call("jxl_stage_png_samples", _pv(planes), _vp(a), C.byref(p), _vp(out))
    return out


TENSOR_DTYPES = {"uint8": abi.TENSOR_U8, "float16": abi.TENSOR_F16, "bfloat16": abi.TENSOR_BF16, "float32": abi.TENSOR_F32}
TENSOR_LAYOUTS = {"CHW": abi.TENSOR_CHW, "HWC": abi.TENSOR_HWC}


def tensorParams(planes, shape, alpha=None, premultiplied=False, writeAlpha=False, dtype="float32", layout="CHW", alphaDepth=None,
                 colorDepth=None, mean=None, invStd=None, **color):
    """jxl_tensor_params: colorParams(planes, **color) (maxValue stays 0) plus the tensor's arguments. alpha: the alpha plane (its
    dtype tells int32 from float32) or None; alphaDepth / colorDepth: the tagged depths (default 8); dtype: a key of
    TENSOR_DTYPES or an abi.TENSOR_* code, layout likewise; mean / invStd: per output channel, both or neither (float dtypes)"""
    p = abi.TensorParams()
    p.color = colorParams(planes, **color)
    p.height, p.width = int(shape[0]), int(shape[1])
    p.has_alpha, p.premultiplied, p.write_alpha = int(alpha is not None), int(bool(premultiplied)), int(bool(writeAlpha))
    p.alpha_is_int = int(alpha is not None and alpha.dtype == np.int32)
    p.alpha_tagged_depth = int(8 if alphaDepth is None else alphaDepth)
    p.color_tagged_depth = int(8 if colorDepth is None else colorDepth)
    p.dtype = TENSOR_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    p.layout = TENSOR_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    if (mean is None) != (invStd is None):
        raise ValueError("mean and invStd come together")
    if mean is not None:
        p.use_norm = 1
        for c, (m, s) in enumerate(zip(mean, invStd)):
            p.mean[c], p.inv_std[c] = float(m), float(s)
    return p


def tensorChannels(p, toneMap=False):
    """the output channels of a jxl_tensor_params (toneMap: on a context whose tone mapping is armed)"""
    return (3 if (p.color.n_planes == 3 or p.color.use_matrix or toneMap) else 1) + int(bool(p.write_alpha))


def tensorSamples(ctx, planes, alpha, out_ptr, **params):
    """The image as a device tensor in one pass (jxl_stage_tensor_samples): the colour stages of pngSamples, un-premultiplication,
    normalisation and the conversion to the tensor's dtype, stored CHW or HWC at the DEVICE address out_ptr (an integer: memory
    of the context's device that holds height * width * channels elements). planes / alpha: host arrays, uploaded once.
    params: tensorParams' keywords. Complete on return; nothing comes down. Returns the jxl_tensor_params it used."""
    planes = [np.ascontiguousarray(a) for a in planes]
    shape = planes[0].shape
    a = _png_alpha(alpha, shape)
    p = tensorParams(planes, shape, alpha=a, **params)
    ctx.call("jxl_stage_tensor_samples", _pv(planes), _vp(a), C.byref(p), C.c_void_p(int(out_ptr)))
    return p


RESIZE_FILTERS = {"triangle": abi.RESIZE_TRIANGLE, "box": abi.RESIZE_BOX}


def resizeParams(shape, size, box=None, resample="triangle"):
    """jxl_resize_params for planes of `shape` (height, width): size = (out height, out width); box = (x0, y0, width, height) in
    source pixels (default: the whole image); resample: a key of RESIZE_FILTERS or an abi.RESIZE_* code"""
    r = abi.ResizeParams()
    x0, y0, bw, bh = (0, 0, shape[1], shape[0]) if box is None else box
    r.box_x0, r.box_y0, r.box_width, r.box_height = int(x0), int(y0), int(bw), int(bh)
    r.out_height, r.out_width = int(size[0]), int(size[1])
    r.filter = RESIZE_FILTERS[resample] if isinstance(resample, str) else int(resample)
    return r


def tensorResized(ctx, planes, alpha, out_ptr, size, box=None, resample="triangle", **params):
    """tensorSamples with a resample to `size` in the same pass (jxl_stage_tensor_resized): the box of the planes is filtered
    behind the colour stages 1-5 (in linear light where the stages pass through it), the output curve and the tensor's tail
    run per output pixel. out_ptr: DEVICE memory for size[0] * size[1] * channels elements. size / box / resample:
    resizeParams'; params: tensorParams' keywords. Returns (jxl_tensor_params, jxl_resize_params)."""
    planes = [np.ascontiguousarray(a) for a in planes]
    shape = planes[0].shape
    a = _png_alpha(alpha, shape)
    p = tensorParams(planes, shape, alpha=a, **params)
    r = resizeParams(shape, size, box, resample)
    ctx.call("jxl_stage_tensor_resized", _pv(planes), _vp(a), C.byref(p), C.byref(r), C.c_void_p(int(out_ptr)))
    return p, r


def tensorBatchItem(size, box=None, resample="triangle", planes=None, alpha=None, canvas=None, resident=None, nColor=3, alphaPlane=None,
                    **params):
    """One jxl_tensor_batch_item: an image where it is, its parameters and its box. Exactly one home: `planes` (host arrays, with
    the host plane `alpha`), `resident` (a ResidentPlanes, with the host plane `alpha`) or `canvas` (a DeviceCanvas: planes
    0 .. nColor - 1 and the plane alphaPlane). size / box / resample: resizeParams'; params: tensorParams' keywords. The item
    keeps the host arrays it points to alive (item.keep)."""
    if (planes is not None) + (resident is not None) + (canvas is not None) != 1:
        raise ValueError("one home: planes, resident or canvas")
    it = abi.TensorBatchItem()
    it.set_id, it.alpha_plane = -1, -1
    if canvas is not None:
        canvas._live()
        ap = -1 if alphaPlane is None else int(alphaPlane)
        a = None if ap < 0 else np.broadcast_to(np.zeros((), _PLANE_DTYPE[canvas.types[ap]]), canvas.shape)
        shape, stand, keep = canvas.shape, canvas._stand_ins(nColor), []
        it.source, it.set_id, it.alpha_plane = abi.BATCH_SET, int(canvas.id), ap
    elif resident is not None:
        resident._need_live()
        shape, stand = resident.shape, resident._stand_ins()
        a = _png_alpha(alpha, shape)
        keep = [a]
        it.source = abi.BATCH_RESIDENT
        it.alpha = None if a is None else a.ctypes.data
    else:
        stand = [np.ascontiguousarray(pl) for pl in planes]
        shape = stand[0].shape
        a = _png_alpha(alpha, shape)
        keep = stand + [a]
        it.source = abi.BATCH_HOST
        for c, pl in enumerate(stand):
            it.in_[c] = pl.ctypes.data
        it.alpha = None if a is None else a.ctypes.data
    it.p = tensorParams(stand, shape, alpha=a, **params)
    it.r = resizeParams(shape, size, box, resample)
    it.keep = keep
    return it


def tensorResizedBatch(ctx, items, out_ptr):
    """N images resampled into one batch tensor in ONE launch (jxl_tensor_resized_batch). items: tensorBatchItem()s that agree
    on size, dtype, layout and channel count; item i is written dense at out_ptr + i * (one tensor's bytes), bit for bit what
    tensorResized of its home writes. out_ptr: DEVICE memory for all of them. All or nothing; complete on return."""
    items = list(items)
    arr = (abi.TensorBatchItem * max(1, len(items)))(*items)  # (the items stay referenced, and with them their host arrays)
    ctx.call("jxl_tensor_resized_batch", len(items), arr, C.c_void_p(int(out_ptr)))
    return arr


def pfmParams(planes, shape, taggedDepths=None):
    """jxl_pfm_params of 1 or 3 planes (each one's dtype tells int32 from float32). taggedDepths: image.getTaggedBitDepth(c)
    per plane, looked at for the int32 planes only"""
    p = abi.PfmParams()
    p.height, p.width, p.n_planes = int(shape[0]), int(shape[1]), len(planes)
    for c, a in enumerate(planes[:3]):
        p.is_int[c] = int(a.dtype == np.int32)
        p.tagged_depth[c] = int(taggedDepths[c]) if taggedDepths is not None else 0
    return p


def pfmSamples(ctx, planes, taggedDepths=None):
    """PFMWriter.write's samples of 1 (grey) or 3 planes (2-D; int32 and float32 may be mixed) in one device pass
    (jxl_stage_pfm_samples): int32 planes cast with their tagged depth, Float.floatToIntBits, big-endian, channels interleaved,
    rows bottom to top. Returns [h][w][planes] uint8 x 4: the file's bytes after the header."""
    planes = [np.ascontiguousarray(a) for a in planes]
    shape = planes[0].shape
    for a in planes:
        if a.dtype not in (np.int32, np.float32) or a.shape != shape or a.ndim != 2:
            raise TypeError("the planes must be 2-D int32 or float32 arrays of one shape")
    p = pfmParams(planes, shape, taggedDepths)
    out = np.empty((shape[0], shape[1], len(planes), 4), np.uint8)
    ctx.call("jxl_stage_pfm_samples", _pv(planes), C.byref(p), _vp(out))
    return out


def varblocks(ctx, planes, blocks, cells):
    """Frame.drawVarblocks (Frame.java:464-503) on three float planes (jxl_stage_varblocks): every block (cy, cx, type) of
    `blocks` -- frame cells of 8 x 8 pixels on the cells = (cells_h, cells_w) grid -- tints its extent by its type and
    blackens its top row and left column; pixels outside the planes or inside no block stay. Returns new planes"""
    pl = _planes(planes, np.float32)
    out = np.empty_like(pl)
    d, keep = abi.make_varblock_desc(blocks, cells)
    ctx.call("jxl_stage_varblocks", _p3(pl, C.c_float), pl.shape[1], pl.shape[2], C.byref(d), _p3(out, C.c_float))
    return out


def pack_sparse(planes, wide=False):
    """The sparse wire format of include/jxlatte_amd.h: the non-zero samples of a 2-D integer plane (at most 256 x 256: one
    group of one channel) as a uint32 array of entries in raster order -- narrow: value << 16 | y << 8 | x; wide: the words
    (y << 8 | x, value) per entry. A sequence of planes gives a list. wide=False refuses a value outside int16."""
    if not (isinstance(planes, np.ndarray) and planes.ndim == 2):
        return [pack_sparse(a, wide) for a in planes]
    a = planes
    if a.shape[0] > 256 or a.shape[1] > 256:
        raise ValueError("a group's plane is at most 256x256, not %dx%d" % a.shape)
    ys, xs = np.nonzero(a)
    v = a[ys, xs].astype(np.int64)
    pos = (ys.astype(np.uint32) << 8) | xs.astype(np.uint32)
    if wide:
        if v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31):
            raise ValueError("value outside int32")
        out = np.empty(2 * v.size, np.uint32)
        out[0::2] = pos
        out[1::2] = (v & 0xffffffff).astype(np.uint32)
        return out
    if v.size and (v.min() < -32768 or v.max() > 32767):
        raise ValueError("value outside int16: use wide=True")
    return ((v & 0xffff).astype(np.uint32) << 16) | pos


def unpack_sparse(entries, shape, wide=False):
    """inverse of pack_sparse: the int32 plane of `shape` that the entries describe (a list of entry arrays with a list of
    shapes gives a list). Duplicate positions add, as on the device; a position outside the plane is a ValueError."""
    if not (isinstance(entries, np.ndarray) and entries.ndim == 1):
        return [unpack_sparse(e, s, wide) for e, s in zip(entries, shape)]
    e = entries.astype(np.uint32, copy=False)
    if wide:
        pos, val = e[0::2], np.ascontiguousarray(e[1::2]).view(np.int32)
    else:
        pos, val = e & 0xffff, (e >> 16).astype(np.uint16).view(np.int16).astype(np.int32)
    ys, xs = (pos >> 8).astype(np.int64), (pos & 255).astype(np.int64)
    if pos.size and (int(pos.max()) >> 16 or ys.max() >= shape[0] or xs.max() >= shape[1]):
        raise ValueError("entry outside the %dx%d plane" % tuple(shape))
    out = np.zeros(shape, np.int64)
    np.add.at(out, (ys, xs), val.astype(np.int64))
    return (out & 0xffffffff).astype(np.uint32).view(np.int32)


class Frame:
    """VarDCT side of J/frame/Frame.java: decodePassGroups tail (Frame.java:361-374), Gab, EPF and the
    colour transform of JXLCodestreamDecoder.performColorTransforms, as one device submission.

        fr = Frame(ctx, params, weights, woffs)
        fr.setLFGroup(g) ...            # HFMetadata / LFCoefficients side info, per LF group
        fr.putGroup(pass_, group, q)    # HFCoefficients.quantizedCoeffs of one (pass, group)
        planes = fr.decodeFrame()       # run + read back
    """

    def __init__(self, ctx, params, weights, woffs):
        self.ctx = ctx
        self.params = params
        self.width, self.height = params.width, params.height
        ctx.call("jxl_vardct_begin_frame", C.byref(params))
        weights = np.ascontiguousarray(weights, np.float32)
        woffs = np.ascontiguousarray(woffs, np.int32)
        ctx.call("jxl_vardct_set_weights", abi.fptr(weights), weights.size, abi.iptr(woffs))

    def setLFGroup(self, g):
        d = abi.make_lfgroup_desc(g)
        self.ctx.call("jxl_vardct_set_lfgroup", C.byref(d))

    def setLFGroupQuant(self, lfg_y, lfg_x, lfQuant, scaledDequant, extraPrecision=0, xFactorLF=128, bFactorLF=128,
                        adaptiveSmoothing=True):
        """row f1: hand over the integer LF image of an LF group instead of the dequantised floats"""
        q = [np.ascontiguousarray(lfQuant[c], np.int32) for c in range(3)]  # planes differ in size when chroma-subsampled
        d = abi.make_lfquant_desc(q, scaledDequant, extraPrecision, xFactorLF, bFactorLF, adaptiveSmoothing, lfg_y, lfg_x)
        self.ctx.call("jxl_vardct_set_lfgroup_lfquant", C.byref(d))

    @staticmethod
    def _rows(a, dt):
        """a 2-D plane as the ABI takes it: samples of a row consecutive, rows `stride` elements apart -- views with a row
        stride (a rectangle of a larger plane, page-locked or not) are passed as they are, anything else is made contiguous"""
        a = np.asarray(a)
        if a.dtype != dt or a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] % a.itemsize or a.strides[0] < a.shape[1] * a.itemsize:
            a = np.ascontiguousarray(a, dt)
        return a

    def putGroup(self, pass_, group, q):
        q = [self._rows(a, np.int32) for a in q]
        pp = (C.POINTER(C.c_int32) * 3)(*[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in q])
        strides = (C.c_int32 * 3)(*[a.strides[0] // 4 for a in q])
        self.ctx.call("jxl_vardct_put_group", pass_, group, pp, strides)
        self._keep = getattr(self, "_keep", []) + [q]  # aligned page-locked sources are read in place: keep them alive until run()

    def putGroupI16(self, pass_, group, q):
        """the int16 wire format (jxl_vardct_put_group_i16): the caller has checked that every |q| fits"""
        q = [self._rows(a, np.int16) for a in q]
        pp = (C.POINTER(C.c_int16) * 3)(*[a.ctypes.data_as(C.POINTER(C.c_int16)) for a in q])
        strides = (C.c_int32 * 3)(*[a.strides[0] // 2 for a in q])
        self.ctx.call("jxl_vardct_put_group_i16", pass_, group, pp, strides)
        self._keep = getattr(self, "_keep", []) + [q]  # aligned page-locked sources are read in place: keep them alive until run()

    def mapCoeffsI16(self, no_fill=False):
        """the frame's three coefficient planes as numpy views over the library's page-locked staging buffer
        (jxl_vardct_map_coeffs_i16): write the groups in place, then commitCoeffsI16(). no_fill: the planes are not
        zero-filled (jxl_vardct_map_coeffs_i16_ex, JXL_MAP_NO_FILL); commit then takes the list of written groups"""
        pp = (C.POINTER(C.c_int16) * 3)()
        strides = (C.c_int32 * 3)()
        if no_fill:
            self.ctx.call("jxl_vardct_map_coeffs_i16_ex", pp, strides, 1)
        else:
            self.ctx.call("jxl_vardct_map_coeffs_i16", pp, strides)
        p = self.params
        out = []
        for c in range(3):
            h, w = self.height >> p.jpeg_upsampling_y[c], self.width >> p.jpeg_upsampling_x[c]
            buf = (C.c_int16 * (h * w)).from_address(C.addressof(pp[c].contents))
            out.append(np.frombuffer(buf, dtype=np.int16).reshape(h, w))
        return out

    def commitCoeffsI16(self, written=None):
        """written: one flag per group (Frame group order) -- the groups whose rectangles were fully written; the others read
        as zero (jxl_vardct_commit_coeffs_i16_groups). None: everything in the mapped planes counts."""
        if written is None:
            self.ctx.call("jxl_vardct_commit_coeffs_i16")
        else:
            w = np.ascontiguousarray(written, np.uint8)
            self.ctx.call("jxl_vardct_commit_coeffs_i16_groups", w.ctypes.data_as(C.POINTER(C.c_uint8)), int(w.size))

    def putGroupSparse(self, pass_, group, q, wide=None):
        """putGroup with the sparse wire format (jxl_vardct_put_group_sparse): the non-zero samples of the three planes as
        (position, value) entries. wide=None picks the narrow form unless a value does not fit int16."""
        q = [np.asarray(a) for a in q]
        if wide is None:
            wide = any(a.size and (int(a.min()) < -32768 or int(a.max()) > 32767) for a in q)
        self.putGroupSparseEntries(pass_, group, [pack_sparse(a, wide) for a in q], wide)

    def putGroupSparseEntries(self, pass_, group, entries, wide=False):
        """entries: three uint32 arrays of packed entries (pack_sparse), handed over as they are -- page-locked, 16-byte
        aligned ones are read by the device in place"""
        e = [a if (isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.ndim == 1 and a.flags["C_CONTIGUOUS"])
             else np.ascontiguousarray(a, np.uint32).reshape(-1) for a in entries]
        per = 2 if wide else 1
        pp = (C.POINTER(C.c_uint32) * 3)(*[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in e])
        n = (C.c_int32 * 3)(*[a.size // per for a in e])
        self.ctx.call("jxl_vardct_put_group_sparse", pass_, group, pp, n, abi.SPARSE_WIDE if wide else 0)
        self._keep = getattr(self, "_keep", []) + [e]  # in-place sources: keep them alive until run()

    def mapSparse(self, capacity):
        """the library's page-locked entry buffer of `capacity` uint32 words as a numpy view (jxl_vardct_map_sparse): write
        runs of entries into it, then commitSparse(runs)"""
        p = C.POINTER(C.c_uint32)()
        self.ctx.call("jxl_vardct_map_sparse", C.c_size_t(int(capacity)), C.byref(p))
        buf = (C.c_uint32 * int(capacity)).from_address(C.addressof(p.contents))
        return np.frombuffer(buf, dtype=np.uint32)

    def commitSparse(self, runs):
        """runs: (group, channel, offset_words, count, wide) per run (jxl_vardct_commit_sparse); entries ADD into the planes"""
        arr = (abi.SparseRun * max(1, len(runs)))()
        for i, (g, ch, off, cnt, wide) in enumerate(runs):
            arr[i].group, arr[i].channel, arr[i].offset_words, arr[i].count = int(g), int(ch), int(off), int(cnt)
            arr[i].flags = wide if isinstance(wide, int) and not isinstance(wide, bool) else (abi.SPARSE_WIDE if wide else 0)
        self.ctx.call("jxl_vardct_commit_sparse", arr, len(runs))

    def sparseRejected(self):
        """entries the device refused since begin_frame (jxl_vardct_sparse_rejected); waits for the stream"""
        n = C.c_int64()
        self.ctx.call("jxl_vardct_sparse_rejected", C.byref(n))
        return n.value

    def run(self):
        """enqueue all stages (asynchronous)"""
        self.ctx.call("jxl_vardct_run")

    @staticmethod
    def runBatch(frames):
        """enqueue a batch of independent frames (one context each): jxl_vardct_run_batch -- the inverse-transform
        stage of all frames shares its launches; results equal those of frame.run() on every frame"""
        from ._lib import check
        hs = (C.c_void_p * len(frames))(*[f.ctx.h for f in frames])
        c0 = frames[0].ctx
        check(c0.h, c0.lib.jxl_vardct_run_batch(hs, len(frames)))

    def _out_array(self):
        es = self.ctx.lib.jxl_vardct_out_elem_size(self.ctx.h)
        p = self.params
        as_int = (p.stages & abi.STAGE_OUT) and p.out_format != abi.OUT_F32
        dt = {4: np.int32 if as_int else np.float32, 2: np.uint16, 1: np.uint8}[es]
        if as_int and p.out_format in (abi.OUT_RGB8, abi.OUT_RGB16):  # row f3: one pixel-interleaved buffer
            return np.empty((self.height, self.width, 3), dt)
        return np.empty((3, self.height, self.width), dt)

    def readOutput(self):
        out = self._out_array()
        if out.shape[-1] == 3 and out.ndim == 3 and out.shape[0] == self.height and out.dtype != np.float32 and \
                self.params.out_format in (abi.OUT_RGB8, abi.OUT_RGB16):
            pp = (C.c_void_p * 3)(out.ctypes.data, None, None)
        else:
            pp = (C.c_void_p * 3)(*[out[c].ctypes.data for c in range(3)])
        self.ctx.call("jxl_vardct_read_output", pp, self.width)
        return out

    def readOutputBegin(self, out=None):
        """queue the copy of the result to the host and return the destination array (jxl_vardct_read_output_begin); valid
        after readOutputWait(). `out`: a (page-locked) array of the result's shape to copy into"""
        if out is None:
            out = self._out_array()
        if self.params.out_format in (abi.OUT_RGB8, abi.OUT_RGB16) and (self.params.stages & abi.STAGE_OUT):
            pp = (C.c_void_p * 3)(out.ctypes.data, None, None)
        else:
            pp = (C.c_void_p * 3)(*[out[c].ctypes.data for c in range(3)])
        self.ctx.call("jxl_vardct_read_output_begin", pp, self.width)
        self._pending_out = out
        return out

    def readOutputWait(self):
        self.ctx.call("jxl_vardct_read_output_wait")
        out, self._pending_out = self._pending_out, None
        return out

    def decodeFrame(self):
        self.run()
        return self.readOutput()

    def lastLaunchCount(self):
        return self.ctx.lib.jxl_vardct_last_launch_count(self.ctx.h)

    def lastRestoreLaunches(self):
        """the fused restoration launches of the context's last run, one code each (jxl_debug_last_restore_launches, a test hook
        outside the C-ABI): [] when the stage kernels ran instead, two for the split three-iteration form. A code is
        restore_fused_variant() of the launch -- Gaborish 64 | EPF iterations << 3 | sink kind -- | 128 for cell-tiled input
        planes | 256 for a batch launch, which every context of the batch reports"""
        return lastRestoreLaunches(self.ctx)

    def keepPlanes(self, *window):
        """run, and keep a window of the result on the device for the stages that follow decodeFrame
        (JXLCodestreamDecoder.java:628-637): -> ResidentPlanes. window: (height, width), the top-left window
        (jxl_planes_from_frame), or (y0, x0, height, width), any window (jxl_planes_from_frame_at)"""
        if len(window) not in (2, 4):
            raise TypeError("keepPlanes takes (height, width) or (y0, x0, height, width)")
        self.run()
        self.ctx.call("jxl_planes_from_frame" if len(window) == 2 else "jxl_planes_from_frame_at", *[int(v) for v in window])
        return ResidentPlanes(self.ctx)

    @classmethod
    def from_synth(cls, ctx, frame, stages=None, via_groups=True):
        """feed a synth.make_vardct_frame dict through the boundary exactly as the Java host would:
        per LF group side info, per (pass, group) coefficient planes."""
        from . import synth
        p = abi.VarDCTParams.from_buffer_copy(frame["params"])
        if stages is not None:
            p.stages = stages
        fr = cls(ctx, p, frame["weights"], frame["woffs"])
        for g in frame["lfgroups"]:
            fr.setLFGroup(g)
        for grp in range(synth.num_groups(frame)):
            fr.putGroup(0, grp, synth.group_view(frame, grp))
        return fr


def lastRestoreLaunches(ctx):
    """Frame.lastRestoreLaunches of a context"""
    fn = ctx.lib.jxl_debug_last_restore_launches
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]
    codes = (C.c_int32 * 2)()
    n = fn(ctx.h, codes)
    return [int(codes[i]) for i in range(n)]


class PinnedArray:
    """numpy view over page-locked host memory from jxl_host_alloc (what a JNI caller wraps with NewDirectByteBuffer): copies
    to / from it are direct DMA, and put_group does not wait for them"""

    def __init__(self, lib, shape, dtype):
        self.lib = lib
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib.jxl_host_alloc(max(n, 1))
        if not self.ptr:
            raise MemoryError("jxl_host_alloc(%d)" % n)
        buf = (C.c_char * max(n, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            self.lib.jxl_host_free(self.ptr)
            self.ptr = None


class ResidentPlanes:
    """the frame's three colour planes on the device between decodeFrame and the blend: Frame.upsample (Frame.java:217-260),
    initializeNoise + synthesizeNoise (:748-831), performColorTransforms (JXLCodestreamDecoder.java:256-276), in the
    reference's order; Frame.renderSplines (Frame.java:739-746) may stay on the device too (splines). The host hook
    (download / upload) is needed only where a host-side stage wants the samples: patches (copies and blends out of host-side
    reference frames), saveBeforeCT, and the splines unless `splines` draws them."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._claim()

    def _claim(self):
        """a context has ONE set of resident planes: the object made last (keepPlanes, upload) or refilled last (replace) owns it"""
        self.gen = self.ctx.planes_gen = getattr(self.ctx, "planes_gen", 0) + 1

    def live(self):
        """the context's resident planes are still this object's (no later frame or upload has taken them)"""
        return getattr(self.ctx, "planes_gen", 0) == self.gen

    def _need_live(self):
        if not self.live():
            raise IllegalStateException(abi.JXL_ERR_STATE, "the context's resident planes now hold a later frame or upload")

    @classmethod
    def upload(cls, ctx, planes):
        pl = _planes(planes, np.float32)
        ctx.call("jxl_planes_upload", _p3(pl, C.c_float), pl[0].shape[0], pl[0].shape[1])
        return cls(ctx)

    @property
    def shape(self):
        h, w = C.c_int32(), C.c_int32()
        self.ctx.call("jxl_planes_shape", C.byref(h), C.byref(w))
        return h.value, w.value

    def upsample(self, k, upWeights):
        w = np.ascontiguousarray(upWeights, np.float32)
        assert w.size == k * k * 25
        self.ctx.call("jxl_planes_upsample", k, abi.fptr(w))

    def noise(self, groupDim, seed0, lut, baseCorrelationX, baseCorrelationB):
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == 8
        self.ctx.call("jxl_planes_noise", groupDim, C.c_uint64(seed0), abi.fptr(lut), C.c_float(baseCorrelationX),
                      C.c_float(baseCorrelationB))

    def noiseAt(self, groupDim, seed0, lut, baseCorrelationX, baseCorrelationB, frameHeight, frameWidth, y0, x0):
        """the planes are the window at (y0, x0) of a frameHeight x frameWidth frame: the whole frame's initializeNoise +
        synthesizeNoise restricted to it (jxl_planes_noise_at)"""
        self._need_live()
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == 8
        self.ctx.call("jxl_planes_noise_at", groupDim, C.c_uint64(seed0 & 0xFFFFFFFFFFFFFFFF), abi.fptr(lut), C.c_float(baseCorrelationX),
                      C.c_float(baseCorrelationB), int(frameHeight), int(frameWidth), int(y0), int(x0))

    def splines(self, splines, baseCorrelationX, baseCorrelationB):
        """Frame.renderSplines on the resident planes (jxl_planes_splines): after upsample / the patches, before noise"""
        d, keep = abi.make_spline_desc(splines, baseCorrelationX, baseCorrelationB)
        self.ctx.call("jxl_planes_splines", C.byref(d))

    def patches(self, extras, ref, pos, blend, ec_is_alpha, ec_alpha_associated):
        """computePatches on the resident colour planes (jxl_planes_patches): after upsample, before the splines. extras: the
        frame's extra channels (C-contiguous host planes; those a position writes are updated in place); ref as for
        computePatches, with 3 + len(extras) planes per slot"""
        n_chan = 3 + len(extras)
        ft = np.array([0, 0, 0] + [_patch_type(a) for a in extras], np.int32)
        for a in extras:
            if not a.flags["C_CONTIGUOUS"] or a.shape != self.shape:
                raise ValueError("dense extra channels of the resident planes' size")
        desc, pp, rt, keep = _patch_call_args(ft, n_chan, ref, pos, blend, 3, ec_is_alpha, ec_alpha_associated)
        ep = (C.c_void_p * max(1, len(extras)))(*[_vp(a) for a in extras])
        et = np.ascontiguousarray(ft[3:]) if len(extras) else np.zeros(1, np.int32)
        self.ctx.call("jxl_planes_patches", C.byref(desc), ep, abi.iptr(et), pp, abi.iptr(rt))

    def invertXYB(self, matrix, opsin_bias, cbrt_opsin_bias, intensityTarget):
        m = OpsinInverseMatrix(matrix, opsin_bias, cbrt_opsin_bias)
        self.ctx.call("jxl_planes_xyb", abi.f9(*m.matrix), abi.f3(*m.opsinBias), abi.f3(*m.cbrtOpsinBias), C.c_float(intensityTarget))

    def ycbcr(self):
        self.ctx.call("jxl_planes_ycbcr")

    def _stand_ins(self):
        return [np.broadcast_to(np.float32(0), self.shape)] * 3  # shape and dtype for colorParams; never read

    def orient(self, orientation):
        """JXLCodestreamDecoder.transposeBuffer of the three planes, on the device (jxl_planes_orient)"""
        self._need_live()
        self.ctx.call("jxl_planes_orient", int(orientation))

    def colorPeak(self, **params):
        """determinePeak of the planes as they stand (jxl_planes_color_peak; colorParams' keywords)"""
        self._need_live()
        p = colorParams(self._stand_ins(), **params)
        peak = C.c_float(0)
        self.ctx.call("jxl_planes_color_peak", C.byref(p), C.byref(peak))
        return np.float32(peak.value)

    def pngSamples(self, alpha=None, **params):
        """pngSamples of the planes as they stand (jxl_planes_png_samples): only the alpha plane goes up, only the PNG's
        samples come down"""
        self._need_live()
        shape = self.shape
        a = _png_alpha(alpha, shape)
        p = pngParams(self._stand_ins(), shape, alpha=a, **params)
        out = _png_out(self.ctx, p, shape)
        self.ctx.call("jxl_planes_png_samples", _vp(a), C.byref(p), _vp(out))
        return out

    def tensorSamples(self, out_ptr, alpha=None, **params):
        """tensorSamples of the planes as they stand (jxl_planes_tensor_samples) to the device address out_ptr: only the alpha
        plane goes up, nothing comes down"""
        self._need_live()
        shape = self.shape
        a = _png_alpha(alpha, shape)
        p = tensorParams(self._stand_ins(), shape, alpha=a, **params)
        self.ctx.call("jxl_planes_tensor_samples", _vp(a), C.byref(p), C.c_void_p(int(out_ptr)))
        return p

    def tensorResized(self, out_ptr, size, box=None, resample="triangle", alpha=None, **params):
        """tensorResized of the planes as they stand (jxl_planes_tensor_resized) to the device address out_ptr: only the alpha
        plane goes up, nothing comes down"""
        self._need_live()
        shape = self.shape
        a = _png_alpha(alpha, shape)
        p = tensorParams(self._stand_ins(), shape, alpha=a, **params)
        r = resizeParams(shape, size, box, resample)
        self.ctx.call("jxl_planes_tensor_resized", _vp(a), C.byref(p), C.byref(r), C.c_void_p(int(out_ptr)))
        return p, r

    def pfmSamples(self):
        """pfmSamples of the planes as they stand (jxl_planes_pfm_samples): nothing goes up, only the PFM's bytes come down"""
        self._need_live()
        shape = self.shape
        p = pfmParams(self._stand_ins(), shape)
        out = np.empty((shape[0], shape[1], 3, 4), np.uint8)
        self.ctx.call("jxl_planes_pfm_samples", C.byref(p), _vp(out))
        return out

    def varblocks(self, blocks, cells):
        """Frame.drawVarblocks on the planes as they stand, in place (jxl_planes_varblocks): after the colour transforms; only
        the cell map and the factor table go up"""
        self._need_live()
        d, keep = abi.make_varblock_desc(blocks, cells)
        self.ctx.call("jxl_planes_varblocks", C.byref(d))

    def download(self):
        h, w = self.shape
        out = np.empty((3, h, w), np.float32)
        self.ctx.call("jxl_planes_download", _p3(out, C.c_float))
        return out

    def replace(self, planes):
        pl = _planes(planes, np.float32)
        self.ctx.call("jxl_planes_upload", _p3(pl, C.c_float), pl[0].shape[0], pl[0].shape[1])
        self._claim()


class ModularChannel:
    """J/frame/modular/ModularChannel.java (squeeze part)"""

    @staticmethod
    def inverseHorizontalSqueeze(ctx, orig, res):
        orig = np.ascontiguousarray(orig, np.int32)
        res = np.ascontiguousarray(res, np.int32)
        h, aw = orig.shape
        if res.shape[0] != h:
            raise ValueError("Corrupted squeeze transform")  # ModularChannel.java:363-366
        out = np.empty((h, aw + res.shape[1]), np.int32)
        ctx.call("jxl_stage_inv_hsqueeze", abi.iptr(orig), aw, abi.iptr(res), res.shape[1], h, abi.iptr(out))
        return out

    @staticmethod
    def inverseVerticalSqueeze(ctx, orig, res):
        orig = np.ascontiguousarray(orig, np.int32)
        res = np.ascontiguousarray(res, np.int32)
        ah, w = orig.shape
        if res.shape[1] != w:
            raise RuntimeError("Corrupted squeeze transform")  # ModularChannel.java:391-394 (IllegalStateException)
        out = np.empty((ah + res.shape[0], w), np.int32)
        ctx.call("jxl_stage_inv_vsqueeze", abi.iptr(orig), ah, abi.iptr(res), res.shape[0], w, abi.iptr(out))
        return out


class ModularStream:
    """Transform part of J/frame/modular/ModularStream.java: the channel list as decoded by the host
    (averages + residuals) plus the squeeze parameters; applyTransforms() undoes Squeeze (and RCT).
    transforms= (instead of squeezeParams / rctType): the whole frame-level chain in bitstream order, the dictionaries
    frontend.transforms() returns, undone on the device in one plan (jxl_modular_begin_chain); channels is then the encoded
    list with its meta channels -- a Palette's palette is channel 0's own data -- and bitDepth the image's."""

    def __init__(self, ctx, channels, squeezeParams=(), rctType=-1, rctBegin=0, transforms=None, bitDepth=8):
        self.ctx = ctx
        self.channels = [np.ascontiguousarray(c, np.int32) for c in channels]
        self.sp = [tuple(int(v) for v in s) for s in squeezeParams]
        self.rctType, self.rctBegin = rctType, rctBegin
        self.transforms = None if transforms is None else [dict(t) for t in transforms]
        self.bitDepth = int(bitDepth)
        self.transformed = False
        self._begun = False

    @staticmethod
    def defaultSqueezeParams(shapes, nbMeta=0):
        """ModularStream.java:110-131 through the C-ABI (shapes: list of (h, w))"""
        from ._lib import load
        ws = np.array([s[1] for s in shapes], np.int32)
        hs = np.array([s[0] for s in shapes], np.int32)
        out = (abi.SqueezeParam * 64)()
        n = load().jxl_modular_default_squeeze_params(abi.iptr(ws), abi.iptr(hs), len(shapes), nbMeta, out, 64)
        if n < 0:
            raise ValueError("status %d" % n)
        return [out[i].as_tuple() for i in range(n)]

    @staticmethod
    def squeezedShapes(shapes, sp):
        from ._lib import load
        ws = np.array([s[1] for s in shapes], np.int32)
        hs = np.array([s[0] for s in shapes], np.int32)
        cap = len(shapes) + sum(p[3] for p in sp) + 1
        ow, oh = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = load().jxl_modular_squeezed_shapes(abi.iptr(ws), abi.iptr(hs), len(shapes), abi.make_squeeze_params(sp), len(sp),
                                               abi.iptr(ow), abi.iptr(oh), cap)
        if n < 0:
            raise ValueError("status %d" % n)
        return [(int(oh[i]), int(ow[i])) for i in range(n)]

    def begin(self):
        ca = abi.make_channels(self.channels)
        if self.transforms is not None:
            tr, keep = abi.make_transforms(self.transforms)
            self.ctx.call("jxl_modular_begin_chain", ca, len(self.channels), tr, len(self.transforms), self.bitDepth)
        else:
            self.ctx.call("jxl_modular_begin", ca, len(self.channels), abi.make_squeeze_params(self.sp), len(self.sp),
                          self.rctType, self.rctBegin)
        self._begun = True

    def run(self):
        if not self._begun:
            self.begin()
        self.ctx.call("jxl_modular_run")

    def getDecodedBuffer(self):
        lib, h = self.ctx.lib, self.ctx.h
        outs = []
        for i in range(lib.jxl_modular_out_count(h)):
            w, hh = C.c_int32(), C.c_int32()
            check(h, lib.jxl_modular_out_shape(h, i, C.byref(w), C.byref(hh)))
            a = np.empty((hh.value, w.value), np.int32)
            self.ctx.call("jxl_modular_read_channel", i, abi.iptr(a) if a.size else None)
            outs.append(a)
        return outs

    def applyTransforms(self):
        """ModularStream.applyTransforms (ModularStream.java:224-380): idempotent like the reference"""
        if self.transformed:
            return self.channels
        self.transformed = True
        self.run()
        self.channels = self.getDecodedBuffer()
        return self.channels


def rct(ctx, v, rctType):
    """RCT branch of ModularStream.applyTransforms (ModularStream.java:255-326)"""
    out = np.array(v, np.int32, order="C", copy=True)
    pp = (C.POINTER(C.c_int32) * 3)(*[abi.iptr(out[c]) for c in range(3)])
    ctx.call("jxl_stage_rct", pp, out[0].size, rctType)
    return out


def inversePalette(ctx, index, palette, numC, nbColors, nbDeltas, dPred, bitDepth, pred=None):
    """Palette branch of ModularStream.applyTransforms (ModularStream.java:327-378) for one transform (jxl_stage_palette):
    index is the h x w index channel, palette the stream's channel 0 (2-D), pred the weighted predictor's values as decoded
    (read for dPred 6). Returns the numC planes as one (numC, h, w) array"""
    idx = np.ascontiguousarray(index, np.int32)
    h, w = idx.shape
    d, keep = abi.make_palette_desc(palette, pred, numC, nbColors, nbDeltas, dPred, bitDepth)
    out = np.empty((max(int(numC), 0), h, w), np.int32)
    pp = (C.POINTER(C.c_int32) * max(len(out), 1))(*[abi.iptr(a) for a in out])
    ctx.call("jxl_stage_palette", C.byref(d), abi.iptr(idx), h, w, pp)
    return out


def lastPalette(ctx):
    """(kernel launches, pixels with index < nbDeltas) of the context's last inversePalette that ran
    (jxl_debug_last_palette, a test hook outside the C-ABI): one launch, or two with the chain kernel behind the lookup"""
    fn = ctx.lib.jxl_debug_last_palette
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    deltas = C.c_int64(0)
    n = fn(ctx.h, C.byref(deltas))
    return int(n), int(deltas.value)


def setPaletteFuse(ctx, on):
    """forces a chain plan's Palette runs into the step form (on=False) or lets them fuse (jxl_debug_set_palette_fuse, a
    process-wide hook outside the C-ABI, read per run); returns the previous setting"""
    fn = ctx.lib.jxl_debug_set_palette_fuse
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    return bool(fn(1 if on else 0))


def lastPaletteRun(ctx):
    """(fused launches, step launches, redone runs) of the context's last jxl_modular_run with whatever its settle ran again
    (jxl_debug_last_palette_run); read it after the plan's outputs"""
    fn = ctx.lib.jxl_debug_last_palette_run
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 3)()
    fn(ctx.h, out)
    return tuple(int(v) for v in out)


def modularToFloat(ctx, a, b, scale):
    """Frame.decodeFrame modular -> float buffer (Frame.java:437-448)"""
    a = np.ascontiguousarray(a, np.int32)
    out = np.empty(a.shape, np.float32)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.int32)
        bp = abi.iptr(b)
    ctx.call("jxl_stage_modular_to_float", abi.iptr(a), bp, a.size, C.c_float(scale), abi.fptr(out))
    return out


# ---- rows f4 / f3: the pixel-domain functions either side of the colour transform -------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def invertSubsampling(ctx, channel, xShift, yShift):
    """Frame.invertSubsampling (Frame.java:681-723) for one channel"""
    a = np.ascontiguousarray(channel, np.float32)
    h, w = a.shape
    out = np.empty((h << yShift, w << xShift), np.float32)
    ctx.call("jxl_stage_chroma_upsample", abi.fptr(a), h, w, xShift, yShift, abi.fptr(out))
    return out


def getUpWeights(k, packed):
    """ImageHeader.getUpWeights (ImageHeader.java:441-470) for one k: [k][k][5][5]"""
    from ._lib import load
    packed = np.ascontiguousarray(packed, np.float32)
    need = {2: 15, 4: 55, 8: 210}.get(k)
    if need is None or packed.size != need:
        raise ValueError("k must be 2, 4 or 8 with 15 / 55 / 210 coefficients")
    out = np.empty((k, k, 5, 5), np.float32)
    st = load().jxl_upsampling_weights(k, abi.fptr(packed), abi.fptr(out))
    if st:
        raise ValueError("status %d" % st)
    return out


def performUpsampling(ctx, channel, k, upWeights):
    """Frame.performUpsampling (Frame.java:217-260)"""
    if k == 1:
        return channel
    a = np.ascontiguousarray(channel, np.float32)
    wts = np.ascontiguousarray(upWeights, np.float32)
    h, w = a.shape
    out = np.empty((h * k, w * k), np.float32)
    ctx.call("jxl_stage_upsample", abi.fptr(a), h, w, k, abi.fptr(wts), abi.fptr(out))
    return out


def initializeNoise(ctx, height, width, seed0, groupDim=256, colors=3):
    """Frame.initializeNoise (Frame.java:748-788)"""
    out = np.empty((colors, height, width), np.float32)
    pp = (C.POINTER(C.c_float) * 3)(*[abi.fptr(out[c]) for c in range(colors)])
    ctx.call("jxl_stage_noise_init", height, width, groupDim, C.c_uint64(seed0 & 0xFFFFFFFFFFFFFFFF), colors, pp)
    return out


def noiseWindow(ctx, planes, groupDim, seed0, lut, baseCorrelationX, baseCorrelationB, frameHeight, frameWidth, y0, x0):
    """Frame.initializeNoise + synthesizeNoise of a frameHeight x frameWidth frame on `planes` ([3][h][w] float32, X, Y, B), the
    frame's window at (y0, x0) (jxl_stage_noise_window); returns the new planes"""
    out = np.array(planes, np.float32, order="C", copy=True)
    lut = np.ascontiguousarray(lut, np.float32)
    assert out.ndim == 3 and out.shape[0] == 3 and lut.size == 8
    ctx.call("jxl_stage_noise_window", _p3(out, C.c_float), out.shape[1], out.shape[2], groupDim, C.c_uint64(seed0 & 0xFFFFFFFFFFFFFFFF),
             abi.fptr(lut), C.c_float(baseCorrelationX), C.c_float(baseCorrelationB), int(frameHeight), int(frameWidth), int(y0), int(x0))
    return out


def synthesizeNoise(ctx, planes, noise, lut, baseCorrelationX, baseCorrelationB):
    """Frame.synthesizeNoise (Frame.java:790-831); returns new planes"""
    out = np.array(planes, np.float32, order="C", copy=True)
    nz = np.ascontiguousarray(noise, np.float32)
    lut = np.ascontiguousarray(lut, np.float32)
    pp = (C.POINTER(C.c_float) * 3)(*[abi.fptr(out[c]) for c in range(3)])
    pn = (C.POINTER(C.c_float) * 3)(*[abi.fptr(nz[c]) for c in range(3)])
    ctx.call("jxl_stage_noise_add", pp, pn, out[0].size, abi.fptr(lut), C.c_float(baseCorrelationX), C.c_float(baseCorrelationB))
    return out


def spline_arcs(splines, baseCorrelationX, baseCorrelationB, height, width):
    """the arcs Frame.renderSplines draws into a height x width frame, in the reference's order (jxl_spline_arcs: host only,
    no context): a numpy record array of abi.SPLINE_ARC_DTYPE"""
    from ._lib import JxlError, load
    lib = load()
    d, keep = abi.make_spline_desc(splines, baseCorrelationX, baseCorrelationB)
    n = lib.jxl_spline_arcs(C.byref(d), height, width, None, 0)
    if n < 0:
        raise JxlError(int(n), "jxl_spline_arcs")
    out = np.zeros(int(n), abi.SPLINE_ARC_DTYPE)
    if n:
        m = lib.jxl_spline_arcs(C.byref(d), height, width, out.ctypes.data_as(C.POINTER(abi.SplineArc)), n)
        assert m == n
    return out


def renderSplines(ctx, planes, splines, baseCorrelationX, baseCorrelationB):
    """Frame.renderSplines (Frame.java:739-746) + Spline.renderSpline (Spline.java:27-200) on three float planes
    (jxl_stage_splines); returns new planes"""
    out = np.array(planes, np.float32, order="C", copy=True)
    if out.ndim != 3 or out.shape[0] != 3:
        raise ValueError("expected planes of shape (3, H, W)")
    d, keep = abi.make_spline_desc(splines, baseCorrelationX, baseCorrelationB)
    ctx.call("jxl_stage_splines", _p3(out, C.c_float), out.shape[1], out.shape[2], C.byref(d))
    return out


def _patch_type(a):
    if a.dtype == np.float32:
        return 0
    if a.dtype == np.int32:
        return 1
    raise TypeError("int32 or float32 planes")


def _patch_call_args(frame_types, n_chan, ref, pos, blend, n_color, ec_is_alpha, ec_alpha_associated):
    """the descriptor and the reference-plane arguments of the patch entries. ref: per slot None or a list of n_chan planes (None:
    a plane blendBuffers would create as zeros); a slot's planes have the size of its plane 0 (computePatches reads refBuffer[0]) --
    an all-zero plane of another size (one a frame before created at ITS size) goes as NULL too. Returns (desc, ref pointer
    array, ref type array, keepalive)."""
    shapes, planes, types = [None] * 4, [None] * (4 * n_chan), np.full(4 * n_chan, -1, np.int32)
    for k in range(4):
        if ref[k] is None:
            continue
        if len(ref[k]) != n_chan:
            raise ValueError("a reference slot holds %d planes, the frame %d" % (len(ref[k]), n_chan))
        shapes[k] = tuple(ref[k][0].shape)  # (AttributeError on a missing plane 0, as in the reference's refBuffer[0].height)
        for d, a in enumerate(ref[k]):
            if a is None:
                continue
            if tuple(a.shape) != shapes[k]:
                if a.any():
                    raise ValueError("planes of one reference slot differ in size")
                continue
            planes[k * n_chan + d] = np.ascontiguousarray(a)
            types[k * n_chan + d] = _patch_type(a)
    desc, keep = abi.make_patch_desc(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, shapes)
    pp = (C.c_void_p * (4 * n_chan))(*[_vp(a) for a in planes])
    return desc, pp, types, (keep, planes)


def patch_bins(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, height, width, frame_types, ref_shapes, ref_types):
    """validation and tile binning of one frame's patch stage (jxl_patch_bins: host only, no context). frame_types[d] /
    ref_types[k][d]: 0 float, 1 int32, -1 (reference planes) absent. Returns (tile, start, list); raises what the stage entries
    raise, with the offending position in `.position`."""
    from ._lib import _ERR, JxlError, load
    lib = load()
    desc, keep = abi.make_patch_desc(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, ref_shapes)
    ft = np.ascontiguousarray(frame_types, np.int32)
    rt = np.ascontiguousarray(ref_types, np.int32).reshape(-1)
    assert ft.size == n_color + len(ec_is_alpha) and rt.size == 4 * ft.size
    n_list, bad = C.c_int64(0), C.c_int32(-1)

    def call(tile, start, lst):
        n = lib.jxl_patch_bins(C.byref(desc), height, width, abi.iptr(ft), abi.iptr(rt), abi.iptr(tile) if tile is not None else None,
                               abi.iptr(start) if start is not None else None, abi.iptr(lst) if lst is not None else None,
                               0 if tile is None else tile.size, 0 if lst is None else lst.size, C.byref(n_list), C.byref(bad))
        if n < 0:
            msg = lib.jxl_last_error(None)
            err = _ERR.get(int(n), JxlError)(int(n), msg.decode("utf-8", "replace") if msg else "")
            err.position = bad.value
            raise err
        return int(n)
    n = call(None, None, None)
    tile, start, lst = np.zeros(max(n, 1), np.int32), np.zeros(n + 1, np.int32), np.zeros(max(n_list.value, 1), np.int32)
    assert call(tile, start, lst) == n
    return tile[:n], start, lst[:n_list.value]


def computePatches(ctx, frame, ref, pos, blend, n_color, ec_is_alpha, ec_alpha_associated):
    """JXLCodestreamDecoder.computePatches (JXLCodestreamDecoder.java:212-254) on the frame's planes (jxl_stage_patches): frame = list
    of C-contiguous int32 / float32 planes, updated IN PLACE and returned; the planes carry the types blendBuffers' casts would
    have given them (decoder.patch_type_plan)"""
    n_chan = len(frame)
    for a in frame:
        if not a.flags["C_CONTIGUOUS"] or a.shape != frame[0].shape:
            raise ValueError("dense planes of one size")
    ft = np.array([_patch_type(a) for a in frame], np.int32)
    desc, pp, rt, keep = _patch_call_args(ft, n_chan, ref, pos, blend, n_color, ec_is_alpha, ec_alpha_associated)
    fp = (C.c_void_p * n_chan)(*[_vp(a) for a in frame])
    ctx.call("jxl_stage_patches", C.byref(desc), fp, abi.iptr(ft), frame[0].shape[0], frame[0].shape[1], pp, abi.iptr(rt))
    return frame


def blend(ctx, mode, canvas, frame, ref, rect, frameAlpha=None, refAlpha=None, isAlpha=False, hasExtra=False, clamp=False,
          premult=False):
    """inner switch of JXLCodestreamDecoder.blendBuffers (JXLCodestreamDecoder.java:285-422); rect =
    (h, w, canvas_y, canvas_x, frame_y, frame_x, ref_y, ref_x); returns the updated canvas"""
    is_int = canvas.dtype == np.int32
    dt = np.int32 if is_int else np.float32
    cv = np.array(canvas, dt, order="C", copy=True)
    fr = np.ascontiguousarray(frame, dt) if frame is not None else None
    rf = np.ascontiguousarray(ref, dt) if ref is not None else None
    fa = np.ascontiguousarray(frameAlpha, np.float32) if frameAlpha is not None else None
    ra = np.ascontiguousarray(refAlpha, np.float32) if refAlpha is not None else None
    flags = (1 if isAlpha else 0) | (2 if hasExtra else 0) | (4 if clamp else 0) | (8 if premult else 0)
    r = abi.BlendRect(*[int(v) for v in rect])
    fh, fw = fr.shape if fr is not None else (fa.shape if fa is not None else (0, 0))
    rh, rw = rf.shape if rf is not None else (ra.shape if ra is not None else (0, 0))
    ctx.call("jxl_stage_blend", mode, flags, 1 if is_int else 0, _vp(cv), cv.shape[0], cv.shape[1], _vp(fr), fh, fw,
             _vp(rf), rh, rw, abi.fptr(fa) if fa is not None else None, abi.fptr(ra) if ra is not None else None, C.byref(r))
    # what jxl_stage_blend moves: the canvas both ways, and up the planes the mode reads (blend_ops.h: blend_op / blend_needs)
    add = mode == abi.BLEND_ADD or (not hasExtra and mode in (abi.BLEND_BLEND, abi.BLEND_MULADD))
    copy_ref = mode == abi.BLEND_MULADD and hasExtra and isAlpha
    reads = [cv, None if copy_ref else fr, None if mode == abi.BLEND_REPLACE else rf,
             fa if not add and not copy_ref and (mode == abi.BLEND_MULADD or (mode == abi.BLEND_BLEND and not isAlpha)) else None,
             ra if not add and mode == abi.BLEND_BLEND and not isAlpha else None]
    _bus(ctx, up=sum(a.nbytes for a in reads if a is not None), down=cv.nbytes)
    return cv


# ---- device plane sets: the canvas and the reference frames on the device (jxl_canvas_*) -------------------------------------
def _bus(ctx, up=0, down=0):
    """bytes the blend path moved over the bus, per context: ctx.blend_bus = [up, down]. Counted where the binding hands a host
    array to the library or takes one back: blend() and the DeviceCanvas transfers"""
    b = getattr(ctx, "blend_bus", None)
    if b is None:
        b = ctx.blend_bus = [0, 0]
    b[0] += int(up)
    b[1] += int(down)


def _plane_code(dtype):
    dt = np.dtype(dtype)
    if dt == np.float32:
        return abi.PLANE_FLOAT
    if dt == np.int32:
        return abi.PLANE_INT32
    raise TypeError("int32 or float32 planes")


_PLANE_DTYPE = {abi.PLANE_FLOAT: np.dtype(np.float32), abi.PLANE_INT32: np.dtype(np.int32)}


class DeviceCanvas:
    """a plane set of the context: ImageBuffer[] on the device (the canvas of JXLCodestreamDecoder.java:640-643, a frame's
    buffers, a reference slot). `types` mirrors the library's tags (abi.PLANE_FLOAT / PLANE_INT32 per plane)."""

    def __init__(self, ctx, id_, types, shape):
        self.ctx, self.id, self.types, self.shape = ctx, id_, list(types), tuple(shape)

    @classmethod
    def create(cls, ctx, types, height, width):
        """zero-filled planes (new ImageBuffer(type, height, width)); types: dtypes or plane codes"""
        codes = [int(t) if isinstance(t, (int, np.integer)) else _plane_code(t) for t in types]
        arr = np.array(codes if codes else [0], np.int32)
        id_ = C.c_int32(-1)
        ctx.call("jxl_canvas_create", len(codes), int(height), int(width), abi.iptr(arr), C.byref(id_))
        return cls(ctx, id_.value, codes, (int(height), int(width)))

    @classmethod
    def fromArrays(cls, ctx, arrays):
        """a set holding the host planes `arrays` (one shape; int32 or float32 each): one upload per plane"""
        cv = cls.create(ctx, [a.dtype for a in arrays], *arrays[0].shape)
        for i, a in enumerate(arrays):
            cv.upload(i, a)
        return cv

    @classmethod
    def fromPlanes(cls, ctx, extraTypes=()):
        """a set whose first three planes (float) hold a copy of the context's resident planes and whose other planes, of
        extraTypes, are zero until they are uploaded (jxl_canvas_from_planes): the colours cross no bus"""
        h, w = C.c_int32(), C.c_int32()
        ctx.call("jxl_planes_shape", C.byref(h), C.byref(w))
        codes = [int(t) if isinstance(t, (int, np.integer)) else _plane_code(t) for t in extraTypes]
        arr = np.array(codes if codes else [0], np.int32)
        id_ = C.c_int32(-1)
        ctx.call("jxl_canvas_from_planes", len(codes), abi.iptr(arr), C.byref(id_))
        return cls(ctx, id_.value, [abi.PLANE_FLOAT] * 3 + codes, (h.value, w.value))

    @classmethod
    def fromModular(cls, ctx, height, width, planes):
        """the Modular context's result channels as a new set (jxl_canvas_from_modular; Frame.java:430-455 for all planes as one
        launch): every plane a channel cropped to height x width. planes: per plane (channel, addChannel or -1, dtype or plane
        code, scale) -- an int32 plane is a copy, a float plane scale * (float)(a [+ b]). Nothing crosses the bus"""
        d = modularPlanesDesc(height, width, planes)
        id_ = C.c_int32(-1)
        ctx.call("jxl_canvas_from_modular", C.byref(d), C.byref(id_))
        return cls(ctx, id_.value, [d.plane[i].type for i in range(d.n_planes)], (int(height), int(width)))

    @classmethod
    def fromModularUp(cls, ctx, height, width, planes, k, upWeights):
        """the Modular context's result channels as a new set of UPSAMPLED float planes, k * height x k * width
        (jxl_canvas_from_modular_up): per plane Frame.performUpsampling (Frame.java:217-260) of castToFloat of the cropped
        channel, all planes as one launch. planes as fromModular's, every one float with its own scale (1f / maxValue);
        upWeights as performUpsampling's. Nothing but the weights crosses the bus"""
        d = modularPlanesDesc(height, width, planes)
        w = np.ascontiguousarray(upWeights, np.float32)
        if k in (2, 4, 8) and w.size != k * k * 25:
            raise ValueError("k * k * 25 upsampling weights")
        id_ = C.c_int32(-1)
        ctx.call("jxl_canvas_from_modular_up", C.byref(d), int(k), abi.fptr(w), C.byref(id_))
        return cls(ctx, id_.value, [abi.PLANE_FLOAT] * d.n_planes, (int(height) * int(k), int(width) * int(k)))

    def _live(self):
        if self.id is None:
            raise IllegalStateException(abi.JXL_ERR_STATE, "the plane set has been released")

    def _stand_ins(self, n):
        return [np.broadcast_to(np.zeros((), _PLANE_DTYPE[self.types[c]]), self.shape) for c in range(n)]  # shape and dtype only; never read

    def orient(self, orientation):
        """JXLCodestreamDecoder.transposeBuffer of every plane, on the device (jxl_canvas_orient)"""
        self._live()
        self.ctx.call("jxl_canvas_orient", self.id, int(orientation))
        if 5 <= int(orientation) <= 8:
            self.shape = (self.shape[1], self.shape[0])

    def colorPeak(self, nColor=3, **params):
        """determinePeak of planes 0 .. nColor - 1 as they stand (jxl_canvas_color_peak; colorParams' keywords)"""
        self._live()
        p = colorParams(self._stand_ins(nColor), **params)
        peak = C.c_float(0)
        self.ctx.call("jxl_canvas_color_peak", self.id, C.byref(p), C.byref(peak))
        return np.float32(peak.value)

    def pngSamples(self, nColor=3, alphaPlane=None, **params):
        """pngSamples of planes 0 .. nColor - 1 and the alpha plane alphaPlane of the set (jxl_canvas_png_samples; pngParams'
        keywords but `alpha`): nothing goes up, only the PNG's samples come down"""
        self._live()
        ap = -1 if alphaPlane is None else int(alphaPlane)
        alpha = None if ap < 0 else np.broadcast_to(np.zeros((), _PLANE_DTYPE[self.types[ap]]), self.shape)
        p = pngParams(self._stand_ins(nColor), self.shape, alpha=alpha, **params)
        out = _png_out(self.ctx, p, self.shape)
        self.ctx.call("jxl_canvas_png_samples", self.id, ap, C.byref(p), _vp(out))
        _bus(self.ctx, down=out.nbytes)
        return out

    def tensorSamples(self, out_ptr, nColor=3, alphaPlane=None, **params):
        """tensorSamples of planes 0 .. nColor - 1 and the alpha plane alphaPlane of the set (jxl_canvas_tensor_samples;
        tensorParams' keywords but `alpha`) to the device address out_ptr: nothing crosses the bus, so nothing is counted"""
        self._live()
        ap = -1 if alphaPlane is None else int(alphaPlane)
        alpha = None if ap < 0 else np.broadcast_to(np.zeros((), _PLANE_DTYPE[self.types[ap]]), self.shape)
        p = tensorParams(self._stand_ins(nColor), self.shape, alpha=alpha, **params)
        self.ctx.call("jxl_canvas_tensor_samples", self.id, ap, C.byref(p), C.c_void_p(int(out_ptr)))
        return p

    def tensorResized(self, out_ptr, size, box=None, resample="triangle", nColor=3, alphaPlane=None, **params):
        """tensorResized of planes 0 .. nColor - 1 and the alpha plane alphaPlane of the set (jxl_canvas_tensor_resized) to the
        device address out_ptr: nothing crosses the bus, so nothing is counted"""
        self._live()
        ap = -1 if alphaPlane is None else int(alphaPlane)
        alpha = None if ap < 0 else np.broadcast_to(np.zeros((), _PLANE_DTYPE[self.types[ap]]), self.shape)
        p = tensorParams(self._stand_ins(nColor), self.shape, alpha=alpha, **params)
        r = resizeParams(self.shape, size, box, resample)
        self.ctx.call("jxl_canvas_tensor_resized", self.id, ap, C.byref(p), C.byref(r), C.c_void_p(int(out_ptr)))
        return p, r

    def pfmSamples(self, nColor=3, taggedDepths=None):
        """pfmSamples of planes 0 .. nColor - 1 (jxl_canvas_pfm_samples): nothing goes up, only the PFM's bytes come down"""
        self._live()
        p = pfmParams(self._stand_ins(nColor), self.shape, taggedDepths)
        out = np.empty((self.shape[0], self.shape[1], nColor, 4), np.uint8)
        self.ctx.call("jxl_canvas_pfm_samples", self.id, C.byref(p), _vp(out))
        _bus(self.ctx, down=out.nbytes)
        return out

    @property
    def dtypes(self):
        return [_PLANE_DTYPE[t] for t in self.types]

    def __len__(self):
        return len(self.types)

    def clone(self):
        """new ImageBuffer(b) per plane (JXLCodestreamDecoder.java:653): a device copy"""
        self._live()
        id_ = C.c_int32(-1)
        self.ctx.call("jxl_canvas_clone", self.id, C.byref(id_))
        return DeviceCanvas(self.ctx, id_.value, self.types, self.shape)

    def upload(self, plane, array):
        self._live()
        a = np.ascontiguousarray(array)
        if a.shape != self.shape:
            raise ValueError("a plane of the set's size")
        code = _plane_code(a.dtype)
        self.ctx.call("jxl_canvas_upload", self.id, int(plane), _vp(a), code)
        self.types[plane] = code
        _bus(self.ctx, up=a.nbytes)

    def download(self, plane):
        self._live()
        out = np.empty(self.shape, _PLANE_DTYPE[self.types[plane]])
        t = C.c_int32(-1)
        self.ctx.call("jxl_canvas_download", self.id, int(plane), _vp(out), C.byref(t))
        assert t.value == self.types[plane], "the binding's plane tags have left the library's"
        _bus(self.ctx, down=out.nbytes)
        return out

    def cast(self, plane, depth):
        """ImageBuffer.castToFloat(depth) of the whole plane in place (jxl_canvas_cast); a float plane stays as it is"""
        self._live()
        self.ctx.call("jxl_canvas_cast", self.id, int(plane), int(depth))
        self.types[plane] = abi.PLANE_FLOAT

    def toPlanes(self):
        """planes 0..2 (float) become the context's resident planes (jxl_canvas_to_planes); the set stays"""
        self._live()
        self.ctx.call("jxl_canvas_to_planes", self.id)
        return ResidentPlanes(self.ctx)

    def takePlanes(self):
        """planes 0..2 become copies of the context's resident planes, tagged float (jxl_canvas_take_planes): toPlanes'
        inverse, for the colour planes that went through a stage on ResidentPlanes"""
        self._live()
        self.ctx.call("jxl_canvas_take_planes", self.id)
        self.types[:3] = [abi.PLANE_FLOAT] * 3

    def release(self):
        if self.id is not None and getattr(self.ctx, "h", None):
            self.ctx.call("jxl_canvas_destroy", self.id)
        self.id = None

    def canvasShape(self):
        s = abi.CanvasShape()
        s.n, s.h, s.w = len(self.types), self.shape[0], self.shape[1]
        for i, t in enumerate(self.types):
            s.types[i] = t
        return s


def modularPlanesDesc(height, width, planes):
    """jxl_modular_planes_desc; planes: per plane (channel, addChannel or -1, dtype or plane code, scale)"""
    d = abi.ModularPlanesDesc()
    d.height, d.width, d.n_planes = int(height), int(width), len(planes)
    for i, (ch, add, t, scale) in enumerate(planes[:abi.CANVAS_MAX_PLANES]):
        k = d.plane[i]
        k.channel, k.add_channel = int(ch), int(add)
        k.type = int(t) if isinstance(t, (int, np.integer)) else _plane_code(t)
        k.scale = float(scale)
    return d


def canvasBlendDesc(canvas_id, frame_id, ref_id, rect, chans):
    """jxl_canvas_blend_desc; chans: per canvas channel (frame_plane, mode, flags, frame_alpha, ref_alpha)"""
    d = abi.CanvasBlendDesc()
    d.canvas, d.frame, d.ref, d.n_chan = int(canvas_id), int(frame_id), int(ref_id), len(chans)
    d.rect = abi.BlendRect(*[int(v) for v in rect])
    for i, ch in enumerate(chans[:abi.CANVAS_MAX_PLANES]):
        k = d.chan[i]
        k.frame_plane, k.mode, k.flags, k.frame_alpha, k.ref_alpha = (int(v) for v in ch)
    return d


def canvas_blend(canvas, frame, ref, rect, chans):
    """JXLCodestreamDecoder.blendFrame as one launch (jxl_canvas_blend), asynchronous. canvas / frame: DeviceCanvas; ref: a
    DeviceCanvas (it may be `canvas` itself) or None for refBuffers == null; rect as blend()'s; chans as canvasBlendDesc's"""
    for s in (canvas, frame, ref):
        if s is not None:
            s._live()
    d = canvasBlendDesc(canvas.id, frame.id, -1 if ref is None else ref.id, rect, chans)
    canvas.ctx.call("jxl_canvas_blend", C.byref(d))


def canvas_blend_check(desc, canvas, frame, ref):
    """jxl_canvas_blend_check: host only (no context, no device). desc: abi.CanvasBlendDesc; the others abi.CanvasShape (ref:
    None when desc.ref is -1). Raises what jxl_canvas_blend would"""
    from . import _lib
    lib = _lib.load()
    st = lib.jxl_canvas_blend_check(C.byref(desc), C.byref(canvas) if canvas is not None else None,
                                    C.byref(frame) if frame is not None else None, C.byref(ref) if ref is not None else None)
    _lib.check(None, st)


def canvas_cast_planes(ctx, items):
    """ImageBuffer.castToFloat of whole planes of plane sets in ONE launch (jxl_canvas_cast_planes), asynchronous. items:
    (DeviceCanvas, plane, depth), each (set, plane) once; a float plane is skipped. The sets' tags follow"""
    items = list(items)
    for s, _, _ in items:
        s._live()
    arr = (abi.CanvasCastItem * max(1, len(items)))()
    for k, (s, plane, depth) in enumerate(items):
        arr[k].set, arr[k].plane, arr[k].depth = s.id, int(plane), int(depth)
    ctx.call("jxl_canvas_cast_planes", len(items), arr)
    for s, plane, _ in items:
        s.types[plane] = abi.PLANE_FLOAT


def canvas_patches(frame, refs, pos, blend, n_color, ec_is_alpha, ec_alpha_associated, colorsResident=False):
    """JXLCodestreamDecoder.computePatches on plane sets (jxl_canvas_patches): one launch, asynchronous, no plane crosses the bus.
    frame: the DeviceCanvas of the frame's n_color + n_extra planes; refs: per reference slot a DeviceCanvas or None (two slots may
    be one set); pos / blend as for computePatches. colorsResident: planes 0..2 of the frame are the context's resident planes
    (the set's own are left alone). No casts: the planes carry the types of decoder.patch_type_plan (canvas_cast_planes)"""
    frame._live()
    for r in refs:
        if r is not None:
            r._live()
    desc, keep = abi.make_patch_desc(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, [None] * 4)
    ids = np.array([-1 if r is None else r.id for r in refs], np.int32)
    frame.ctx.call("jxl_canvas_patches", C.byref(desc), frame.id, 1 if colorsResident else 0, abi.iptr(ids))


def canvas_patches_check(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, frame, refs, colorsResident=False):
    """jxl_canvas_patches_check: host only (no context, no device). frame: abi.CanvasShape; refs: per slot an abi.CanvasShape or
    None -- the frame's own object where the frame set is that slot's set. Raises what jxl_canvas_patches would, with the
    offending position in `.position`"""
    from . import _lib
    lib = _lib.load()
    desc, keep = abi.make_patch_desc(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, [None] * 4)
    rp = (C.POINTER(abi.CanvasShape) * 4)(*[C.pointer(r) if r is not None else None for r in refs])
    bad = C.c_int32(-1)
    st = lib.jxl_canvas_patches_check(C.byref(desc), C.byref(frame) if frame is not None else None, 1 if colorsResident else 0, rp,
                                      C.byref(bad))
    if st != 0:
        msg = lib.jxl_last_error(None)
        err = _lib._ERR.get(int(st), _lib.JxlError)(int(st), msg.decode("utf-8", "replace") if msg else "")
        err.position = bad.value
        raise err


def transposeBuffer(ctx, src, orientation):
    """JXLCodestreamDecoder.transposeBuffer (JXLCodestreamDecoder.java:43-184)"""
    if src.dtype not in (np.int32, np.float32):
        raise TypeError("int32 or float32 planes")
    a = np.ascontiguousarray(src)
    h, w = a.shape
    out = np.empty((w, h) if orientation > 4 else (h, w), a.dtype)
    ctx.call("jxl_stage_orient", _vp(a), h, w, orientation, _vp(out))
    return out


def packSamples(ctx, planes, bitDepth, alpha=None, premultiplied=False, taggedDepth=None, bigEndian=False):
    """PNGWriter ctor tail + writeIDAT sample order (PNGWriter.java:79-111, 191-203): planes = 1 or 3 colour planes
    (int32 or float32 each), optional alpha plane; returns [h][w][channels] uint8 / uint16"""
    pl = [np.ascontiguousarray(p) for p in planes] + ([np.ascontiguousarray(alpha)] if alpha is not None else [])
    h, w = pl[0].shape
    p = abi.PackParams()
    p.height, p.width, p.n_color, p.has_alpha = h, w, len(planes), 1 if alpha is not None else 0
    p.premultiplied, p.bit_depth, p.big_endian = int(bool(premultiplied)), bitDepth, int(bool(bigEndian))
    for i, a in enumerate(pl):
        if a.dtype not in (np.int32, np.float32) or a.shape != (h, w):
            raise TypeError("planes must be int32 or float32 of one shape")
        p.is_int[i] = 1 if a.dtype == np.int32 else 0
        p.tagged_depth[i] = (taggedDepth[i] if taggedDepth is not None else bitDepth)
    out = np.empty((h, w, len(pl)), np.uint8 if bitDepth == 8 else np.uint16)
    pp = (C.c_void_p * 4)(*([_vp(a) for a in pl] + [None] * (4 - len(pl))))
    ctx.call("jxl_stage_pack", pp, C.byref(p), _vp(out))
    return out
