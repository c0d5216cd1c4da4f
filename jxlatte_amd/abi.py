"""ctypes mirror of include/jxlatte_amd.h (structures, constants, transform-type table).

Shared by the product binding (jxlatte_amd._lib) and, as plain type definitions, by the
oracle's test wrapper (oracle/pyoracle.py). No compute lives here.
"""
import ctypes as C

import numpy as np

JXL_OK = 0
JXL_ERR_INVALID_ARGUMENT = -1
JXL_ERR_INVALID_BITSTREAM = -2
JXL_ERR_UNSUPPORTED = -3
JXL_ERR_DEVICE = -4
JXL_ERR_OOM = -5
JXL_ERR_STATE = -6

TRANSFER_NONE, TRANSFER_PQ, TRANSFER_SRGB, TRANSFER_PQ_EXACT = 0, 1, 2, 3
# jxl_color_params.tf_in / tf_out (jxl_stage_color_convert / jxl_stage_color_peak)
TF_LINEAR, TF_SRGB, TF_BT709, TF_PQ, TF_GAMMA, TF_HLG = 0, 1, 2, 3, 4, 5
OUT_F32, OUT_U16, OUT_U8, OUT_RGB8, OUT_RGB16 = 0, 1, 2, 3, 4
BLEND_REPLACE, BLEND_ADD, BLEND_BLEND, BLEND_MULADD, BLEND_MULT = 0, 1, 2, 3, 4
BLEND_FLAG_IS_ALPHA, BLEND_FLAG_HAS_EXTRA, BLEND_FLAG_CLAMP, BLEND_FLAG_PREMULT = 1, 2, 4, 8
STAGE_IDCT, STAGE_GAB, STAGE_EPF, STAGE_XYB, STAGE_OUT = 1, 2, 4, 8, 16
STAGE_ALL = 31

# (type, parameterIndex, orderID, method, pixelHeight, pixelWidth): TransformType.java:10-36
# (kept in sync with include/jxl_transform_types.h; tests/test_abi.py checks it against the .so)
METHOD_DCT, METHOD_DCT2, METHOD_DCT4, METHOD_HORNUSS, METHOD_DCT8_4, METHOD_DCT4_8, METHOD_AFV = range(7)
TRANSFORM_TYPES = [
    ("DCT8", 0, 0, 0, METHOD_DCT, 8, 8), ("HORNUSS", 1, 1, 1, METHOD_HORNUSS, 8, 8),
    ("DCT2", 2, 2, 1, METHOD_DCT2, 8, 8), ("DCT4", 3, 3, 1, METHOD_DCT4, 8, 8),
    ("DCT16", 4, 4, 2, METHOD_DCT, 16, 16), ("DCT32", 5, 5, 3, METHOD_DCT, 32, 32),
    ("DCT16_8", 6, 6, 4, METHOD_DCT, 16, 8), ("DCT8_16", 7, 6, 4, METHOD_DCT, 8, 16),
    ("DCT32_8", 8, 7, 5, METHOD_DCT, 32, 8), ("DCT8_32", 9, 7, 5, METHOD_DCT, 8, 32),
    ("DCT32_16", 10, 8, 6, METHOD_DCT, 32, 16), ("DCT16_32", 11, 8, 6, METHOD_DCT, 16, 32),
    ("DCT4_8", 12, 9, 1, METHOD_DCT4_8, 8, 8), ("DCT8_4", 13, 9, 1, METHOD_DCT8_4, 8, 8),
    ("AFV0", 14, 10, 1, METHOD_AFV, 8, 8), ("AFV1", 15, 10, 1, METHOD_AFV, 8, 8),
    ("AFV2", 16, 10, 1, METHOD_AFV, 8, 8), ("AFV3", 17, 10, 1, METHOD_AFV, 8, 8),
    ("DCT64", 18, 11, 7, METHOD_DCT, 64, 64), ("DCT64_32", 19, 12, 8, METHOD_DCT, 64, 32),
    ("DCT32_64", 20, 12, 8, METHOD_DCT, 32, 64), ("DCT128", 21, 13, 9, METHOD_DCT, 128, 128),
    ("DCT128_64", 22, 14, 10, METHOD_DCT, 128, 64), ("DCT64_128", 23, 14, 10, METHOD_DCT, 64, 128),
    ("DCT256", 24, 15, 11, METHOD_DCT, 256, 256), ("DCT256_128", 25, 16, 12, METHOD_DCT, 256, 128),
    ("DCT128_256", 26, 16, 12, METHOD_DCT, 128, 256),
]
TT_NAME = {t[1]: t[0] for t in TRANSFORM_TYPES}
TT_BY_NAME = {t[0]: t[1] for t in TRANSFORM_TYPES}


def tt_pixel_size(t):
    return TRANSFORM_TYPES[t][5], TRANSFORM_TYPES[t][6]


def tt_param_index(t):
    return TRANSFORM_TYPES[t][2]


def tt_matrix_size(param_index):
    """matrixHeight x matrixWidth of the (non-vertical) type of a parameter index
    (TransformType.getByParameterIndex, TransformType.java:70-73)."""
    for _, _, p, _, _, ph, pw in TRANSFORM_TYPES:
        if p == param_index and not ph > pw:
            return min(ph, pw), max(ph, pw)
    raise KeyError(param_index)


def iptr(a):
    assert a.dtype == np.int32
    return ptr(a, C.c_int32)


f3 = C.c_float * 3
f8 = C.c_float * 8
f9 = C.c_float * 9


class VarDCTParams(C.Structure):
    """struct jxl_vardct_params"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("stages", C.c_uint32),
        ("scale_factor", f3), ("quant_bias", f3), ("quant_bias_numerator", C.c_float),
        ("base_corr_x", C.c_float), ("base_corr_b", C.c_float), ("color_factor", C.c_int32),
        ("gab", C.c_int32), ("gab_w1", f3), ("gab_w2", f3),
        ("epf_iters", C.c_int32), ("global_scale_f", C.c_float), ("epf_sharp_lut", f8),
        ("epf_channel_scale", f3), ("epf_pass0_sigma_scale", C.c_float),
        ("epf_pass2_sigma_scale", C.c_float), ("epf_border_sad_mul", C.c_float),
        ("xyb", C.c_int32), ("opsin_matrix", f9), ("opsin_bias", f3), ("cbrt_opsin_bias", f3),
        ("intensity_target", C.c_float), ("transfer", C.c_int32), ("out_format", C.c_int32),
        ("jpeg_upsampling_y", C.c_int32 * 3), ("jpeg_upsampling_x", C.c_int32 * 3),
    ]


class LFGroupDesc(C.Structure):
    """struct jxl_lfgroup_desc"""
    _fields_ = [
        ("lfg_y", C.c_int32), ("lfg_x", C.c_int32), ("cells_h", C.c_int32), ("cells_w", C.c_int32),
        ("dct_select", C.POINTER(C.c_uint8)), ("hf_mul", C.POINTER(C.c_int32)),
        ("sharpness", C.POINTER(C.c_int32)), ("x_from_y", C.POINTER(C.c_int32)),
        ("b_from_y", C.POINTER(C.c_int32)), ("block_yx", C.POINTER(C.c_int32)),
        ("n_blocks", C.c_int32), ("lf", C.POINTER(C.c_float) * 3),
    ]


class LFQuantDesc(C.Structure):
    """struct jxl_lfquant_desc (row f1: integer LF image of one LF group)"""
    _fields_ = [
        ("lfg_y", C.c_int32), ("lfg_x", C.c_int32), ("cells_h", C.c_int32), ("cells_w", C.c_int32),
        ("lf_quant", C.POINTER(C.c_int32) * 3), ("extra_precision", C.c_int32), ("scaled_dequant", f3),
        ("x_factor_lf", C.c_int32), ("b_factor_lf", C.c_int32), ("adaptive_smoothing", C.c_int32),
    ]


def make_lfquant_desc(lf_quant, scaled_dequant, extra_precision=0, x_factor_lf=128, b_factor_lf=128, adaptive_smoothing=True,
                      lfg_y=0, lfg_x=0, cells=None):
    """lf_quant: int32 array [3][H][W] in X,Y,B order, or (chroma-subsampled frames) a list of three contiguous int32 planes
    of different sizes together with cells=(cells_h, cells_w) of the LF group. Kept alive by the caller."""
    planes = [lf_quant[c] for c in range(3)]
    for a in planes:
        assert a.dtype == np.int32 and a.ndim == 2 and a.flags["C_CONTIGUOUS"]
    d = LFQuantDesc()
    d.lfg_y, d.lfg_x = lfg_y, lfg_x
    d.cells_h, d.cells_w = cells if cells is not None else max(a.shape for a in planes)
    for c in range(3):
        d.lf_quant[c] = iptr(planes[c])
        d.scaled_dequant[c] = scaled_dequant[c]
    d.extra_precision, d.x_factor_lf, d.b_factor_lf = extra_precision, x_factor_lf, b_factor_lf
    d.adaptive_smoothing = 1 if adaptive_smoothing else 0
    return d


class LFImageDesc(C.Structure):
    """struct jxl_lf_image_desc (the LF image of a whole frame as the picture at 1:8)"""
    _fields_ = [
        ("n_groups", C.c_int32), ("cells_h", C.c_int32), ("cells_w", C.c_int32), ("color_factor", C.c_int32),
        ("groups", C.POINTER(LFQuantDesc)), ("base_corr_x", C.c_float), ("base_corr_b", C.c_float), ("xyb", C.c_int32),
        ("opsin_matrix", f9), ("opsin_bias", f3), ("cbrt_opsin_bias", f3), ("intensity_target", C.c_float),
    ]


def make_lf_image_desc(groups, cells, base_corr_x=0.0, base_corr_b=1.0, color_factor=84, xyb=None):
    """groups: the frame's LF groups, dicts of lfg_y, lfg_x, lf_quant (three C-contiguous int32 planes of the group's size, X, Y, B
    order), scaled_dequant, extra_precision, x_factor_lf, b_factor_lf, adaptive_smoothing. cells: (cells_h, cells_w) of the output.
    xyb: None, or (matrix[9], opsin_bias[3], cbrt_opsin_bias[3], intensity_target). Returns (desc, keepalive)."""
    keep = []
    arr = (LFQuantDesc * max(1, len(groups)))()
    for i, g in enumerate(groups):
        planes = [np.ascontiguousarray(g["lf_quant"][c], np.int32) for c in range(3)]
        keep.append(planes)
        if len({a.shape for a in planes}) != 1:
            raise ValueError("the three LF planes of an LF group must have one size")
        arr[i] = make_lfquant_desc(planes, g["scaled_dequant"], g.get("extra_precision", 0), g.get("x_factor_lf", 128), g.get("b_factor_lf", 128),
                                   g.get("adaptive_smoothing", True), g["lfg_y"], g["lfg_x"])
    d = LFImageDesc()
    d.n_groups = len(groups)
    d.cells_h, d.cells_w = cells
    d.color_factor = color_factor
    d.groups = C.cast(arr, C.POINTER(LFQuantDesc))
    d.base_corr_x, d.base_corr_b = base_corr_x, base_corr_b
    if xyb is not None:
        matrix, bias, cbrt, intensity_target = xyb
        d.xyb = 1
        d.opsin_matrix, d.opsin_bias, d.cbrt_opsin_bias = f9(*[float(v) for v in matrix]), f3(*[float(v) for v in bias]), f3(*[float(v) for v in cbrt])
        d.intensity_target = intensity_target
    keep.append(arr)
    return d, keep


SPARSE_WIDE = 1


class SparseRun(C.Structure):
    """struct jxl_sparse_run (one run of entries of the sparse coefficient feed)"""
    _fields_ = [("group", C.c_int32), ("channel", C.c_int32), ("flags", C.c_int32), ("count", C.c_int32),
                ("offset_words", C.c_int64)]


class BlendRect(C.Structure):
    """struct jxl_blend_rect"""
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("canvas_y", C.c_int32), ("canvas_x", C.c_int32),
                ("frame_y", C.c_int32), ("frame_x", C.c_int32), ("ref_y", C.c_int32), ("ref_x", C.c_int32)]


CANVAS_MAX_PLANES = 16
PLANE_FLOAT, PLANE_INT32 = 0, 1


class CanvasBlendChan(C.Structure):
    """struct jxl_canvas_blend_chan"""
    _fields_ = [("frame_plane", C.c_int32), ("mode", C.c_int32), ("flags", C.c_uint32), ("frame_alpha", C.c_int32),
                ("ref_alpha", C.c_int32)]


class CanvasBlendDesc(C.Structure):
    """struct jxl_canvas_blend_desc"""
    _fields_ = [("canvas", C.c_int32), ("frame", C.c_int32), ("ref", C.c_int32), ("n_chan", C.c_int32), ("rect", BlendRect),
                ("chan", CanvasBlendChan * CANVAS_MAX_PLANES)]


class CanvasShape(C.Structure):
    """struct jxl_canvas_shape"""
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("types", C.c_int32 * CANVAS_MAX_PLANES)]


class CanvasCastItem(C.Structure):
    """struct jxl_canvas_cast_item"""
    _fields_ = [("set", C.c_int32), ("plane", C.c_int32), ("depth", C.c_int32)]


CANVAS_MAX_CASTS = 5 * CANVAS_MAX_PLANES


class ModularPlane(C.Structure):
    """struct jxl_modular_plane"""
    _fields_ = [("channel", C.c_int32), ("add_channel", C.c_int32), ("type", C.c_int32), ("scale", C.c_float)]


class ModularPlanesDesc(C.Structure):
    """struct jxl_modular_planes_desc"""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("n_planes", C.c_int32), ("plane", ModularPlane * CANVAS_MAX_PLANES)]


class PackParams(C.Structure):
    """struct jxl_pack_params"""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("n_color", C.c_int32), ("has_alpha", C.c_int32),
                ("premultiplied", C.c_int32), ("bit_depth", C.c_int32), ("big_endian", C.c_int32),
                ("is_int", C.c_int32 * 4), ("tagged_depth", C.c_int32 * 4)]


class ColorParams(C.Structure):
    """struct jxl_color_params"""
    _fields_ = [("n_planes", C.c_int32), ("in_is_int", C.c_int32), ("in_max", C.c_int32 * 3), ("tf_in", C.c_int32),
                ("gamma_in", C.c_int32), ("use_scale", C.c_int32), ("scale", C.c_float), ("use_matrix", C.c_int32),
                ("matrix", f9), ("tf_out", C.c_int32), ("gamma_out", C.c_int32), ("max_value", C.c_int32)]


class ToneMapParams(C.Structure):
    """struct jxl_tone_map"""
    _fields_ = [("lum", C.c_float * 3), ("unit_nits", C.c_float), ("source_nits", C.c_float), ("target_nits", C.c_float),
                ("gamut", C.c_int32)]


class PngParams(C.Structure):
    """struct jxl_png_params"""
    _fields_ = [("color", ColorParams), ("height", C.c_int32), ("width", C.c_int32), ("has_alpha", C.c_int32),
                ("premultiplied", C.c_int32), ("bit_depth", C.c_int32), ("big_endian", C.c_int32), ("alpha_is_int", C.c_int32),
                ("alpha_tagged_depth", C.c_int32), ("color_tagged_depth", C.c_int32)]


TENSOR_U8, TENSOR_F16, TENSOR_BF16, TENSOR_F32 = 0, 1, 2, 3
TENSOR_CHW, TENSOR_HWC = 0, 1


class TensorParams(C.Structure):
    """struct jxl_tensor_params"""
    _fields_ = [("color", ColorParams), ("height", C.c_int32), ("width", C.c_int32), ("has_alpha", C.c_int32),
                ("premultiplied", C.c_int32), ("write_alpha", C.c_int32), ("alpha_is_int", C.c_int32),
                ("alpha_tagged_depth", C.c_int32), ("color_tagged_depth", C.c_int32), ("dtype", C.c_int32), ("layout", C.c_int32),
                ("use_norm", C.c_int32), ("mean", C.c_float * 4), ("inv_std", C.c_float * 4)]


assert C.sizeof(TensorParams) == C.sizeof(ColorParams) + 4 * (11 + 8)

RESIZE_TRIANGLE, RESIZE_BOX = 0, 1


class ResizeParams(C.Structure):
    """struct jxl_resize_params"""
    _fields_ = [("box_x0", C.c_int32), ("box_y0", C.c_int32), ("box_width", C.c_int32), ("box_height", C.c_int32),
                ("out_height", C.c_int32), ("out_width", C.c_int32), ("filter", C.c_int32)]


assert C.sizeof(ResizeParams) == 28

TENSOR_BATCH_MAX = 1024
BATCH_HOST, BATCH_RESIDENT, BATCH_SET = 0, 1, 2


class TensorBatchItem(C.Structure):
    """struct jxl_tensor_batch_item"""
    _fields_ = [("source", C.c_int32), ("set_id", C.c_int32), ("alpha_plane", C.c_int32), ("in_", C.c_void_p * 3),
                ("alpha", C.c_void_p), ("p", TensorParams), ("r", ResizeParams)]


# three int32 and 4 bytes of padding before the pointers; the two parameter blocks are 4-byte aligned, the whole 8-byte aligned
assert C.sizeof(TensorBatchItem) == (16 + 4 * C.sizeof(C.c_void_p) + C.sizeof(TensorParams) + C.sizeof(ResizeParams) + 7) // 8 * 8


class PfmParams(C.Structure):
    """struct jxl_pfm_params"""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("n_planes", C.c_int32), ("is_int", C.c_int32 * 3),
                ("tagged_depth", C.c_int32 * 3)]


class VarblockDesc(C.Structure):
    """struct jxl_varblock_desc"""
    _fields_ = [("n_blocks", C.c_int32), ("blocks", C.POINTER(C.c_int32)), ("cells_h", C.c_int32), ("cells_w", C.c_int32)]


def make_varblock_desc(blocks, cells):
    """blocks: n x (cy, cx, type) in frame cells; cells: (cells_h, cells_w). Returns (desc, keep): `keep` owns the memory the
    descriptor points into"""
    b = np.ascontiguousarray(np.asarray(blocks, np.int32).reshape(-1, 3))
    d = VarblockDesc()
    d.n_blocks = b.shape[0]
    d.blocks = iptr(b) if b.shape[0] else None
    d.cells_h, d.cells_w = int(cells[0]), int(cells[1])
    return d, b


class PaletteDesc(C.Structure):
    """struct jxl_palette_desc"""
    _fields_ = [("num_c", C.c_int32), ("nb_colors", C.c_int32), ("nb_deltas", C.c_int32), ("d_pred", C.c_int32),
                ("bit_depth", C.c_int32), ("pal_h", C.c_int32), ("pal_w", C.c_int32), ("palette", C.POINTER(C.c_int32)),
                ("pred", C.POINTER(C.c_int32))]


def make_palette_desc(palette, pred, num_c, nb_colors, nb_deltas, d_pred, bit_depth):
    """palette: the 2-D palette channel; pred: the weighted predictor's plane or None. Returns (desc, keep): `keep` owns the
    memory the descriptor points into"""
    pal = np.ascontiguousarray(palette, np.int32)
    assert pal.ndim == 2, pal.shape
    pr = np.ascontiguousarray(pred, np.int32) if pred is not None else None
    d = PaletteDesc()
    d.num_c, d.nb_colors, d.nb_deltas, d.d_pred, d.bit_depth = int(num_c), int(nb_colors), int(nb_deltas), int(d_pred), int(bit_depth)
    d.pal_h, d.pal_w = pal.shape
    d.palette = iptr(pal) if pal.size else None
    d.pred = iptr(pr) if pr is not None else None
    return d, (pal, pr)


class SplineDesc(C.Structure):
    """struct jxl_spline_desc (SplinesBundle.java + the two LFChannelCorrelation factors)"""
    _fields_ = [("quant_adjust", C.c_int32), ("n_splines", C.c_int32), ("n_control", C.POINTER(C.c_int32)),
                ("control", C.POINTER(C.c_int32)), ("coeff", C.POINTER(C.c_int32)), ("base_corr_x", C.c_float),
                ("base_corr_b", C.c_float)]


class SplineArc(C.Structure):
    """struct jxl_spline_arc: one drawing arc sample of Spline.renderSpline, 48 bytes"""
    _fields_ = [("y", C.c_float), ("x", C.c_float), ("sigma", C.c_float), ("inv_sigma", C.c_float), ("mul", C.c_float * 3),
                ("x0", C.c_int32), ("x1", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32), ("reserved", C.c_int32)]


# the same record as a numpy structured dtype (host.spline_arcs)
SPLINE_ARC_DTYPE = [("y", "<f4"), ("x", "<f4"), ("sigma", "<f4"), ("inv_sigma", "<f4"), ("mul", "<f4", (3,)), ("x0", "<i4"),
                    ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"), ("reserved", "<i4")]


def make_spline_desc(splines, base_corr_x, base_corr_b):
    """splines: the list frontend.Frontend.splines() returns (dicts of quant_adjust, control [(y, x)...], coeff [4][32]).
    Returns (desc, keepalive)."""
    import numpy as np
    n_control = np.array([len(sp["control"]) for sp in splines], np.int32)
    control = np.ascontiguousarray(np.concatenate([np.asarray(sp["control"], np.int32).reshape(-1, 2) for sp in splines])
                                   if splines else np.zeros((0, 2)), np.int32)
    coeff = np.ascontiguousarray(np.stack([np.asarray(sp["coeff"], np.int32).reshape(4, 32) for sp in splines])
                                 if splines else np.zeros((0, 4, 32)), np.int32)
    d = SplineDesc()
    d.quant_adjust = int(splines[0]["quant_adjust"]) if splines else 0
    d.n_splines = len(splines)
    d.n_control, d.control, d.coeff = ptr(n_control, C.c_int32), ptr(control, C.c_int32), ptr(coeff, C.c_int32)
    d.base_corr_x, d.base_corr_b = float(base_corr_x), float(base_corr_b)
    return d, (n_control, control, coeff)


class PatchPos(C.Structure):
    """struct jxl_patch_pos: one position of one patch, 32 bytes"""
    _fields_ = [("y0", C.c_int32), ("x0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("ref", C.c_int32), ("ref_y0", C.c_int32),
                ("ref_x0", C.c_int32), ("blend", C.c_int32)]


PATCH_POS_DTYPE = [("y0", "<i4"), ("x0", "<i4"), ("h", "<i4"), ("w", "<i4"), ("ref", "<i4"), ("ref_y0", "<i4"), ("ref_x0", "<i4"),
                   ("blend", "<i4")]


class PatchDesc(C.Structure):
    """struct jxl_patch_desc (the patch stage of one frame: JXLCodestreamDecoder.computePatches)"""
    _fields_ = [("n_pos", C.c_int32), ("pos", C.POINTER(PatchPos)), ("n_rows", C.c_int32), ("blend", C.POINTER(C.c_int32)),
                ("n_color", C.c_int32), ("n_extra", C.c_int32), ("ec_is_alpha", C.POINTER(C.c_int32)),
                ("ec_alpha_associated", C.POINTER(C.c_int32)), ("ref_h", C.c_int32 * 4), ("ref_w", C.c_int32 * 4)]


def make_patch_desc(pos, blend, n_color, ec_is_alpha, ec_alpha_associated, ref_shapes):
    """pos: record array of PATCH_POS_DTYPE in stage order; blend: int32 [n_rows][n_color + n_extra][3] (mode, alphaChannel, clamp);
    ref_shapes: per reference slot (h, w) or None for an absent slot. Returns (desc, keepalive)."""
    pos = np.ascontiguousarray(pos, PATCH_POS_DTYPE)
    n_extra = len(ec_is_alpha)
    blend = np.ascontiguousarray(blend, np.int32).reshape(-1, int(n_color) + n_extra, 3)
    isa = np.ascontiguousarray([1 if v else 0 for v in ec_is_alpha], np.int32)
    assoc = np.ascontiguousarray([1 if v else 0 for v in ec_alpha_associated], np.int32)
    d = PatchDesc()
    d.n_pos, d.pos = len(pos), pos.ctypes.data_as(C.POINTER(PatchPos))
    d.n_rows, d.blend = blend.shape[0], ptr(blend, C.c_int32)
    d.n_color, d.n_extra = int(n_color), n_extra
    d.ec_is_alpha, d.ec_alpha_associated = ptr(isa, C.c_int32), ptr(assoc, C.c_int32)
    for k in range(4):
        d.ref_h[k], d.ref_w[k] = ref_shapes[k] if ref_shapes[k] is not None else (0, 0)
    return d, (pos, blend, isa, assoc)


class SqueezeParam(C.Structure):
    """struct jxl_squeeze_param (SqueezeParam.java)"""
    _fields_ = [("horizontal", C.c_int32), ("in_place", C.c_int32), ("begin_c", C.c_int32), ("num_c", C.c_int32)]

    def as_tuple(self):
        return (self.horizontal, self.in_place, self.begin_c, self.num_c)


class Channel(C.Structure):
    """struct jxl_channel"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.POINTER(C.c_int32))]


def ptr(a, ctype):
    """pointer to a C-contiguous numpy array's data (array must stay alive)."""
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.POINTER(ctype))


def fptr(a):
    assert a.dtype == np.float32
    return ptr(a, C.c_float)




def make_lfgroup_desc(g):
    """g: dict with numpy arrays (see synth.make_vardct_frame). Returns (desc, keepalive)."""
    d = LFGroupDesc()
    d.lfg_y, d.lfg_x = int(g["lfg_y"]), int(g["lfg_x"])
    d.cells_h, d.cells_w = g["dct_select"].shape
    d.dct_select = ptr(g["dct_select"], C.c_uint8)
    d.hf_mul = iptr(g["hf_mul"])
    d.sharpness = iptr(g["sharpness"])
    d.x_from_y = iptr(g["x_from_y"])
    d.b_from_y = iptr(g["b_from_y"])
    d.block_yx = iptr(g["block_yx"])
    d.n_blocks = g["block_yx"].shape[0]
    if g.get("lf") is not None:
        for c in range(3):
            d.lf[c] = fptr(g["lf"][c])
    return d


def make_channels(arrs):
    """list of 2-D int32 arrays -> (Channel array, keepalive)."""
    arr = (Channel * max(1, len(arrs)))()
    for i, a in enumerate(arrs):
        assert a.dtype == np.int32 and a.ndim == 2 and a.flags["C_CONTIGUOUS"]
        arr[i].height, arr[i].width = a.shape
        arr[i].data = iptr(a) if a.size else C.POINTER(C.c_int32)()
    return arr


def make_squeeze_params(sp):
    arr = (SqueezeParam * max(1, len(sp)))()
    for i, (h, ip, b, n) in enumerate(sp):
        arr[i].horizontal, arr[i].in_place, arr[i].begin_c, arr[i].num_c = int(h), int(ip), int(b), int(n)
    return arr


class ModularTransform(C.Structure):
    """struct jxl_modular_transform"""
    _fields_ = [("kind", C.c_int32), ("begin_c", C.c_int32), ("num_c", C.c_int32), ("rct_type", C.c_int32), ("nb_colors", C.c_int32),
                ("nb_deltas", C.c_int32), ("d_pred", C.c_int32), ("sp", C.POINTER(SqueezeParam)), ("n_sp", C.c_int32)]


def make_transforms(transforms):
    """the dictionaries frontend.transforms() returns (bitstream order; a Squeeze carries `steps`, the expanded step list) ->
    (ModularTransform array, keepalive)"""
    arr = (ModularTransform * max(1, len(transforms)))()
    keep = []
    for i, t in enumerate(transforms):
        for k in ("kind", "begin_c", "num_c", "rct_type", "nb_colors", "nb_deltas", "d_pred"):
            setattr(arr[i], k, int(t.get(k, 0)))
        steps = list(t.get("steps", ()))
        if steps:
            sp = make_squeeze_params(steps)
            keep.append(sp)
            arr[i].sp = C.cast(sp, C.POINTER(SqueezeParam))
        arr[i].n_sp = len(steps)
    return arr, keep
