"""A writer of bare JPEG XL codestreams that hold Modular frames only, every sample coded losslessly: test infrastructure, numpy only.

It is a second reading of the format, made from the reference's reader (the Java file and line each field is read at is cited
beside the code that writes it) and not from jxlatte_amd/frontend: what this module writes, the front-end must read back as the
arrays that went in. Size does not matter; every choice is the simplest legal one:

  * one entropy form: prefix codes over a 64-symbol alphabet whose symbols all have length 6 (the complex prefix header with a
    single level-1 symbol, PrefixSymbolDistribution.java:75-178), hybrid-uint configuration 0-0-0 (the token is the value's bit
    length), one cluster, no LZ77;
  * every channel fits one group, so the frame is one TOC entry and every sample lies in GlobalModular (Frame.java:144-178); only
    the four header bits of the group streams that inherit an EMPTY channel follow it (write_frame);
  * a global MA tree of one leaf, or of one split on the channel index with two leaves (MATree.java:34-88), multiplier 1, offset 0;
  * the forward transforms (RCT, Squeeze with its tendency term, Palette with and without delta entries) are computed here, and the
    residuals come from the predictor the tree names, the weighted one (ModularChannel.java:185-236) included.

encode(image) takes one dict:
  width, height, bits, grey=False, exp_bits=0, orientation=1, animation=False,
  intensity_target=None | an exact half, opsin=None | dict(matrix[9], opsin_bias[3], quant_bias[3], quant_bias_numerator) of exact
  halves (XYB images), up_weights=None | {2: [15], 4: [55], 8: [210]} (any subset) -- used by jxl_writer_vardct.py,
  extra=[dict(type="alpha" | "other", bits=8, exp_bits=0, alpha_associated=False)],
  frames=[dict(planes=[2-D integer arrays, colours then extra channels, each of the frame's coded size],
               type=0 (regular) | 1 (LF frame, with lf_level=1..4 and planes of ceil(image / 8 ** lf_level); write_frame is its entry,
               jxl_writer_vardct.encode_stream the stream's) | 2 (reference only) | 3 (skip progressive), crop=None | (x0, y0),
               upsampling=1, ec_upsampling=[..],
               blend=dict(mode, alpha, clamp, source), ec_blend=[dict..], duration=0, is_last=True, save_as_reference=0,
               save_before_ct=False, group_size_shift=1, predictor=5 | tree=dict(value=v, predictors=(left, right)),
               transforms=[("rct", begin_c, rct_type) | ("palette", begin_c, num_c, nb_deltas, d_pred) | ("squeeze", None | [(horizontal,
               in_place, begin_c, num_c), ..])], patches=None | [..], patch_clusters=None | (map of 10, configs),
               splines=None | dict(quant_adjust, splines=[..], clusters) as write_splines takes it, noise=None | [8 ints of 10 bits],
               ycbcr=False, lf_dequant=None | [3 exact halves: the dequantiser is value / 128],
               restoration=dict(gab=False, gab_weights=None | [(w1, w2)] * 3, epf_iters=0, epf_channel_scale=None | [3],
                                pass0, pass2, border_sad_mul (all three or none: the custom sigma block of a Modular frame),
                                sigma_for_modular=1.0))]
Float samples travel as their int32 bit patterns (exp_bits 8, bits 32).

What is not lossless integer RGB (every default writes the bytes the writer wrote without these keys): xyb=True makes the image
XYB-encoded; a Modular frame of such an image has no do_ycbcr bit (FrameHeader.java:88) and THREE colour planes, in a grey image too
(LFGlobal.java:88-96), which are the stream's channels in stream order: Y, X, B - Y (Frame.java:430-455). A frame with ycbcr=True has
three colour planes as well (LFGlobal.java:89: ecStart is 1 only without do_ycbcr), in stream order Cb, Y, Cr.
VARIANTS names writers that are wrong on purpose (encode(im, variant=..)); the tests show that a decode tells each from the true one."""
import numpy as np

REGULAR, LF_FRAME, REFERENCE_ONLY, SKIP_PROGRESSIVE = 0, 1, 2, 3  # FrameFlags.java:4-7
REPLACE, ADD, BLEND, MULADD, MULT = 0, 1, 2, 3, 4  # FrameFlags.java:18-22
FLAG_NOISE, FLAG_PATCHES, FLAG_SPLINES = 1, 2, 16  # FrameFlags.java:12-14
EC_ALPHA, EC_DEPTH = 0, 1  # ExtraChannelType.java:5-6
I64 = np.int64
VARIANTS = ("sigma_for_modular_before_sigma_block", "quant_mul_in_a_modular_frame", "do_ycbcr_bit_in_an_xyb_image")
# writers that are wrong about the patch dictionary, the splines or their place in LfGlobal (jxl_writer_features_cases.py); both
# frame writers know them
FEATURE_VARIANTS = ("spline_start_y_before_x", "spline_points_as_first_differences", "spline_count_without_the_one",
                    "quant_adjust_before_the_start_positions", "spline_coefficients_y_x_b_sigma", "splines_before_patches",
                    "noise_before_splines", "patch_position_differences_unsigned")


# ---- bits ---------------------------------------------------------------------------------------------------------------
class BitWriter:
    """least significant bit first, as Bitreader.readBits takes them (Bitreader.java:108-136)"""

    def __init__(self):
        self.vals, self.lens, self.pos = [], [], 0

    def bits(self, v, n):
        assert 0 <= n <= 32 and 0 <= v < (1 << n), (v, n)
        if n:
            self.vals.append(np.array([v], np.uint64))
            self.lens.append(np.array([n], np.uint8))
            self.pos += n

    def many(self, vals, lens):
        self.vals.append(np.asarray(vals, np.uint64))
        self.lens.append(np.asarray(lens, np.uint8))
        self.pos += int(np.asarray(lens, I64).sum())

    def bool(self, b):
        self.bits(1 if b else 0, 1)

    def u32(self, v, *dist):  # Bitreader.java:29-34: dist = four (constant, bits)
        for sel, (c, u) in enumerate(dist):
            if c <= v < c + (1 << u):
                self.bits(sel, 2)
                self.bits(v - c, u)
                return
        raise ValueError("%d does not fit %r" % (v, dist))

    def u64(self, v):  # Bitreader.java:36-55
        if v == 0:
            self.bits(0, 2)
        elif v <= 16:
            self.bits(1, 2), self.bits(v - 1, 4)
        elif v <= 272:
            self.bits(2, 2), self.bits(v - 17, 8)
        else:
            assert v < (1 << 20)
            self.bits(3, 2), self.bits(v & 4095, 12), self.bool(True), self.bits(v >> 12, 8), self.bool(False)

    def enum(self, v):  # Bitreader.java:65-70
        self.u32(v, (0, 0), (1, 0), (2, 4), (18, 6))

    def f16(self, v):  # Bitreader.java:57-63: sixteen bits of an IEEE half, finite
        h = np.float16(v)
        assert np.isfinite(h) and float(h) == float(v), v
        self.bits(int(h.view(np.uint16)), 16)

    def pad(self):  # Bitreader.java:159-166
        self.bits(0, -self.pos % 8)

    def tobytes(self):
        self.pad()
        if not self.vals:
            return b""
        vals, lens = np.concatenate(self.vals), np.concatenate(self.lens)
        cols = np.arange(48, dtype=np.uint64)
        bits = ((vals[:, None] >> cols[None, :]) & np.uint64(1)).astype(np.uint8)
        keep = cols[None, :] < lens[:, None]
        return np.packbits(bits[keep], bitorder="little").tobytes()


def pack_signed(v):  # the inverse of MathHelper.unpackSigned (MathHelper.java:32-34)
    v = np.asarray(v, I64)
    return np.where(v >= 0, 2 * v, -2 * v - 1).astype(np.uint64)


_REV6 = np.array([int("{:06b}".format(i)[::-1], 2) for i in range(64)], np.uint64)


def write_symbols(w, values):
    """hybrid integers of configuration 0-0-0 (EntropyStream.java:239-252: token 0 is 0, token t >= 1 is 1 << (t - 1) plus t - 1 raw
    bits) under the flat 6-bit prefix code: VLCTable.java:47-59 indexes its table by the bit-reversed canonical code, and the
    canonical code of symbol s among 64 symbols of length 6 is s itself"""
    u = np.asarray(values, np.uint64).reshape(-1)
    assert u.size == 0 or int(u.max()) < (1 << 32)
    token = np.zeros(u.shape, I64)
    for k in range(32):
        token += u >= np.uint64(1 << k)
    n = np.maximum(token - 1, 0)
    extra = np.where(token > 0, u - (np.uint64(1) << n.astype(np.uint64)), np.uint64(0)).astype(np.uint64)
    w.many(_REV6[token] | (extra << np.uint64(6)), 6 + n)


def write_entropy_header(w, num_dists):
    """EntropyStream.java:106-156"""
    w.bool(False)  # :112 no LZ77
    if num_dists > 1:  # :45-53 simple clustering, zero bits per entry: one cluster
        w.bool(True)
        w.bits(0, 2)
    w.bool(True)  # :129 prefix codes, log alphabet size 15
    w.bits(0, 4)  # HybridIntegerConfig.java:22: split exponent 0 in ceilLog1p(15) = 4 bits; msb and lsb then take no bits (:27-30)
    w.bool(True)  # :141-143 alphabet size 1 + (1 << 5) + 31 = 64
    w.bits(5, 4)
    w.bits(31, 5)
    w.bits(0, 2)  # PrefixSymbolDistribution.java:190 hskip 0: the complex form
    # :83-94 eighteen level-1 lengths in the order of codelenMap {1, 2, 3, 4, 0, 5, 17, 6, ...}, each by level0Table (:13-16: two
    # bits 00 say length 0, two bits 10 -- the value 1, least significant bit first -- say length 4). Only symbol 6, the eighth,
    # has a length: a level-1 code of one symbol takes no bits (:112-113), so all 64 level-2 lengths are 6 and cost nothing
    for i in range(18):
        w.bits(1 if i == 7 else 0, 2)


# hybrid-integer configurations (split_exponent, msb_in_token, lsb_in_token) whose tokens stay below 64 for every value of at
# least sixteen bits: the clusters of an EntropyCoder take different ones, so a symbol read under another cluster's
# configuration takes another number of raw bits
CONFIGS = ((0, 0, 0), (4, 1, 0), (2, 0, 1), (3, 1, 1), (4, 2, 0), (1, 0, 0), (2, 1, 0), (3, 0, 1))


class EntropyCoder:
    """a stream of several clusters (EntropyStream.java:106-156): the context map in its simple form (:49-53), prefix codes, one
    HybridIntegerConfig per cluster (HybridIntegerConfig.java:21-33), every cluster the flat 6-bit code of write_entropy_header"""

    def __init__(self, cluster_map, configs):
        self.map = np.asarray(cluster_map, I64).reshape(-1)
        self.configs = [tuple(c) for c in configs]
        assert self.map.min() >= 0 and int(self.map.max()) + 1 == len(self.configs) <= min(8, len(self.map))
        for se, msb, lsb in self.configs:
            assert 0 <= se < 15 and 0 <= msb and 0 <= lsb and msb + lsb <= se

    def write_header(self, w):
        w.bool(False)  # :112 no LZ77
        if len(self.map) > 1:
            nbits = (len(self.configs) - 1).bit_length()
            w.bool(True)  # :49 simple clustering
            w.bits(nbits, 2)  # :51
            if nbits:
                w.many(self.map.astype(np.uint64), np.full(len(self.map), nbits))  # :52-53
        w.bool(True)  # :129 prefix codes, log alphabet size 15
        for se, msb, lsb in self.configs:  # :133-134
            w.bits(se, 4)  # HybridIntegerConfig.java:22 in ceilLog1p(15) bits
            w.bits(msb, se.bit_length())  # :27
            w.bits(lsb, (se - msb).bit_length())  # :30
        for _ in self.configs:  # :139-147 alphabet size 1 + (1 << 5) + 31 = 64
            w.bool(True)
            w.bits(5, 4)
            w.bits(31, 5)
        for _ in self.configs:  # :148-149, the code of write_entropy_header
            w.bits(0, 2)
            for i in range(18):
                w.bits(1 if i == 7 else 0, 2)

    def write(self, w, contexts, values):
        """the inverse of readHybridInteger (:239-252) per symbol, under the configuration of its context's cluster"""
        u = np.asarray(values, np.uint64).reshape(-1)
        if u.size == 0:
            return
        ctx = np.asarray(contexts, I64).reshape(-1)
        assert ctx.shape == u.shape and ctx.min() >= 0 and ctx.max() < len(self.map) and int(u.max()) < (1 << 32)
        cfg = np.array(self.configs, I64)[self.map[ctx]]
        se, msb, lsb = cfg[:, 0], cfg[:, 1], cfg[:, 2]
        v = u.astype(I64)
        b = np.zeros(v.shape, I64)  # the position of the leading one
        for k in range(1, 33):
            b += v >= (1 << k)
        small = v < (1 << se)  # :241-242
        n = np.where(small, 0, b - msb - lsb)  # :243-244
        top = (v >> np.maximum(b - msb, 0)) & ((1 << msb) - 1)
        token = np.where(small, v, (1 << se) + ((b - se) << (msb + lsb)) + (top << lsb) + (v & ((1 << lsb) - 1)))
        assert int(token.max()) < 64, "the value does not fit the 64 tokens of its cluster's configuration"
        raw = (v >> lsb) & ((1 << n) - 1)
        w.many(_REV6[token] | (raw.astype(np.uint64) << np.uint64(6)), 6 + n)


# ---- headers --------------------------------------------------------------------------------------------------------------
def _bit_depth(w, bits, exp_bits):  # BitDepthHeader.java:19-28
    w.bool(exp_bits != 0)
    if exp_bits:
        w.u32(bits, (32, 0), (16, 0), (24, 0), (1, 6))
        w.bits(exp_bits - 1, 4)
    else:
        w.u32(bits, (8, 0), (10, 0), (12, 0), (1, 6))


def _size(w, height, width):  # ImageHeader.java:154-169: not a multiple-of-8 form, no ratio
    w.bool(False)
    w.u32(height, (1, 9), (1, 13), (1, 18), (1, 30))
    w.bits(0, 3)
    w.u32(width, (1, 9), (1, 13), (1, 18), (1, 30))


def write_image_header(w, im):
    """ImageHeader.java:206-312"""
    extra = im.get("extra", [])
    orientation, animation = im.get("orientation", 1), im.get("animation", False)
    w.bits(0x0AFF, 16)  # :208
    _size(w, im["height"], im["width"])
    w.bool(False)  # :213 all_default
    target = im.get("intensity_target")
    extra_fields = orientation != 1 or animation or target is not None
    w.bool(extra_fields)  # :214
    if extra_fields:
        w.bits(orientation - 1, 3)  # :217
        w.bool(False)  # :219 intrinsic size
        w.bool(False)  # :222 preview
        w.bool(animation)  # :225
        if animation:  # AnimationHeader.java:11-14: 100 / 1 ticks per second, loops forever, no timecodes
            w.u32(100, (100, 0), (1000, 0), (1, 10), (1, 30))
            w.u32(1, (1, 0), (1001, 0), (1, 8), (1, 10))
            w.u32(0, (0, 0), (0, 3), (0, 16), (0, 32))
            w.bool(False)
    _bit_depth(w, im["bits"], im.get("exp_bits", 0))  # :243
    w.bool(im["bits"] <= 12)  # :244 modular_16bit_buffers
    w.u32(len(extra), (0, 0), (1, 0), (2, 4), (1, 12))  # :245
    for e in extra:  # ExtraChannelInfo.java:19-60
        w.bool(False)  # :20 d_alpha
        alpha = e.get("type", "alpha") == "alpha"
        w.enum(EC_ALPHA if alpha else EC_DEPTH)  # :22
        _bit_depth(w, e.get("bits", 8), e.get("exp_bits", 0))  # :25
        w.u32(0, (0, 0), (3, 0), (4, 0), (1, 3))  # :26 dim_shift
        w.u32(0, (0, 0), (0, 4), (16, 5), (48, 10))  # :27 no name
        if alpha:
            w.bool(e.get("alpha_associated", False))  # :35
    w.bool(im.get("xyb", False))  # :254 xyb_encoded
    if im.get("grey", False):  # ColorEncodingBundle.java:29-76
        w.bool(False)  # :30 all_default
        w.bool(False)  # :31 no ICC
        w.enum(1)  # :33 CE_GRAY
        w.enum(1)  # :39 WP_D65; a grey space has no primaries (:48)
        w.bool(False)  # :63 no gamma
        w.enum(13)  # :67 TF_SRGB
        w.enum(1)  # :70 RI_RELATIVE
    else:
        w.bool(True)
    if extra_fields:
        w.bool(target is None)  # ToneMapping.java:22 default
        if target is not None:
            w.f16(target)  # :28 intensity_target
            w.f16(0.0)  # :31 min_nits
            w.bool(False)  # :36 relative_to_max_display
            w.f16(0.0)  # :37 linear_below
    w.u64(0)  # :259 extensions
    opsin, up = im.get("opsin"), im.get("up_weights") or {}
    assert opsin is None or im.get("xyb", False)  # :263: the matrix is in the stream of an XYB image only
    w.bool(opsin is None and not up)  # :261 default matrix, default upsampling weights
    if opsin is not None or up:
        if im.get("xyb", False):
            w.bool(opsin is None)  # OpsinInverseMatrix.java:55
            if opsin is not None:
                assert len(opsin["matrix"]) == 9
                for v in list(opsin["matrix"]) + list(opsin["opsin_bias"]) + list(opsin["quant_bias"]):
                    w.f16(v)  # :62-72 the matrix by rows, opsin_bias, quant_bias
                w.f16(opsin["quant_bias_numerator"])  # :73
        w.bits(sum(1 << i for i, k in enumerate((2, 4, 8)) if k in up), 3)  # :266 cw_mask
        for k, n in ((2, 15), (4, 55), (8, 210)):  # :268-293
            if k in up:
                assert len(up[k]) == n
                for v in up[k]:
                    w.f16(v)
    w.pad()  # :309


def _blend_info(w, b, extra, full_frame):  # BlendingInfo.java:26-43
    mode = b.get("mode", REPLACE)
    w.u32(mode, (0, 0), (1, 0), (2, 0), (3, 2))
    if extra and mode in (BLEND, MULADD):
        w.u32(b.get("alpha", 0), (0, 0), (1, 0), (2, 0), (3, 3))
    if extra and mode in (BLEND, MULT, MULADD):
        w.bool(b.get("clamp", False))
    if mode != REPLACE or not full_frame:
        w.bits(b.get("source", 0), 2)


_CROP = ((0, 8), (256, 11), (2304, 14), (18688, 30))


def write_restoration(w, vardct, gab, gab_weights=None, epf_iters=0, sharp_lut=None, channel_scale=None, sigma=None,
                      sigma_for_modular=1.0, variant=None):
    """RestorationFilter.java:46-79, for either encoding. gab_weights: three (w1, w2) pairs; sharp_lut: VarDCT only (:57); sigma: the
    custom sigma block, (quant_mul, pass0, pass2, border_sad_mul) in a VarDCT frame and (pass0, pass2, border_sad_mul) in a Modular
    one (:70 reads quant_mul for VarDCT only); sigma_for_modular: a Modular frame with EPF iterations always holds it, last (:74-75)"""
    w.bool(False)  # :47 all_default
    w.bool(gab)  # :48
    if gab:
        w.bool(gab_weights is not None)  # :49
        if gab_weights is not None:
            assert len(gab_weights) == 3
            for w1, w2 in gab_weights:  # :51-54
                w.f16(w1)
                w.f16(w2)
    w.bits(epf_iters, 2)  # :56
    if epf_iters > 0:
        if vardct:
            w.bool(sharp_lut is not None)  # :57-58
            if sharp_lut is not None:
                for v in sharp_lut:
                    w.f16(v)  # :61
        else:
            assert sharp_lut is None
        w.bool(channel_scale is not None)  # :63
        if channel_scale is not None:
            assert len(channel_scale) == 3
            for v in channel_scale:
                w.f16(v)  # :66
            w.bits(0, 32)  # :67
        if not vardct and variant == "sigma_for_modular_before_sigma_block":
            w.f16(sigma_for_modular)
        w.bool(sigma is not None)  # :69
        if sigma is not None:
            assert len(sigma) == (4 if vardct else 3)
            if not vardct and variant == "quant_mul_in_a_modular_frame":
                w.f16(0.5)
            for v in sigma:
                w.f16(v)  # :70-73
        if not vardct and variant != "sigma_for_modular_before_sigma_block":
            w.f16(sigma_for_modular)  # :74-75
    w.u64(0)  # :76 extensions


def colour_planes(im, fr):
    """the colour channels of a Modular frame's stream (LFGlobal.java:88-96)"""
    return 1 if im.get("grey", False) and not im.get("xyb", False) and not fr.get("ycbcr", False) else 3


def write_frame_header(w, im, fr, variant=None):
    """FrameHeader.java:83-204"""
    n_extra = len(im.get("extra", []))
    ftype = fr.get("type", REGULAR)
    up = fr.get("upsampling", 1)
    h, wd = fr["planes"][0].shape
    crop = fr.get("crop")
    level = fr.get("lf_level", 0)  # an LF frame's: 1..4
    assert (ftype == LF_FRAME) == (level > 0) and level <= 4
    if level:  # FrameHeader.java:163-164: the coded size of an LF frame is ceil(image / 8 ** lf_level); it has no crop (:140)
        assert crop is None and up == 1 and (h, wd) == (-(-im["height"] // (1 << 3 * level)), -(-im["width"] // (1 << 3 * level)))
    elif crop is None and (h * up, wd * up) != (im["height"], im["width"]):
        crop = (0, 0)
    w.bool(False)  # :84 all_default
    w.bits(ftype, 2)  # :85
    w.bits(1, 1)  # :86 Modular
    w.u64((FLAG_PATCHES if fr.get("patches") else 0) | (FLAG_SPLINES if fr.get("splines") else 0) |
          (FLAG_NOISE if fr.get("noise") is not None else 0))  # :87
    if not im.get("xyb", False) or variant == "do_ycbcr_bit_in_an_xyb_image":
        w.bool(fr.get("ycbcr", False))  # :88 do_ycbcr: in the stream of an image that is not XYB only
    else:
        assert not fr.get("ycbcr", False)
    if fr.get("ycbcr", False):
        for _ in range(3):
            w.bits(0, 2)  # :91-110 jpeg_upsampling mode 0 per channel: no subsampling
    w.bits({1: 0, 2: 1, 4: 2, 8: 3}[up], 2)  # :114
    ec_up = fr.get("ec_upsampling", [up] * n_extra)
    for k in ec_up:
        w.bits({1: 0, 2: 1, 4: 2, 8: 3}[k], 2)  # :116
    w.bits(fr.get("group_size_shift", 1), 2)  # :121
    if ftype != REFERENCE_ONLY:
        w.u32(1, (1, 0), (2, 0), (3, 0), (4, 3))  # PassesInfo.java:25 one pass
    if level:
        w.bits(level - 1, 2)  # :139 lf_level, of an LF frame only
    if not level or variant == "crop_bit_in_an_lf_frame_header":
        w.bool(crop is not None)  # :140: not in an LF frame
    x0 = y0 = 0
    if crop is not None:
        if ftype != REFERENCE_ONLY:
            x0, y0 = crop
            w.u32(int(pack_signed(x0)), *_CROP)  # :144-147
            w.u32(int(pack_signed(y0)), *_CROP)
        w.u32(wd * up, *_CROP)  # :150-151: the size before the division by the upsampling factor (:161-162)
        w.u32(h * up, *_CROP)
    normal = ftype in (REGULAR, SKIP_PROGRESSIVE)
    full = crop is None or (x0 <= 0 and y0 <= 0 and y0 + h * up >= im["height"] and x0 + wd * up >= im["width"])  # :157-159
    blend = fr.get("blend", {})
    if normal:
        _blend_info(w, blend, n_extra > 0, full)  # :167
        for b in fr.get("ec_blend", [{}] * n_extra):
            _blend_info(w, b, True, full)  # :169
    duration = fr.get("duration", 0)
    if normal and im.get("animation", False):
        w.u32(duration, (0, 0), (1, 0), (0, 8), (0, 32))  # :174
    else:
        assert duration == 0
    is_last = fr.get("is_last", True) if normal else ftype == REGULAR
    if normal:
        w.bool(is_last)  # :178
    save = fr.get("save_as_reference", 0)
    if not is_last and ftype != LF_FRAME:
        w.bits(save, 2)  # :179: not in an LF frame
    else:
        assert save == 0
    if ftype == REFERENCE_ONLY or (full and normal and (duration == 0 or save != 0) and not is_last and blend.get("mode", REPLACE) == REPLACE):
        w.bool(fr.get("save_before_ct", False))  # :180-184
    else:
        assert not fr.get("save_before_ct", False), "the header has no place for save_before_ct here"
    w.u32(0, (0, 0), (0, 4), (16, 5), (48, 10))  # :188 no name
    rf = fr.get("restoration", {})  # RestorationFilter.java:47 never all_default: the default has Gaborish and two EPF iterations
    assert not set(rf) - {"gab", "gab_weights", "epf_iters", "epf_channel_scale", "pass0", "pass2", "border_sad_mul", "sigma_for_modular"}
    block = [rf[k] for k in ("pass0", "pass2", "border_sad_mul") if k in rf]
    assert len(block) in (0, 3)
    write_restoration(w, False, rf.get("gab", False), rf.get("gab_weights"), rf.get("epf_iters", 0), None, rf.get("epf_channel_scale"),
                      block or None, rf.get("sigma_for_modular", 1.0), variant)
    w.u64(0)  # FrameHeader.java:195 extensions


# ---- predictors --------------------------------------------------------------------------------------------------------------
def _tdiv(a, b):
    """Java's int division: towards zero"""
    a = np.asarray(a, I64)
    return np.where(a >= 0, a // b, -((-a) // b))


def _neighbours(a):
    """W, N, NW, NE, NN, NEE, WW of every sample (ModularChannel.java:95-121), from the true values"""
    a = np.asarray(a, I64)
    h, w = a.shape
    z = np.zeros((h, w), I64)
    left = z.copy()
    left[:, 1:] = a[:, :-1]
    up = z.copy()
    up[1:] = a[:-1]
    x = np.arange(w)[None, :] + z
    y = np.arange(h)[:, None] + z
    W = np.where(x > 0, left, np.where(y > 0, up, 0))
    N = np.where(y > 0, up, np.where(x > 0, left, 0))
    upleft = z.copy()
    upleft[1:, 1:] = a[:-1, :-1]
    NW = np.where(x > 0, np.where(y > 0, upleft, left), np.where(y > 0, up, 0))
    upright = z.copy()
    upright[1:, :-1] = a[:-1, 1:]
    NE = np.where((x + 1 < w) & (y > 0), upright, N)
    up2 = z.copy()
    up2[2:] = a[:-2]
    NN = np.where(y > 1, up2, N)
    upright2 = z.copy()
    upright2[1:, :-2] = a[:-1, 2:]
    NEE = np.where((x + 2 < w) & (y > 0), upright2, NE)
    left2 = z.copy()
    left2[:, 2:] = a[:, :-2]
    WW = np.where(x > 1, left2, W)
    return W, N, NW, NE, NN, NEE, WW


def predict(a, k):
    """ModularChannel.prediction (ModularChannel.java:143-183) for every sample at once; not the weighted predictor"""
    W, N, NW, NE, NN, NEE, WW = _neighbours(a)
    if k == 0:
        return np.zeros(W.shape, I64)
    if k == 1:
        return W
    if k == 2:
        return N
    if k == 3:
        return _tdiv(W + N, 2)
    if k == 4:
        return np.where(np.abs(N - NW) < np.abs(W - NW), W, N)
    if k == 5:
        return np.clip(W + N - NW, np.minimum(W, N), np.maximum(W, N))
    if k == 7:
        return NE
    if k == 8:
        return NW
    if k == 9:
        return WW
    if k == 10:
        return _tdiv(W + NW, 2)
    if k == 11:
        return _tdiv(N + NW, 2)
    if k == 12:
        return _tdiv(N + NE, 2)
    if k == 13:
        return _tdiv(6 * N - 2 * NN + 7 * W + WW + NEE + 3 * NE + 8, 16)
    raise ValueError(k)


class WeightedPredictor:
    """ModularChannel.prePredictWP and the error update of decode (ModularChannel.java:185-236, :347-351), default WPParams
    (WPParams.java:19-24), sample by sample. Python ints: the reference's 32-bit wraps are not reached by the test images"""
    P1, P2, P3 = 16, 10, (7, 7, 7, 0, 0)
    WEIGHT = (13, 12, 12, 12)
    DIV = [(1 << 24) // (i + 1) for i in range(64)]

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.buf = [[0] * w for _ in range(h)]
        self.err = [[[0] * w for _ in range(h)] for _ in range(5)]
        self.sub = [0] * 4
        self.pred = 0

    @staticmethod
    def _floor_log1p(x):  # MathHelper.java:168-174
        c = x.bit_length()
        return c - 1 if ((x + 1) & x) != 0 else c

    def predict(self, y, x):
        """sets self.pred (pred[y][x]) and self.sub; returns the prediction (pred + 3) >> 3"""
        b, w = self.buf, self.w
        W = b[y][x - 1] if x > 0 else b[y - 1][x] if y > 0 else 0
        N = b[y - 1][x] if y > 0 else W
        NW = (b[y - 1][x - 1] if y > 0 else b[y][x - 1]) if x > 0 else (b[y - 1][x] if y > 0 else 0)
        NE = b[y - 1][x + 1] if x + 1 < w and y > 0 else N
        NN = b[y - 2][x] if y > 1 else N
        n3, nw3, ne3, w3, nn3 = N << 3, NW << 3, NE << 3, W << 3, NN << 3

        def eN(e):
            return self.err[e][y - 1][x] if y > 0 else 0

        def eW(e):
            return self.err[e][y][x - 1] if x > 0 else 0

        def eWW(e):
            return self.err[e][y][x - 2] if x > 1 else 0

        def eNW(e):
            return self.err[e][y - 1][x - 1] if x > 0 and y > 0 else eN(e)

        def eNE(e):
            return self.err[e][y - 1][x + 1] if x + 1 < w and y > 0 else eN(e)
        tN, tW, tNE, tNW = eN(4), eW(4), eNE(4), eNW(4)
        sub = self.sub
        sub[0] = w3 + ne3 - n3
        sub[1] = n3 - (((tW + tN + tNE) * self.P1) >> 5)
        sub[2] = w3 - (((tW + tN + tNW) * self.P2) >> 5)
        p = self.P3
        sub[3] = n3 - ((tNW * p[0] + tN * p[1] + tNE * p[2] + (nn3 - n3) * p[3] + (nw3 - w3) * p[4]) >> 5)
        weight = [0] * 4
        for e in range(4):
            s = eN(e) + eW(e) + eNW(e) + eWW(e) + eNE(e)
            if x + 1 == w:
                s += eW(e)
            shift = max(self._floor_log1p(s) - 5, 0)
            weight[e] = 4 + ((self.WEIGHT[e] * self.DIV[s >> shift]) >> shift)
        log_weight = self._floor_log1p(sum(weight) - 1) - 4
        weight = [v >> log_weight for v in weight]
        wsum = sum(weight)
        s = (wsum >> 1) - 1
        for e in range(4):
            s += sub[e] * weight[e]
        pred = (s * self.DIV[wsum - 1]) >> 24
        if ((tN ^ tW) | (tN ^ tNW)) <= 0:
            lo, hi = min(w3, n3, ne3), max(w3, n3, ne3)
            pred = lo if pred < lo else hi if pred > hi else pred
        self.pred = pred
        return (pred + 3) >> 3

    def update(self, y, x, true):
        self.buf[y][x] = true
        for e in range(4):
            self.err[e][y][x] = (abs(self.sub[e] - (true << 3)) + 3) >> 3
        self.err[4][y][x] = self.pred - (true << 3)


def weighted_predictions(a):
    """the weighted predictor's prediction of every sample of `a`, in decoding order"""
    h, w = a.shape
    wp = WeightedPredictor(h, w)
    out = np.zeros((h, w), I64)
    rows = a.tolist()
    for y in range(h):
        for x in range(w):
            out[y, x] = wp.predict(y, x)
            wp.update(y, x, rows[y][x])
    return out


# ---- forward transforms ------------------------------------------------------------------------------------------------------
_PERM = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0))  # ModularStream.java:35-38


def forward_rct(chans, begin_c, rct_type):
    """the forward of ModularStream.java:255-326: the inverse leaves v[j] at begin_c + perm[j] (:325-326)"""
    perm, t = _PERM[rct_type // 7], rct_type % 7
    a, b, c = (np.asarray(chans[begin_c + perm[j]], I64) for j in range(3))
    if t == 1:
        c = c - a
    elif t == 2:
        b = b - a
    elif t == 3:
        b, c = b - a, c - a
    elif t == 4:
        b = b - ((a + c) >> 1)
    elif t == 5:
        b, c = b - ((a + c) >> 1), c - a
    elif t == 6:  # :309-320: out0 = f + b, out1 = c + tmp, out2 = f with tmp = a - (c >> 1), f = tmp - (b >> 1)
        r, g, bl = a, b, c
        b = r - bl
        tmp = bl + (b >> 1)
        c = g - tmp
        a = tmp + (c >> 1)
    chans[begin_c:begin_c + 3] = [a, b, c]


def _tendency(a, b, c):
    """ModularChannel.tendency (ModularChannel.java:23-47)"""
    a, b, c = (np.asarray(v, I64) for v in (a, b, c))
    d, e = 2 * (a - b), 2 * (b - c)
    x = _tdiv(4 * a - 3 * c - b + 6, 12)
    x = np.where((x - (x & 1)) > d, d + 1, x)
    x = np.where((x + (x & 1)) > e, e, x)
    down = x
    x = _tdiv(4 * a - 3 * c - b - 6, 12)
    x = np.where((x + (x & 1)) < d, d - 1, x)
    x = np.where((x - (x & 1)) < e, e, x)
    up = x
    return np.where((a >= b) & (b >= c), down, np.where((a <= b) & (b <= c), up, 0))


def forward_hsqueeze(x):
    """the forward of inverseHorizontalSqueeze (ModularChannel.java:361-387): first = avg + diff / 2 (towards zero), second =
    first - diff, diff = residual + tendency(left, avg, next average)"""
    x = np.asarray(x, I64)
    h, w = x.shape
    nr = w // 2
    A, B = x[:, 0:2 * nr:2], x[:, 1:2 * nr:2]
    diff = A - B
    avg = np.zeros((h, (w + 1) // 2), I64)
    avg[:, :nr] = A - _tdiv(diff, 2)
    if w & 1:
        avg[:, nr] = x[:, w - 1]
    cur = avg[:, :nr]
    nxt = np.concatenate([avg, avg[:, -1:]], 1)[:, 1:nr + 1]  # :372 the next average, or this one at the end
    left = cur.copy()  # :373 the sample before, or the average at the start
    if nr > 1:
        left[:, 1:] = B[:, :-1]
    return avg, diff - _tendency(left, cur, nxt)


def forward_squeeze_step(chans, horizontal, in_place, begin_c, num_c):
    """the channel list after one step, as ModularStream.java:137-167 lays it out"""
    end = begin_c + num_c - 1
    offset = end + 1 if in_place else len(chans)
    for k in range(begin_c, end + 1):
        if horizontal:
            avg, res = forward_hsqueeze(chans[k])
        else:
            avg, res = forward_hsqueeze(np.asarray(chans[k]).T)
            avg, res = avg.T, res.T
        chans[k] = avg
        chans.insert(offset + k - begin_c, res)


def default_squeeze_params(chans, nb_meta):
    """ModularStream.java:110-131, the size of channel 0 as the reference takes it (:113)"""
    first, count = nb_meta, len(chans) - nb_meta
    h, w = chans[0].shape
    out = []
    if count > 2 and chans[first + 1].shape == (h, w):
        out += [(True, False, first + 1, 2), (False, False, first + 1, 2)]
    if h >= w and h > 8:
        out.append((False, True, first, count))
        h = (h + 1) // 2
    while w > 8 or h > 8:
        if w > 8:
            out.append((True, True, first, count))
            w = (w + 1) // 2
        if h > 8:
            out.append((False, True, first, count))
            h = (h + 1) // 2
    return out


def forward_palette(chans, begin_c, num_c, nb_deltas, d_pred):
    """channels begin_c .. begin_c + num_c - 1 become one index channel and the palette goes to the front (ModularStream.java:97-107,
    :327-378). With nb_deltas > 0 the most frequent (sample - prediction) tuples are the first entries and a pixel takes one where
    it can; every other pixel names a colour. Returns (nb_colors, the weighted predictor's pred plane or None)"""
    src = [np.asarray(chans[begin_c + c], I64) for c in range(num_c)]
    h, w = src[0].shape
    flat = np.stack([s.reshape(-1) for s in src], 1)
    if nb_deltas == 0:
        colours, index = np.unique(flat, axis=0, return_inverse=True)
        palette, index = colours.T, index.reshape(h, w)
    elif d_pred != 6:
        delta = np.stack([(s - predict(s, d_pred)).reshape(-1) for s in src], 1)
        tuples, counts = np.unique(delta, axis=0, return_counts=True)
        deltas = tuples[np.argsort(-counts, kind="stable")[:nb_deltas]]
        nb_deltas = len(deltas)
        which = np.full(h * w, -1, I64)
        for k in range(nb_deltas - 1, -1, -1):
            which[(delta == deltas[k]).all(1)] = k
        # (one pixel in three that could be a delta stays a colour: both kinds of entry meet in every neighbourhood)
        which[np.arange(h * w) % 3 == 0] = -1
        colours, inv = np.unique(flat[which < 0], axis=0, return_inverse=True)
        index = which.copy()
        index[which < 0] = nb_deltas + inv.reshape(-1)
        palette, index = np.concatenate([deltas, colours]).T, index.reshape(h, w)
    else:
        # :369 reads pred[y][x] of the index channel's own decode (forceWP, :105-106), so the index of a pixel depends on the
        # indices before it. One channel only: the reference's copies of the index channel carry no pred plane (ModularChannel.java:73-83)
        assert num_c == 1
        rows = src[0].tolist()
        deltas = list(range(-(nb_deltas // 2), nb_deltas - nb_deltas // 2))
        colours = sorted(set(src[0].reshape(-1).tolist()))
        where = {v: nb_deltas + i for i, v in enumerate(colours)}
        wp = WeightedPredictor(h, w)
        index = np.zeros((h, w), I64)
        for y in range(h):
            for x in range(w):
                d = rows[y][x] - wp.predict(y, x)
                i = deltas.index(d) if d in deltas and (x + y) % 3 else where[rows[y][x]]
                index[y, x] = i
                wp.update(y, x, i)
        palette = np.array([deltas + colours], I64)
    del chans[begin_c + 1:begin_c + num_c]
    chans[begin_c] = index
    chans.insert(0, palette)
    return palette.shape[1], nb_deltas


def forward_transforms(planes, transforms):
    """the encoded channel list, the transform records as the bitstream holds them, and the set of channel-list positions decoded
    with forceWP"""
    chans = [np.asarray(p, I64) for p in planes]
    nb_meta, records = 0, []
    for t in transforms:
        if t[0] == "rct":
            forward_rct(chans, t[1], t[2])
            records.append(dict(tr=0, begin_c=t[1], rct_type=t[2]))
        elif t[0] == "palette":
            _, begin_c, num_c, nb_deltas, d_pred = t
            nb_colors, nb_deltas = forward_palette(chans, begin_c, num_c, nb_deltas, d_pred)
            nb_meta = nb_meta + 2 - num_c if begin_c < nb_meta else nb_meta + 1  # ModularStream.java:98-101
            records.append(dict(tr=1, begin_c=begin_c, num_c=num_c, nb_colors=nb_colors, nb_deltas=nb_deltas, d_pred=d_pred))
        elif t[0] == "squeeze":
            params = t[1]
            for hor, in_place, begin_c, num_c in (params if params is not None else default_squeeze_params(chans, nb_meta)):
                if begin_c < nb_meta:  # :141-147
                    assert in_place and begin_c + num_c - 1 < nb_meta
                    nb_meta += num_c
                forward_squeeze_step(chans, hor, in_place, begin_c, num_c)
            records.append(dict(tr=2, params=params or []))
        else:
            raise ValueError(t)
    return chans, records


def _force_wp(n_chans, planes_shapes, records):
    """which positions of the final channel list decode with forceWP: replay the list's bookkeeping (ModularStream.java:96-107,
    :137-167) on labels"""
    flags = [False] * len(planes_shapes)
    for r in records:
        if r["tr"] == 1:
            del flags[r["begin_c"] + 1:r["begin_c"] + r["num_c"]]
            if r["nb_deltas"] > 0 and r["d_pred"] == 6:
                flags[r["begin_c"]] = True
            flags.insert(0, False)
        elif r["tr"] == 2:
            for hor, in_place, begin_c, num_c in r["steps"]:
                end = begin_c + num_c - 1
                offset = end + 1 if in_place else len(flags)
                for k in range(begin_c, end + 1):
                    flags.insert(offset + k - begin_c, flags[k])  # new ModularChannel(chan) copies forceWP (ModularChannel.java:73-75)
    assert len(flags) == n_chans
    return flags


def _write_transform(w, r):  # TransformInfo.java:22-48
    w.bits(r["tr"], 2)
    if r["tr"] != 2:
        w.u32(r["begin_c"], (0, 3), (8, 6), (72, 10), (1096, 13))
    if r["tr"] == 0:
        w.u32(r["rct_type"], (6, 0), (0, 2), (2, 4), (10, 6))
    if r["tr"] == 1:
        w.u32(r["num_c"], (1, 0), (3, 0), (4, 0), (1, 13))
        w.u32(r["nb_colors"], (0, 8), (256, 10), (1280, 12), (5376, 16))
        w.u32(r["nb_deltas"], (0, 0), (1, 8), (257, 10), (1281, 16))
        w.bits(r["d_pred"], 4)
    if r["tr"] == 2:
        w.u32(len(r["params"]), (0, 0), (1, 4), (9, 6), (41, 8))
        for hor, in_place, begin_c, num_c in r["params"]:  # SqueezeParam.java:13-18
            w.bool(hor)
            w.bool(in_place)
            w.u32(begin_c, (0, 3), (8, 6), (72, 10), (1096, 13))
            w.u32(num_c, (1, 0), (2, 0), (3, 0), (4, 4))


def write_tree(w, fr):
    """MATree.java:34-88: the tree's own stream has six contexts (one cluster here); nodes breadth first. Returns leaf(channel
    index) -> (context, predictor)"""
    write_entropy_header(w, 6)
    tree = fr.get("tree")
    if tree is None:
        p = fr.get("predictor", 5)
        write_symbols(w, [0, p, 0, 0, 0])  # :42 property + 1 = 0: a leaf; :56 predictor; :59 offset; :60 mul_log; :63 mul_bits
        leaves = 1
        leaf = lambda ci: p  # noqa: E731
    else:
        v, (pl, pr) = tree["value"], tree["predictors"]
        # :42 property 0 (the channel index) + 1; :45 its value; then the left leaf (property > value, :126) and the right one
        write_symbols(w, [1, int(pack_signed(v)), 0, pl, 0, 0, 0, 0, pr, 0, 0, 0])
        leaves = 2
        leaf = lambda ci: pl if ci > v else pr  # noqa: E731
    write_entropy_header(w, leaves)  # :78: (nodes + 1) / 2 contexts
    return leaf


def write_patches(w, patches, num_alpha, clusters=None, variant=None):
    """LFGlobal.java:34-43 and Patch.readPatch (Patch.java:21-64): one stream of ten contexts on the same coder. patches:
    [dict(ref, x0, y0, width, height, positions=[(x, y)], blend=[[dict(mode, alpha, clamp)]] per position: the colours, then each
    extra channel)]; mode is the patch blend mode 0..7. clusters=(map of 10, configs): the stream on an EntropyCoder with that
    clustering, every symbol under the context the reader names; without it the one flat cluster the writer always wrote"""
    syms, ctxs = [len(patches)], [0]  # LFGlobal.java:36

    def put(ctx, *vals):
        syms.extend(int(v) for v in vals)
        ctxs.extend([ctx] * len(vals))
    for p in patches:
        put(1, p["ref"])  # Patch.java:23
        put(3, p["x0"], p["y0"])  # :24-25
        put(2, p["width"] - 1, p["height"] - 1)  # :26-27
        put(7, len(p["positions"]) - 1)  # :29
        px = py = 0
        for j, (x, y) in enumerate(p["positions"]):
            if j == 0:
                put(4, x, y)  # :36-37
            elif variant == "patch_position_differences_unsigned":  # a difference that is not negative written as it is
                put(6, *[d if d >= 0 else int(pack_signed(d)) for d in (x - px, y - py)])
            else:
                put(6, int(pack_signed(x - px)), int(pack_signed(y - py)))  # :39-42
            px, py = x, y
            for b in p["blend"][j]:
                put(5, b["mode"])  # :47
                if b["mode"] > 3 and num_alpha > 1:
                    put(8, b.get("alpha", 0))  # :52-53
                if b["mode"] > 2:
                    put(9, 1 if b.get("clamp", False) else 0)  # :57-58
    if clusters is None:
        write_entropy_header(w, 10)
        write_symbols(w, syms)
    else:
        assert len(clusters[0]) == 10
        coder = EntropyCoder(*clusters)
        coder.write_header(w)
        coder.write(w, ctxs, syms)


def write_splines(w, sp, variant=None):
    """SplinesBundle.java:24-75: one stream of six contexts. sp: dict(quant_adjust, splines=[dict(control=[(x, y), ..],
    coeff=[X[32], Y[32], B[32], sigma[32]])], clusters=(map of 6, configs))"""
    coder = EntropyCoder(*sp["clusters"])
    assert len(sp["clusters"][0]) == 6 and len(sp["clusters"][1]) >= 3
    coder.write_header(w)  # :25
    syms, ctxs = [], []

    def put(ctx, *vals):
        syms.extend(int(v) for v in vals)
        ctxs.extend([ctx] * len(vals))
    splines = sp["splines"]
    put(2, len(splines) - (0 if variant == "spline_count_without_the_one" else 1))  # :26
    if variant == "quant_adjust_before_the_start_positions":
        put(0, pack_signed(sp["quant_adjust"]))
    px = py = 0
    for i, s in enumerate(splines):  # :28-36 the first start position raw, the later ones signed differences; x before y
        x, y = s["control"][0]
        if i == 0:
            assert x >= 0 and y >= 0
            pair = (x, y)
        else:
            pair = (pack_signed(x - px), pack_signed(y - py))
        put(1, *(pair[::-1] if variant == "spline_start_y_before_x" else pair))
        px, py = x, y
    if variant != "quant_adjust_before_the_start_positions":
        put(0, pack_signed(sp["quant_adjust"]))  # :37
    for s in splines:
        pts = [(int(x), int(y)) for x, y in s["control"]]
        put(3, len(pts) - 1)  # :45
        dx = dy = 0
        for j in range(1, len(pts)):  # :50-63: the reader sums the symbols twice, so they are second differences
            fx, fy = pts[j][0] - pts[j - 1][0], pts[j][1] - pts[j - 1][1]
            if variant == "spline_points_as_first_differences":
                put(4, pack_signed(fx), pack_signed(fy))
            else:
                put(4, pack_signed(fx - dx), pack_signed(fy - dy))  # :51-52 x before y
            dx, dy = fx, fy
        cx, cy, cb, cs = s["coeff"]
        assert all(len(c) == 32 for c in s["coeff"])
        for c in ((cy, cx, cb, cs) if variant == "spline_coefficients_y_x_b_sigma" else (cx, cy, cb, cs)):  # :64-71
            put(5, *[pack_signed(v) for v in c])
    coder.write(w, ctxs, syms)


def write_frame(im, fr, variant=None):
    head = BitWriter()
    write_frame_header(head, im, fr, variant)
    w = BitWriter()
    def patches():
        if fr.get("patches"):  # LFGlobal.java:34-43
            write_patches(w, fr["patches"], sum(1 for e in im.get("extra", []) if e.get("type", "alpha") == "alpha"),
                          fr.get("patch_clusters"), variant)

    def splines():
        if fr.get("splines"):  # :46-49
            write_splines(w, fr["splines"], variant)

    def noise():
        for v in fr.get("noise") or []:
            w.bits(v, 10)  # :53-58
    order = [patches, splines, noise]  # :34-61
    if variant == "splines_before_patches":
        order = [splines, patches, noise]
    elif variant == "noise_before_splines":
        order = [patches, noise, splines]
    for field in order:
        field()
    lfd = fr.get("lf_dequant")
    w.bool(lfd is None)  # LFGlobal.java:62 default LF dequantisation
    if lfd is not None:
        assert len(lfd) == 3
        for v in lfd:
            w.f16(v)  # :64 times 1 / 128
    w.bool(True)  # :82 a global tree
    leaf = write_tree(w, fr)
    w.bool(True)  # ModularStream.java:78 use the global tree
    w.bool(True)  # WPParams.java:18 default parameters
    chans, records = forward_transforms(fr["planes"], fr.get("transforms", []))
    # the squeeze steps a record stands for, for the forceWP bookkeeping
    replay, nb_meta = [np.zeros(p.shape, np.int8) for p in fr["planes"]], 0
    shifts = [(0, 0)] * len(replay)  # (vshift, hshift) of every channel of the list: dim_shift is 0 here (ModularStream.java:88-89)
    for r in records:
        if r["tr"] == 1:
            del replay[r["begin_c"] + 1:r["begin_c"] + r["num_c"]]
            del shifts[r["begin_c"] + 1:r["begin_c"] + r["num_c"]]
            replay.insert(0, np.zeros((r["num_c"], r["nb_colors"]), np.int8))
            shifts.insert(0, (-1, -1))  # :107
            nb_meta = nb_meta + 2 - r["num_c"] if r["begin_c"] < nb_meta else nb_meta + 1
        elif r["tr"] == 2:
            r["steps"] = list(r["params"]) or default_squeeze_params(replay, nb_meta)
            for s in r["steps"]:
                if s[2] < nb_meta:
                    nb_meta += s[3]
                forward_squeeze_step(replay, *s)
                end = s[2] + s[3] - 1
                offset = end + 1 if s[1] else len(shifts)
                for k in range(s[2], end + 1):  # :152-165: the step's axis gains a shift, the residual is a copy
                    v, h = shifts[k]
                    shifts[k] = (v, h + 1) if s[0] else (v + 1, h)
                    shifts.insert(offset + k - s[2], shifts[k])
    force = _force_wp(len(chans), [p.shape for p in fr["planes"]], records)
    w.u32(len(records), (0, 0), (1, 0), (2, 4), (18, 8))  # ModularStream.java:80
    for r in records:
        _write_transform(w, r)
    ci = 0
    for a, forced in zip(chans, force):  # :194-204: an empty channel takes no channel index
        if a.size == 0:
            continue
        assert a.min() >= -(1 << 31) and a.max() < (1 << 31)
        k = leaf(ci)
        pred = weighted_predictions(a) if k == 6 else predict(a, k)
        write_symbols(w, pack_signed(a - pred))  # ModularChannel.java:344-346: multiplier 1, offset 0
        ci += 1
    # An empty channel is allocated, not decoded (ModularStream.java:198-199; ModularChannel.decoded stays false), so the reference
    # still hands it on: with both shifts >= 3 to the LF group's stream (Frame.java:266-273), else with 0 <= min(shift) < 3 to the
    # pass group's (Pass.java:33-41: one pass, minShift 0, maxShift 3). Each such stream has a channel list, so its header is read
    # (ModularStream.java:78-83: the global tree, default WP parameters, no transforms) although no channel of it holds a sample.
    assert len(shifts) == len(chans)
    empty = [s for a, s in zip(chans, shifts) if a.size == 0]
    for members in ([s for s in empty if s[0] >= 3 and s[1] >= 3], [s for s in empty if 0 <= min(s) < 3]):
        if members:
            w.bool(True)
            w.bool(True)
            w.u32(0, (0, 0), (1, 0), (2, 4), (18, 8))
    body = w.tobytes()
    head.bool(False)  # Frame.java:153 no permutation
    head.pad()  # :168
    head.u32(len(body), (0, 10), (1024, 14), (17408, 22), (4211712, 30))  # :173 the one TOC entry
    return head.tobytes() + body  # :177 padded, then the section (a single entry is read from the same reader, :388-390)


def encode(im, variant=None):
    assert variant is None or variant in VARIANTS + FEATURE_VARIANTS
    for fr in im["frames"]:
        assert len(fr["planes"]) == colour_planes(im, fr) + len(im.get("extra", []))
        gd = 128 << fr.get("group_size_shift", 1)
        for p in fr["planes"]:
            assert p.shape == fr["planes"][0].shape and p.shape[0] <= gd and p.shape[1] <= gd, "every channel fits one group"
    w = BitWriter()
    write_image_header(w, im)
    return w.tobytes() + b"".join(write_frame(im, fr, variant) for fr in im["frames"])
