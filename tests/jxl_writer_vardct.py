"""A writer of bare JPEG XL codestreams that hold one VarDCT frame: test infrastructure, numpy only, built on jxl_writer.py.

Like jxl_writer.py it is a second reading of the format made from the reference's READER (the Java file and line each field is read
at is cited beside the code that writes it; J = com/traneptora/jxlatte), not from jxlatte_amd/frontend: what encode() writes from the
SOURCE arrays, the front-end must hand out as the same integers. Every context of the HF coefficient stream is computed here
(predicted non-zeros, block context, non-zero context, coefficient context with `prev`), and every entropy stream has several
clusters with different hybrid-integer configurations (jxl_writer.EntropyCoder), so a symbol read under a wrong context desynchronises
the stream. No ANS, no LZ77.

One fact of the reference that shapes the cases: a VarDCT frame has no group_size_shift field -- FrameHeader.java:121 reads it for
Modular frames only, so group_dim is 256 and an LF group 2048 pixels for every VarDCT frame.

encode(src, variant=None) takes the SOURCE dict:
  width, height; xyb=True; do_ycbcr=False, shift_y=[0, 0, 0], shift_x=[0, 0, 0] (the channel's final shifts, X / Y / B or Cb / Y / Cr);
  xqm=3, bqm=2; pass_shifts=[] (one per pass but the last), downsample=[], last_pass=[]; skip_smoothing=False;
  gab=True, gab_weights=None | ([3], [3]); epf_iters=0..3, sharp_lut=None | [8], channel_scale=None | [3],
  sigma=None | (quant_mul, pass0, pass2, border_sad_mul);
  lf_dequant=None | [3] (the F16 values; the dequantiser is value / 128), global_scale, quant_lf;
  block_ctx=None | dict(lf_thresholds=[3 lists], qf_thresholds=[..], cluster_map=[..]);
  corr=None | dict(colour_factor, base_x, base_b, x_factor_lf, b_factor_lf);
  tree=dict(property=0 | 1, value, predictors=(left, right)), tree_clusters=(cluster map of the two leaves, configs);
  lfgroups=[dict(extra_precision, lf_quant=[3 int arrays, buffer order], blocks=[(y, x, type)], hf_mul=[cells], sharpness=[cells],
                 x_from_y=[tiles], b_from_y=[tiles])];
  quant=None | [17 dicts(mode=0..7, dct, par, p44, denominator)] in the shape of quant_weights_ref (par of the 64 x / AFV modes as the
        reader leaves them: already times 64);
  num_presets, presets=[pass][group]; orders=[pass]{order id: [3 permutations]}, order_clusters=(map of 8, configs);
  hf_clusters=[pass](cluster map of 495 * presets * block clusters, configs);
  coeff_passes=[pass][3 int arrays of the channel's padded size]: the SOURCE coefficient is sum_p coeff_passes[p] << shift_p;
  what the frame's tail depends on (every default writes the bytes the writer wrote without these keys):
  upsampling=1 | 2 | 4 | 8 with image_height, image_width (width and height stay the frame's coded size: the image header carries
        the image's, the frame header no crop, and ceil(image / upsampling) is the frame);
  extra=[dict(bits=8, alpha_associated=False, plane=2-D ints of the frame's size, upsampling=k)]: alpha channels, in the global
        Modular stream at the end of LfGlobal, or -- larger than a group -- as group crops in the pass groups' Modular streams;
  noise=None | [8 ints of 10 bits]; opsin, up_weights, intensity_target as jxl_writer.write_image_header takes them;
  what makes the frame one of several (encode_stream writes one image header and a list of frames, each from write_frame here or from
  jxl_writer.write_frame; encode is the stream of one frame):
  lf_level=0 | 1..4: an LF frame of that level, whose coded size width x height is ceil(image / 8 ** lf_level);
  use_lf_frame=False: the frame's LF comes from the LF frame stored before it -- as the REFERENCE reads such a frame, which is not in
        every point as the format has it: the header holds no jpeg-upsampling modes and no upsampling fields (FrameHeader.java:91, :113),
        an LF group neither extra_precision nor an LF stream (LFCoefficients.java:44-57), and every cell's LF index is 0 (:24);
        lf_quant of the LF groups is then not written (only the variant that is wrong about the LF index reads it);
  crop=None | (x0, y0): width x height at that origin of the image; is_last=True;
  permutation=None | [entries]: the TOC's (Frame.java:153-168): logical section i lies in slot permutation[i] (:190), the lengths are
        in slot order; perm_clusters=(map of 8, configs) is its entropy stream's.
  the features of LfGlobal and the reference slots (jxl_writer_features_cases.py):
  patches=None | [..] with patch_clusters=None | (map of 10, configs), and splines=None | dict(..): as jxl_writer.write_patches and
        write_splines take them; they set flags 2 and 16 and lie in front of the noise values, in that order (LFGlobal.java:34-61);
  type=REGULAR | SKIP_PROGRESSIVE | REFERENCE_ONLY (a reference-only frame has no passes field, no crop origin, no blending info and
        no is_last bit, and is never the last: FrameHeader.java:138-178); save_as_reference=0..3 of a frame that is not the last (:179);
        save_before_ct where :180-184 read it -- an assertion where the header has no place for the bit.
VARIANTS, LF_VARIANTS and FEATURE_VARIANTS name writers that are wrong on purpose; the tests show that the front-end tells each from
the true one."""
import numpy as np

import jxl_writer as W
from jxl_writer import BitWriter, EntropyCoder, pack_signed

I64 = np.int64
GROUP_DIM = 256  # FrameHeader.java:121-122
FLAG_NOISE = 1 << 0  # FrameFlags.java:12
FLAG_PATCHES, FLAG_SPLINES = W.FLAG_PATCHES, W.FLAG_SPLINES  # :13-14
FLAG_USE_LF_FRAME = 1 << 5  # FrameFlags.java:15
FLAG_SKIP_ADAPTIVE_LF_SMOOTHING = 1 << 7  # FrameFlags.java:16
C_MAP = (1, 0, 2)  # Frame.java:42 cMap

VARIANTS = ("predicted_rounded_down", "block_ctx_channel_not_exchanged", "prev_inverted", "nonzero_ctx_without_4", "vertical_not_flipped",
            "shift_on_token", "lf_buffer_order", "block_info_rows_exchanged", "raw_stream_index_off_by_one", "noise_lut_after_lf_dequant",
            "extra_group_stream_index_off_by_one")
# writers that are wrong about an LF frame, a frame that uses one, or a permuted TOC (the cases of jxl_writer_lfframe_cases.py)
LF_VARIANTS = ("upsampling_bits_in_a_use_lf_frame_header", "lf_stream_in_a_use_lf_frame_group",
               "lf_index_from_thresholds_in_a_use_lf_frame_group", "crop_bit_in_an_lf_frame_header", "toc_lengths_in_logical_order",
               "toc_permutation_inverted")

# writers that are wrong about the patch dictionary, the splines or their place in LfGlobal (the cases of jxl_writer_features_cases.py)
FEATURE_VARIANTS = W.FEATURE_VARIANTS

# (parameterIndex, orderID, transformMethod, pixelHeight, pixelWidth) by type: TransformType.java:10-36
TYPES = ((0, 0, 0, 8, 8), (1, 1, 3, 8, 8), (2, 1, 1, 8, 8), (3, 1, 2, 8, 8), (4, 2, 0, 16, 16), (5, 3, 0, 32, 32), (6, 4, 0, 16, 8),
         (6, 4, 0, 8, 16), (7, 5, 0, 32, 8), (7, 5, 0, 8, 32), (8, 6, 0, 32, 16), (8, 6, 0, 16, 32), (9, 1, 5, 8, 8), (9, 1, 4, 8, 8),
         (10, 1, 6, 8, 8), (10, 1, 6, 8, 8), (10, 1, 6, 8, 8), (10, 1, 6, 8, 8), (11, 7, 0, 64, 64), (12, 8, 0, 64, 32),
         (12, 8, 0, 32, 64), (13, 9, 0, 128, 128), (14, 10, 0, 128, 64), (14, 10, 0, 64, 128), (15, 11, 0, 256, 256),
         (16, 12, 0, 256, 128), (16, 12, 0, 128, 256))


def cells(t):  # dctSelectHeight, dctSelectWidth (:152-153)
    return TYPES[t][3] >> 3, TYPES[t][4] >> 3


def order_id(t):
    return TYPES[t][1]


def flip(t):  # TransformType.flip (:129-131)
    _, _, method, ph, pw = TYPES[t]
    return ph > pw or (method == 0 and ph == pw)


def vertical(t):  # :121-123
    return TYPES[t][3] > TYPES[t][4]


def matrix_size(index):  # of the first type that is not vertical (:69-72, :154-155)
    ph, pw = next((t[3], t[4]) for t in TYPES if t[0] == index and t[3] <= t[4])
    return min(ph, pw), max(ph, pw)


_natural = {}


def natural_order(oid):
    """HFPass.getNaturalOrder (HFPass.java:17-65): the LLF corner in raster order, then a zig-zag over the square the block is
    scaled to; Arrays.sort on objects is stable, so ties keep the raster order. Returns [(y, x)] of the order id's horizontal type"""
    if oid not in _natural:
        ph, pw = next((t[3], t[4]) for t in TYPES if t[1] == oid and t[3] <= t[4])  # TransformType.java:74-77
        dsh, dsw = ph >> 3, pw >> 3
        maxd = max(dsh, dsw)

        def key(p):
            y, x = p
            if y < dsh and x < dsw:  # :22-32
                return (0, y, x)
            sy, sx = y * maxd // dsh, x * maxd // dsw  # :33-36
            k1, k2 = sy + sx, sx - sy
            return (1, k1, -k2 if k1 & 1 else k2)  # :37-47
        _natural[oid] = sorted([(y, x) for y in range(ph) for x in range(pw)], key=key)
    return _natural[oid]


def ceil_log1p(x):  # MathHelper.java:156-158
    return int(x).bit_length()


def padded_size(src):
    """Frame.getPaddedFrameSize (Frame.java:924-941) of the frame's bounds (FrameHeader.java:196-199)"""
    fy, fx = 1 << max(src.get("shift_y", [0] * 3)), 1 << max(src.get("shift_x", [0] * 3))
    h, w = -(-src["height"] // fy) * fy, -(-src["width"] // fx) * fx
    return (-(-((h + 7) >> 3) // fy) * fy) << 3, (-(-((w + 7) >> 3) // fx) * fx) << 3


def geometry(src):
    ph, pw = padded_size(src)
    cols = -(-src["width"] // GROUP_DIM)  # Frame.java:127-130: from the bounds, not the padded size
    rows = -(-src["height"] // GROUP_DIM)
    lcols = -(-src["width"] // (GROUP_DIM << 3))
    lrows = -(-src["height"] // (GROUP_DIM << 3))
    return dict(ph=ph, pw=pw, cols=cols, num_groups=cols * rows, lcols=lcols, num_lf_groups=lcols * lrows)


def num_passes(src):
    return len(src.get("pass_shifts", [])) + 1


def image_size(src):
    """(height, width) of the image header: the frame's own size unless the frame is upsampled, an LF frame or a crop"""
    k = src.get("upsampling", 1) << (3 * src.get("lf_level", 0))
    ih, iw = src.get("image_height", src["height"] * k), src.get("image_width", src["width"] * k)
    # FrameHeader.java:161-164 on the image's size (:153), or on the crop's (:150-151)
    assert src.get("crop") is not None or (-(-ih // k) == src["height"] and -(-iw // k) == src["width"])
    return ih, iw


def extras_in_groups(src):
    """whether the extra channels are left to the pass groups: decodeChannels(reader, true) stops at the first channel larger than
    a group (ModularStream.java:196-197), and every channel here has the frame's size (:86-90)"""
    return bool(src.get("extra")) and max(src["height"], src["width"]) > GROUP_DIM


# ---- headers ---------------------------------------------------------------------------------------------------------------
def frame_flags(src):
    return (FLAG_SKIP_ADAPTIVE_LF_SMOOTHING if src.get("skip_smoothing", False) else 0) | \
        (FLAG_NOISE if src.get("noise") is not None else 0) | (FLAG_USE_LF_FRAME if src.get("use_lf_frame", False) else 0) | \
        (FLAG_PATCHES if src.get("patches") else 0) | (FLAG_SPLINES if src.get("splines") else 0)


def write_frame_header(w, src, variant=None):
    """FrameHeader.java:83-204 for one VarDCT frame: regular -- the whole image, 1 / upsampling of it, or a crop -- or an LF frame"""
    xyb = src.get("xyb", True)
    level, use_lf = src.get("lf_level", 0), src.get("use_lf_frame", False)
    ftype = src.get("type", W.REGULAR)
    assert 0 <= level <= 4 and ftype in (W.REGULAR, W.SKIP_PROGRESSIVE, W.REFERENCE_ONLY) and not (level and ftype != W.REGULAR)
    w.bool(False)  # :84 all_default
    w.bits(W.LF_FRAME if level else ftype, 2)  # :85
    w.bits(0, 1)  # :86 VARDCT
    w.u64(frame_flags(src))  # :87
    sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
    if not xyb:
        w.bool(src.get("do_ycbcr", False))  # :88
    if use_lf:  # :91, :113: neither the jpeg-upsampling modes nor the upsampling fields are in the stream
        assert not any(sy) and not any(sx) and src.get("upsampling", 1) == 1 and not src.get("extra")
    elif src.get("do_ycbcr", False):
        # :91-110 read a mode per channel, :196-203 turn it into max - mode: the mode is the channel's sampling factor
        my, mx = max(sy), max(sx)
        for c in range(3):
            w.bits({(0, 0): 0, (1, 1): 1, (0, 1): 2, (1, 0): 3}[(my - sy[c], mx - sx[c])], 2)
    else:
        assert not any(sy) and not any(sx)
    code = {1: 0, 2: 1, 4: 2, 8: 3}
    extra = src.get("extra", [])
    if not use_lf or variant == "upsampling_bits_in_a_use_lf_frame_header":
        w.bits(code[src.get("upsampling", 1)], 2)  # :114
        for e in extra:
            w.bits(code[e.get("upsampling", 1)], 2)  # :116
    # :121 no group_size_shift for a VarDCT frame
    if xyb:
        w.bits(src.get("xqm", 3), 3)  # :128-129
        w.bits(src.get("bqm", 2), 3)
    shifts, ds, last = src.get("pass_shifts", []), src.get("downsample", []), src.get("last_pass", [])
    n = len(shifts) + 1
    if ftype == W.REFERENCE_ONLY:
        assert n == 1  # FrameHeader.java:138: a reference-only frame has the default PassesInfo and no field for it
    else:
        w.u32(n, (1, 0), (2, 0), (3, 0), (4, 3))  # PassesInfo.java:25
    if n != 1:
        w.u32(len(ds), (0, 0), (1, 0), (2, 0), (3, 1))  # :26
        assert len(ds) < n and len(last) == len(ds)
        for s in shifts:
            w.bits(s, 2)  # :31
        for d in ds:
            w.bits({1: 0, 2: 1, 4: 2, 8: 3}[d], 2)  # :35
        for p in last:
            w.u32(p, (0, 0), (1, 0), (2, 0), (0, 3))  # :38
    crop = src.get("crop")
    if level:
        w.bits(level - 1, 2)  # FrameHeader.java:139 lf_level, of an LF frame only
        # :140 no crop bit, :155 and :166 no blending info, :178 no is_last, :179 no save_as_reference in an LF frame; its coded size
        # is ceil(image / 8 ** lf_level) (:163-164)
        assert crop is None and not extra
        if variant == "crop_bit_in_an_lf_frame_header":
            w.bool(False)
    else:
        w.bool(crop is not None)  # :140
        full = True
        if crop is not None:
            x0, y0 = crop
            if ftype != W.REFERENCE_ONLY:
                w.u32(int(pack_signed(x0)), *W._CROP)  # :144-147
                w.u32(int(pack_signed(y0)), *W._CROP)
            else:
                assert (x0, y0) == (0, 0)  # :143
            w.u32(src["width"] * src.get("upsampling", 1), *W._CROP)  # :150-151
            w.u32(src["height"] * src.get("upsampling", 1), *W._CROP)
            ih, iw = image_size(src)
            full = x0 <= 0 and y0 <= 0 and y0 + src["height"] * src.get("upsampling", 1) >= ih and \
                x0 + src["width"] * src.get("upsampling", 1) >= iw  # :157-159
        normal = ftype != W.REFERENCE_ONLY  # :155
        if normal:
            W._blend_info(w, {}, len(extra) > 0, full)  # BlendingInfo.java:27 REPLACE: on the full frame nothing else
            for _ in extra:
                W._blend_info(w, {}, True, full)  # :169 one per extra channel
        is_last = src.get("is_last", True) if normal else False  # :178: a reference-only frame is not the last
        if normal:
            w.bool(is_last)
        save = src.get("save_as_reference", 0)
        assert 0 <= save <= 3
        if not is_last:
            w.bits(save, 2)  # :179 save_as_reference
        else:
            assert save == 0, "the header has no place for save_as_reference in the last frame"
        if not normal or (full and not is_last):
            w.bool(src.get("save_before_ct", False))  # :180-184: reference only, or a full REPLACE frame of duration 0 that is not the last
        else:
            assert not src.get("save_before_ct", False), "the header has no place for save_before_ct here"
    w.u32(0, (0, 0), (0, 4), (16, 5), (48, 10))  # :188 no name
    gw = src.get("gab_weights")
    W.write_restoration(w, True, src.get("gab", True), None if gw is None else list(zip(gw[0], gw[1])), src.get("epf_iters", 0),
                        src.get("sharp_lut"), src.get("channel_scale"), src.get("sigma"))  # RestorationFilter.java:46-79
    w.u64(0)  # FrameHeader.java:195 extensions


class Modular:
    """the frame's global MA tree (MATree.java:34-88) and the sub-streams that use it: one split on the channel index (property
    0) or the stream index (property 1, MATree.java:111-127), two leaves with their own predictor and context, and the tree's
    symbol stream in two clusters"""

    def __init__(self, src):
        t = src.get("tree", dict(property=0, value=0, predictors=(5, 1)))
        self.prop, self.value, self.pred = t["property"], t["value"], tuple(t["predictors"])
        cmap, cfgs = src.get("tree_clusters", ([0, 1], [W.CONFIGS[0], W.CONFIGS[1]]))
        self.coder = EntropyCoder(cmap, cfgs)

    def write_tree(self, w):
        W.write_entropy_header(w, 6)  # :36
        pl, pr = self.pred
        # :42 property + 1, :45 the value; then two leaves: :56 predictor, :59 offset 0, :60 mul_log 0, :63 mul_bits 0
        W.write_symbols(w, [self.prop + 1, int(pack_signed(self.value)), 0, pl, 0, 0, 0, 0, pr, 0, 0, 0])
        self.coder.write_header(w)  # :78: (3 + 1) / 2 contexts, the left leaf 0 and the right one 1 (:55)

    def leaf(self, channel_index, stream_index):
        left = (channel_index if self.prop == 0 else stream_index) > self.value  # :126
        return (0, self.pred[0]) if left else (1, self.pred[1])

    def write_stream(self, w, channels, stream_index, header_only=False):
        """ModularStream.java:66-83 and decodeChannels (:191-204): nothing at all for a stream without channels. header_only: the
        global stream whose channels are larger than a group, which decodeChannels(reader, true) leaves to the pass groups (:196-197)"""
        if not channels:
            return
        w.bool(True)  # :78 the global tree
        w.bool(True)  # WPParams.java:18 default
        w.u32(0, (0, 0), (1, 0), (2, 4), (18, 8))  # :80 no transforms
        if header_only:
            return
        ci = 0
        for a in channels:
            a = np.asarray(a, I64)
            if a.size == 0:  # :198-199
                continue
            ctx, k = self.leaf(ci, stream_index)
            pred = W.weighted_predictions(a) if k == 6 else W.predict(a, k)
            r = pack_signed(a - pred).reshape(-1)  # ModularChannel.java:344-346: multiplier 1, offset 0
            self.coder.write(w, np.full(r.shape, ctx), r)
            ci += 1


DEFAULT_BLOCK_CLUSTERS = (0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6, 6, 6, 7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14,
                          7, 8, 9, 9, 10, 11, 12, 13, 14, 14, 14, 14, 14)  # HFBlockContext.java:21-25


def block_ctx_of(src):
    """(cluster map, clusters, qf thresholds, lf thresholds) as HFBlockContext.java:18-57 leaves them"""
    b = src.get("block_ctx")
    if b is None:
        return list(DEFAULT_BLOCK_CLUSTERS), 15, [], [[], [], []]
    return list(b["cluster_map"]), max(b["cluster_map"]) + 1, list(b["qf_thresholds"]), [list(t) for t in b["lf_thresholds"]]


def write_lf_global(w, src, mod, variant=None):
    """LFGlobal.java:30-98"""
    def patches():
        if src.get("patches"):  # :34-43; Patch.readPatch takes the image's alpha channels (:39)
            W.write_patches(w, src["patches"], len(src.get("extra", [])), src.get("patch_clusters"), variant)

    def splines():
        if src.get("splines"):  # :46-49
            W.write_splines(w, src["splines"], variant)

    def noise():
        for v in src.get("noise") or []:
            w.bits(v, 10)  # :53-58 eight values of ten bits, in front of the LF dequant fields
    order = [patches, splines] + ([noise] if variant != "noise_lut_after_lf_dequant" else [])  # :34-61
    if variant == "splines_before_patches":
        order = [splines, patches, noise]
    elif variant == "noise_before_splines":
        order = [patches, noise, splines]
    for field in order:
        field()
    lfd = src.get("lf_dequant")
    w.bool(lfd is None)  # :62
    if lfd is not None:
        for v in lfd:
            w.f16(v)  # :64
    if variant == "noise_lut_after_lf_dequant":
        noise()
    w.u32(src["global_scale"], (1, 11), (2049, 11), (4097, 12), (8193, 16))  # :68
    w.u32(src["quant_lf"], (16, 0), (1, 5), (1, 8), (1, 16))  # :69
    b = src.get("block_ctx")
    w.bool(b is None)  # HFBlockContext.java:19
    if b is not None:
        size = 39 * (len(b["qf_thresholds"]) + 1)
        for i in range(3):
            w.bits(len(b["lf_thresholds"][i]), 4)  # :35
            size *= len(b["lf_thresholds"][i]) + 1
            for t in b["lf_thresholds"][i]:
                w.u32(int(pack_signed(t)), (0, 4), (16, 8), (272, 16), (65808, 32))  # :39-40
        w.bits(len(b["qf_thresholds"]), 4)  # :44
        for t in b["qf_thresholds"]:
            w.u32(t - 1, (0, 2), (4, 3), (12, 5), (44, 8))  # :48
        cmap = list(b["cluster_map"])
        assert len(cmap) == size <= 39 * 64  # :49-53
        nbits = max(cmap).bit_length()
        assert nbits <= 3
        w.bool(True)  # EntropyStream.java:49 simple clustering
        w.bits(nbits, 2)
        for v in cmap:
            w.bits(v, nbits)
    c = src.get("corr")
    w.bool(c is None)  # LFChannelCorrelation.java:32
    if c is not None:
        w.u32(c["colour_factor"], (84, 0), (256, 0), (2, 8), (258, 16))  # :34
        w.f16(c["base_x"])  # :35-36
        w.f16(c["base_b"])
        w.bits(c["x_factor_lf"], 8)  # :37-38
        w.bits(c["b_factor_lf"], 8)
    w.bool(True)  # LFGlobal.java:82 a global tree
    mod.write_tree(w)
    # :96-97 the global Modular stream of a VarDCT frame holds the extra channels, each of the frame's size (ModularStream.java:86-90);
    # without them it has no channel and :71-76 reads nothing
    mod.write_stream(w, [e["plane"] for e in src.get("extra", [])], 0, header_only=extras_in_groups(src))


def place_blocks(blocks, ch, cw, taken=None):
    """HFMetadata.placeBlock (HFMetadata.java:93-119) run on the types in the order given: the positions the reader will find.
    taken: a dict that counts the two branches -- "too_wide" (:100-101) and "occupied" (:103-108) by a block other than the last"""
    sel = -np.ones((ch, cw), I64)
    out, ly, lx = [], 0, 0
    taken = {} if taken is None else taken
    for _, _, t in blocks:
        bh, bw = cells(t)
        y, x, pos = ly, lx, None
        while y < ch and pos is None:
            while x < cw:
                if bw + x > cw:  # :100-101
                    taken["too_wide"] = taken.get("too_wide", 0) + 1
                    break
                occ = [ix for ix in range(bw) if sel[y, x + ix] >= 0]
                if occ:  # :103-108
                    if (y, x + occ[0]) != (ly, lx) and not (ly <= y < ly + cells(int(sel[ly, lx]))[0] and sel[y, x + occ[0]] == sel[ly, lx]
                                                          and lx <= x + occ[0] < lx + cells(int(sel[ly, lx]))[1]):
                        taken["occupied"] = taken.get("occupied", 0) + 1
                    x += cells(int(sel[y, x + occ[0]]))[1] - 1 + 1
                    continue
                pos = (y, x)
                break
            if pos is None:
                y, x = y + 1, 0
        assert pos is not None, "Could not find place for block"
        sel[pos[0]:pos[0] + bh, pos[1]:pos[1] + bw] = t
        out.append(pos)
        ly, lx = pos
    return out


def lf_index(src, g, y, x, variant=None):
    """LFCoefficients.getLFIndex (LFCoefficients.java:182-202); 0 in a frame that uses an LF frame: lfIndex is allocated (:24) and the
    constructor returns (:56) before populateLFIndex (:102)"""
    if src.get("use_lf_frame", False) and variant != "lf_index_from_thresholds_in_a_use_lf_frame_group":
        return 0
    thr = block_ctx_of(src)[3]
    sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
    idx = [sum(int(g["lf_quant"][i][y >> sy[i], x >> sx[i]]) > t for t in thr[i]) for i in range(3)]
    return (idx[0] * (len(thr[2]) + 1) + idx[2]) * (len(thr[1]) + 1) + idx[1]


def write_lf_group(w, src, mod, index, geo, variant=None):
    """LFGroup.java:25-49: LFCoefficients.java:59-62, the frame's Modular channels of this group (none), HFMetadata.java:23-35"""
    g = src["lfgroups"][index]
    ch, cw = np.asarray(g["hf_mul"]).shape
    # LFCoefficients.java:44-57: a frame that uses an LF frame copies its LF out of lfBuffer and returns before :59-60
    if not src.get("use_lf_frame", False) or variant == "lf_stream_in_a_use_lf_frame_group":
        w.bits(g.get("extra_precision", 0), 2)  # LFCoefficients.java:59
        q = [np.asarray(a, I64) for a in g["lf_quant"]]
        sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
        for c in range(3):
            assert q[c].shape == (ch >> sy[c], cw >> sx[c])  # :37-40
        order = (0, 1, 2) if variant == "lf_buffer_order" else C_MAP  # :39: info[cMap[i]] is channel i: the stream holds Y, X, B
        mod.write_stream(w, [q[c] for c in order], 1 + index)  # :60
    # LFGroup.java:36-39: stream 1 + numLFGroups + index has no channel
    blocks = sorted(g["blocks"])  # raster order of the corners: the order placeBlock reproduces for a complete tiling
    assert place_blocks(blocks, ch, cw) == [(y, x) for y, x, _ in blocks]
    w.bits(len(blocks) - 1, ceil_log1p(ch * cw - 1))  # HFMetadata.java:25-26
    hf = np.asarray(g["hf_mul"], I64)
    info = np.array([[t for _, _, t in blocks], [int(hf[y, x]) - 1 for y, x, _ in blocks]], I64)  # :45, :49
    if variant == "block_info_rows_exchanged":
        info = info[::-1]
    th, tw = (ch + 7) // 8, (cw + 7) // 8  # :27-28
    assert np.asarray(g["x_from_y"]).shape == (th, tw) == np.asarray(g["b_from_y"]).shape
    mod.write_stream(w, [g["x_from_y"], g["b_from_y"], info, g["sharpness"]], 1 + 2 * geo["num_lf_groups"] + index)  # :29-35


def write_quant(w, src, mod, geo, variant=None):
    """HFGlobal.java:194-213 and setupDCTParam (:215-302)"""
    quant = src.get("quant")
    w.bool(quant is None)  # :195

    def dct_params(rows):  # readDCTParams (:30-40)
        w.bits(len(rows[0]) - 1, 4)
        for r in rows:
            w.f16(r[0] / 64.0)
            for v in r[1:]:
                w.f16(v)
    for index, q in enumerate(quant or []):
        mode = q["mode"]
        w.bits(mode, 3)  # :216
        if mode in (1, 2, 3):  # :225-250
            for r in q["par"]:
                assert len(r) == {1: 3, 2: 6, 3: 2}[mode]
                for v in r:
                    w.f16(v / 64.0)
            if mode == 3:
                dct_params(q["dct"])
        elif mode == 6:  # :252-254
            dct_params(q["dct"])
        elif mode == 7:  # :255-278
            w.f16(q["denominator"])
            mh, mw = matrix_size(index)
            stream = 1 + 3 * geo["num_lf_groups"] + index  # :265
            if variant == "raw_stream_index_off_by_one":
                stream -= 1
            mod.write_stream(w, [np.asarray(r, I64).reshape(mh, mw) for r in q["par"]], stream)
        elif mode == 4:  # :279-285
            for r in q["par"]:
                w.f16(r[0])
            dct_params(q["dct"])
        elif mode == 5:  # :286-298
            for r in q["par"]:
                for x, v in enumerate(r):
                    w.f16(v / 64.0 if x < 6 else v)
            dct_params(q["dct"])
            dct_params(q["p44"])
        else:
            assert mode == 0  # :222-224
    w.bits(src.get("num_presets", 1) - 1, ceil_log1p(geo["num_groups"] - 1))  # :212


def lehmer(perm, skip):
    """the Lehmer code Frame.readPermutation (Frame.java:195-215) turns back into `perm`, and how many of its entries after
    `skip` have to be written: the rest are zero"""
    perm = [int(v) for v in perm]
    assert sorted(perm) == list(range(len(perm))) and perm[:skip] == list(range(skip))
    rest, code = list(range(len(perm))), []
    for v in perm:
        code.append(rest.index(v))  # :211-212: permutation[i] = temp.remove(lehmer[i])
        rest.pop(code[-1])
    end = max([i + 1 for i, v in enumerate(code) if v] + [skip]) - skip
    return code, end


def write_hf_pass(w, src, p, geo):
    """HFPass.java:71-92"""
    orders = src.get("orders", [{}] * num_passes(src))[p]
    used = sum(1 << b for b in orders)
    if used == 0x5F:  # :72
        w.bits(0, 2)
    elif used == 0x13:
        w.bits(1, 2)
    elif used == 0:
        w.bits(2, 2)
    else:
        w.bits(3, 2)
        w.bits(used, 13)
    if used:
        coder = EntropyCoder(*src["order_clusters"])
        coder.write_header(w)  # :73 eight contexts
        ctx = lambda v: min(7, ceil_log1p(v))  # noqa: E731  Frame.java:196
        ctxs, vals = [], []
        for b in range(13):  # :74-87
            if b not in orders:
                continue
            n = len(natural_order(b))
            for c in range(3):
                code, end = lehmer(orders[b][c], n // 64)  # :80
                ctxs.append(ctx(n))  # Frame.java:197
                vals.append(end)
                for i in range(n // 64, n // 64 + end):  # :201-202
                    ctxs.append(ctx(code[i - 1] if i > n // 64 else 0))
                    vals.append(code[i])
        coder.write(w, ctxs, vals)
    cmap, cfgs = src["hf_clusters"][p]
    assert len(cmap) == 495 * src.get("num_presets", 1) * block_ctx_of(src)[1]  # :90
    EntropyCoder(cmap, cfgs).write_header(w)  # :91


def pass_order(src, p, oid, c):
    """HFPass.order[orderID][c] (:78-85)"""
    nat = natural_order(oid)
    orders = src.get("orders", [{}] * num_passes(src))[p]
    return [nat[i] for i in orders[oid][c]] if oid in orders else nat


COEFF_FREQ_CTX = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 21, 21, 22, 22,
                  23, 23, 23, 23, 24, 24, 24, 24, 25, 25, 25, 25, 26, 26, 26, 26, 27, 27, 27, 27, 28, 28, 28, 28, 29, 29, 29, 29, 30,
                  30, 30, 30)  # HFCoefficients.java:19-26
COEFF_NUM_NONZERO_CTX = (-1, 0, 31, 62, 62, 93, 93, 93, 93, 123, 123, 123, 123) + (152,) * 8 + (180,) * 12 + (206,) * 31  # :28-36
assert len(COEFF_FREQ_CTX) == 64 == len(COEFF_NUM_NONZERO_CTX)


def write_pass_group(w, src, mod, p, group, geo, variant=None):
    """HFCoefficients.java:49-138; then the group's Modular stream (PassGroup.java:77-79): the group's crop of every channel that
    the global stream left undecoded (Pass.java:33-41, Frame.java:327-338), none otherwise"""
    presets = src.get("num_presets", 1)
    preset = src.get("presets", [[0] * geo["num_groups"]] * num_passes(src))[p][group]
    w.bits(preset, ceil_log1p(presets - 1))  # :50-51
    cmap, clusters, qf_thr, lf_thr = block_ctx_of(src)
    n_lf_ctx = (len(lf_thr[0]) + 1) * (len(lf_thr[1]) + 1) * (len(lf_thr[2]) + 1)  # HFBlockContext.java:33-43
    offset = 495 * clusters * preset  # :56
    shift = (list(src.get("pass_shifts", [])) + [0])[p]  # :58, PassesInfo.java:30-32
    sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
    gy, gx = group // geo["cols"], group % geo["cols"]
    lfg = (gy >> 3) * geo["lcols"] + (gx >> 3)  # Frame.java:849-852
    g = src["lfgroups"][lfg]
    pos_y, pos_x = (gy & 7) << 5, (gx & 7) << 5  # :71-73
    lfg_y0, lfg_x0 = (lfg // geo["lcols"]) << 11, (lfg % geo["lcols"]) << 11
    hf = np.asarray(g["hf_mul"], I64)
    nz = np.zeros((3, 32, 32), I64)  # :61
    coeff = [np.asarray(a, I64) for a in src["coeff_passes"][p]]
    ctxs, vals = [], []
    for by, bx, t in sorted(g["blocks"]):  # :75-76 the block list in its order
        gry, grx = by - pos_y, bx - pos_x
        if gry < 0 or grx < 0 or gry >= 32 or grx >= 32:  # :79-82
            continue
        bh, bw = cells(t)
        nb = bh * bw
        oid = order_id(t)
        li = lf_index(src, g, by, bx, variant)  # :87
        for c in C_MAP:  # :89
            sgy, sgx = gry >> sy[c], grx >> sx[c]
            if gry != sgy << sy[c] or grx != sgx << sx[c]:  # :92-95
                continue
            # getPredictedNonZeroes (:257-265)
            if sgx == 0 and sgy == 0:
                predicted = 32
            elif sgx == 0:
                predicted = int(nz[c, sgy - 1, 0])
            elif sgy == 0:
                predicted = int(nz[c, 0, sgx - 1])
            else:
                predicted = int(nz[c, sgy - 1, sgx] + nz[c, sgy, sgx - 1] + (0 if variant == "predicted_rounded_down" else 1)) >> 1
            # getBlockContext (:231-240)
            idx = (c if variant == "block_ctx_channel_not_exchanged" else (1 - c if c < 2 else c)) * 13 + oid
            idx = idx * (len(qf_thr) + 1) + sum(int(hf[by, bx]) > q for q in qf_thr)
            block_ctx = cmap[idx * n_lf_ctx + li]
            # getNonZeroContext (:242-249)
            predicted = min(predicted, 64)
            if predicted < 8:
                nz_ctx = block_ctx + clusters * predicted
            else:
                nz_ctx = block_ctx + clusters * ((0 if variant == "nonzero_ctx_without_4" else 4) + predicted // 2)
            # the coefficients of this block in the pass's order (:111-122): position [k + numBlocks] of the order is sample
            # (flip ? x : y, flip ? y : x) of the block
            order = pass_order(src, p, oid, c)
            fl = flip(t) and not (variant == "vertical_not_flipped" and vertical(t))
            y0 = (((lfg_y0 >> 3) + by) >> sy[c]) << 3  # the block's corner on the channel's plane of the frame
            x0 = (((lfg_x0 >> 3) + bx) >> sx[c]) << 3
            pts = np.array(order[nb:], I64)
            py, px = (pts[:, 1], pts[:, 0]) if fl else (pts[:, 0], pts[:, 1])
            if variant == "vertical_not_flipped" and vertical(t):  # the reader's positions leave the block: mirror back in
                py, px = py % TYPES[t][3], px % TYPES[t][4]
            v = coeff[c][y0 + py, x0 + px]
            if variant == "shift_on_token":  # the magnitude of the packed token divided, not the value
                u = (pack_signed(v << shift).astype(I64) + (1 << shift) - 1) >> shift
            else:
                u = pack_signed(v).astype(I64)  # :122: the reader shifts the unpacked value up
            non_zero = int((u != 0).sum())
            ctxs.append(offset + nz_ctx)  # :100-101
            vals.append(non_zero)
            nz[c, sgy:sgy + bh, sgx:sgx + bw] = (non_zero + nb - 1) // nb  # :103-107
            if non_zero == 0:  # :109-110
                continue
            size = len(order)
            hist = offset + 458 * block_ctx + 37 * clusters  # :113
            last = int(np.nonzero(u)[0][-1])  # :123-126 the reader stops after the last non-zero
            ul = u[:last + 1].tolist()
            left = non_zero
            for k, uk in enumerate(ul):
                if k == 0:  # :116
                    prev = 0 if left > size // 16 else 1
                else:
                    prev = 1 if ul[k - 1] != 0 else 0
                if variant == "prev_inverted":
                    prev = 1 - prev
                # getCoefficientContext(k + numBlocks, nonZero, numBlocks, prev) (:251-255) with the count still to come
                ctxs.append(hist + (COEFF_NUM_NONZERO_CTX[(left + nb - 1) // nb] + COEFF_FREQ_CTX[(k + nb) // nb]) * 2 + prev)
                vals.append(uk)
                if uk != 0:
                    left -= 1
    cm, cfgs = src["hf_clusters"][p]
    EntropyCoder(cm, cfgs).write(w, ctxs, vals)
    if extras_in_groups(src):
        assert num_passes(src) == 1  # Pass.java:22-39: the one pass has minShift 0 <= 0 < maxShift 3 and takes every channel
        crops = []
        for e in src["extra"]:
            a = np.asarray(e["plane"], I64)
            stride = -(-a.shape[1] // GROUP_DIM)  # Frame.java:330-336
            oy, ox = (group // stride) * GROUP_DIM, (group % stride) * GROUP_DIM
            crops.append(a[oy:oy + GROUP_DIM, ox:ox + GROUP_DIM])
        stream = 18 + 3 * geo["num_lf_groups"] + geo["num_groups"] * p + group  # PassGroup.java:77-78
        if variant == "extra_group_stream_index_off_by_one":
            stream += 1
        mod.write_stream(w, crops, stream)


# ---- the frame ---------------------------------------------------------------------------------------------------------------
def write_toc_permutation(w, perm, clusters):
    """Frame.java:155-156 and readPermutation (:195-215) with skip 0: an entropy stream of eight contexts, `end`, then the Lehmer code"""
    coder = EntropyCoder(*clusters)
    coder.write_header(w)  # :155
    ctx = lambda v: min(7, ceil_log1p(v))  # noqa: E731  :196
    code, end = lehmer(perm, 0)
    ctxs, vals = [ctx(len(perm))], [end]  # :197
    for i in range(end):  # :201-202
        ctxs.append(ctx(code[i - 1] if i > 0 else 0))
        vals.append(code[i])
    coder.write(w, ctxs, vals)  # (prefix codes: the final state of :157 is always valid)


def write_frame(src, variant=None):
    """one frame from its header to its last section, a whole number of bytes (Frame.java:124 pads before the next header)"""
    geo = geometry(src)
    mod = Modular(src)
    n_pass = num_passes(src)
    for e in src.get("extra", []):
        assert np.asarray(e["plane"]).shape == (src["height"], src["width"])
    head = BitWriter()
    write_frame_header(head, src, variant)
    sections = []
    single = geo["num_groups"] == 1 and n_pass == 1  # :146-151

    def section():
        if not single or not sections:
            sections.append(BitWriter())
        return sections[-1]
    write_lf_global(section(), src, mod, variant)
    for i in range(geo["num_lf_groups"]):
        write_lf_group(section(), src, mod, i, geo, variant)
    w = section()  # Frame.java:418-423: HfGlobal and every pass's HFPass come from one reader
    write_quant(w, src, mod, geo, variant)
    for p in range(n_pass):
        write_hf_pass(w, src, p, geo)
    for p in range(n_pass):
        for grp in range(geo["num_groups"]):  # :326
            write_pass_group(section(), src, mod, p, grp, geo, variant)
    bodies = [s.tobytes() for s in sections]
    assert len(bodies) == (1 if single else 2 + geo["num_lf_groups"] + geo["num_groups"] * n_pass)
    perm = src.get("permutation")
    head.bool(perm is not None)  # Frame.java:153
    lengths = [len(b) for b in bodies]
    if perm is not None:
        perm = [int(v) for v in perm]
        assert sorted(perm) == list(range(len(bodies)))
        inverse = [perm.index(slot) for slot in range(len(perm))]
        write_toc_permutation(head, inverse if variant == "toc_permutation_inverted" else perm, src["perm_clusters"])
        # :190: section i is read from slot permutation[i] (a single section from slot 0: the permutation is read and not used);
        # :169-174: the lengths are the slots', in the order the slots lie in the stream
        bodies = [bodies[i] for i in inverse]
        if variant != "toc_lengths_in_logical_order":
            lengths = [len(b) for b in bodies]
    head.pad()  # :168
    for n in lengths:
        head.u32(n, (0, 10), (1024, 14), (17408, 22), (4211712, 30))  # :173
    return head.tobytes() + b"".join(bodies)  # :177 padded, then the sections


def image_of(src):
    """the image header's dict (jxl_writer.write_image_header) of a stream whose frames are like this one"""
    ih, iw = image_size(src)
    extra = [dict(type="alpha", bits=e.get("bits", 8), alpha_associated=e.get("alpha_associated", False)) for e in src.get("extra", [])]
    return dict(width=iw, height=ih, bits=8, xyb=src.get("xyb", True), extra=extra, opsin=src.get("opsin"),
                up_weights=src.get("up_weights"), intensity_target=src.get("intensity_target"))


def encode_stream(image, frames, variant=None):
    """one image header (a dict as jxl_writer.write_image_header takes it), then the frames: a SOURCE dict of this module, or a frame
    dict of jxl_writer (one with "planes"). Only the last frame is the last: every other is an LF frame, or has is_last=False.
    A variant reaches the frames of the writer that knows it"""
    assert variant is None or variant in VARIANTS + LF_VARIANTS + FEATURE_VARIANTS + W.VARIANTS
    head = BitWriter()
    W.write_image_header(head, image)  # (padded: ImageHeader.java:309)
    out = [head.tobytes()]
    for i, fr in enumerate(frames):
        modular = "planes" in fr
        level = fr.get("lf_level", 0)
        last = fr.get("is_last", True) and not level and fr.get("type", W.REGULAR) != W.REFERENCE_ONLY
        assert last == (i == len(frames) - 1)
        if modular:
            out.append(W.write_frame(image, fr, variant if variant in W.VARIANTS + FEATURE_VARIANTS + ("crop_bit_in_an_lf_frame_header",) else None))
        else:
            assert image_size(fr) == (image["height"], image["width"]) and fr.get("xyb", True) == image.get("xyb", False)
            out.append(write_frame(fr, variant if variant in VARIANTS + LF_VARIANTS + FEATURE_VARIANTS else None))
    return b"".join(out)


def encode(src, variant=None):
    assert variant is None or variant in VARIANTS + LF_VARIANTS + FEATURE_VARIANTS
    return encode_stream(image_of(src), [src], variant)
