"""Seeded codestreams of SEVERAL frames for tests/jxl_writer_vardct.encode_stream: LF frames of level 1 and 2 (VarDCT ones, and Modular
ones from jxl_writer.write_frame), VarDCT frames that take their LF from such a frame (USE_LF_FRAME), and frames whose TOC is permuted;
and what a decoder must make of each frame, computed from the SOURCE alone -- never through jxlatte_amd.

The expectation is a chain of the float64 models the project has, each with its magnitude companion A:

  * an LF frame is a frame like any other up to the restoration filters: vardct_ref64's stages on its padded planes (a VarDCT one),
    jxl_writer_lossy_cases.model's cut after the EPF on planes of its own size (a Modular one). What it leaves in
    lfBuffer[lf_level - 1] are those planes, BEFORE the colour transforms (JXLCodestreamDecoder.java:615-619);
  * a frame with USE_LF_FRAME copies, per LF group, the window rows (lfg_y << 8) .., columns (lfg_x << 8) .. of those planes, cast to
    float where they are integers (v * (1f / maxValue)), as its dequantised LF: window() restates LFCoefficients.java:44-57 here. No
    chroma from luma, no smoothing (:56 returns before :77-100). The planes it copies carry the LF frame's error, K_store u (A_lf +
    |lf|), so its own companion is made with A_lf + |lf| in the place of |lf| (the same stages run on that field: every stage's
    companion is its computation on absolute values);
  * a consumer's tail is jxl_writer_vardct_cases.tail_model; the noise seed of the image's first visible frame is (1 << 32) | 0
    whatever LF frames came before it: :618-619 leaves the loop before the counters of :622-627.

`wrong=` selects expectations that are WRONG on purpose (WRONG: the CPU test shows that the bound tells each from a decode).

Sizes: an LF frame of 72 x 40 is 9 x 5, padded to 16 x 8 -- the consumer's 9 x 5 cells are a proper part of the stored planes; 136 x 72
has a level-2 frame of 3 x 2 (one cell) and a level-1 frame of 17 x 9; 2056 x 16 has 257 x 2 cells in LF groups of 256 columns and of
one column. A VarDCT frame has no group_size_shift (FrameHeader.java:121), so 264 x 264 in two passes is the smallest frame with a TOC
of more than a handful of entries: 1 + 1 + 1 + 4 * 2 = 11 (Frame.java:150)."""
import functools

import numpy as np

import jxl_writer as W
import jxl_writer_lossy_cases as LC
import jxl_writer_vardct as V
import jxl_writer_vardct_cases as VC
import pixel_ref64 as P
import vardct_ref64 as M

F, D = np.float32, np.float64
WRONG = ("inverse XYB applied to the stored planes", "planes stored before Gaborish and the EPF", "smoothing applied to the copied LF",
         "chroma from luma applied to the copied LF", "window origin lfg_x << 11", "the consumer's LF read from the level-2 planes",
         "integer planes cast by 1 / 256", "noise seeded as if the LF frame had been a visible frame")
PERM_CLUSTERS = ([0, 1, 2, 3, 0, 1, 2, 3], list(W.CONFIGS[2:6]))  # the TOC permutation's stream: eight contexts, four clusters


# ---- drawing --------------------------------------------------------------------------------------------------------------------
def _lf_frame(seed, width, height, level=1, **kw):
    """a VarDCT LF frame of `level` for an image of width x height"""
    k = 1 << (3 * level)
    return VC.fit(lambda s: VC.draw(s, -(-width // k), -(-height // k), lf_level=level, image_width=width, image_height=height, **kw), seed)


def _consumer(seed, width, height, **kw):
    """a VarDCT frame that uses an LF frame. (draw makes lf_quant all the same: the writer leaves it out, and the one variant that is
    wrong about the LF index reads it. The EPF's conditions are the model's here, not jxl_writer_vardct_cases.conditions': checked
    where the case is modelled)"""
    return VC.draw(seed, width, height, use_lf_frame=True, **kw)


def _block_ctx(seed):
    """non-empty LF thresholds inside the drawn lf_quant's +-60, and a cluster map that tells an LF index of 0 from every other one"""
    rng = np.random.default_rng(seed)
    b = dict(lf_thresholds=[[-10, 12], [0], [-20]], qf_thresholds=[4])
    n_lf = 3 * 2 * 2
    cm = rng.integers(0, 6, 39 * 2 * n_lf)
    cm[:6] = np.arange(6)
    cm = cm.reshape(-1, n_lf)
    cm[:, 1:] = (cm[:, :1] + 1 + rng.integers(0, 5, (cm.shape[0], n_lf - 1))) % 6  # never the cluster of index 0
    b["cluster_map"] = cm.reshape(-1).tolist()
    return b


def _image(width, height, xyb=True):
    return dict(width=width, height=height, bits=8, xyb=xyb, extra=[], opsin=None, up_weights=None, intensity_target=None)


MIXED = (0, 4, 7, 14)  # DCT8, DCT16, DCT8_16, AFV0
# a consumer whose own LF dequantiser is large: scaled_dequant = 65536 * 8 / global_scale is in the hundreds, so the reference's
# adaptive smoothing, run on the copied LF by mistake, would have a gap over 0.75 nearly everywhere and replace the cell by its
# weighted neighbourhood (LFCoefficients.java:141-152, :174); with the usual 1 / 512 it would change nothing and go unseen
LOUD_LF = dict(lf_dequant=[1024.0, 1024.0, 1024.0], quant_lf=1)


def _lf1_vardct(perm=False):
    lf = _lf_frame(8101, 72, 40, gab=True, epf_iters=1, **VC.SMOOTH)
    kw = dict(pass_shifts=[2], amp=40, density=0.2) if perm else {}
    co = _consumer(8102, 72, 40, allowed=MIXED, first=[4, 7, 14, 0], block_ctx=_block_ctx(8103), **LOUD_LF, **kw)
    if perm:
        lf.update(permutation=[0], perm_clusters=PERM_CLUSTERS)  # one section: read and not used (Frame.java:190)
        co.update(permutation=[2, 4, 0, 1, 3], perm_clusters=PERM_CLUSTERS)
    return dict(image=_image(72, 40), frames=[lf, co])


def _lf1_modular_xyb():
    """the shape libjxl's progressive DC has: a Modular XYB LF frame, float planes scaled by lf_dequant, Gaborish and two EPF rounds"""
    rng = np.random.default_rng(8110)
    lf = dict(planes=LC.xyb_planes(rng, 5, 9), type=W.LF_FRAME, lf_level=1, restoration=LC._rf(True, 2, 1.0), lf_dequant=[0.0625, 0.125, 0.75])
    return dict(image=_image(72, 40), frames=[lf, _consumer(8111, 72, 40, allowed=MIXED)])


def _lf2_chain():
    f2 = _lf_frame(8120, 136, 72, level=2, allowed=(0,), gab=False)
    f1 = VC.draw(8121, 17, 9, lf_level=1, use_lf_frame=True, image_width=136, image_height=72, allowed=(0, 1, 3, 12))
    return dict(image=_image(136, 72), frames=[f2, f1, _consumer(8122, 136, 72, allowed=MIXED)])


def _lf1_two_lfgroups():
    lf = _lf_frame(8130, 2056, 16, allowed=(0, 2, 7), density=0.05)
    return dict(image=_image(2056, 16), frames=[lf, _consumer(8131, 2056, 16, allowed=(0, 1, 2, 3, 4, 7, 12, 14), density=0.03)])


def _lf1_int_ycbcr():
    """integer planes Cb, Y, Cr of an 8-bit image that is not XYB: the consumer casts them, v * (1f / 255)"""
    rng = np.random.default_rng(8140)
    lf = dict(planes=LC.int_planes(rng, 5, 9, 8, 3, centred=(0, 1, 2)), type=W.LF_FRAME, lf_level=1, restoration=LC._rf())
    co = _consumer(8141, 72, 40, xyb=False, do_ycbcr=True, allowed=MIXED)
    return dict(image=_image(72, 40, xyb=False), frames=[lf, co])


def _lf1_noise_up():
    """a consumer with noise. Its 25 LF values are the samples of a Modular XYB LF frame without filters, whose Y runs from -0.2 to 2.5
    (integers of -100 .. 1300 at 1 / 512): the noise strength's inputs 3 (Y +- X) lie on both sides of [0, 7) and in between"""
    rng = np.random.default_rng(8150)
    planes = [rng.permutation(np.linspace(-100, 1300, 25).astype(np.int64)).reshape(5, 5), rng.integers(-200, 201, (5, 5)),
              rng.integers(-8, 9, (5, 5))]  # Y, X, B - Y
    lf = dict(planes=planes, type=W.LF_FRAME, lf_level=1, restoration=LC._rf())
    return dict(image=_image(40, 40), frames=[lf, _consumer(8151, 40, 40, noise=list(VC.NOISE_LUT))])


def _toc_perm_1group():
    src = VC.fit(lambda s: VC.draw(s, 40, 40, allowed=VC.SMALL_TYPES), 8160)
    return dict(image=_image(40, 40), frames=[dict(src, permutation=[0], perm_clusters=PERM_CLUSTERS)])


TOC_PERM = (3, 0, 5, 1, 2, 4, 8, 6, 7, 9, 10)  # not its own inverse; the last two stay, so the Lehmer code ends before the size


def _toc_perm_groups():
    src = VC.fit(lambda s: VC.draw(s, 264, 264, allowed=VC.MID_TYPES, pass_shifts=[2], amp=40, density=0.03), 8170)
    return dict(image=_image(264, 264), frames=[dict(src, permutation=list(TOC_PERM), perm_clusters=PERM_CLUSTERS)])


CASES = {
    "lf1_vardct": _lf1_vardct, "lf1_modular_xyb": _lf1_modular_xyb, "lf2_chain": _lf2_chain, "lf1_two_lfgroups": _lf1_two_lfgroups,
    "lf1_int_ycbcr": _lf1_int_ycbcr, "lf1_noise_up": _lf1_noise_up, "toc_perm_1group": _toc_perm_1group,
    "toc_perm_groups": _toc_perm_groups, "toc_perm_lf": functools.partial(_lf1_vardct, perm=True),
}
NAMES = sorted(CASES)
LF_CASES = tuple(n for n in NAMES if n.startswith("lf"))
PERM_CASES = tuple(n for n in NAMES if n.startswith("toc_perm"))
_built, _bytes = {}, {}


def case(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def encoded(name, variant=None):
    if (name, variant) not in _bytes:
        c = case(name)
        _bytes[name, variant] = V.encode_stream(c["image"], c["frames"], variant)
    return _bytes[name, variant]


def unpermuted(name):
    """the bytes' own twin: the same frames with the sections in their logical order"""
    c = case(name)
    return V.encode_stream(c["image"], [{k: v for k, v in fr.items() if k not in ("permutation", "perm_clusters")} for fr in c["frames"]])


# the cases the writer variants are shown on. (A crop bit in the header of an LF frame WITHOUT Gaborish and EPF cannot be seen: every
# bit behind lf_level is 0 up to the byte's end -- no name, no filter, no extensions, no permutation -- so one more 0 is the same
# header; lf2_chain's level-2 frame is such a one, its level-1 frame is not)
VARIANT_CASES = {
    "upsampling_bits_in_a_use_lf_frame_header": ("lf1_vardct", "lf1_int_ycbcr"),
    "lf_stream_in_a_use_lf_frame_group": ("lf1_vardct", "lf1_two_lfgroups"),
    "lf_index_from_thresholds_in_a_use_lf_frame_group": ("lf1_vardct",),
    "crop_bit_in_an_lf_frame_header": ("lf1_vardct", "lf1_modular_xyb", "lf2_chain"),
    "toc_lengths_in_logical_order": ("toc_perm_groups", "toc_perm_lf"),
    "toc_permutation_inverted": ("toc_perm_groups", "toc_perm_lf"),
}


# ---- the expectation ------------------------------------------------------------------------------------------------------------
def is_modular(fr):
    return "planes" in fr


def window(planes, lfg_y, lfg_x, cells_h, cells_w, shift=8, pad=False):
    """LFCoefficients.java:44-57: rows pY .. pY + cells_h, columns pX .. pX + cells_w of every plane, pY = lfg_y << 8, pX = lfg_x << 8.
    The reference's arraycopy throws where the window leaves the plane; pad: a WRONG expectation reads zeros there instead"""
    py, px = lfg_y << shift, lfg_x << shift
    out = []
    for p in planes:
        p = np.asarray(p)
        if pad:
            p = np.pad(p, ((0, max(0, py + cells_h - p.shape[0])), (0, max(0, px + cells_w - p.shape[1]))))
        w = p[py:py + cells_h, px:px + cells_w]
        assert w.shape == (cells_h, cells_w), "the window leaves the stored planes"
        out.append(w)
    return out


def cast_stored(stored, bits, wrong=None):
    """ImageBuffer.castToFloat on the stored planes (LFCoefficients.java:50): integer planes times 1f / maxValue"""
    x, a = stored
    if a is not None:
        return np.asarray(x, D), np.asarray(a, D)
    maxv = F(1 << bits) if wrong == "integer planes cast by 1 / 256" else F((1 << bits) - 1)
    pairs = [P.modular_to_float(p, None, F(1) / maxv) for p in x]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _smoothed(lf, sd):
    """LFCoefficients.adaptiveSmooth (:113-180) on float64 planes: what a consumer's LF is NOT put through"""
    x = np.stack(lf)
    if min(x.shape[1:]) < 3:
        return lf
    w0, w1, w2 = (float(F(v)) for v in P.LF_W)
    ctr = x[:, 1:-1, 1:-1]
    wgt = w0 * ctr + w1 * (x[:, 1:-1, :-2] + x[:, 1:-1, 2:] + x[:, :-2, 1:-1] + x[:, 2:, 1:-1]) + \
        w2 * (x[:, :-2, :-2] + x[:, :-2, 2:] + x[:, 2:, :-2] + x[:, 2:, 2:])
    gap = np.maximum(0.5, (np.abs(ctr - wgt) * np.asarray(sd, D)[:, None, None]).max(axis=0))
    out = x.copy()
    out[:, 1:-1, 1:-1] = (ctr - wgt) * np.maximum(0.0, 3.0 - 4.0 * gap) + wgt
    return [out[0], out[1], out[2]]


def vardct_cuts(src, lf=None, wrong=None):
    """{"idct", "gab", "epf"}: (planes, companion) of one VarDCT frame on its padded planes after each stage set, and "frame": the
    model's frame dict. lf: None (the frame's own LF stream) or (planes, companion) of the stored planes the frame copies its LF from"""
    frame = VC.model_frame(src)
    shadow = None
    if lf is not None:
        p = frame["params"]
        shadow = dict(frame, lfgroups=[dict(g) for g in frame["lfgroups"]])
        frame = dict(frame, lfgroups=[dict(g) for g in frame["lfgroups"]])
        for g, s in zip(frame["lfgroups"], shadow["lfgroups"]):
            ch, cw = np.asarray(g["hf_mul"]).shape
            shift = 11 if wrong == "window origin lfg_x << 11" else 8
            pad = wrong in ("window origin lfg_x << 11", "the consumer's LF read from the level-2 planes")
            g["lf"] = window(lf[0], g["lfg_y"], g["lfg_x"], ch, cw, shift, pad)
            s["lf"] = [a + np.abs(x) for a, x in zip(window(lf[1], g["lfg_y"], g["lfg_x"], ch, cw, shift, pad), g["lf"])]
            if wrong == "smoothing applied to the copied LF":
                g["lf"] = _smoothed(g["lf"], [float(v) for v in p.scaled_dequant])
            if wrong == "chroma from luma applied to the copied LF":  # LFCoefficients.java:81-93
                kx = float(p.base_corr_x) + (p.x_factor_lf - 128.0) / p.color_factor
                kb = float(p.base_corr_b) + (p.b_factor_lf - 128.0) / p.color_factor
                g["lf"] = [g["lf"][0] + kx * g["lf"][1], g["lf"][1], g["lf"][2] + kb * g["lf"][1]]
    inp = M.frame_inputs(frame)
    pp = inp["p"]
    x, a = M.idct_stage(inp)
    if shadow is not None:
        a = M.idct_stage(M.frame_inputs(shadow))[1]
    out = dict(frame=frame, idct=(x, a))
    if pp["gab"]:
        x, a = M.gab(x, a, pp["gab_w1"], pp["gab_w2"])
    out["gab"] = (x, a)
    if pp["epf_iters"] > 0:
        sig = M.epf_sigma(inp["hf_mul"], inp["sharpness"], pp["global_scale_f"], pp["epf_sharp_lut"])
        assert not M.epf_undecided_cells(sig).any(), "an inverse sigma at the EPF's copy threshold"
        x, a = M.epf(x, a, pp["epf_iters"], sig, pp["epf_channel_scale"], pp["epf_pass0_sigma_scale"], pp["epf_pass2_sigma_scale"],
                     pp["epf_border_sad_mul"])
    out["epf"] = (x, a)
    return out


def _models(name, wrong):
    c = case(name)
    im = c["image"]
    stored, out = [None] * 4, []
    for fr in c["frames"]:
        level = fr.get("lf_level", 0)
        if is_modular(fr):
            plain = wrong == "planes stored before Gaborish and the EPF"
            e = dict(stored=LC.model(dict(im, frames=[dict(fr, restoration={}) if plain else fr]))["epf"])
        else:
            lf = None
            if fr.get("use_lf_frame", False):
                src_level = level
                if wrong == "the consumer's LF read from the level-2 planes" and level == 0 and stored[1] is not None:
                    src_level = 1
                assert stored[src_level] is not None, "LF Level too large"
                lf = cast_stored(stored[src_level], im["bits"], wrong)
            e = vardct_cuts(fr, lf, wrong)
            e["stored"] = e["idct"] if wrong == "planes stored before Gaborish and the EPF" else e["epf"]
            if wrong == "inverse XYB applied to the stored planes" and level:
                p = e["frame"]["params"]
                e["stored"] = M.xyb(*e["stored"], p.opsin_matrix, p.opsin_bias, p.cbrt_opsin_bias, float(p.intensity_target))
            if not level:
                seed0 = 2 << 32 if wrong == "noise seeded as if the LF frame had been a visible frame" else VC.NOISE_SEED0
                t = VC.tail_model(fr, model=e["epf"], seed0=seed0)
                e["final"] = (t["x"], t["a"])
                e["tail"] = {k: v for k, v in t.items() if k not in ("x", "a")}
        if level:
            stored[level - 1] = e["stored"]
        out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def models(name, wrong=None):
    """per frame of the case a dict: stored -- (planes, companion | None for integer planes), what an LF frame leaves in lfBuffer, on
    its padded planes; a VarDCT frame also idct / gab / epf, and a frame that is no LF frame final: the cut after the colour transforms"""
    assert wrong is None or wrong in WRONG
    return _models(name, wrong)
