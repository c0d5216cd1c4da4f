/*
 * jxlatte_frontend.h -- C API of the host-side JPEG XL front-end.
 *
 * The reference keeps bitstream parsing on the Java host (container demux, headers, ANS / prefix / LZ77 entropy
 * decoding, MA trees and predictors, TOC, LfGlobal / LfGroup / HfGlobal / pass groups). No JVM exists in this image,
 * so the same job is done by this C++ library: it turns a .jxl file into exactly the tensors that
 * include/jxlatte_amd.h takes (quantised coefficients per pass and group, LF images, varblock maps, modular channel
 * lists + transform descriptors). Inverse Squeeze / RCT of the frame's modular stream are delegated to the caller through
 * jxf_hooks (the device library), and so is its inverse Palette where the caller sets the palette hook: with all three hooks
 * set, this library runs NO transform-stage arithmetic on frame-level data. What stays on the host: the frame-level Palette
 * when that hook is null, a Palette with predictor 6 whose weighted-predictor plane was not kept, and every transform of the
 * per-group sub-streams (LF coefficients, HF metadata, quant tables, modular groups), which are small and sit inside entropy
 * decoding. The VarDCT pipeline is not present here at all. Plain CPU code (g++), no GPU needed.
 */
#ifndef JXLATTE_FRONTEND_H
#define JXLATTE_FRONTEND_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct jxf_dec jxf_dec;

#define JXF_OK 0
#define JXF_END 1              /* no more frames */
#define JXF_ERR_BITSTREAM -2   /* InvalidBitstreamException */
#define JXF_ERR_UNSUPPORTED -3 /* UnsupportedOperationException */
#define JXF_ERR_ARGUMENT -1
#define JXF_ERR_STATE -6

#define JXF_MAX_EXTRA 16

typedef struct jxf_image_info { /* J/bundle/ImageHeader.java */
    int32_t width, height, level, orientation;
    int32_t bits_per_sample, exp_bits, modular_16bit;
    int32_t num_extra, xyb_encoded;
    int32_t colour_space, white_point, primaries, transfer, rendering_intent, use_icc;
    float white_xy[2], prim_xy[6];
    float intensity_target, min_nits, linear_below;
    int32_t relative_to_max_display;
    float opsin_matrix[9], opsin_bias[3], quant_bias[3], quant_bias_numerator;
    int32_t have_animation, have_preview;
    int32_t custom_up[3];
    int32_t ec_type[JXF_MAX_EXTRA], ec_bits[JXF_MAX_EXTRA], ec_exp_bits[JXF_MAX_EXTRA], ec_dim_shift[JXF_MAX_EXTRA],
        ec_alpha_associated[JXF_MAX_EXTRA];
} jxf_image_info;

typedef struct jxf_frame_info { /* J/frame/FrameHeader.java + LFGlobal.java + HFGlobal.numHfPresets */
    int32_t type, encoding, do_ycbcr, upsampling, group_dim, xqm, bqm, lf_level;
    uint64_t flags;
    int32_t jpeg_up_y[3], jpeg_up_x[3];
    int32_t ec_upsampling[JXF_MAX_EXTRA];
    int32_t num_passes, pass_shift[11];
    int32_t x0, y0, width, height, padded_width, padded_height;
    int32_t blend_mode, blend_alpha, blend_clamp, blend_source;
    int32_t ec_blend_mode[JXF_MAX_EXTRA], ec_blend_alpha[JXF_MAX_EXTRA], ec_blend_clamp[JXF_MAX_EXTRA],
        ec_blend_source[JXF_MAX_EXTRA];
    uint32_t duration;
    int32_t is_last, save_as_reference, save_before_ct;
    /* RestorationFilter */
    int32_t gab, epf_iters;
    float gab1[3], gab2[3], epf_sharp_lut[8], epf_channel_scale[3];
    float epf_pass0_sigma, epf_pass2_sigma, epf_border_sad_mul, epf_sigma_modular;
    /* geometry */
    int32_t num_groups, num_lf_groups, group_cols, lf_group_cols;
    /* LfGlobal */
    int32_t num_patches, has_splines, has_noise;
    float noise[8];
    float lf_dequant[3], scaled_dequant[3];
    int32_t global_scale, quant_lf;
    int32_t colour_factor, x_factor_lf, b_factor_lf;
    float base_corr_x, base_corr_b;
    /* HfGlobal */
    int32_t quant_all_default, num_hf_presets;
    /* modular */
    int32_t num_modular_channels;
} jxf_frame_info;

typedef struct jxf_chan {
    int32_t w, h, hshift, vshift;
    int32_t* data; /* h * w, row-major */
} jxf_chan;

typedef struct jxf_squeeze_step { /* same layout as jxl_squeeze_param */
    int32_t horizontal, in_place, begin_c, num_c;
} jxf_squeeze_step;

/* Hooks through which the frame-level modular transforms reach the device library. Return 0 on success.
 * squeeze: in[n_in] = the stream's channel list before the inverse, steps in bitstream order (undone last to first),
 *          out[n_out] = pre-allocated result channels (the list after the inverse). Bind to jxl_modular_apply.
 * rct:     three planes of n samples, updated in place and left in OUTPUT channel order (permutation applied), as
 *          jxl_stage_rct does. */
typedef struct jxf_hooks {
    void* user;
    int32_t (*squeeze)(void* user, const jxf_chan* in, int32_t n_in, const jxf_squeeze_step* steps, int32_t n_steps,
                       jxf_chan* out, int32_t n_out);
    int32_t (*rct)(void* user, int32_t* v0, int32_t* v1, int32_t* v2, int64_t n, int32_t rct_type);
    /* palette: one Palette transform (ModularStream.java:327-378) of the frame-level stream. index = height x width indices,
     *          palette = the stream's channel 0 (pal_h x pal_w; NULL when it is empty), pred = the weighted predictor's
     *          values as decoded (height x width) or NULL, out[num_c] = the result planes (out[0] is index itself). Bind to
     *          jxl_stage_palette. OPTIONAL, unlike the two above: NULL keeps the transform in this library. */
    int32_t (*palette)(void* user, const int32_t* index, int32_t height, int32_t width, const int32_t* palette, int32_t pal_h,
                       int32_t pal_w, const int32_t* pred, int32_t num_c, int32_t nb_colors, int32_t nb_deltas, int32_t d_pred,
                       int32_t bit_depth, int32_t* const* out);
} jxf_hooks;

typedef struct jxf_lfgroup_view { /* one LF group: J/frame/group/LFGroup.java, LFCoefficients (integers), HFMetadata */
    int32_t cells_h, cells_w;
    int32_t extra_precision, has_lf_quant;
    const int32_t* lf_quant[3]; /* X, Y, B buffer order (lfQuant[cMap[i]]) */
    int32_t lf_h[3], lf_w[3];
    int32_t n_blocks;
    const uint8_t* dct_select; /* [cells_h][cells_w] */
    const int32_t* hf_mul;
    const int32_t* sharpness;
    const int32_t* x_from_y; /* [ceil(cells_h/8)][ceil(cells_w/8)] */
    const int32_t* b_from_y;
    const int32_t* block_yx; /* n_blocks x (y, x) */
} jxf_lfgroup_view;

typedef struct jxf_coeff_view { /* HFCoefficients.quantizedCoeffs of one (pass, group), X, Y, B order */
    const int32_t* q[3];
    int32_t h[3], w[3];
} jxf_coeff_view;

/* The same samples as the decode loop produced them (HFCoefficients.java:112-127: one store per decoded symbol, up to the
 * block's last non-zero): the NON-ZERO ones of each channel in decode order, in the sparse wire format of jxlatte_amd.h
 * (jxl_vardct_put_group_sparse). Channel c holds n[c] entries: narrow (one word: value << 16 | y << 8 | x) unless wide[c],
 * then two words (y << 8 | x, value) -- wide when a value of the channel does not fit int16. h, w as in jxf_coeff_view. */
typedef struct jxf_sparse_view {
    const uint32_t* entries[3];
    int32_t n[3], wide[3];
    int32_t h[3], w[3];
} jxf_sparse_view;

typedef struct jxf_quant_view { /* one DCTParams set (HFGlobal.java); arrays are [3][n] flattened */
    int32_t mode;
    float denominator;
    int32_t n_dct, n_par, n_p44;
    const float* dct;
    const float* par;
    const float* p44;
} jxf_quant_view;

typedef struct jxf_patch_view { /* J/frame/features/Patch.java */
    int32_t ref, x0, y0, w, h, n_positions, n_blend; /* n_blend = 1 + extra channels */
    const int32_t* positions;                        /* n_positions x (y, x) */
    const int32_t* blend;                            /* n_positions x n_blend x (mode, alpha, clamp) */
} jxf_patch_view;

typedef struct jxf_spline_view { /* one spline of J/frame/features/spline/SplinesBundle.java */
    int32_t quant_adjust;      /* SplinesBundle.quantAdjust (frame-wide) */
    int32_t n_control;
    const int32_t* control;    /* n_control x (y, x) */
    const int32_t* coeff;      /* [4][32]: X, Y, B, sigma */
} jxf_spline_view;

/* Parses the container (if any) and the image header. data is copied. Returns NULL and fills err on failure. */
jxf_dec* jxf_open(const uint8_t* data, size_t size, char* err, size_t err_len);
void jxf_close(jxf_dec* d);
const char* jxf_last_error(const jxf_dec* d);
int32_t jxf_get_image_info(const jxf_dec* d, jxf_image_info* out);
/* custom upsampling weights of the image header (15 / 55 / 210 floats) when custom_up[k] is set; count returned */
int32_t jxf_get_up_weights(const jxf_dec* d, int32_t k_index, float* out, int32_t cap);

/* Decodes the next frame's bitstream (all sections). JXF_OK, JXF_END, or a negative status. hooks may be NULL: the
 * frame-level modular transforms then FAIL (JXF_ERR_STATE) if the frame needs an inverse Squeeze or RCT -- there is no
 * CPU fallback for the frame-level stream. */
int32_t jxf_next_frame(jxf_dec* d, const jxf_hooks* hooks);
int32_t jxf_get_frame_info(const jxf_dec* d, jxf_frame_info* out);
int32_t jxf_get_lfgroup(const jxf_dec* d, int32_t index, jxf_lfgroup_view* out);
int32_t jxf_get_coeffs(const jxf_dec* d, int32_t pass, int32_t group, jxf_coeff_view* out);
int32_t jxf_get_coeffs_sparse(const jxf_dec* d, int32_t pass, int32_t group, jxf_sparse_view* out);
int32_t jxf_get_quant_params(const jxf_dec* d, int32_t index, jxf_quant_view* out);
int32_t jxf_get_patch(const jxf_dec* d, int32_t index, jxf_patch_view* out);
/* number of splines of the current frame, and one of them */
int32_t jxf_num_splines(const jxf_dec* d);
int32_t jxf_get_spline(const jxf_dec* d, int32_t index, jxf_spline_view* out);
/* channel i of the frame-level modular stream after its inverse transforms -- of the ENCODED channel list, meta channels
 * included, while the transforms are pending (jxf_set_defer_transforms) */
int32_t jxf_get_modular_channel(const jxf_dec* d, int32_t index, jxf_chan* out);

/* ---- deferred frame-level transforms: the caller undoes them itself (on the device, where the result may stay) ----
 * on != 0: frames decoded from now on leave the inverse transforms of the FRAME-LEVEL stream undone; per-group and other
 * sub-streams are untouched. The list is still walked over the channels' shapes at decode time, and a chain the front-end's own
 * loop refuses ("RCT channel range", "RCT must be performed on three equal size channels", "Palette channel range") is refused
 * by jxf_next_frame with the same error. Default off: jxf_next_frame then behaves exactly as before. */
int32_t jxf_set_defer_transforms(jxf_dec* d, int32_t on);
/* ---- LF-only decoding: the frame's LF image and nothing behind it (the 1:8 preview of a VarDCT frame) ----
 * on != 0: of a VarDCT frame decoded from now on jxf_next_frame reads LfGlobal and, of every LF-group section, the LF
 * coefficients only -- no HF metadata, no HfGlobal, no pass group. The frame then needs only the bytes up to the end of its
 * last LF-group section: a missing tail is reported when the NEXT frame is asked for. jxf_get_lfgroup answers lf_quant,
 * extra_precision and the cell sizes with n_blocks == 0 and null block maps; jxf_get_coeffs* answer JXF_ERR_STATE; the
 * HfGlobal fields of jxf_frame_info say nothing about the frame. A frame whose LF-group sections carry modular channels (extra channels at
 * 1:8) is refused with JXF_ERR_UNSUPPORTED. Modular frames ignore the switch. Default off: nothing behaves differently. */
int32_t jxf_set_lf_only(jxf_dec* d, int32_t on);
/* ---- region decoding: only the sections that a box of the frame needs ----
 * The box is in the FRAME's coordinates and is set before jxf_next_frame; w == 0 clears it. Of a VarDCT frame with more than one
 * TOC section jxf_next_frame then reads LfGlobal, HfGlobal with the pass headers, and only
 *   - the pass-group sections of the groups that the box, grown by the margin M and clipped to the padded frame, touches
 *     (padding columns and rows lie in the last real pixel's group), in every pass, and
 *   - the LF-group sections (LF coefficients and HF metadata) of the LF groups that hold those groups.
 * M = (gab ? 1 : 0) + {0, 2, 3, 6}[epf_iters] is how far Gaborish and the edge-preserving filter carry a sample: further than M
 * from an unread group every pixel of a read group is the full decode's. An unselected section is neither opened nor checked
 * against the file's length, so a file that ends inside one decodes; a missing tail is reported when the NEXT frame is asked for.
 * jxf_get_lfgroup / jxf_get_coeffs* of an unselected LF group / group answer JXF_ERR_STATE. Modular frames, single-section
 * frames, frames whose LF-group or pass-group sections carry modular channels, and frames that the box is not inside of, are
 * decoded whole (applied == 0). Together with jxf_set_lf_only: JXF_ERR_STATE from jxf_next_frame. */
int32_t jxf_set_region(jxf_dec* d, int32_t x0, int32_t y0, int32_t w, int32_t h);
typedef struct jxf_region_plan { /* what the current frame did with the box */
    int32_t applied;                                          /* 1: the selection above was made; 0: every section was read */
    int32_t margin;                                           /* M */
    int32_t group_x0, group_y0, group_w, group_h;             /* the groups read, in groups (the whole grid when not applied) */
    int32_t lf_group_x0, lf_group_y0, lf_group_w, lf_group_h; /* the LF groups read, in LF groups */
    int32_t groups_read, groups_total, lf_groups_read, lf_groups_total;
    int64_t section_bytes_read, section_bytes_total;          /* TOC lengths: read (all passes) / of the frame */
} jxf_region_plan;
int32_t jxf_get_region_plan(const jxf_dec* d, jxf_region_plan* out);
/* NOT part of the interface: the tests show with it that a smaller margin is wrong. m = -1: the frame's own M again */
int32_t jxf_debug_set_region_margin(jxf_dec* d, int32_t m);
#define JXF_TRANSFORM_RCT 0
#define JXF_TRANSFORM_PALETTE 1
#define JXF_TRANSFORM_SQUEEZE 2
typedef struct jxf_transform_view { /* J/frame/modular/TransformInfo.java */
    int32_t kind; /* JXF_TRANSFORM_* */
    int32_t begin_c, num_c, rct_type, nb_colors, nb_deltas, d_pred;
    int32_t n_steps;               /* Squeeze: the expanded list the squeeze hook gets (the default plan where none is coded) */
    const jxf_squeeze_step* steps; /* valid until the next jxf_get_transform */
} jxf_transform_view;
/* the current frame's frame-level transform list, in bitstream order (the inverse runs last to first); deferring or not */
int32_t jxf_get_transform_count(const jxf_dec* d);
int32_t jxf_get_transform(const jxf_dec* d, int32_t index, jxf_transform_view* out);
/* 1 while the current frame's transforms are pending */
int32_t jxf_transforms_pending(const jxf_dec* d);
/* channels jxf_get_modular_channel answers for now (equals jxf_frame_info.num_modular_channels) */
int32_t jxf_modular_channel_count(const jxf_dec* d);
/* Runs the pending transforms exactly as jxf_next_frame would have, through the same hooks. Idempotent: a second call, or a
 * call on a frame decoded without deferring, does nothing. Afterwards jxf_get_modular_channel means what it means by default. */
int32_t jxf_apply_transforms(jxf_dec* d, const jxf_hooks* hooks);

#ifdef __cplusplus
}
#endif
#endif
