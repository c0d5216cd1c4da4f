/*
 * jxlatte_amd.h -- C-ABI of the MI355X (gfx950) transform back-end for jxlatte.
 *
 * The reference (Traneptora/jxlatte, pure Java) has no FFI; this header is the
 * boundary *cut* at the call sites of its per-frame transform stage
 * (J/ = java/com/traneptora/jxlatte/ in the reference tree):
 *
 *   J/frame/Frame.java:361-374      decodePassGroups VarDCT tail -> PassGroup.invertVarDCT
 *   J/frame/Frame.java:427          globalModular.applyTransforms()
 *   J/frame/Frame.java:430-461      modular->buffer, Gab, EPF
 *   J/JXLCodestreamDecoder.java:637 performColorTransforms (invertXYB)
 *   J/io/PNGWriter.java:65,105-111  transfer (PQ/sRGB) + castToIntWithMax
 *
 * Plain pointers and sizes only. Every function returns a jxl_status
 * (0 = OK, negative = error); no exception crosses the ABI. The two reference
 * exception families map 1:1: InvalidBitstreamException -> JXL_ERR_INVALID_BITSTREAM,
 * UnsupportedOperationException -> JXL_ERR_UNSUPPORTED.
 *
 * Layout everywhere: planar, row-major, 32-bit elements, channel order X,Y,B
 * (buffer index 0,1,2 as in Frame.buffer[]). "cell" = 8x8 px, "tile" = 64x64 px
 * (chroma-from-luma granularity), "group" = 256x256 px, "LF group" = 2048x2048 px.
 */
#ifndef JXLATTE_AMD_H
#define JXLATTE_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t jxl_status;
#define JXL_OK                      0
#define JXL_ERR_INVALID_ARGUMENT  (-1)
#define JXL_ERR_INVALID_BITSTREAM (-2) /* J/io/InvalidBitstreamException.java:5 */
#define JXL_ERR_UNSUPPORTED       (-3) /* UnsupportedOperationException, PassGroup.java:326-327 */
#define JXL_ERR_DEVICE            (-4)
#define JXL_ERR_OOM               (-5)
#define JXL_ERR_STATE             (-6) /* IllegalStateException (call order) */

/* TransformType.type values, J/frame/vardct/TransformType.java:10-36 */
#define JXL_NUM_TRANSFORM_TYPES 27
/* number of quant-weight parameter sets, HFGlobal.weights[17][3][][] (HFGlobal.java:191) */
#define JXL_NUM_WEIGHT_SETS 17

/* output stage selector (PNGWriter ctor: tf = hdr ? PQ : sRGB; bit depth 8/16) */
#define JXL_TRANSFER_NONE 0 /* stop after invertXYB: linear float */
#define JXL_TRANSFER_PQ   1 /* TransferFunction.TF_PQ.fromLinear, TransferFunction.java:83-87 */
#define JXL_TRANSFER_SRGB 2 /* TransferFunction.TF_SRGB.fromLinearF, :39-44. With 8-bit or 16-bit output (max 255 / 65535) transfer and
                            * quantisation go through tables of the composite's thresholds: the ORACLE's integer for every float
                            * input (all 2^32 checked for both). The thresholds are bisected on the host with glibc's pow(), the
                            * oracle's form; Java's Math.pow is a HotSpot intrinsic specified to 1 ulp, so a threshold that sits on
                            * such a disagreement may move one code value against a JVM (unpinned until a JVM runs tests/test_jvm_pin.py).
                            * Float output evaluates the double pow on the device */
/* Tolerance of the PQ entries against the reference's (float)Math.pow(double) form. JXL_TRANSFER_PQ evaluates a table of
 * quadratic segments (jxl_fastpow.h): as FLOAT output over ALL 2^32 inputs 99.96 % identical, the rest off by exactly 1 ulp, none
 * worse (profiles/r3_pq_sweep.txt). With 16-bit output (JXL_OUT_U16 / RGB16, max 65535) the quantised sample is the oracle's
 * integer (glibc pow) for EVERY input (r3: the table value is settled against the composite's 65 535 thresholds, profiles/r3_pq16_sweep.txt);
 * an 8-bit PQ sample likewise (binary search in its 255 thresholds, profiles/r3_pq8_sweep.txt). JXL_TRANSFER_PQ_EXACT evaluates the two
 * pow() in double precision on the device (3x the instructions; the pre-round-2 form). Both are accepted by
 * jxl_vardct_params.transfer and jxl_stage_transfer. */
#define JXL_TRANSFER_PQ_EXACT 3
#define JXL_OUT_F32 0       /* float planes */
#define JXL_OUT_U16 1       /* ImageBuffer.castToIntWithMax(65535), ImageBuffer.java:129-147 */
#define JXL_OUT_U8  2       /* ImageBuffer.castToIntWithMax(255) */
/* row f3: the same quantised samples, pixel-interleaved R,G,B in the order PNGWriter.writeIDAT emits them
 * (PNGWriter.java:191-203); one buffer of height*width*3 elements (out[0]; out[1], out[2] unused). u16 is host order. */
#define JXL_OUT_RGB8  3
#define JXL_OUT_RGB16 4

/* stage mask bits for jxl_vardct_params.stages */
#define JXL_STAGE_IDCT 1u  /* dequant + CfL + LLF + inverse transforms (PassGroup.invertVarDCT) */
#define JXL_STAGE_GAB  2u  /* Frame.performGabConvolution */
#define JXL_STAGE_EPF  4u  /* Frame.performEdgePreservingFilter */
#define JXL_STAGE_XYB  8u  /* OpsinInverseMatrix.invertXYB */
#define JXL_STAGE_OUT 16u  /* transfer + int quantisation */

typedef struct jxl_ctx jxl_ctx;

/* Frame-constant parameters of one VarDCT frame. All float fields are produced by
 * the host exactly as the reference computes them (file:line given per field). */
typedef struct jxl_vardct_params {
    int32_t width;   /* Frame.getPaddedFrameSize().width  (Frame.java:924-941), multiple of 8 */
    int32_t height;  /* Frame.getPaddedFrameSize().height */
    uint32_t stages; /* JXL_STAGE_* mask; gab/epf/xyb bits are ANDed with the flags below */

    /* HFCoefficients.dequantizeHFCoefficients (HFCoefficients.java:267-275) */
    float scale_factor[3];      /* {gs*(float)pow(0.8,xqm-2), gs, gs*(float)pow(0.8,bqm-2)}, gs = 65536f/globalScale */
    float quant_bias[3];        /* OpsinInverseMatrix.quantBias */
    float quant_bias_numerator; /* OpsinInverseMatrix.quantBiasNumerator */

    /* HFCoefficients.chromaFromLuma (:146-192), LFChannelCorrelation */
    float base_corr_x;
    float base_corr_b;
    int32_t color_factor;

    /* RestorationFilter (RestorationFilter.java:12-79) */
    int32_t gab;         /* restorationFilter.gab */
    float gab_w1[3];     /* gab1Weights */
    float gab_w2[3];     /* gab2Weights */
    int32_t epf_iters;   /* epfIterations 0..3 */
    float global_scale_f;    /* 65536f / lfGlobal.globalScale (Frame.java:554) */
    float epf_sharp_lut[8];  /* epfSharpLut, already multiplied by epfQuantMul (:78) */
    float epf_channel_scale[3];
    float epf_pass0_sigma_scale;
    float epf_pass2_sigma_scale;
    float epf_border_sad_mul;

    /* OpsinInverseMatrix (OpsinInverseMatrix.java:105-142) */
    int32_t xyb;             /* matrix != null in performColorTransforms */
    float opsin_matrix[9];   /* adapted matrix (getMatrix), NOT yet scaled by 255/intensityTarget */
    float opsin_bias[3];
    float cbrt_opsin_bias[3];/* (float)Math.cbrt(opsinBias[c]) (:83) */
    float intensity_target;

    int32_t transfer;   /* JXL_TRANSFER_* */
    int32_t out_format; /* JXL_OUT_* */

    /* row a16, JPEG-recompressed frames: FrameHeader.jpegUpsamplingY/X[c] AFTER the header's normalisation
     * (FrameHeader.java:190-195: max - own), i.e. the shift by which channel c (X/Cb, Y, B/Cr buffer order) is smaller
     * than the padded frame. All zero for ordinary frames. With a non-zero shift: put_group planes, lf[] planes and the
     * coefficient positions of channel c are in its own subsampled geometry (PassGroup.java:213-226), chroma-from-luma
     * is skipped (HFCoefficients.java:149-151), and Frame.invertSubsampling (Frame.java:681-723) runs right after the
     * inverse transforms, before Gab / EPF. */
    int32_t jpeg_upsampling_y[3];
    int32_t jpeg_upsampling_x[3];
} jxl_vardct_params;

/* One LF group's side information, in the reference's own per-LF-group shape
 * (HFMetadata.java:16-52, LFCoefficients.dequantLFCoeff). Host pointers. */
typedef struct jxl_lfgroup_desc {
    int32_t lfg_y, lfg_x;       /* Frame.getLFGroupLocation: position in LF-group units */
    int32_t cells_h, cells_w;   /* LFGroup.size in 8x8 cells (<= 256) */
    const uint8_t* dct_select;  /* [cells_h][cells_w] TransformType.type of the covering varblock */
    const int32_t* hf_mul;      /* [cells_h][cells_w] hfMultiplier */
    const int32_t* sharpness;   /* [cells_h][cells_w] hfStreamBuffer[3] */
    const int32_t* x_from_y;    /* [ceil(cells_h/8)][ceil(cells_w/8)] hfStreamBuffer[0] */
    const int32_t* b_from_y;    /* same shape, hfStreamBuffer[1] */
    const int32_t* block_yx;    /* blockList: n_blocks x {y,x} in cells, placement order */
    int32_t n_blocks;
    const float* lf[3];         /* dequantLFCoeff[c] [cells_h][cells_w] */
} jxl_lfgroup_desc;

/* SqueezeParam (J/frame/modular/SqueezeParam.java) */
typedef struct jxl_squeeze_param {
    int32_t horizontal;
    int32_t in_place;
    int32_t begin_c;
    int32_t num_c;
} jxl_squeeze_param;

/* A modular channel plane (ModularChannel.buffer + size). Host pointer. */
typedef struct jxl_channel {
    int32_t width;
    int32_t height;
    int32_t* data; /* [height][width], may be NULL when width*height == 0 */
} jxl_channel;

/* ---- context ------------------------------------------------------------------ */
/* One ctx = one HIP device + one stream + a device arena reused across frames.
 * Single-threaded like a JXLDecoder instance; distinct ctxs are independent. */
jxl_status jxl_ctx_create(int32_t device, jxl_ctx** out);
void       jxl_ctx_destroy(jxl_ctx* ctx);
const char* jxl_last_error(const jxl_ctx* ctx);
const char* jxl_version(void);
jxl_status jxl_ctx_synchronize(jxl_ctx* ctx);
/* HIP stream handle (hipStream_t) the ctx launches on; for event timing by callers. */
void*      jxl_ctx_stream(jxl_ctx* ctx);
/* Launch on a caller-owned HIP stream instead (e.g. several frame contexts sharing one stream, or
 * torch's current stream). The ctx no longer owns a stream after this call.
 *
 * Contexts put on one stream (and the context that owns it, once others have been put on it) share
 * the planes that hold the inverse transforms' output between the two launches of jxl_vardct_run:
 * one set per frame size and stream instead of one per context. The stream serialises their runs,
 * and results are never kept in the shared planes, so outputs are those of private streams. What a
 * caller should know:
 *  - a run that uses the shared planes holds a per-stream mutex while it enqueues its launches
 *    (microseconds), so that threads driving different contexts of one stream do not interleave;
 *  - the inverse transforms' output of such a run is not kept. Nothing could read it before either:
 *    stages are fixed by jxl_vardct_begin_frame, which starts every frame from zeroed planes, so a
 *    frame opened with JXL_STAGE_IDCT clear restores zero planes on any context, shared stream or not;
 *  - stage-masked runs whose result is that output, three EPF iterations, chroma-subsampled frames
 *    and jxl_vardct_run_batch keep private planes;
 *  - the environment variable JXL_SHARED_PLANES=0 (read once per process) gives every context
 *    private planes, as if each had its own stream. */
jxl_status jxl_ctx_set_stream(jxl_ctx* ctx, void* hip_stream);

/* ---- VarDCT frame path: replaces Frame.decodePassGroups tail .. performColorTransforms */
/* call order: begin_frame, set_weights, set_lfgroup* , put_group*, (run | finish_frame) */
jxl_status jxl_vardct_begin_frame(jxl_ctx* ctx, const jxl_vardct_params* params);
/* HFGlobal.weights (already reciprocal, HFGlobal.java:421-431): 17 sets x 3 channels, each
 * matrixHeight x matrixWidth row-major; offs[p*3+c] = element offset of set p channel c in w. */
jxl_status jxl_vardct_set_weights(jxl_ctx* ctx, const float* w, size_t n_floats, const int32_t* offs /*[51]*/);
jxl_status jxl_vardct_set_lfgroup(jxl_ctx* ctx, const jxl_lfgroup_desc* lfg);
/* Row f1 (LF stage on device): instead of lfg->lf[] (already dequantised), hand over the INTEGER LF image of the LF
 * group and let the device run LFCoefficients.java:65-75 (dequant), :78-95 (LF chroma-from-luma) and :113-180
 * (adaptiveSmooth). Call after jxl_vardct_set_lfgroup for the same LF group (its lf[] pointers may then be NULL).
 * lf_quant[i]: lfQuant[cMap[i]] i.e. already in X,Y,B buffer order, [cells_h][cells_w] int32;
 * scaled_dequant = LFGlobal.scaledDequant (X,Y,B); x/b_factor_lf = LFChannelCorrelation.xFactorLF/bFactorLF. */
typedef struct jxl_lfquant_desc {
    int32_t lfg_y, lfg_x;
    int32_t cells_h, cells_w;
    const int32_t* lf_quant[3];
    int32_t extra_precision;     /* reader.readBits(2), LFCoefficients.java:61 */
    float scaled_dequant[3];
    int32_t x_factor_lf, b_factor_lf;
    int32_t adaptive_smoothing;  /* (flags & (SKIP_ADAPTIVE_LF_SMOOTHING | USE_LF_FRAME)) == 0 */
} jxl_lfquant_desc;
jxl_status jxl_vardct_set_lfgroup_lfquant(jxl_ctx* ctx, const jxl_lfquant_desc* d);

/* quantizedCoeffs of one (pass, group) (HFCoefficients.java:43,68): q[c] is [gh][gw] with row
 * stride[c] elements; gh,gw = Frame.getGroupSize(group). pass > 0 accumulates
 * (PassGroup.java:174-200).
 * Buffer lifetime -- NOT "retains nothing after the call" for every source: pageable sources (and page-locked ones that are
 * not 16-byte aligned in address and row stride) are copied before the call returns and may be reused at once. Aligned
 * page-locked sources (jxl_host_alloc, or memory the caller registered) are read by the DEVICE in place, asynchronously, by a
 * kernel queued on the context's stream: keep them unchanged until a call that waits for that stream has returned --
 * jxl_vardct_finish_frame / jxl_vardct_read_output / jxl_vardct_read_output_wait of this frame, or jxl_ctx_synchronize
 * (jxl_vardct_run only queues work). A caller that wants the copy semantics with page-locked memory passes a pointer that is
 * not 16-byte aligned, or copies itself. The JNI shim's callers (integration/jni/GpuFrameBridge.java) hand over fresh pageable
 * direct ByteBuffers: always the copying path. The call itself never waits for the device except when more than 8 puts are
 * still in flight. */
jxl_status jxl_vardct_put_group(jxl_ctx* ctx, int32_t pass, int32_t group,
                                const int32_t* const q[3], const int32_t stride[3]);
/* The same with 16-bit samples -- the wire format for the PCIe leg: quantised HF coefficients of photographic content fit
 * int16 (|q| < 32768; the Java host checks while it fills the buffer and falls back to jxl_vardct_put_group for a group that
 * does not), which halves the bytes of the dominant transfer. The device widens into the same int32 planes; everything
 * downstream is identical. */
jxl_status jxl_vardct_put_group_i16(jxl_ctx* ctx, int32_t pass, int32_t group,
                                    const int16_t* const q[3], const int32_t stride[3]);
/* The whole frame's coefficients in ONE page-locked buffer the library owns: the entropy decoder writes its groups in place
 * (planes[c] is [H >> sy][W >> sx] int16 with row stride strides[c]; group g occupies the rectangle Frame.getGroupLocation /
 * getGroupSize give it, HFCoefficients.java:64-69) and jxl_vardct_commit_coeffs_i16 moves the three planes with three DMA
 * transfers instead of three per group (405 per 4K frame: their fixed cost, not their bytes, is what the per-group entry
 * pays). map zero-fills the planes (the reference's `new int[..]`, HFCoefficients.java:68: only non-zero coefficients are
 * ever written) and is valid until the next begin_frame; commit is asynchronous (jxl_vardct_run is ordered behind it) and
 * may be followed by jxl_vardct_put_group for groups whose samples did not fit 16 bits, or for later passes. */
jxl_status jxl_vardct_map_coeffs_i16(jxl_ctx* ctx, int16_t* planes[3], int32_t strides[3]);
/* Rows of the three mapped planes ((paddedHeight >> jpegUpsamplingY[c]), HFCoefficients.java:64-69): plane c holds
 * rows[c] * strides[c] samples. The JNI shim sizes its direct ByteBuffers from this, never from a caller-supplied count. */
jxl_status jxl_vardct_coeff_plane_rows(jxl_ctx* ctx, int32_t rows[3]);
/* Geometry of the open frame, for callers that must size buffers from the library's own numbers (the JNI shim checks every
 * direct buffer it is handed against these): info[0..2] = plane width of channel c (paddedWidth >> jpegUpsamplingX[c]),
 * info[3..5] = plane height, info[6..7] = the two shifts (x, y) of channel 0, [8..9] of channel 1, [10..11] of channel 2,
 * info[12] = bytes per output sample. Group g of a frame covers Frame.getGroupLocation / getGroupSize (J/frame/Frame.java:767-786):
 * jxl_vardct_group_size gives its width and height per channel. */
jxl_status jxl_vardct_geometry(jxl_ctx* ctx, int32_t info[13]);
/* Geometry of the OUTPUT of the open frame (valid from begin_frame on; what jxl_vardct_read_output* / finish_frame write): info[0],
 * info[1] = width and height of every output plane -- always the full padded frame, also for chroma-subsampled frames (the planes of
 * jxl_vardct_geometry are the COEFFICIENT planes) --, info[2] = bytes per sample, info[3] = 1 if the three colours are interleaved
 * into out[0] (JXL_OUT_RGB8 / JXL_OUT_RGB16: rows of 3 * width samples; out[1], out[2] are ignored), info[4] = number of buffers
 * that must be non-null (1 or 3). A buffer with row stride `s` pixels (>= width) holds
 *     info[2] * (info[3] ? 3 : 1) * ((info[1] - 1) * s + info[0])   bytes.
 * Stands for the sizes the reference states implicitly: Frame.buffer[c] = new float[paddedHeight][paddedWidth]
 * (J/frame/Frame.java:331-340) and PNGWriter's interleaved rows (J/io/PNGWriter.java:191-212). */
jxl_status jxl_vardct_output_geometry(jxl_ctx* ctx, int32_t info[5]);
jxl_status jxl_vardct_group_size(jxl_ctx* ctx, int32_t group, int32_t gw[3], int32_t gh[3]);
jxl_status jxl_vardct_commit_coeffs_i16(jxl_ctx* ctx);
/* The same pair without the zero-fill (r4): a decoder writes EVERY sample of every group it decodes (HFCoefficients.java:76-138
 * leaves the untouched samples of its fresh int[][] at zero -- the caller of this form stores those zeros itself, or keeps its
 * own cleared scratch and copies whole groups), so map's 50 MB of host stores per 4K frame are wasted on it. With
 * JXL_MAP_NO_FILL the planes come back as they are; commit_..._groups names the groups whose rectangles the caller has fully
 * written (group_written[g] != 0, g in Frame group order, n_groups = all groups of the frame); every other group reads as zero
 * (its rectangle is cleared in the staging buffer before the transfer). map also no longer waits for the context's whole
 * stream, only for the previous commit's transfers to have read the buffer. */
#define JXL_MAP_NO_FILL 1
jxl_status jxl_vardct_map_coeffs_i16_ex(jxl_ctx* ctx, int16_t* planes[3], int32_t strides[3], int32_t flags);
jxl_status jxl_vardct_commit_coeffs_i16_groups(jxl_ctx* ctx, const uint8_t* group_written, int32_t n_groups);
/* ---- sparse coefficient feed: only the non-zero coefficients cross the bus -------------------------------------------------
 * HFCoefficients' decode loop makes one store per decoded symbol and stops at a block's last non-zero
 * (HFCoefficients.java:112-127): a list of (position, value) pairs is what the host has in hand before it scatters them into
 * a cleared int[][] (:68). These entries take that list as it is. An ENTRY names one sample of one (group, channel) in that
 * channel's own geometry (jxl_vardct_group_size; shifted for chroma-subsampled frames, PassGroup.java:213-226):
 *     pos = (y << 8) | x,   y < gh[c], x < gw[c]
 * narrow entry: one uint32_t, pos in the low 16 bits, the value as int16 in the high 16 bits;
 * wide entry (JXL_SPARSE_WIDE, per call or per run): two uint32_t, pos (its high 16 bits zero), then the value as int32 --
 * the part jxl_vardct_put_group plays for the int16 entries.
 * An entry whose value is 0 changes nothing. The device takes the first `count` entries of a list and reads nothing behind
 * them: what pads a list to the next 16-byte boundary is never interpreted (zero entries, as callers usually write, are
 * fine). Positions inside one call or one run are distinct (the reference's coefficient order is a permutation,
 * HFCoefficients.java:112-127); with duplicates the sample receives the SUM of their values (Java int wrap), the same on every
 * run. An entry whose position lies outside the group's rectangle is never stored anywhere. */
#define JXL_SPARSE_WIDE 1
/* One group, like jxl_vardct_put_group_i16 (quantizedCoeffs of one (pass, group), HFCoefficients.java:43,68): pass 0 REPLACES the
 * group's rectangle (a fresh zeroed int[][] plus the entries), pass > 0 adds (PassGroup.java:174-200, Java int wrap).
 * entries[c]: n_entries[c] entries of channel c (n_entries[c] == 0 is legal, entries[c] may then be NULL). Buffer rules as for
 * jxl_vardct_put_group: page-locked, 16-byte aligned lists are read by the device in place, asynchronously (keep them until a
 * call that waits for the stream has returned); anything else is copied through the staging ring before the call returns. On
 * the copying path an entry outside the rectangle is JXL_ERR_INVALID_ARGUMENT and nothing is queued; on the in-place path the
 * device refuses such entries and counts them (jxl_vardct_sparse_rejected). */
jxl_status jxl_vardct_put_group_sparse(jxl_ctx* ctx, int32_t pass, int32_t group,
                                       const uint32_t* const entries[3], const int32_t n_entries[3], int32_t flags);
/* The whole frame from ONE page-locked buffer the library owns: the sparse sibling of jxl_vardct_map_coeffs_i16 / commit. The
 * entropy decoder appends the entries of each (group, channel) as a RUN: `count` entries starting `offset_words` words into the
 * buffer (a multiple of 4: runs start on 16-byte boundaries), all of one form (flags: 0 or JXL_SPARSE_WIDE).
 * map: `words` has room for capacity_words uint32_t and is valid until the next begin_frame; a larger capacity than any
 * before reallocates (the earlier contents are not kept). It waits only for the previous commits' reads of the buffer.
 * commit ADDS the runs' entries into the planes as they stand: on a fresh frame they are zero (HFCoefficients.java:68), so
 * groups no run names read as zero; a second commit is a later pass (PassGroup.java:174-200). Asynchronous (jxl_vardct_run is
 * ordered behind it); may be mixed with jxl_vardct_put_group* afterwards. One scatter launch per 2048 non-empty runs, however
 * many groups they name. Every run is checked before anything is queued (group, channel, flags, alignment, extent within
 * capacity_words): JXL_ERR_INVALID_ARGUMENT leaves no work in flight. JXL_ERR_STATE before map_sparse in this frame. */
typedef struct jxl_sparse_run { int32_t group, channel, flags, count; int64_t offset_words; } jxl_sparse_run;
jxl_status jxl_vardct_map_sparse(jxl_ctx* ctx, size_t capacity_words, uint32_t** words);
jxl_status jxl_vardct_commit_sparse(jxl_ctx* ctx, const jxl_sparse_run* runs, int32_t n_runs);
/* Entries the device refused (position outside the group's rectangle) since begin_frame -- the guard the reference gets from
 * Java's array bounds check (HFCoefficients.java:125 would throw ArrayIndexOutOfBoundsException). Waits for the context's stream. */
jxl_status jxl_vardct_sparse_rejected(jxl_ctx* ctx, int64_t* n);
/* Page-locked host memory for the buffers that cross the bus (coefficient planes in, pixel planes out; a JNI caller wraps it
 * with NewDirectByteBuffer). put_group / put_group_i16 / read_output recognise such pointers: the device reads / writes them
 * in place at bus speed instead of through a staged copy out of pageable memory, and put_group returns without waiting
 * (the buffer must stay untouched until jxl_vardct_run or jxl_ctx_synchronize). NULL on failure. */
void* jxl_host_alloc(size_t bytes);
void jxl_host_free(void* p);
/* Host-side preparation a run needs and would otherwise do on first use: varblock binning by transform type
 * (the device counterpart of walking HFMetadata.blockList, HFCoefficients.java:76-85), the chroma-from-luma
 * cache-order masks (HFCoefficients.java:159-181), upload of the side tables, LF dequantisation jobs. Synchronous.
 * Idempotent until the frame's inputs change; jxl_vardct_run calls it implicitly. bench.py times it as
 * `host_prepare_ms`.
 * Deliberate refusal (JXL_ERR_UNSUPPORTED): a varblock with a 128- or 256-sample edge in a CHROMA-SUBSAMPLED frame. The
 * reference transforms every channel's copy of such a block at the channel's own geometry (PassGroup.java:203-233,
 * TransformType.java:10-36), where the copies of neighbouring blocks overlap in the subsampled planes and the later one
 * overwrites the earlier: its output depends on its visiting order, no encoder emits such frames (libjxl's only subsampled
 * frames are JPEG recompressions, DCT8 throughout), and a device that transforms blocks concurrently has no such order to
 * reproduce. Frames without subsampling take these blocks through the three-launch path of k_idct.hip (dequantise, column
 * pass, row pass through a scratch plane). */
jxl_status jxl_vardct_prepare(jxl_ctx* ctx);
/* Launch every enabled stage on the ctx stream; inputs are resident after put_group.
 * Asynchronous: returns after enqueue. Re-runnable (inputs are not consumed). */
jxl_status jxl_vardct_run(jxl_ctx* ctx);
/* Run n independent frames (one context each, all on one device; every context prepared exactly as for jxl_vardct_run).
 * The reference decodes its frames one after the other (JXLCodestreamDecoder.decode, :506-720); this entry is what a
 * batched caller (BASELINE config 5: 8 frames per GPU) uses instead of n jxl_vardct_run calls: the inverse-transform stage
 * of all frames is enqueued as one launch per kernel class, the remaining stages per frame on the frames' own streams.
 * Same results, same completion rule (synchronise / read each context as usual). Frames the shared launches do not cover
 * are run one by one. Measured on MI355X: the faster form for small, launch-bound frames (8 x 1280x720: +16 %, 8 x 512x512:
 * +40..70 %); for 4K frames n jxl_vardct_run calls on n contexts are 5 % faster. */
jxl_status jxl_vardct_run_batch(jxl_ctx* const* ctxs, int32_t n);
/* run + synchronize + copy result planes to the host. out[c]: width*height elements of
 * float (JXL_OUT_F32) / uint16 / uint8, row stride = out_stride elements. */
jxl_status jxl_vardct_finish_frame(jxl_ctx* ctx, void* const out[3], int64_t out_stride);
/* copy the last run's result planes (device) to host without re-running */
jxl_status jxl_vardct_read_output(jxl_ctx* ctx, void* const out[3], int64_t out_stride);
/* read_output in two halves (r4): _begin queues the device-to-host copies behind the frame's kernels and returns, _wait blocks
 * until they have landed. In between the host may drive the NEXT frame of this context (begin_frame ... commit ... run: its
 * device work queues behind the copies), which is how one context overlaps the host's share of frame n+1 with the device's share
 * of frame n -- what the reference's one-frame-at-a-time loop (JXLCodestreamDecoder.decode, :506-720) leaves on the table. The
 * destination must stay valid until _wait and should be page-locked (jxl_host_alloc): a page-locked, 16-byte aligned destination
 * with dense rows is written by a kernel through its device alias (r5: no runtime copy call -- with several contexts streaming
 * frames each hipMemcpyAsync held its caller for 1.6-2.5 ms), anything else goes through the runtime's copy. A host that runs
 * several decoder contexts should start with GPU_MAX_HW_QUEUES=16 in its environment (the runtime's default of 4 hardware
 * queues makes one context's launches wait behind the others' bus transfers). */
jxl_status jxl_vardct_read_output_begin(jxl_ctx* ctx, void* const out[3], int64_t out_stride);
jxl_status jxl_vardct_read_output_wait(jxl_ctx* ctx);
/* ---- the frame's colour planes kept on the device between the stages that follow decodeFrame --------------------------
 * JXLCodestreamDecoder.decode runs, on the frame's own buffers and in this order (JXLCodestreamDecoder.java:628-637):
 * Frame.upsample, Frame.initializeNoise, computePatches, Frame.renderSplines, Frame.synthesizeNoise,
 * performColorTransforms. The jxl_stage_* entries take and return host planes; these entries run the same kernels on a set
 * of three float planes that STAYS in device memory, so a frame with upsampling / noise costs one transfer in (its
 * coefficients) and one out (its pixels). Splines may stay on the device too (jxl_planes_splines), and so may the patches
 * (jxl_planes_patches: the reference frames stay host arrays and are uploaded for the frame that reads them). A host that
 * applies the patches itself brackets them with jxl_planes_download / jxl_planes_upload, only for frames that have them. */
/* adopt the top-left height x width window (Frame bounds; the restoration filters worked on the padded size) of the last
 * jxl_vardct_run's result as the resident planes. The run must have produced float planes (no transfer / integer output;
 * XYB stage off if the later stages need XYB samples). */
jxl_status jxl_planes_from_frame(jxl_ctx* ctx, int32_t height, int32_t width);
/* the same for ANY window of the result: rows [y0, y0 + height), columns [x0, x0 + width), which must lie inside it
 * (JXL_ERR_INVALID_ARGUMENT otherwise). jxl_planes_from_frame is the (0, 0) case. A region decode runs a sub-frame of whole LF
 * groups and adopts the region's box with this. */
jxl_status jxl_planes_from_frame_at(jxl_ctx* ctx, int32_t y0, int32_t x0, int32_t height, int32_t width);
/* Frame.performUpsampling (Frame.java:217-260) of the three planes, k = 2, 4, 8; weights as for jxl_stage_upsample */
jxl_status jxl_planes_upsample(jxl_ctx* ctx, int32_t k, const float* weights);
/* Frame.initializeNoise (Frame.java:748-788) + Frame.synthesizeNoise (:790-831) on the resident planes */
jxl_status jxl_planes_noise(jxl_ctx* ctx, int32_t group_dim, uint64_t seed0, const float lut[8], float base_corr_x, float base_corr_b);
/* ---- noise on a window of a frame ----
 * The resident planes are the window [y0, y0 + rp_h) x [x0, x0 + rp_w) of a frame_h x frame_w frame (rp_h x rp_w: their size).
 * The result is Frame.initializeNoise + synthesizeNoise of the WHOLE frame restricted to the window, bit for bit: XorShiro runs
 * for exactly the groups that the window, grown by 2 and clipped to the frame, touches, seeded with their absolute origin and
 * advanced through all three channels in the reference's order; the 5x5 high-pass mirrors against the frame's size. Two
 * launches. JXL_ERR_INVALID_ARGUMENT where the window is not inside the frame, group_dim is not a power of two >= 16 or the frame
 * has more than 2^30 pixels; JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_noise_at(jxl_ctx* ctx, int32_t group_dim, uint64_t seed0, const float lut[8], float base_corr_x, float base_corr_b,
                               int32_t frame_h, int32_t frame_w, int32_t y0, int32_t x0);
/* the same on three host planes of height x width floats (X, Y, B), in place; the resident planes are left alone */
jxl_status jxl_stage_noise_window(jxl_ctx* ctx, float* const planes[3], int32_t height, int32_t width, int32_t group_dim, uint64_t seed0,
                                  const float lut[8], float base_corr_x, float base_corr_b, int32_t frame_h, int32_t frame_w, int32_t y0,
                                  int32_t x0);
/* OpsinInverseMatrix.invertXYB / the YCbCr branch of performColorTransforms on the resident planes */
jxl_status jxl_planes_xyb(jxl_ctx* ctx, const float matrix[9], const float opsin_bias[3], const float cbrt_opsin_bias[3],
                          float intensity_target);
jxl_status jxl_planes_ycbcr(jxl_ctx* ctx);
/* ---- the LF image as the picture at 1:8 (JXLDecoder(downsample=8)) ----------------------------------------------------------
 * A VarDCT frame's LF image is the frame at one sample per 8x8 cell. This turns the INTEGER LF images of ALL the frame's LF
 * groups into three float planes of cells_h x cells_w samples in ONE launch behind ONE transfer: per LF group the LF stage of
 * jxl_vardct_set_lfgroup_lfquant / jxl_stage_lf_dequant (LFCoefficients.java:65-75 dequant, :78-95 LF chroma-from-luma,
 * :113-180 adaptiveSmooth -- per LF group: its border cells are copied, nothing is smoothed across a seam), then, with xyb != 0,
 * OpsinInverseMatrix.invertXYB as jxl_planes_xyb runs it. No HF coefficient is involved: this is a 1:8 preview (the full decode
 * box-averaged 8x8 up to the restoration filters and the LLF of large varblocks), not the reference's pixels.
 * groups: the frame's LF groups in any order, each at its (lfg_y, lfg_x) with all three planes cells_h x cells_w; LF group
 * (gy, gx) must be min(256, cells - 256 g) cells in each axis, and every position of the ceil(cells_h / 256) x
 * ceil(cells_w / 256) grid must occur exactly once. */
typedef struct jxl_lf_image_desc {
    int32_t n_groups;
    int32_t cells_h, cells_w;       /* the output: ceil(frame_h / 8) x ceil(frame_w / 8) */
    int32_t color_factor;           /* LFChannelCorrelation.colorFactor, != 0 */
    const jxl_lfquant_desc* groups; /* [n_groups] */
    float base_corr_x, base_corr_b;
    int32_t xyb;                    /* != 0: the inverse XYB follows, with the four fields below as jxl_planes_xyb takes them */
    float opsin_matrix[9], opsin_bias[3], cbrt_opsin_bias[3], intensity_target;
} jxl_lf_image_desc;
/* the planes become the context's resident planes (cells_h x cells_w): jxl_planes_ycbcr, jxl_planes_orient, the writers and the
 * tensor entries of the resident planes follow as after jxl_planes_from_frame. Nothing comes down. */
jxl_status jxl_planes_from_lf(jxl_ctx* ctx, const jxl_lf_image_desc* d);
/* the same launch into three host planes of cells_h x cells_w floats; the resident planes are left alone */
jxl_status jxl_stage_lf_image(jxl_ctx* ctx, const jxl_lf_image_desc* d, float* const out[3]);
/* ---- splines: Frame.renderSplines (J/frame/Frame.java:739-746) + Spline.renderSpline (J/frame/features/spline/Spline.java:27-200) ----
 * The splines of one frame as SplinesBundle.java:22-73 decodes them, plus the two LFChannelCorrelation factors computeCoeffs reads
 * (Spline.java:133-152). coeff: per spline 4 rows of 32 -- coeffX, coeffY, coeffB, coeffSigma. */
typedef struct jxl_spline_desc {
    int32_t quant_adjust;        /* SplinesBundle.quantAdjust */
    int32_t n_splines;           /* SplinesBundle.numSplines */
    const int32_t* n_control;    /* [n_splines] control points of each spline (>= 1) */
    const int32_t* control;      /* all splines back to back: (y, x) pairs, Spline.controlPoints */
    const int32_t* coeff;        /* [n_splines][4][32] */
    float base_corr_x, base_corr_b; /* LFChannelCorrelation.baseCorrelationX / B */
} jxl_spline_desc;
/* One arc sample of Spline.renderSpline's loop (Spline.java:162-199) that draws: everything of it that does not depend on the
 * pixel. mul[c] = (0.25f * values[c]) * sigma, the per-arc prefix of `0.25f * values[c] * sigma * factor * factor` (:192, left to
 * right); x0..y1 the clamped box of :174-179, inclusive. 48 bytes. */
typedef struct jxl_spline_arc {
    float y, x;                  /* SplineArc.locationY / locationX */
    float sigma, inv_sigma;      /* :170-171 */
    float mul[3];
    int32_t x0, x1, y0, y1;
    int32_t reserved;            /* 0 */
} jxl_spline_arc;
/* Host only, needs no context and no device: the arcs that Frame.renderSplines draws into a height x width frame, in the
 * reference's order (splines in order, arcs in order). upsampleControlPoints (Spline.java:27-87), computeIntermediarySamples(1.0f)
 * (:89-123), computeCoeffs (:133-152), fourierICT (:125-131) and the per-arc part of renderSpline (:159-179) in the reference's
 * float operations, with its quirks kept: every spline is drawn with the coefficients of spline 0 (the constructor never stores
 * the id, :23-25), MathHelper.max(float...) is the minimum (MathHelper.java:190-195), MathHelper.round is (int)(d + 0.5f) with
 * Java's saturating cast (:36-38). A spline with arcLength <= 0 has no arcs (:160-161); an arc whose maxDist is not finite or
 * whose box is empty is left out. Returns the number of arcs (also when it exceeds cap) and writes the first min(count, cap)
 * of them to out (out may be NULL when cap is 0), or a negative jxl_status: JXL_ERR_INVALID_ARGUMENT (null pointers, negative
 * counts, a spline without control points, height or width < 1), JXL_ERR_OOM (the table does not fit memory, or has more than
 * 2^26 arcs). */
int64_t    jxl_spline_arcs(const jxl_spline_desc* d, int32_t height, int32_t width, jxl_spline_arc* out, int64_t cap);
/* Frame.renderSplines (Frame.java:739-746) on three host planes of height x width floats, in place. Every pixel receives the
 * terms of the arcs whose box holds it in the reference's order, one `+=` per arc and channel (Spline.java:180-197), from one
 * kernel launch; a pixel no arc touches keeps its bits. Tolerance: every operation is the reference's float operation except
 * (float)Math.exp(double) (MathHelper.java:53, :61), evaluated in double on the device (jxl_fastpow.h: fp_exp): a sample may
 * differ only where one of its exp results falls on the other side of a float rounding boundary. n_splines == 0
 * leaves the planes alone. */
jxl_status jxl_stage_splines(jxl_ctx* ctx, float* const planes[3], int32_t height, int32_t width, const jxl_spline_desc* d);
/* the same on the resident planes: its place is after jxl_planes_upsample (and the patches), before jxl_planes_noise
 * (JXLCodestreamDecoder.java:628-637). Asynchronous. JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_splines(jxl_ctx* ctx, const jxl_spline_desc* d);
/* ---- patches: JXLCodestreamDecoder.computePatches (JXLCodestreamDecoder.java:212-254) + blendBuffers (:415-513) ----
 * One position of one patch (Patch.positions[j] of patches[i]), the positions of a frame in the order computePatches visits
 * them: patches in order, positions in order. */
typedef struct jxl_patch_pos {
    int32_t y0, x0;          /* Patch.positions[j]: where the rectangle lands in the frame (:231-232) */
    int32_t h, w;            /* Patch.bounds.size */
    int32_t ref;             /* Patch.ref: the reference slot (:220-222) */
    int32_t ref_y0, ref_x0;  /* Patch.bounds.origin: the rectangle's origin in the slot's planes */
    int32_t blend;           /* row of jxl_patch_desc.blend: Patch.blendingInfos[j] (:240) */
} jxl_patch_pos;
/* The patch stage of one frame. Channels are numbered as computePatches numbers them (:238): d < n_color the colour planes,
 * n_color + e extra channel e. A blend row holds one entry of three ints (mode 0..7, alphaChannel, clamp) per channel d: the
 * BlendingInfo computePatches hands to blendBuffers for it (blendingInfos[j][0] for every colour channel, [1 + e] for extra
 * channel e, :239-240). The image facts are those blendBuffers reads (:418-431). */
typedef struct jxl_patch_desc {
    int32_t n_pos;
    const jxl_patch_pos* pos;
    int32_t n_rows;
    const int32_t* blend;               /* [n_rows][n_color + n_extra][3] */
    int32_t n_color;                    /* imageHeader.getColorChannelCount(), which must be the frame's too: 1 or 3 */
    int32_t n_extra;                    /* imageHeader.getExtraChannelCount() */
    const int32_t* ec_is_alpha;         /* [n_extra] ExtraChannelInfo.type == ALPHA (:426) */
    const int32_t* ec_alpha_associated; /* [n_extra] ExtraChannelInfo.alphaAssociated (:431) */
    int32_t ref_h[4], ref_w[4];         /* size of the planes of reference[k]; 0 x 0: reference[k] == null (:225-226) */
} jxl_patch_desc;
/* Host only, needs no context and no device: validates the stage and bins its positions over the 32 x 8 pixel tiles of the kernel.
 * Walks the positions in order: a position whose slot is absent is skipped (:225-226), then "Patch out of range" (:220-221),
 * "Patch too large" (:228-229) and "Patch size out of bounds" (:233-237) -- the first offence returns JXL_ERR_INVALID_BITSTREAM
 * with that text in jxl_last_error(NULL) and its position in *first_bad. Then every (position, channel) with mode != 0 is mapped
 * to its blend function as blendBuffers does (:466-512, modes 5 / 6 / 7 remapped, old and new swapped for the "below" modes) and
 * checked as jxl_stage_blend checks one call: "Illegal blend mode" (JXL_ERR_INVALID_BITSTREAM; a mode outside 0..7, and mode 1,
 * which :484 maps to BLEND_REPLACE, for which the switch of :493-512 has no case), float functions on int planes,
 * planes of the wrong type, rectangles outside a plane it reads (JXL_ERR_INVALID_ARGUMENT). frame_type[d]: 0 float, 1 int32;
 * ref_type[4][n_color + n_extra]: the same, or -1 for a plane that is NULL (reads as zeros). JXL_ERR_UNSUPPORTED: a "below" mode
 * (5, 7) whose reference rectangle is not the frame rectangle itself in planes of the frame's size -- blendBuffers then reads the
 * frame away from the pixel it writes, which one in-place launch cannot replay.
 * Returns the number of non-empty tiles and *n_list, and writes tile[] (index ty * ceil(width / 32) + tx, ascending), start[]
 * (n + 1 CSR offsets) and list[] (position indices, per tile in stage order) when they fit cap_tiles / cap_list. */
int64_t    jxl_patch_bins(const jxl_patch_desc* d, int32_t height, int32_t width, const int32_t* frame_type, const int32_t* ref_type,
                          int32_t* tile, int32_t* start, int32_t* list, int64_t cap_tiles, int64_t cap_list, int64_t* n_list,
                          int32_t* first_bad);
/* computePatches (:212-254) on host planes, in place: frame[d] is height x width of frame_type[d]; ref[k * (n_color + n_extra) + d]
 * is plane d of reference[k] (ref_h[k] x ref_w[k] of ref_type), or NULL: zeros, the `new ImageBuffer` of :441-442 and :449-451.
 * No casts: the planes have the types blendBuffers would have given them (:433-465) -- the caller's type plan. Everything is
 * validated as by jxl_patch_bins before anything is queued; then one upload of the planes, ONE kernel launch in which every pixel
 * replays, in the reference's order (position, then channel), the applications whose rectangle holds it (blendAdd :285-318,
 * blendMult :320-339, blendBlend :341-379, blendMulAdd :381-413 with copyToCanvas :390 for the alpha channel itself), and one
 * download of the frame planes some position writes. A pixel no position covers keeps its bits. Bit-exact. */
jxl_status jxl_stage_patches(jxl_ctx* ctx, const jxl_patch_desc* d, void* const* frame, const int32_t* frame_type, int32_t height,
                             int32_t width, const void* const* ref, const int32_t* ref_type);
/* the same with the three colour planes being the resident planes (float; n_color == 3): its place is after jxl_planes_upsample,
 * before jxl_planes_splines / jxl_planes_noise (JXLCodestreamDecoder.java:628-637). extra[e] (extra_type[e]) are the frame's
 * extra channels on the host; those some position writes are updated in place (the call then waits for the device), otherwise
 * the call is asynchronous. JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_patches(jxl_ctx* ctx, const jxl_patch_desc* d, void* const* extra, const int32_t* extra_type,
                              const void* const* ref, const int32_t* ref_type);
/* current size of the resident planes */
jxl_status jxl_planes_shape(const jxl_ctx* ctx, int32_t* height, int32_t* width);
/* the host hook (patches, saveBeforeCT references; splines unless jxl_planes_splines draws them) and the way out: dense
 * height x width float planes */
jxl_status jxl_planes_download(jxl_ctx* ctx, float* const out[3]);
jxl_status jxl_planes_upload(jxl_ctx* ctx, const float* const in[3], int32_t height, int32_t width);

/* device-to-device copy of the result into caller-owned device memory (e.g. an RCCL send
 * buffer): dst = 3 planes back to back, width*height elements each. Async on the ctx stream. */
jxl_status jxl_vardct_copy_output_device(jxl_ctx* ctx, void* dst_device);
/* bytes of one output element for the configured out_format */
int32_t    jxl_vardct_out_elem_size(const jxl_ctx* ctx);
/* number of kernel launches the last jxl_vardct_run enqueued (diagnostics); after jxl_vardct_run_batch the launches the
 * frames share count on the first context only, so the counts of the batch's contexts add up to its launches */
int32_t    jxl_vardct_last_launch_count(const jxl_ctx* ctx);
/* HIP-event timing on the ctx stream, averaged over the runs recorded since timing was enabled
 * (ring of the 32 most recent): which = 0 whole run, 1 IDCT stage, 2 restoration+colour stage (from the end of the IDCT stage's last
 * launch: the boundary between the two launches is inside), 3 the fused restoration kernel's own start -> stop (what a profiler reports
 * for that launch; JXL_ERR_STATE if the timed runs did not take that kernel). */
jxl_status jxl_vardct_last_stage_ms(jxl_ctx* ctx, int32_t which, float* ms);
jxl_status jxl_vardct_enable_stage_timing(jxl_ctx* ctx, int32_t on);

/* ---- stage-level entry points (host planes in, host planes out; synchronous) --- */
/* One per reference function on the path; used by the parity tests. */

/* MathHelper.inverseDCT2D (MathHelper.java:96-122) on one h x w block. */
jxl_status jxl_stage_idct2d(jxl_ctx* ctx, const float* src, float* dst, int32_t h, int32_t w, int32_t transposed);
/* MathHelper.forwardDCT2D (MathHelper.java:124-136). */
jxl_status jxl_stage_fdct2d(jxl_ctx* ctx, const float* src, float* dst, int32_t h, int32_t w);
/* Frame.performGabConvolution (Frame.java:505-542). */
jxl_status jxl_stage_gab(jxl_ctx* ctx, const float* const in[3], float* const out[3],
                         int32_t height, int32_t width, const float w1[3], const float w2[3]);
/* Frame.performEdgePreservingFilter (Frame.java:544-636). inv_sigma: [ceil(h/8)][ceil(w/8)]
 * map for VarDCT, or NULL to use the constant inv_sigma_modular (Frame.java:573-575). */
/* The fused restoration launch of the frame path -- Gaborish -> EPF -> XYB in one kernel, float planes out -- on caller planes
 * of ANY height x width >= 8 (the frame path reaches it with padded sizes only). hf_mul / sharpness: ceil(height / 8) x
 * ceil(width / 8) cell maps (needed when epf_iters > 0); of `params` the restoration and colour fields are read (gab, gab_w1/2,
 * epf_*, global_scale_f, xyb, opsin_*, intensity_target); stages, transfer and out_format are ignored. */
jxl_status jxl_stage_restore_fused(jxl_ctx* ctx, const float* const in[3], float* const out[3], int32_t height, int32_t width,
                                   const int32_t* hf_mul, const int32_t* sharpness, const jxl_vardct_params* params);
jxl_status jxl_stage_epf(jxl_ctx* ctx, const float* const in[3], float* const out[3],
                         int32_t height, int32_t width, int32_t iterations,
                         const float* inv_sigma, float inv_sigma_modular,
                         const float channel_scale[3], float pass0_sigma_scale,
                         float pass2_sigma_scale, float border_sad_mul);
/* inverse-sigma map of Frame.java:552-571 from hfMul + sharpness cell maps. */
jxl_status jxl_stage_epf_sigma(jxl_ctx* ctx, const int32_t* hf_mul, const int32_t* sharpness,
                               int32_t bh, int32_t bw, float global_scale_f,
                               const float sharp_lut[8], float* inv_sigma);
/* LFCoefficients dequant + LF CfL + adaptiveSmooth (LFCoefficients.java:65-180) of one LF group: out[c] [cells_h][cells_w].
 * base_corr_x/b and color_factor as in jxl_vardct_params. */
jxl_status jxl_stage_lf_dequant(jxl_ctx* ctx, const jxl_lfquant_desc* d, float base_corr_x, float base_corr_b,
                                int32_t color_factor, float* const out[3]);
/* OpsinInverseMatrix.invertXYB (OpsinInverseMatrix.java:105-142), in place on planes[3]. */
jxl_status jxl_stage_xyb(jxl_ctx* ctx, float* const planes[3], int64_t n,
                         const float matrix[9], const float opsin_bias[3],
                         const float cbrt_opsin_bias[3], float intensity_target);
/* YCbCr branch of performColorTransforms (JXLCodestreamDecoder.java:270-281), in place. */
jxl_status jxl_stage_ycbcr(jxl_ctx* ctx, float* const planes[3], int64_t n);
/* JXLImage.transferInPlace + ImageBuffer.castToInt0: transfer = JXL_TRANSFER_*,
 * max_value = 0 keeps float output in out_f, else writes clamped ints to out_i. */
jxl_status jxl_stage_transfer(jxl_ctx* ctx, const float* in, int64_t n, int32_t transfer,
                              int32_t max_value, float* out_f, int32_t* out_i);
/* ---- colour management: JXLImage.transform (J/JXLImage.java:185-286) as one device pass ----
 * Transfer functions of TransferFunction.java / ColorManagement.getTransferFunction (ColorManagement.java:149-170), both
 * directions. (The JXL_TRANSFER_* values above keep their meaning for jxl_vardct_params.transfer and jxl_stage_transfer.) */
#define JXL_TF_LINEAR 0 /* TransferFunction.java:7-27 */
#define JXL_TF_SRGB   1 /* :29-61, toLinearF / fromLinearF in their float forms */
#define JXL_TF_BT709  2 /* :63-79 */
#define JXL_TF_PQ     3 /* :81-93. toLinear is NaN for inputs below ~7.3e-7, zero included (a negative base), as in the reference */
#define JXL_TF_GAMMA  4 /* GammaTransferFunction.java: pow(f, 1e7 / g) to linear, pow(f, 1e-7 * g) from linear; TF_DCI is g = 3846154 (:95) */
#define JXL_TF_HLG    5 /* JXL_ERR_UNSUPPORTED: the reference throws too (ColorManagement.java:161-162) */
/* One call = the stages below in this order, each one switchable; the samples of a pixel meet only in the matrix.
 *   1. cast          int32 samples -> float, v * (1.0f / in_max[c])     ImageBuffer.castToFloatWithMax (ImageBuffer.java:94-97, 112-127)
 *   2. toLinearF     of tf_in                                           JXLImage.linearize (:260-267)
 *   3. grey -> RGB   n_planes == 1 with use_matrix                      JXLImage.fillColor (:143-164)
 *   4. matrix        (m0 a + m1 b) + m2 c in float                      JXLImage.toneMapLinear (:114-141), MathHelper.java:242-252
 *   5. scale         f * scale                                          JXLImage.transfer, peak detection (:278-280)
 *   6. fromLinearF   of tf_out                                          JXLImage.transferInPlace (:244-258, :283)
 *   7. quantise      max_value > 0: ImageBuffer.castToInt0              ImageBuffer.java:129-145
 * The scale follows the matrix because transform() calls toneMapLinear before transfer(), where the peak is taken and applied.
 * Tolerance: the cast, the matrix, the scale, the linear segments and the quantisation of a given float are the reference's
 * float operations, bit for bit. Every curve that goes through a double pow is within 1 float ulp of the reference's
 * (float)Math.pow form (NaN, zero and infinite results equal), like JXL_TRANSFER_PQ_EXACT above. LINEAR / SRGB / PQ as tf_out
 * are jxl_stage_transfer's functions and, with max_value 255 or 65535, its exact threshold tables. */
typedef struct jxl_color_params {
    int32_t n_planes;      /* 1 or 3 input planes */
    int32_t in_is_int;     /* int32 samples, cast with in_max[c]; else float samples */
    int32_t in_max[3];     /* >= 1 where used */
    int32_t tf_in;         /* JXL_TF_* of the samples */
    int32_t gamma_in;      /* JXL_TF_GAMMA: the header's integer, 1 .. 2^24-1 */
    int32_t use_scale;
    float scale;
    int32_t use_matrix;    /* three planes out; a one-plane input is replicated first */
    float matrix[9];       /* row-major */
    int32_t tf_out;
    int32_t gamma_out;
    int32_t max_value;     /* 0: float planes out, else int32 planes clamped to 0..max_value */
} jxl_color_params;
/* n samples per plane. in: n_planes host planes. out: three host planes when n_planes == 3 or use_matrix, else one (out may
 * be the input planes). JXL_ERR_INVALID_ARGUMENT (nothing written): unknown selector, gamma out of range, n_planes not 1 or
 * 3, n < 0, a missing plane -- a grey output asked of a matrix included --, in_max < 1, max_value < 0. n == 0 does nothing. */
jxl_status jxl_stage_color_convert(jxl_ctx* ctx, const void* const in[3], int64_t n, const jxl_color_params* p,
                                   void* const out[3]);
/* JXLImage.determinePeak (:214-223) of the image that stages 1-4 of `p` make of in (h x w samples per plane; scale, tf_out
 * and max_value are not looked at): of its plane 1, or plane 0 when it has one plane. Float samples: per row
 * MathHelper.max(float...) (MathHelper.java:190-195: the row MINIMUM; a NaN first sample sticks, later NaNs are passed over,
 * of equal zeros the first stays), then the maximum over rows in Float.compareTo order (NaN greatest, -0 < +0); bit for bit
 * given the samples, any NaN for NaN. int32 samples that are linear and go through no matrix: the maximum sample divided by
 * (float)in_max (:219). w <= 2^30. */
jxl_status jxl_stage_color_peak(jxl_ctx* ctx, const void* const in[3], int32_t h, int32_t w, const jxl_color_params* p,
                                float* peak);
/* HDR -> SDR in the colour passes (jxlatte_amd/csrc/tone_map_ops.h has the definition; not the reference's): per pixel, behind
 * stage 4 and instead of stage 5, the BT.2408 Annex 5 curve on the pixel's luminance (standard PQ, no black lift), all three
 * samples multiplied by the one factor, then -- gamut 1 -- the least mix toward the pixel's own grey that brings it into [0, 1].
 * lum: the Y row of the RGB -> XYZ matrix of the primaries the samples are in behind stage 4; unit_nits: nits of a linear 1.0;
 * source_nits: the content's mastering peak; target_nits: the peak of the display the output is for (a linear 1.0 behind it). */
typedef struct jxl_tone_map { float lum[3]; float unit_nits, source_nits, target_nits; int32_t gamut; } jxl_tone_map;
/* arms (tm != NULL) or clears (NULL) tone mapping for the colour passes of this context: while armed, jxl_stage_color_convert,
 * the three *_png_samples, the three *_tensor_samples, the three *_tensor_resized entries and jxl_tensor_resized_batch (all items
 * share the block) apply it and write three colour channels, a one-plane image as three equal ones, as with use_matrix; a
 * jxl_color_params with use_scale set is JXL_ERR_INVALID_ARGUMENT there (nothing written). jxl_stage_color_peak, the PFM
 * entries and everything else ignore it. JXL_ERR_INVALID_ARGUMENT (the context keeps what it had): non-finite or non-positive
 * nits, source_nits > 10000, a non-finite weight, a weight sum outside (0, 2], gamut other than 0 or 1. */
jxl_status jxl_ctx_set_tone_map(jxl_ctx* ctx, const jxl_tone_map* tm);
/* 1 while tone mapping is armed, else 0 (a null ctx: 0): what a caller that sizes an output buffer from a jxl_color_params asks,
 * since an armed context writes three colour channels of a one-plane image */
int32_t jxl_ctx_tone_map_armed(const jxl_ctx* ctx);
/* ModularChannel.inverseHorizontalSqueeze / inverseVerticalSqueeze
 * (ModularChannel.java:361-413). out is (h) x (aw+rw) resp. (ah+rh) x (w). */
jxl_status jxl_stage_inv_hsqueeze(jxl_ctx* ctx, const int32_t* avg, int32_t aw, const int32_t* res, int32_t rw,
                                  int32_t h, int32_t* out);
jxl_status jxl_stage_inv_vsqueeze(jxl_ctx* ctx, const int32_t* avg, int32_t ah, const int32_t* res, int32_t rh,
                                  int32_t w, int32_t* out);
/* RCT branch of ModularStream.applyTransforms (ModularStream.java:255-326): in place on
 * v[3] of n samples; rct_type = permutation*7 + type. On return v[] holds the planes in
 * output channel order (the permutation is applied). */
jxl_status jxl_stage_rct(jxl_ctx* ctx, int32_t* const v[3], int64_t n, int32_t rct_type);
/* Palette branch of ModularStream.applyTransforms (ModularStream.java:327-378) for one transform: sample (y, x) of output
 * plane c is the colour its index names -- palette[c][index] for 0 <= index < nb_colors, the implicit colours above that (a
 * 64-entry cube, then the / 5 ladder, :346-356), kDeltaPalette below zero (:357-366; 0 for c >= 3) -- and, where index <
 * nb_deltas, that colour plus ModularChannel.prediction (ModularChannel.java:143-183) with predictor d_pred on plane c's own
 * samples, which are final for every neighbour the predictors read (:95-121). All of it in Java int arithmetic: sums,
 * products, negations and left shifts wrap at 32 bits, / and % truncate toward zero, shift counts count mod 32.
 * bit_depth is the image's bitsPerSample (:331). */
typedef struct jxl_palette_desc {
    int32_t num_c, nb_colors, nb_deltas, d_pred, bit_depth;
    int32_t pal_h, pal_w;
    const int32_t* palette;   /* pal_h x pal_w: channel 0 of the stream */
    const int32_t* pred;      /* height x width weighted-predictor values as decoded (before (p + 3) >> 3), or NULL */
} jxl_palette_desc;
/* index: height x width host samples; out: num_c host planes of height x width (out[0] may be index). Every input goes up
 * once (the index plane, nb_colors entries of the first num_c palette rows, pred when d_pred is 6) and every output plane comes
 * down once. One launch -- two when d_pred is neither 0 nor 6 and some pixel has index < nb_deltas: those pixels are then
 * resolved by a second kernel, in dependency order. With d_pred 6 and no pred plane the prediction is 0.
 * JXL_ERR_INVALID_ARGUMENT (nothing queued, out untouched): a null pointer, height or width below 1 or more than INT32_MAX
 * samples, num_c < 1, nb_colors or nb_deltas < 0, pal_w < nb_colors or pal_h < num_c (the reference's
 * ArrayIndexOutOfBoundsException), d_pred outside 0..13, d_pred 6 with nb_deltas > 0 and no pred plane, bit_depth outside
 * 1..32. */
jxl_status jxl_stage_palette(jxl_ctx* ctx, const jxl_palette_desc* d, const int32_t* index, int32_t height, int32_t width,
                             int32_t* const* out /* num_c planes */);
/* Frame.decodeFrame modular->buffer (Frame.java:430-455) for one output channel:
 * out = scale * (a + b) (b may be NULL) as float. */
jxl_status jxl_stage_modular_to_float(jxl_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n,
                                      float scale, float* out);

/* ---- row f4: pixel-domain stencils that run between EPF and the colour transform ---- */
/* Frame.invertSubsampling (Frame.java:681-723) for one channel: x_shift horizontal doublings then y_shift
 * vertical doublings (3/4, 1/4 triangle, replicated edges). out is (h << y_shift) x (w << x_shift). */
jxl_status jxl_stage_chroma_upsample(jxl_ctx* ctx, const float* in, int32_t h, int32_t w, int32_t x_shift,
                                     int32_t y_shift, float* out);
/* ImageHeader.getUpWeights index expansion (ImageHeader.java:441-470): packed = the k==2: 15, k==4: 55,
 * k==8: 210 coefficient list of the image header; out = [k][k][5][5]. Host-only helper, no device work. */
jxl_status jxl_upsampling_weights(int32_t k, const float* packed, float* out);
/* Frame.performUpsampling (Frame.java:217-260): k in {2,4,8}, weights [k][k][5][5], mirrored edges,
 * result clamped to the reference's [min, max] window (max starts at Float.MIN_VALUE, :237). out is (h*k) x (w*k). */
jxl_status jxl_stage_upsample(jxl_ctx* ctx, const float* in, int32_t h, int32_t w, int32_t k, const float* weights,
                              float* out);
/* Frame.initializeNoise (Frame.java:748-788): per-group XorShiro streams (features/XorShiro.java) turned into
 * floats in [1,2), then the 5x5 "laplacian" high-pass with mirrored edges. seed0 = (visibleFrames << 32) |
 * invisibleFrames (JXLCodestreamDecoder.java:629). out[c]: h x w, c < colors. */
jxl_status jxl_stage_noise_init(jxl_ctx* ctx, int32_t h, int32_t w, int32_t group_dim, uint64_t seed0, int32_t colors,
                                float* const out[3]);
/* Frame.synthesizeNoise (Frame.java:790-831), in place on the XYB planes[3] (X, Y, B); lut = LFGlobal.noiseParameters[8]. */
jxl_status jxl_stage_noise_add(jxl_ctx* ctx, float* const planes[3], const float* const noise[3], int64_t n,
                               const float lut[8], float base_corr_x, float base_corr_b);

/* ---- row f3: output stage (blending, orientation, sample packing) ---- */
#define JXL_BLEND_REPLACE 0 /* FrameFlags.java:18-22 */
#define JXL_BLEND_ADD     1
#define JXL_BLEND_BLEND   2
#define JXL_BLEND_MULADD  3
#define JXL_BLEND_MULT    4
#define JXL_BLEND_FLAG_IS_ALPHA  1u /* this channel is the alpha channel itself */
#define JXL_BLEND_FLAG_HAS_EXTRA 2u /* the image has extra channels (else BLEND / MULADD degrade to ADD) */
#define JXL_BLEND_FLAG_CLAMP     4u /* BlendingInfo.clamp */
#define JXL_BLEND_FLAG_PREMULT   8u /* alpha is associated */
typedef struct jxl_blend_rect {
    int32_t h, w;               /* blendSize */
    int32_t canvas_y, canvas_x; /* patchStart: where the rectangle lands on the canvas */
    int32_t frame_y, frame_x;   /* frameOffset: its origin inside the frame buffers */
    int32_t ref_y, ref_x;       /* refOffset: its origin inside the reference buffers */
} jxl_blend_rect;
/* One channel of JXLCodestreamDecoder.blendBuffers' inner switch (JXLCodestreamDecoder.java:26-40 copyToCanvas,
 * :285-318 blendAdd, :320-340 blendMult, :342-386 blendBlend, :388-422 blendMulAdd). "frame" and "ref" are the
 * arguments those functions receive under these names. canvas is ch x cw and updated in place inside the rectangle;
 * frame / frame_alpha are fh x fw; ref / ref_alpha are rh x rw. is_int: samples are int32 (REPLACE and the ADD
 * cases only), else float. Unused planes may be NULL. */
jxl_status jxl_stage_blend(jxl_ctx* ctx, int32_t mode, uint32_t flags, int32_t is_int,
                           void* canvas, int32_t ch, int32_t cw, const void* frame, int32_t fh, int32_t fw,
                           const void* ref, int32_t rh, int32_t rw, const float* frame_alpha, const float* ref_alpha,
                           const jxl_blend_rect* rect);

/* ---- device plane sets: the canvas and the reference frames of JXLCodestreamDecoder.decode kept on the device ----
 * A plane set is n planes (1..JXL_CANVAS_MAX_PLANES) of h x w 4-byte samples in device memory, each tagged float or int32 as an
 * ImageBuffer is (ImageBuffer.java:9-10); the tag changes only through the cast below. A context owns its sets and frees what
 * is left of them when it is destroyed; a set is addressed by a small integer id (>= 0). An unknown id is
 * JXL_ERR_INVALID_ARGUMENT, more than JXL_CANVAS_MAX_PLANES planes JXL_ERR_UNSUPPORTED. */
#define JXL_CANVAS_MAX_PLANES 16
#define JXL_PLANE_FLOAT 0 /* ImageBuffer.TYPE_FLOAT */
#define JXL_PLANE_INT32 1 /* ImageBuffer.TYPE_INT */
/* One canvas channel of a blendFrame call, with what blendBuffers resolves before its inner switch (:420-465) already resolved:
 * frame_plane is the remapped frame index of :420; mode is JXL_BLEND_REPLACE where :437 takes the short cut; flags carry isAlpha
 * (:426), hasExtra (:423), BlendingInfo.clamp and premult (:431). frame_alpha / ref_alpha: the planes frameColors + alphaChannel
 * of the frame set and colors + alphaChannel of the reference set (:444-445), looked at only where the mode reads them. */
typedef struct jxl_canvas_blend_chan {
    int32_t  frame_plane;
    int32_t  mode;   /* JXL_BLEND_* 0..4 */
    uint32_t flags;  /* JXL_BLEND_FLAG_* */
    int32_t  frame_alpha;
    int32_t  ref_alpha;
} jxl_canvas_blend_chan;
typedef struct jxl_canvas_blend_desc {
    int32_t canvas, frame; /* set ids; they differ */
    int32_t ref;           /* set id, -1 for refBuffers == null (every channel is then a copy), or the canvas id itself */
    int32_t n_chan;        /* the canvas set's plane count: blendFrame visits every canvas channel (:530) */
    jxl_blend_rect rect;
    jxl_canvas_blend_chan chan[JXL_CANVAS_MAX_PLANES];
} jxl_canvas_blend_desc;
/* shape and plane types of a set, for the check below */
typedef struct jxl_canvas_shape {
    int32_t n, h, w;
    int32_t types[JXL_CANVAS_MAX_PLANES];
} jxl_canvas_shape;
/* new ImageBuffer(type, height, width) per plane (JXLCodestreamDecoder.java:640-643, :441-442): zero-filled */
jxl_status jxl_canvas_create(jxl_ctx* ctx, int32_t n, int32_t h, int32_t w, const int32_t* types, int32_t* id);
jxl_status jxl_canvas_destroy(jxl_ctx* ctx, int32_t id);
/* plane count, size and plane tags of a set (ImageBuffer.getType, .height, .width) */
jxl_status jxl_canvas_describe(jxl_ctx* ctx, int32_t id, jxl_canvas_shape* out);
/* new ImageBuffer(b) per plane (:653, :631-632): a device copy, independent of its source from then on */
jxl_status jxl_canvas_clone(jxl_ctx* ctx, int32_t id, int32_t* new_id);
/* src: h * w samples of `type`, which becomes the plane's tag */
jxl_status jxl_canvas_upload(jxl_ctx* ctx, int32_t id, int32_t plane, const void* src, int32_t type);
/* dst: h * w samples; *type (may be NULL): the plane's tag */
jxl_status jxl_canvas_download(jxl_ctx* ctx, int32_t id, int32_t plane, void* dst, int32_t* type);
/* A new set of 3 + n_extra planes: the first three are float and hold a copy of the context's resident planes (Frame.getBuffer
 * of the colour channels at :528 without the host), the others are zero-filled planes of extra_types for the frame's extra
 * channels -- a blend reads the colours and the alpha of a frame from ONE set. JXL_ERR_STATE without resident planes. */
jxl_status jxl_canvas_from_planes(jxl_ctx* ctx, int32_t n_extra, const int32_t* extra_types, int32_t* id);
/* ImageBuffer.castToFloat(depth) of the whole plane in place (ImageBuffer.java:99-127): sample = (float)v * (1.0f / max), max =
 * ~(~0 << depth); nothing happens to a float plane. "invalid Max Value" (JXL_ERR_INVALID_ARGUMENT) as jxl_stage_pfm_samples. */
jxl_status jxl_canvas_cast(jxl_ctx* ctx, int32_t id, int32_t plane, int32_t depth);
/* JXLCodestreamDecoder.blendFrame (:515-537) as ONE launch over every channel, asynchronous on the context's stream. A lane
 * owns pixels of the rectangle and walks the channels in canvas order, its loads and stores in program order: with ref ==
 * canvas every sample is read at the position the lane itself writes later, so a later channel that reads an already blended
 * alpha plane sees the new value, as the reference's aliased ImageBuffer does. No casts happen here: the planes have the
 * types blendBuffers' casts (:433-465) would have given them -- the caller's type plan. jxl_canvas_blend_check runs first and
 * nothing is queued when it refuses. */
jxl_status jxl_canvas_blend(jxl_ctx* ctx, const jxl_canvas_blend_desc* d);
/* planes 0..2 of the set, which must be float, copied into the context's resident planes (the canvas handed to
 * transposeBuffer at :672-674 and to the writers); the set stays as it is */
jxl_status jxl_canvas_to_planes(jxl_ctx* ctx, int32_t id);
/* What jxl_canvas_blend refuses, without a context or a device (the reason: jxl_last_error of a NULL context). Per channel what
 * jxl_stage_blend answers: "Illegal blend mode" (JXL_ERR_INVALID_BITSTREAM), a float function on int32 planes, planes of a
 * channel that differ in type, alpha planes that are not float, a rectangle outside a plane that is read or written
 * (JXL_ERR_INVALID_ARGUMENT). JXL_ERR_UNSUPPORTED for what one in-place launch cannot replay: a reference that is the canvas
 * read anywhere but at the pixel that is written (refOffset != patchStart; blendMulAdd's alpha copy with frameOffset !=
 * patchStart, :390). ref: NULL when d->ref is -1; the canvas' own shape when d->ref == d->canvas. */
jxl_status jxl_canvas_blend_check(const jxl_canvas_blend_desc* d, const jxl_canvas_shape* canvas, const jxl_canvas_shape* frame,
                                  const jxl_canvas_shape* ref);
/* The Modular context's result channels as a new plane set: Frame.decodeFrame's modular -> buffer loop (Frame.java:430-455) for
 * all output planes as ONE launch. Plane i is result channel plane[i].channel (jxl_modular_out_shape's index) cropped to height x
 * width -- the frame's bounds; the source pitch is the channel's own width -- and either copied as int32 samples
 * (JXL_PLANE_INT32) or made float as jxl_stage_modular_to_float makes it (JXL_PLANE_FLOAT): scale * (float)(a [+ b]), the sum
 * in Java int arithmetic (wrapping), the conversion rounded first, then one f32 multiply. The XYB rule (Y, X, B - Y -> X, Y, B
 * with lfDequant) is the caller's choice of channel, add_channel and scale. The plan is settled first, as
 * jxl_modular_read_channel settles it; the set owns a copy (the result channels die with the next jxl_modular_begin). */
typedef struct jxl_modular_plane {
    int32_t channel;      /* index into the Modular context's result list */
    int32_t add_channel;  /* -1, or a second channel added first (Java int add, wrapping) */
    int32_t type;         /* JXL_PLANE_INT32: copy; JXL_PLANE_FLOAT: scale * (float)v */
    float   scale;
} jxl_modular_plane;
typedef struct jxl_modular_planes_desc {
    int32_t height, width, n_planes;   /* the frame's bounds; every named channel is at least that large */
    jxl_modular_plane plane[JXL_CANVAS_MAX_PLANES];
} jxl_modular_planes_desc;
/* Refused with nothing queued and *id untouched: no plan has run since jxl_modular_begin (JXL_ERR_STATE); more than
 * JXL_CANVAS_MAX_PLANES planes (JXL_ERR_UNSUPPORTED); JXL_ERR_INVALID_ARGUMENT for n_planes or a size below 1, a channel index
 * outside the result list, a channel smaller than the bounds, an add_channel on an int32 plane or of another size than its
 * channel, a type other than the two. */
jxl_status jxl_canvas_from_modular(jxl_ctx* ctx, const jxl_modular_planes_desc* d, int32_t* id);
/* The same result channels as a new set of UPSAMPLED float planes, k * height x k * width: Frame.upsample's loop over the frame's
 * buffers (Frame.java:725-728) for all planes as ONE launch. Plane i is Frame.performUpsampling (Frame.java:217-260) of
 * ImageBuffer.castToFloat (ImageBuffer.java:99-127; Frame.java:226-228) of the cropped channel: every tap is scale * (float)(a [+ b])
 * as above -- plane[i].scale is the plane's own 1f / maxValue -- read through MathHelper.mirrorCoordinate (MathHelper.java:323-329)
 * of the height x width crop, and the output is jxl_stage_upsample's, operation for operation (:233-256: window minimum from
 * Float.MAX_VALUE, maximum from Float.MIN_VALUE, the sum from 0f in iy, ix order, the clamp). k is 2, 4 or 8; weights: k * k * 25
 * floats as for jxl_stage_upsample (jxl_upsampling_weights). Every plane must be JXL_PLANE_FLOAT: the reference casts before it
 * upsamples. Complete on return. Refused with nothing queued and *id untouched: everything jxl_canvas_from_modular refuses, with
 * its status; JXL_ERR_INVALID_ARGUMENT for a k other than 2, 4 or 8, null weights, an int32 plane, and a k * height or k * width
 * beyond what a set holds (2^31 - 1). */
jxl_status jxl_canvas_from_modular_up(jxl_ctx* ctx, const jxl_modular_planes_desc* d, int32_t k, const float* weights, int32_t* id);
/* The inverse of jxl_canvas_to_planes: planes 0..2 of the set become copies of the context's resident planes and are tagged float,
 * whatever they were -- Frame.getBuffer of the colour channels (JXLCodestreamDecoder.java:528) after the stages that ran on the
 * resident planes (Frame.renderSplines :739-746, synthesizeNoise :790-831), with the frame's other planes left where they are.
 * Asynchronous. Refused with the set untouched: an unknown set, fewer than three planes, resident planes of another size than the
 * set (JXL_ERR_INVALID_ARGUMENT); no resident planes (JXL_ERR_STATE). */
jxl_status jxl_canvas_take_planes(jxl_ctx* ctx, int32_t id);
/* jxl_stage_orient of every plane of the set, whatever its type (the kernels move 4-byte words); orientations 5-8 exchange the
 * set's height and width. JXL_ERR_STATE: an orientation outside 1..8, as jxl_planes_orient. */
jxl_status jxl_canvas_orient(jxl_ctx* ctx, int32_t id, int32_t orientation);
/* ImageBuffer.castToFloat(depth) of every named plane in ONE launch: the hoisted casts of a patch segment or a blend (the frame's
 * planes and the reference planes of up to four slots: at most 5 * JXL_CANVAS_MAX_PLANES items). Bits and tags afterwards are those
 * of jxl_canvas_cast called per item; a plane that is float already is skipped. Asynchronous. Refused with nothing queued and no
 * tag changed (JXL_ERR_INVALID_ARGUMENT), the items looked at in order: an unknown set, a plane outside the set, the same
 * (set, plane) named twice -- two slots that are one set are one id: the caller names each plane once --, "invalid Max Value"
 * exactly where jxl_canvas_cast says it (an int32 plane whose depth gives max < 1); before all of these, more items than
 * 5 * JXL_CANVAS_MAX_PLANES. */
typedef struct jxl_canvas_cast_item {
    int32_t set, plane, depth;
} jxl_canvas_cast_item;
jxl_status jxl_canvas_cast_planes(jxl_ctx* ctx, int32_t n, const jxl_canvas_cast_item* items);
/* computePatches (JXLCodestreamDecoder.java:212-254 + blendBuffers :415-513) as jxl_stage_patches defines it, with every plane taken
 * from device plane sets: frame_set holds the frame's n_color + n_extra planes, of any types; ref_set[k] is the set of reference
 * slot k, or -1 for reference[k] == null (two slots may name one set). d->ref_h / ref_w are filled from the sets: what the caller
 * put there is ignored. colors_resident != 0: planes 0..2 of the frame are the context's resident planes (float, of the set's
 * size) and the set's own planes 0..2 are not touched -- a VarDCT frame's colours never leave the resident planes, only its extra
 * channels sit in the set; JXL_ERR_STATE without resident planes, JXL_ERR_INVALID_ARGUMENT when their size is not the set's.
 * No casts: the planes have the types the caller's type plan gave them (jxl_canvas_cast_planes). Everything
 * jxl_canvas_patches_check refuses is refused with nothing queued. Then the tables go up in one page-locked transfer and ONE
 * k_patches launch runs on the context's stream: asynchronous, no plane crosses the bus. Nothing writes a reference plane, and the
 * frame set is never a reference set. */
jxl_status jxl_canvas_patches(jxl_ctx* ctx, const jxl_patch_desc* d, int32_t frame_set, int32_t colors_resident, const int32_t ref_set[4]);
/* What jxl_canvas_patches refuses, without a context or a device (the reason: jxl_last_error of a NULL context). First the sets:
 * a frame or a reference set whose plane count is not n_color + n_extra (JXL_ERR_INVALID_ARGUMENT), more than
 * JXL_CANVAS_MAX_PLANES planes (JXL_ERR_UNSUPPORTED), colors_resident with n_color != 3, a frame set that is a reference set -- here:
 * ref[k] == frame, the same shape object -- (JXL_ERR_INVALID_ARGUMENT). Then exactly jxl_patch_bins' validation with the sizes and
 * plane types of the sets (colours float under colors_resident), its status, message and *first_bad. ref[k]: NULL for
 * reference[k] == null. */
jxl_status jxl_canvas_patches_check(const jxl_patch_desc* d, const jxl_canvas_shape* frame, int32_t colors_resident,
                                    const jxl_canvas_shape* const ref[4], int32_t* first_bad);

/* JXLCodestreamDecoder.transposeBufferFloat / transposeBufferInt (:43-177): EXIF orientation 1..8 of one plane of
 * 4-byte samples. out is h x w for orientation <= 4, else w x h. */
jxl_status jxl_stage_orient(jxl_ctx* ctx, const void* in, int32_t h, int32_t w, int32_t orientation, void* out);
/* PNGWriter ctor tail + writeIDAT sample order (PNGWriter.java:79-111, 191-203): coerce to float when needed,
 * un-premultiply, quantise / clamp to bit_depth, and interleave colour channels then alpha. */
typedef struct jxl_pack_params {
    int32_t height, width;
    int32_t n_color;         /* 1 (gray) or 3 */
    int32_t has_alpha;       /* planes[n_color] is the alpha plane */
    int32_t premultiplied;   /* image.isAlphaPremultiplied() */
    int32_t bit_depth;       /* 8 or 16 */
    int32_t big_endian;      /* 16-bit samples as DataOutput.writeShort emits them (PNG), else host order */
    int32_t is_int[4];       /* plane holds int32 samples (else float) */
    int32_t tagged_depth[4]; /* image.getTaggedBitDepth(c) */
} jxl_pack_params;
/* out: height * width * (n_color + has_alpha) samples of 1 or 2 bytes */
jxl_status jxl_stage_pack(jxl_ctx* ctx, const void* const planes[4], const jxl_pack_params* p, void* out);

/* ---- the PNG's samples from the colour planes in one pass: stages 1-6 of jxl_stage_color_convert, then jxl_stage_pack ----
 * What PNGWriter's constructor makes of an image, JXLImage.transform included, without the float planes between the two: per
 * pixel the colour stages of `color` (max_value must be 0: they end in float samples), then PNGWriter.java:79-111, 191-203 on
 * those samples and the alpha plane: an int32 alpha plane is cast with its tagged depth when the image is premultiplied or
 * the depth is not the PNG's (else clamped as it is), the colours are divided by a premultiplied alpha, every float becomes
 * (int)(v * max + 0.5f) clamped to 0..max, and the samples leave interleaved, colour then alpha. The bytes are those of
 * jxl_stage_color_convert (float output) followed by jxl_stage_pack, one for one: the same float operations in the same order,
 * hence the same tolerance against the reference (the curves' 1 ulp, seen through the quantiser). */
typedef struct jxl_png_params {
    jxl_color_params color;     /* the planes and stages 1-6; max_value 0 */
    int32_t height, width;
    int32_t has_alpha;          /* an alpha plane follows the colours */
    int32_t premultiplied;      /* image.isAlphaPremultiplied() */
    int32_t bit_depth;          /* 8 or 16 */
    int32_t big_endian;         /* 16-bit samples as DataOutput.writeShort emits them (PNG), else host order */
    int32_t alpha_is_int;       /* the alpha plane holds int32 samples (else float) */
    int32_t alpha_tagged_depth; /* image.getTaggedBitDepth(alpha) */
    int32_t color_tagged_depth; /* image.getTaggedBitDepth(colour): int32 colour planes whose color.in_max[c] is 0 are cast
                                 * with 2^depth - 1, PNGWriter's coercion of an image that went through no transform */
} jxl_png_params;
/* in: color.n_planes host planes of height * width samples; alpha: a host plane or NULL. out: height * width * (nc +
 * has_alpha) samples of bit_depth / 8 bytes, nc = 3 when color.n_planes == 3 or color.use_matrix, else 1. One upload, one
 * launch, one download. JXL_ERR_INVALID_ARGUMENT (nothing queued, out untouched): what jxl_stage_color_convert and
 * jxl_stage_pack refuse, color.max_value != 0, sizes below 1. */
jxl_status jxl_stage_png_samples(jxl_ctx* ctx, const void* const in[3], const void* alpha, const jxl_png_params* p, void* out);
/* The same launch on the resident planes (three float planes: color.n_planes 3, in_is_int 0, height and width theirs);
 * alpha: a host plane in that geometry, uploaded once, or NULL. out is filled on return: the only samples that cross the bus
 * are the PNG's. JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_png_samples(jxl_ctx* ctx, const void* alpha, const jxl_png_params* p, void* out);
/* jxl_stage_color_peak on the resident planes (row order: that of the planes as they stand, so orient them first). */
jxl_status jxl_planes_color_peak(jxl_ctx* ctx, const jxl_color_params* p, float* peak);
/* jxl_stage_orient of the three resident planes, on the device; orientations 5-8 exchange the planes' height and width.
 * JXL_ERR_STATE: no resident planes, or an orientation outside 1..8. */
jxl_status jxl_planes_orient(jxl_ctx* ctx, int32_t orientation);
/* jxl_stage_png_samples with the colour planes 0 .. color.n_planes - 1 and the alpha plane (alpha_plane, -1: none) taken from
 * the plane set `id`: nothing goes up, only the PNG's samples come down. color.n_planes is 1 or 3 and no more than the set
 * holds; color.in_is_int must equal the tag of every colour plane, alpha_is_int that of the alpha plane, has_alpha must say
 * whether alpha_plane names one, and height and width are the set's -- else JXL_ERR_INVALID_ARGUMENT. Everything
 * jxl_stage_png_samples refuses is refused here, with out untouched. */
jxl_status jxl_canvas_png_samples(jxl_ctx* ctx, int32_t id, int32_t alpha_plane, const jxl_png_params* p, void* out);
/* jxl_stage_color_peak on planes 0 .. p->n_planes - 1 of the set (in_is_int must equal their tags) */
jxl_status jxl_canvas_color_peak(jxl_ctx* ctx, int32_t id, const jxl_color_params* p, float* peak);

/* ---- the image as a device tensor in one pass: the third exit beside the PNG's and the PFM's samples ----
 * Per pixel: the colour stages 1-6 of `color` exactly as jxl_stage_png_samples evaluates them (max_value must be 0); the alpha
 * sample (a float plane as it is; an int32 plane as (float)a * (1.0f / (2^depth - 1)) for the float dtypes, and by
 * jxl_stage_png_samples' rule at bit_depth 8 for JXL_TENSOR_U8); colour / alpha, the correctly rounded f32 division, when
 * `premultiplied` (whether or not alpha is written; a zero alpha gives what the division gives); for the float dtypes with
 * use_norm (v - mean[c]) * inv_std[c], two separately rounded f32 operations, c the OUTPUT channel (alpha, when written, is the
 * channel after the colours); then the conversion: F32 the bits as they are; F16 / BF16 round to nearest even (overflow to
 * infinity, F16 subnormals kept, every NaN 0x7E00 / 0x7FC0); U8 (int)(v * 255 + 0.5f) clamped to 0..255, the PNG's quantiser.
 * Output channels: nc = 3 when color.n_planes == 3 or color.use_matrix, else 1, plus 1 with write_alpha. JXL_TENSOR_CHW: channel
 * c at out + c * height * width elements, rows top to bottom; JXL_TENSOR_HWC: the channels interleaved per pixel.
 * out_device is DEVICE memory of the context's device, element-aligned (it may be a slice of a larger allocation), dense. The
 * launch is queued on the context's stream and the stream is synchronised before return; no sample comes down.
 * JXL_ERR_INVALID_ARGUMENT, nothing queued and out_device untouched: everything jxl_stage_png_samples refuses at bit_depth 8; an
 * unknown dtype or layout; use_norm with JXL_TENSOR_U8 or with an inv_std that is not finite; write_alpha or premultiplied
 * without has_alpha; an int32 alpha plane whose depth is outside 1..31 where it is cast; an out_device that is not device memory
 * of the context's device (a host pointer never reaches a kernel) or whose allocation ends before the tensor does. */
#define JXL_TENSOR_U8 0
#define JXL_TENSOR_F16 1
#define JXL_TENSOR_BF16 2
#define JXL_TENSOR_F32 3
#define JXL_TENSOR_CHW 0
#define JXL_TENSOR_HWC 1
typedef struct jxl_tensor_params {
    jxl_color_params color;     /* the planes and stages 1-6; max_value 0 */
    int32_t height, width;
    int32_t has_alpha;          /* an alpha plane is given */
    int32_t premultiplied;      /* the colours are divided by alpha */
    int32_t write_alpha;        /* alpha is the last output channel */
    int32_t alpha_is_int;       /* as in jxl_png_params */
    int32_t alpha_tagged_depth;
    int32_t color_tagged_depth;
    int32_t dtype;              /* JXL_TENSOR_U8 / F16 / BF16 / F32 */
    int32_t layout;             /* JXL_TENSOR_CHW / HWC */
    int32_t use_norm;           /* float dtypes only */
    float mean[4], inv_std[4];  /* per output channel */
} jxl_tensor_params;
/* in: color.n_planes host planes of height * width samples, alpha: a host plane or NULL; uploaded once. */
jxl_status jxl_stage_tensor_samples(jxl_ctx* ctx, const void* const in[3], const void* alpha, const jxl_tensor_params* p, void* out_device);
/* The same launch on the three resident float planes (color.n_planes 3, in_is_int 0, height and width theirs); alpha: a host
 * plane, uploaded once, or NULL. JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_tensor_samples(jxl_ctx* ctx, const void* alpha, const jxl_tensor_params* p, void* out_device);
/* The same launch on planes 0 .. color.n_planes - 1 and the alpha plane (alpha_plane, -1: none) of the plane set `id`, with
 * jxl_canvas_png_samples' checks of the set's geometry and tags: nothing crosses the bus in either direction. */
jxl_status jxl_canvas_tensor_samples(jxl_ctx* ctx, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, void* out_device);

/* ---- the image as a device tensor of a GIVEN SIZE in one pass: a box of the planes resampled to out_height x out_width ----
 * This stage has no counterpart in the reference (which never resamples an image): its contract is stated here and in DESIGN
 * 4.5o. The separable filter sits between stages 5 and 6 of jxl_stage_tensor_samples, so that it averages LINEAR samples
 * wherever the colour stages pass through linear light, and the output curve runs per output pixel only.
 * Tap tables, per axis, in IEEE double on the host (box length L, output length O; these are Pillow's precompute_coeffs):
 *   s = L / O, fs = max(s, 1), sup = r * fs with r = 1 (JXL_RESIZE_TRIANGLE) or 0.5 (JXL_RESIZE_BOX); for output o:
 *   c = (o + 0.5) * s, lo = max(0, floor(c - sup + 0.5)), hi = min(L, floor(c + sup + 0.5)); the weight of source j in
 *   [lo, hi), t = (j + 0.5 - c) / fs: triangle max(0, 1 - |t|); box 1 where -0.5 < t <= 0.5, else 0; the weights are divided by
 *   their sum (ascending j) and rounded to f32; trailing, then leading taps of f32 weight 0 are dropped, one tap is kept at
 *   least (an identity size: one tap of weight 1, an exact copy). A range wider than 1024 taps is refused.
 * Per output element, in f32, every multiply and add rounded separately, the VERTICAL pass first, each sum sequential in
 * ascending index: V(x) = wy[0] * S(y0, x), V = V + wy[k] * S(y0 + k, x); R = wx[0] * V(x0), R = R + wx[k] * V(x0 + k). S is
 * the stage 1-5 value of the source pixel; alpha is filtered the same way from its float value (a float plane as it is, an
 * int32 plane as (float)a * (1.0f / (2^depth - 1)) -- for JXL_TENSOR_U8 as well: there is no integer left to clamp, and the
 * depth must be 1..31 wherever the plane is read); premultiplied colours are filtered as they are. A zero weight that survives
 * the trim multiplies like any other (0 * inf is NaN). Behind R: fromLinearF, colour / alpha when premultiplied,
 * normalisation, the conversion and the layout, exactly as jxl_stage_tensor_samples has them behind its stage 5.
 * p->height and p->width stay the SOURCE planes' size; the tensor is out_height x out_width, and out_device must hold it.
 * The box is in whole source pixels, inside the image. JXL_ERR_INVALID_ARGUMENT, nothing queued and out_device untouched:
 * everything the unresized entry refuses (with the tensor's size the output's), a box outside the image or empty, an output
 * size <= 0, an unknown filter, more than 1024 taps. The tap tables go up once per call; the stream is synchronised. */
#define JXL_RESIZE_TRIANGLE 0
#define JXL_RESIZE_BOX 1
typedef struct jxl_resize_params {
    int32_t box_x0, box_y0, box_width, box_height; /* the source box, in source pixels */
    int32_t out_height, out_width;                 /* the tensor's size */
    int32_t filter;                                /* JXL_RESIZE_TRIANGLE / BOX */
} jxl_resize_params;
jxl_status jxl_stage_tensor_resized(jxl_ctx* ctx, const void* const in[3], const void* alpha, const jxl_tensor_params* p,
                                    const jxl_resize_params* r, void* out_device);
/* The same launch on the three resident float planes, as jxl_planes_tensor_samples. */
jxl_status jxl_planes_tensor_resized(jxl_ctx* ctx, const void* alpha, const jxl_tensor_params* p, const jxl_resize_params* r,
                                     void* out_device);
/* The same launch on the planes of the plane set `id`, as jxl_canvas_tensor_samples. */
jxl_status jxl_canvas_tensor_resized(jxl_ctx* ctx, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p,
                                     const jxl_resize_params* r, void* out_device);

/* ---- N images resampled into one batch tensor in ONE launch ----
 * Item i's tensor is dense at out_device + i * out_height * out_width * n_out elements, and its bytes are exactly what the
 * single-image entry of its source kind -- jxl_stage_tensor_resized (JXL_BATCH_HOST), jxl_planes_tensor_resized
 * (JXL_BATCH_RESIDENT), jxl_canvas_tensor_resized (JXL_BATCH_SET) -- writes for the same p and r, bit for bit: the arithmetic is
 * the one stated above, every sum one lane's and sequential, so that neither the tile nor the grid nor the batch changes a bit.
 * All items share out_height, out_width, dtype, layout and the output channel count; everything else is per item: source size,
 * box, filter, colour parameters, alpha type and depth, premultiplied, normalisation. Two items may name the same set; at most
 * one item is JXL_BATCH_RESIDENT (a context has one set of resident planes). n is 1 .. JXL_TENSOR_BATCH_MAX: the descriptors
 * live in device memory, not in the kernel's argument block.
 * One transfer carries every descriptor, the work list and the tap tables (a table is shared by the items of one length, output
 * length and filter); one launch; the stream is synchronised once before return.
 * All or nothing -- if any item is refused nothing is queued and out_device is untouched: JXL_ERR_INVALID_ARGUMENT (JXL_ERR_STATE
 * for a resident item without resident planes), jxl_last_error "tensor batch: item <i>: <the single-image entry's reason>".
 * Refused as a batch: n out of range, null arguments, an unknown source, items that disagree on size, dtype, layout or channel
 * count, a second resident item, an out_device that is not device memory of the context's device or whose allocation ends
 * before the n-th tensor does. */
#define JXL_TENSOR_BATCH_MAX 1024
#define JXL_BATCH_HOST 0      /* in[], alpha: host planes, uploaded once */
#define JXL_BATCH_RESIDENT 1  /* the context's three resident float planes; alpha: a host plane or NULL */
#define JXL_BATCH_SET 2       /* planes 0 .. n_planes-1 and alpha_plane (-1: none) of the plane set set_id */
typedef struct jxl_tensor_batch_item {
    int32_t source, set_id, alpha_plane;
    const void* in[3];
    const void* alpha;
    jxl_tensor_params p;      /* this image's planes, colour stages, alpha rule */
    jxl_resize_params r;      /* this image's box; out_height / out_width / filter */
} jxl_tensor_batch_item;
jxl_status jxl_tensor_resized_batch(jxl_ctx* ctx, int32_t n, const jxl_tensor_batch_item* items, void* out_device);

/* ---- the PFM's samples in one pass: replaces the body of PFMWriter.write (PFMWriter.java:30-48) after the header ----
 * The planes are the image's own samples (image.getBuffer(false), :30): no colour transform, no peak scale, no transfer
 * function. An int32 plane is cast as castToFloat(image.getTaggedBitDepth(c)) casts it (:33-35; ImageBuffer.java:99-101,
 * 112-127): max = ~(~0 << depth) in Java int arithmetic, sample = (float)v * (1.0f / max), the conversion rounded before the one
 * f32 multiply. Every sample leaves as DataOutputStream.writeFloat writes it (:46): Float.floatToIntBits, so every NaN is
 * 0x7fc00000 while -0.0f, the infinities and the subnormals keep their bits, most significant byte first. Channels are
 * interleaved per pixel, pixels left to right, rows bottom to top (:43-47). The header line (:27-29) stays with the caller. */
typedef struct jxl_pfm_params {
    int32_t height, width;
    int32_t n_planes;           /* 1: CE_GRAY ("Pf"), 3: every other image ("PF"); alpha and extra channels are never written */
    int32_t is_int[3];          /* plane c holds int32 samples (else float); planes of mixed kind are legal */
    int32_t tagged_depth[3];    /* image.getTaggedBitDepth(c), looked at for the int32 planes only */
} jxl_pfm_params;
/* in: n_planes host planes of height * width samples. out: 4 * n_planes * width * height bytes. One upload, one launch, one
 * download. JXL_ERR_INVALID_ARGUMENT (nothing queued, out untouched): sizes below 1, n_planes other than 1 or 3, an int32 plane
 * whose depth gives max < 1 ("invalid Max Value", ImageBuffer.java:115-116: depth 0 or 32), a null pointer. */
jxl_status jxl_stage_pfm_samples(jxl_ctx* ctx, const void* const in[3], const jxl_pfm_params* p, void* out);
/* The same launch on the three resident float planes, as they stand (after jxl_planes_orient): n_planes 3, no is_int, height
 * and width theirs -- anything else is JXL_ERR_INVALID_ARGUMENT. out is filled on return: the only bytes that cross the bus are
 * the PFM's (PFMWriter.java:30-48 without image.getBuffer). JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_pfm_samples(jxl_ctx* ctx, const jxl_pfm_params* p, void* out);
/* The same launch on planes 0 .. n_planes - 1 of the plane set `id`: is_int[c] must equal the planes' tags and height and width
 * the set's (JXL_ERR_INVALID_ARGUMENT otherwise, and for everything jxl_stage_pfm_samples refuses; out untouched). */
jxl_status jxl_canvas_pfm_samples(jxl_ctx* ctx, int32_t id, const jxl_pfm_params* p, void* out);

/* ---- the varblock map drawn onto the picture: replaces Frame.drawVarblocks (Frame.java:464-503), which
 * JXLCodestreamDecoder.java:638-639 calls right after performColorTransforms when JXLOptions.renderVarblocks is set ----
 * Every block (cy, cx, type) tints the pixels of its pixelHeight x pixelWidth extent (include/jxl_transform_types.h) at
 * (cy << 3, cx << 3) by its type (Frame.java:476-479: hue = (((float)type * PHI_BAR) % 1.0f) * 2f * (float)Math.PI, three
 * factors from (float)Math.cos) and blackens its top row and left column (:488-491); every other pixel of it becomes
 * factor_c * 0.5f + 0.5f * sample_c / light with light = (float)Math.cbrt(0.25f * (R + B) + 0.5f * G) * 0.5f + 0.25f (:493-497),
 * every product, sum and quotient rounded on its own. The coordinates are FRAME cells: the caller adds the LF group's offset
 * (:470-472, :480-481). A pixel outside the planes, or inside no block, is left alone: the block coordinates are those of the
 * frame before upsampling whatever the planes' size (the reference's own behaviour on an upsampled frame).
 * (float)Math.cos is the host library's cos and (float)Math.cbrt the device library's double-precision cbrt: each is within
 * an ulp or two of the correctly rounded double, like Java's (specified to 1 ulp), so a sample can differ from a JVM's where
 * the double lies that close to the middle between two floats. */
typedef struct jxl_varblock_desc {
    int32_t n_blocks;
    const int32_t* blocks;      /* n_blocks x (cy, cx, type): frame cells (8 x 8 pixels) and TransformType.type, 0..26 */
    int32_t cells_h, cells_w;   /* the cell grid the blocks live on: every block lies inside it, no two share a cell */
} jxl_varblock_desc;
/* in, out: three host planes of height x width floats each (out[c] may be in[c]). One upload, one launch, one download.
 * JXL_ERR_INVALID_ARGUMENT (nothing queued, out untouched): a null pointer, a size below 1, a type above 26, a block that
 * leaves the cell grid, two blocks that claim one cell. */
jxl_status jxl_stage_varblocks(jxl_ctx* ctx, const float* const in[3], int32_t height, int32_t width, const jxl_varblock_desc* d,
                               float* const out[3]);
/* The same launch (Frame.java:464-503) on the three resident planes, in place, after jxl_planes_xyb / jxl_planes_ycbcr: nothing
 * but the cell map (one byte per cell) and the 27 x 3 factors crosses the bus. Asynchronous. The same refusals, with the planes
 * untouched. JXL_ERR_STATE without resident planes. */
jxl_status jxl_planes_varblocks(jxl_ctx* ctx, const jxl_varblock_desc* d);

/* ---- Modular path: replaces ModularStream.applyTransforms squeeze/RCT branches ---- */
/* Default squeeze parameter list of ModularStream.java:110-131 for a channel list whose
 * first nb_meta channels are meta channels. Returns the count (<= cap) or a negative status. */
int32_t    jxl_modular_default_squeeze_params(const int32_t* widths, const int32_t* heights, int32_t n_channels,
                                              int32_t nb_meta, jxl_squeeze_param* out, int32_t cap);
/* Forward shape replay of ModularStream.java:137-167: given the n_channels image channels,
 * produce the encoded channel list's shapes (count returned; <= cap). */
int32_t    jxl_modular_squeezed_shapes(const int32_t* widths, const int32_t* heights, int32_t n_channels,
                                       const jxl_squeeze_param* sp, int32_t n_sp,
                                       int32_t* out_w, int32_t* out_h, int32_t cap);
/* Upload the encoded channel list (averages + residuals as decoded by the host) and the
 * transform to undo. n_out = number of channels after the inverse. rct_type < 0 = no RCT,
 * otherwise applied on channels rct_begin..+2 after the squeeze. */
jxl_status jxl_modular_begin(jxl_ctx* ctx, const jxl_channel* chans, int32_t n_chans,
                             const jxl_squeeze_param* sp, int32_t n_sp,
                             int32_t rct_type, int32_t rct_begin);
/* enqueue the inverse steps (asynchronous, re-runnable) */
jxl_status jxl_modular_run(jxl_ctx* ctx);
/* number / shape of result channels */
int32_t    jxl_modular_out_count(const jxl_ctx* ctx);
jxl_status jxl_modular_out_shape(const jxl_ctx* ctx, int32_t idx, int32_t* w, int32_t* h);
/* synchronize + copy result channel idx to host */
jxl_status jxl_modular_read_channel(jxl_ctx* ctx, int32_t idx, int32_t* dst);
/* begin + run + read of all channels: out[i].data must hold out w*h elements */
jxl_status jxl_modular_apply(jxl_ctx* ctx, const jxl_channel* chans, int32_t n_chans,
                             const jxl_squeeze_param* sp, int32_t n_sp,
                             int32_t rct_type, int32_t rct_begin,
                             jxl_channel* out, int32_t n_out);
int32_t    jxl_modular_last_launch_count(const jxl_ctx* ctx);
/* how often a plan had to be run again with in-order verification because a segment boundary of the speculative run did not
 * match (diagnostics; the result is exact either way) */
int32_t    jxl_modular_redo_count(const jxl_ctx* ctx);

/* One frame-level transform as the bitstream lists it (TransformInfo.java). kind: the front-end's numbering. */
#define JXL_TRANSFORM_RCT     0
#define JXL_TRANSFORM_PALETTE 1
#define JXL_TRANSFORM_SQUEEZE 2
typedef struct jxl_modular_transform {
    int32_t kind;
    int32_t begin_c, num_c;       /* RCT: begin_c; Palette: both */
    int32_t rct_type;
    int32_t nb_colors, nb_deltas, d_pred;
    const jxl_squeeze_param* sp;  /* Squeeze: the expanded step list (defaults already filled in) */
    int32_t n_sp;
} jxl_modular_transform;
/* jxl_modular_begin for any transform chain: tr[0 .. n_tr) in bitstream order, undone last to first exactly as
 * ModularStream.applyTransforms does (ModularStream.java:224-380); chans is the encoded list, meta channels included, and
 * every begin_c is read against the list as it stands at that point of the inverse walk. An inverse Palette (:327-378) reads
 * its palette from the device copy of channel 0: nothing crosses the bus between transforms. jxl_modular_run, _out_*,
 * _read_channel, jxl_canvas_from_modular* work on the result as on jxl_modular_begin's. A chain that jxl_modular_begin can
 * express ([], [RCT], [Squeeze], [RCT, Squeeze]) is handed to it unchanged.
 * Refused with nothing queued and the context usable: what jxl_stage_palette refuses for a single transform, with the sizes
 * of the channels at that point of the walk; a Palette whose index channel begin_c + 1 is not in the list; an RCT outside the
 * list (JXL_ERR_INVALID_ARGUMENT) or over channels of unequal size (JXL_ERR_INVALID_BITSTREAM); a Squeeze step outside the
 * list (JXL_ERR_INVALID_BITSTREAM); an unknown kind; and, JXL_ERR_UNSUPPORTED, a Palette with nb_deltas > 0 and d_pred 6 (the
 * weighted predictor's plane exists only while the host decodes the channel). */
jxl_status jxl_modular_begin_chain(jxl_ctx* ctx, const jxl_channel* chans, int32_t n_chans,
                                   const jxl_modular_transform* tr, int32_t n_tr, int32_t bit_depth);

#ifdef __cplusplus
}
#endif
#endif /* JXLATTE_AMD_H */
