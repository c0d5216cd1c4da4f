package com.traneptora.jxlatte.gpu;

import java.nio.ByteBuffer;

/**
 * JNI mirror of include/jxlatte_amd.h for the jxlatte Java host (row f4 of the scope table).
 *
 * NOT COMPILED OR TESTED IN THIS REPOSITORY: the build image has no JDK (no javac, no jni.h). It is the binding a jxlatte
 * maintainer adds; INTEGRATION.md lists the five call sites of the reference it is used from. All bulk data crosses as
 * DIRECT ByteBuffers in native byte order because Java float[][] / int[][] rows are separate heap arrays.
 */
public final class NativeBackend implements AutoCloseable {
    static {
        System.loadLibrary("jxlatte_amd_jni"); // links libjxlatte_amd.so
    }

    private long ctx; // jxl_ctx*

    public NativeBackend(int device) {
        ctx = create(device);
    }

    @Override
    public void close() {
        destroy(ctx);
        ctx = 0;
    }

    private static native long create(int device);                 // jxl_ctx_create
    private static native void destroy(long ctx);                  // jxl_ctx_destroy

    /** params: struct jxl_vardct_params packed by the caller (4-byte fields, C layout). */
    public native void beginFrame(ByteBuffer params);              // jxl_vardct_begin_frame
    public native void setWeights(ByteBuffer weights, int[] offs); // jxl_vardct_set_weights
    public native void setLFGroup(int lfgY, int lfgX, int cellsH, int cellsW, ByteBuffer dctSelect, ByteBuffer hfMul,
        ByteBuffer sharpness, ByteBuffer xFromY, ByteBuffer bFromY, ByteBuffer blockYX, int nBlocks,
        ByteBuffer lfX, ByteBuffer lfY, ByteBuffer lfB);           // jxl_vardct_set_lfgroup
    public native void setLFGroupQuant(int lfgY, int lfgX, int cellsH, int cellsW, ByteBuffer qX, ByteBuffer qY, ByteBuffer qB,
        int extraPrecision, float[] scaledDequant, int xFactorLF, int bFactorLF, boolean adaptiveSmoothing); // ..._lfquant
    public native void putGroup(int pass, int group, ByteBuffer qX, ByteBuffer qY, ByteBuffer qB, int strideX, int strideY,
        int strideB);                                              // jxl_vardct_put_group
    /** int16 wire format: the caller has checked that every coefficient of the group fits (else putGroup). */
    public native void putGroupI16(int pass, int group, ByteBuffer qX, ByteBuffer qY, ByteBuffer qB, int strideX, int strideY,
        int strideB);                                              // jxl_vardct_put_group_i16
    /** The frame's three int16 coefficient planes in page-locked memory the library owns (zero-filled): the entropy
     *  decoder stores its non-zero coefficients in place (row stride = plane width), then commitCoeffsI16(). */
    public native ByteBuffer[] mapCoeffsI16();                     // jxl_vardct_map_coeffs_i16 + jxl_vardct_coeff_plane_rows + NewDirectByteBuffer
    public native int[] coeffPlaneRows();                          // jxl_vardct_coeff_plane_rows -> rows of the three mapped planes
    public native void commitCoeffsI16();                          // jxl_vardct_commit_coeffs_i16
    /** the same planes without the zero-fill: the decoder writes every sample of the groups it then names in commitCoeffsI16Groups */
    public native ByteBuffer[] mapCoeffsI16NoFill();               // jxl_vardct_map_coeffs_i16_ex(JXL_MAP_NO_FILL)
    public native void commitCoeffsI16Groups(byte[] groupWritten); // jxl_vardct_commit_coeffs_i16_groups
    /** Sparse coefficient feed: only the non-zero coefficients, as the entries HFCoefficients' decode loop produces
     *  (HFCoefficients.java:112-127). Narrow entry: one int, value << 16 | y << 8 | x; wide: two ints, (y << 8 | x, value).
     *  nX/nY/nB entries in the three direct buffers (a channel without entries may pass null). Pass 0 replaces the group. */
    public native void putGroupSparse(int pass, int group, ByteBuffer eX, ByteBuffer eY, ByteBuffer eB, int nX, int nY, int nB,
        boolean wide);                                             // jxl_vardct_put_group_sparse
    /** The library's page-locked entry buffer (capacityWords ints): append runs of entries, each starting at a multiple of
     *  four ints, then commitSparse. Valid until the next beginFrame. */
    public native ByteBuffer mapSparse(long capacityWords);        // jxl_vardct_map_sparse + NewDirectByteBuffer
    /** runs: five ints per run {group, channel, flags (1 = wide), count, offsetWords}; the entries ADD into the planes. */
    public native void commitSparse(int[] runs);                   // jxl_vardct_commit_sparse
    public native long sparseRejected();                           // jxl_vardct_sparse_rejected
    /** Page-locked direct buffers for planes that cross the bus (coefficients in, pixels out). */
    public static native ByteBuffer hostAlloc(long bytes);         // jxl_host_alloc + NewDirectByteBuffer
    public static native void hostFree(ByteBuffer b);              // jxl_host_free(GetDirectBufferAddress(b))
    public native void finishFrame(ByteBuffer outX, ByteBuffer outY, ByteBuffer outB, long stride); // jxl_vardct_finish_frame
    /** Asynchronous form for independent frames decoded side by side (one NativeBackend each): run() enqueues the frame
     *  on its context's stream, readOutput() waits for it. runBatch hands several prepared frames to one call. */
    public native void run();                                      // jxl_vardct_run
    public native void readOutput(ByteBuffer outX, ByteBuffer outY, ByteBuffer outB, long stride); // jxl_vardct_read_output
    /** readOutput in two halves: between them the host may drive the next frame of this context (buffers from hostAlloc) */
    public native void readOutputBegin(ByteBuffer outX, ByteBuffer outY, ByteBuffer outB, long stride); // jxl_vardct_read_output_begin
    public native void readOutputWait();                                                           // jxl_vardct_read_output_wait
    public static void runBatch(NativeBackend[] frames) {          // jxl_vardct_run_batch
        long[] h = new long[frames.length];
        for (int i = 0; i < frames.length; i++) h[i] = frames[i].ctx;
        runBatch0(h);
    }
    private static native void runBatch0(long[] ctxs);
    /** Binning, chroma-from-luma masks and side-table upload of the frame that was just described (setLFGroup calls done);
     *  run() does the same on first use. Lets the host overlap this with the entropy decoding of the HF groups. */
    public native void prepare();                                  // jxl_vardct_prepare

    // ---- the stages between decodeFrame and the blend on planes that stay on the device (JXLCodestreamDecoder.java:628-637)
    public native void planesFromFrame(int height, int width);     // jxl_planes_from_frame (after run(); header.bounds size)
    public native void planesUpload(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, int height, int width); // jxl_planes_upload
    public native void planesUpsample(int k, float[] weights);     // jxl_planes_upsample   (Frame.upsample)
    public native void planesNoise(int groupDim, long seed0, float[] lut, float baseCorrX, float baseCorrB); // jxl_planes_noise
    public native void planesFromFrameAt(int y0, int x0, int height, int width); // jxl_planes_from_frame_at: any window of the result
    // the resident planes are the window at (y0, x0) of a frameH x frameW frame: the whole frame's noise restricted to it
    public native void planesNoiseAt(int groupDim, long seed0, float[] lut, float baseCorrX, float baseCorrB, int frameH, int frameW,
        int y0, int x0);                                               // jxl_planes_noise_at
    /** computePatches (:212-254) on the resident colour planes, after planesUpsample and before planesSplines / planesNoise; extra[e]:
     *  the frame's extra channels as direct buffers (written in place where a position stores into them); the rest as stagePatches. */
    public native void planesPatches(ByteBuffer[] extra, int[] extraType, ByteBuffer[] ref, int[] refType, int[] pos, int[] blend,
                                     int[] ecIsAlpha, int[] ecAlphaAssociated, int[] refShape);                        // jxl_planes_patches
    /** Frame.renderSplines (Frame.java:739-746) on the resident planes, after planesUpsample / the patches and before planesNoise.
     *  The splines as SplinesBundle holds them, flattened: nControl[s] points per spline, control = all (y, x) pairs, coeff =
     *  per spline coeffX, coeffY, coeffB, coeffSigma (4 x 32); baseCorrX / B from LFChannelCorrelation. */
    public native void planesSplines(int quantAdjust, int[] nControl, int[] control, int[] coeff, float baseCorrX, float baseCorrB); // jxl_planes_splines
    public native void planesXYB(float[] matrix, float[] opsinBias, float[] cbrtOpsinBias, float intensityTarget); // jxl_planes_xyb
    public native void planesYCbCr();                              // jxl_planes_ycbcr
    public native int[] planesShape();                             // jxl_planes_shape -> {height, width}
    public native void planesDownload(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2); // jxl_planes_download
    // ---- context, diagnostics
    public static native String version();                         // jxl_version
    public native void synchronize();                              // jxl_ctx_synchronize (JXLCodestreamDecoder.java:637: before the host reads)
    public native long stream();                                   // jxl_ctx_stream (hipStream_t as a long, for callers that own a HIP runtime)
    public native void setStream(long hipStream);                  // jxl_ctx_set_stream
    public native void copyOutputDevice(long dstDevice);           // jxl_vardct_copy_output_device (D2D into an RCCL send buffer)
    public native int outElemSize();                               // jxl_vardct_out_elem_size
    public native int lastLaunchCount();                           // jxl_vardct_last_launch_count
    public native void enableStageTiming(boolean on);              // jxl_vardct_enable_stage_timing
    public native float lastStageMs(int which);                    // jxl_vardct_last_stage_ms (0 frame, 1 inverse transforms, 2 restoration)

    // ---- stage entries: one reference function each, host planes in / out (what the parity tests drive)
    public native void stageIdct2d(ByteBuffer src, ByteBuffer dst, int h, int w, boolean transposed);  // jxl_stage_idct2d (MathHelper.inverseDCT2D)
    public native void stageFdct2d(ByteBuffer src, ByteBuffer dst, int h, int w);                      // jxl_stage_fdct2d (MathHelper.forwardDCT2D)
    public native void stageGab(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2, int h, int w,
        float[] w1, float[] w2);                                   // jxl_stage_gab (Frame.performGabConvolution)
    /** jxl_stage_restore_fused: Gaborish, EPF and XYB as the frame path's one fused launch on planes of any size from 8 x 8; hfMul and
     *  sharpness are ceil(h / 8) x ceil(w / 8) int maps (may be null without EPF), params a direct buffer holding jxl_vardct_params */
    public native void stageRestoreFused(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2, int h, int w,
                                         ByteBuffer hfMul, ByteBuffer sharpness, ByteBuffer params);
    public native void stageEpf(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2, int h, int w,
        int iterations, ByteBuffer invSigma, float invSigmaModular, float[] channelScale, float pass0SigmaScale, float pass2SigmaScale,
        float borderSadMul);                                       // jxl_stage_epf (Frame.performEdgePreservingFilter)
    public native void stageEpfSigma(ByteBuffer hfMul, ByteBuffer sharpness, int bh, int bw, float globalScale, float[] sharpLut,
        ByteBuffer invSigma);                                      // jxl_stage_epf_sigma (Frame.java:552-571)
    public native void stageLfDequant(int lfgY, int lfgX, int cellsH, int cellsW, ByteBuffer qX, ByteBuffer qY, ByteBuffer qB,
        int extraPrecision, float[] scaledDequant, int xFactorLF, int bFactorLF, boolean adaptiveSmoothing, float baseCorrX,
        float baseCorrB, int colorFactor, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2); // jxl_stage_lf_dequant (LFCoefficients)
    // the LF image of a frame as the picture at 1:8 in one launch. heads = per LF group {lfgY, lfgX, cellsH, cellsW, extraPrecision,
    // xFactorLF, bFactorLF, adaptiveSmoothing}; scaledDequant = 3 floats per group; ints = every group's X, Y, B planes back to back;
    // xyb = null or {matrix[9], opsinBias[3], cbrtOpsinBias[3], intensityTarget}; o0..o2 all null: the planes stay resident
    public native void lfImage(int[] heads, float[] scaledDequant, ByteBuffer ints, int cellsH, int cellsW, float baseCorrX, float baseCorrB,
        int colorFactor, float[] xyb, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2);   // jxl_stage_lf_image / jxl_planes_from_lf
    public native void stageXyb(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, long n, float[] matrix, float[] opsinBias, float[] cbrtOpsinBias,
        float intensityTarget);                                    // jxl_stage_xyb (OpsinInverseMatrix.invertXYB)
    public native void stageYcbcr(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, long n);               // jxl_stage_ycbcr
    public native void stageTransfer(ByteBuffer in, long n, int transfer, int maxValue, ByteBuffer outF, ByteBuffer outI); // jxl_stage_transfer
    /** params: struct jxl_color_params packed by the caller (4-byte fields, C layout); i1, i2 / o1, o2 null for one plane. */
    public native void stageColorConvert(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, long n, ByteBuffer params, ByteBuffer o0, ByteBuffer o1,
        ByteBuffer o2);                                            // jxl_stage_color_convert (JXLImage.transform)
    public native float stageColorPeak(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, int h, int w, ByteBuffer params); // jxl_stage_color_peak
    /** tm: struct jxl_tone_map packed by the caller (7 four-byte fields) arms HDR to SDR tone mapping in the colour passes, null clears it. */
    public native void setToneMap(ByteBuffer tm);                  // jxl_ctx_set_tone_map
    public native void stageInvHSqueeze(ByteBuffer avg, int aw, ByteBuffer res, int rw, int h, ByteBuffer out); // jxl_stage_inv_hsqueeze
    public native void stageInvVSqueeze(ByteBuffer avg, int ah, ByteBuffer res, int rh, int w, ByteBuffer out); // jxl_stage_inv_vsqueeze
    public native void stageRct(ByteBuffer v0, ByteBuffer v1, ByteBuffer v2, long n, int rctType);    // jxl_stage_rct
    // Palette branch of ModularStream.applyTransforms (ModularStream.java:327-378): params = {numC, nbColors, nbDeltas, dPred, bitDepth};
    // index / pred (or null): height * width ints; palette: channel 0 of the stream (palH x palW); out: numC planes, out[0] may be index
    public native void stagePalette(ByteBuffer index, int height, int width, ByteBuffer palette, int palH, int palW, ByteBuffer pred,
                                    int[] params, ByteBuffer[] out);                                    // jxl_stage_palette
    public native void stageModularToFloat(ByteBuffer a, ByteBuffer b, long n, float scale, ByteBuffer out); // jxl_stage_modular_to_float
    public native void stageChromaUpsample(ByteBuffer in, int h, int w, int xShift, int yShift, ByteBuffer out); // jxl_stage_chroma_upsample
    /** JXLCodestreamDecoder.computePatches (:212-254) on host planes, in place, as one kernel launch: frame[d] direct buffers of
     *  height x width samples (frameType[d]: 0 float, 1 int), ref[k * channels + d] = plane d of reference[k]
     *  (null or refType -1: reads as zeros), pos = 8 ints per position in stage order (y0, x0, h, w, ref, refY0, refX0, blend row),
     *  blend = rows of channels x (mode, alphaChannel, clamp), refShape = (h, w) per slot, (0, 0) for reference[k] == null. The
     *  planes carry the types blendBuffers' casts (:433-465) would have given them. */
    public native void stagePatches(ByteBuffer[] frame, int[] frameType, int height, int width, ByteBuffer[] ref, int[] refType, int[] pos,
                                    int[] blend, int nColor, int[] ecIsAlpha, int[] ecAlphaAssociated, int[] refShape); // jxl_stage_patches
    /** host only: computePatches' checks and the tile lists: { tiles, entries, tile[], start[tiles + 1], list[entries] } */
    public static native int[] patchBins(int height, int width, int[] frameType, int[] refType, int[] pos, int[] blend, int nColor,
                                         int[] ecIsAlpha, int[] ecAlphaAssociated, int[] refShape);                    // jxl_patch_bins
    public native void stageSplines(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, int height, int width, int quantAdjust, int[] nControl,
                                    int[] control, int[] coeff, float baseCorrX, float baseCorrB);   // jxl_stage_splines
    /** host only: the arcs Spline.renderSpline draws, 12 ints per arc (jxl_spline_arc; floats as raw bits) */
    public static native int[] splineArcs(int height, int width, int quantAdjust, int[] nControl, int[] control, int[] coeff,
                                          float baseCorrX, float baseCorrB);                         // jxl_spline_arcs
    public static native float[] upsamplingWeights(int k, float[] packed);                            // jxl_upsampling_weights
    public native void stageUpsample(ByteBuffer in, int h, int w, int k, float[] weights, ByteBuffer out); // jxl_stage_upsample
    public native void stageNoiseInit(int h, int w, int groupDim, long seed0, int colors, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2); // jxl_stage_noise_init
    public native void stageNoiseAdd(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, ByteBuffer n0, ByteBuffer n1, ByteBuffer n2, long n,
        float[] lut, float baseCorrX, float baseCorrB);            // jxl_stage_noise_add
    // p0..p2: the window at (y0, x0) of a frameH x frameW frame, h x w floats each, in place
    public native void stageNoiseWindow(ByteBuffer p0, ByteBuffer p1, ByteBuffer p2, int h, int w, int groupDim, long seed0, float[] lut,
        float baseCorrX, float baseCorrB, int frameH, int frameW, int y0, int x0); // jxl_stage_noise_window
    /** rect: {h, w, canvasY, canvasX, frameY, frameX, refY, refX}. */
    public native void stageBlend(int mode, int flags, boolean isInt, ByteBuffer canvas, int ch, int cw, ByteBuffer frame, int fh, int fw,
        ByteBuffer ref, int rh, int rw, ByteBuffer frameAlpha, ByteBuffer refAlpha, int[] rect); // jxl_stage_blend
    public native void stageOrient(ByteBuffer in, int h, int w, int orientation, ByteBuffer out);     // jxl_stage_orient
    /** params: {height, width, nColor, hasAlpha, premultiplied, bitDepth, bigEndian, isInt[4], taggedDepth[4]}. */
    public native void stagePack(ByteBuffer[] planes, int[] params, ByteBuffer out);                  // jxl_stage_pack
    // the PNG's samples in one pass: params = struct jxl_png_params in a direct buffer; i1, i2, alpha may be null
    public native void stagePngSamples(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer alpha, ByteBuffer params,
            ByteBuffer out);                                                                          // jxl_stage_png_samples
    public native void planesPngSamples(ByteBuffer alpha, ByteBuffer params, ByteBuffer out);         // jxl_planes_png_samples
    public native float planesColorPeak(ByteBuffer params);                                           // jxl_planes_color_peak
    public native void planesOrient(int orientation);                                                 // jxl_planes_orient
    // the PFM's samples in one pass: params = {height, width, n_planes, is_int[3], tagged_depth[3]}; i1, i2 null for a grey image;
    // out holds exactly 4 * n_planes * width * height bytes
    public native void stagePfmSamples(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, int[] params, ByteBuffer out);  // jxl_stage_pfm_samples
    public native void planesPfmSamples(int[] params, ByteBuffer out);                                // jxl_planes_pfm_samples
    // Frame.drawVarblocks (Frame.java:464-503; JXLCodestreamDecoder.java:638-639): blocks = nBlocks x (cy, cx, type) in frame cells
    // (block.y + (lfGroupRow << 8), block.x + (lfGroupColumn << 8), dctSelect[block.y][block.x].type) on a cellsH x cellsW grid
    public native void stageVarblocks(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, int height, int width, int[] blocks, int nBlocks,
                                      int cellsH, int cellsW, ByteBuffer o0, ByteBuffer o1, ByteBuffer o2);   // jxl_stage_varblocks
    public native void planesVarblocks(int[] blocks, int nBlocks, int cellsH, int cellsW);            // jxl_planes_varblocks

    // ---- device plane sets: the canvas and the reference frames on the device; a set is addressed by its id
    public native int canvasCreate(int h, int w, int[] types);     // jxl_canvas_create (types: 0 float, 1 int32 per plane)
    public native void canvasDestroy(int id);                      // jxl_canvas_destroy
    public native int[] canvasDescribe(int id);                    // jxl_canvas_describe -> {n, h, w, type[n]}
    public native int canvasClone(int id);                         // jxl_canvas_clone
    public native void canvasUpload(int id, int plane, ByteBuffer src, int type);   // jxl_canvas_upload (src: h * w samples)
    public native int canvasDownload(int id, int plane, ByteBuffer dst);            // jxl_canvas_download -> the plane's type
    public native int canvasFromPlanes(int[] extraTypes);          // jxl_canvas_from_planes (extraTypes may be null)
    public native void canvasCast(int id, int plane, int depth);   // jxl_canvas_cast
    /** desc: {canvas, frame, ref, nChan, rect[8] as stageBlend's, then per channel {framePlane, mode, flags, frameAlpha, refAlpha}}. */
    public native void canvasBlend(int[] desc);                    // jxl_canvas_blend
    public native void canvasToPlanes(int id);                     // jxl_canvas_to_planes
    /** desc: {height, width, nPlanes, then per plane {channel, addChannel (-1: none), type}}; scales: one float per plane. */
    public native int canvasFromModular(int[] desc, float[] scales);   // jxl_canvas_from_modular -> the new set's id
    /** The same channels as upsampled float planes (Frame.performUpsampling of castToFloat of each, Frame.java:217-260): desc and
     *  scales as canvasFromModular's, every type 0 (float); k 2, 4 or 8; weights: k * k * 25 floats as planesUpsample's. */
    public native int canvasFromModularUp(int[] desc, float[] scales, int k, float[] weights);   // jxl_canvas_from_modular_up -> the new set's id
    public native void canvasTakePlanes(int id);                   // jxl_canvas_take_planes (canvasToPlanes' inverse: planes 0..2 <- the resident planes)
    public native void canvasOrient(int id, int orientation);      // jxl_canvas_orient
    // the writers on a set: params as the stage entries'; nothing goes up
    public native void canvasPngSamples(int id, int alphaPlane, ByteBuffer params, ByteBuffer out);   // jxl_canvas_png_samples (alphaPlane -1: none)
    public native float canvasColorPeak(int id, ByteBuffer params);                                   // jxl_canvas_color_peak
    public native void canvasPfmSamples(int id, int[] params, ByteBuffer out);                        // jxl_canvas_pfm_samples (out: exactly 4 * n_planes * width * height bytes)
    // the image as a device tensor in one pass: params = struct jxl_tensor_params in a direct buffer; out = the DEVICE address of
    // height * width * channels elements (the library refuses anything that is not device memory of its device, or too short)
    public native void stageTensorSamples(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer alpha, ByteBuffer params,
            long out);                                                                                // jxl_stage_tensor_samples
    public native void planesTensorSamples(ByteBuffer alpha, ByteBuffer params, long out);            // jxl_planes_tensor_samples
    public native void canvasTensorSamples(int id, int alphaPlane, ByteBuffer params, long out);      // jxl_canvas_tensor_samples (alphaPlane -1: none)
    // the same, resampled to a given size in the pass: resize = struct jxl_resize_params in a direct buffer (the source box, the
    // tensor's size, the filter); params' height / width stay the source planes'; out holds out_height x out_width pixels
    public native void stageTensorResized(ByteBuffer i0, ByteBuffer i1, ByteBuffer i2, ByteBuffer alpha, ByteBuffer params,
            ByteBuffer resize, long out);                                                             // jxl_stage_tensor_resized
    public native void planesTensorResized(ByteBuffer alpha, ByteBuffer params, ByteBuffer resize, long out);  // jxl_planes_tensor_resized
    public native void canvasTensorResized(int id, int alphaPlane, ByteBuffer params, ByteBuffer resize, long out);  // jxl_canvas_tensor_resized
    // n images into one batch tensor in ONE launch: heads = 3 ints per item {source (0 host planes, 1 the resident planes, 2 a set),
    // set id, alpha plane}; params / resize = n jxl_tensor_params / jxl_resize_params back to back; the host planes of all items in
    // one direct buffer `planes` (null when no item names one), offsets = 4 longs per item: the byte offsets of its three colour
    // planes and its alpha plane there, -1: none. Item i is written at out + i * (one tensor's bytes); all or nothing
    public native void tensorResizedBatch(int[] heads, ByteBuffer planes, long[] offsets, ByteBuffer params, ByteBuffer resize,
            long out);                                                                                // jxl_tensor_resized_batch
    /** shapes: {n, h, w, type[n]}; ref null when desc names no reference. Throws what canvasBlend would; no device needed. */
    public static native void canvasBlendCheck(int[] desc, int[] canvas, int[] frame, int[] ref);    // jxl_canvas_blend_check

    /** items: 3 ints per plane {set, plane, depth}, each (set, plane) once, at most 80 planes: ImageBuffer.castToFloat(depth) of all
     *  of them in one launch; float planes are skipped. */
    public native void canvasCastPlanes(int[] items);              // jxl_canvas_cast_planes
    /** computePatches on plane sets: frameSet holds the frame's nColor + ecIsAlpha.length planes, refSet the set id of each of the
     *  four reference slots (-1: absent); pos, blend, ecIsAlpha, ecAlphaAssociated as stagePatches'. colorsResident != 0: planes 0..2
     *  of the frame are the resident planes. One launch, asynchronous; no plane crosses the bus. */
    public native void canvasPatches(int frameSet, int colorsResident, int[] refSet, int[] pos, int[] blend, int nColor, int[] ecIsAlpha,
                                     int[] ecAlphaAssociated);     // jxl_canvas_patches
    /** What canvasPatches would throw; no device needed. frame: {n, h, w, type[n]}; refs: 4 x 19 ints, per slot {n, h, w, type[16]}
     *  with n == 0 for an absent slot and n == -1 for a slot that is the frame set itself. Returns -1. */
    public static native int canvasPatchesCheck(int[] frame, int colorsResident, int[] refs, int[] pos, int[] blend, int nColor,
                                                int[] ecIsAlpha, int[] ecAlphaAssociated);   // jxl_canvas_patches_check

    // ---- Modular: plan once (begin), run, read channel by channel
    public static native int[] modularDefaultSqueezeParams(int[] widths, int[] heights, int nbMeta);  // jxl_modular_default_squeeze_params
    public static native int[] modularSqueezedShapes(int[] widths, int[] heights, int[] squeezeParams); // jxl_modular_squeezed_shapes
    public native void modularBegin(ByteBuffer[] chans, int[] widths, int[] heights, int[] squeezeParams, int rctType, int rctBegin); // jxl_modular_begin
    /** any frame-level chain as one plan: transforms = 8 ints per transform in bitstream order (kind, begin_c, num_c, rct_type,
     *  nb_colors, nb_deltas, d_pred, n_sp), squeezeSteps = the expanded steps of every Squeeze, 4 ints each, back to back */
    public native void modularBeginChain(ByteBuffer[] chans, int[] widths, int[] heights, int[] transforms, int[] squeezeSteps, int bitDepth); // jxl_modular_begin_chain
    public native void modularRun();                               // jxl_modular_run
    public native int modularOutCount();                           // jxl_modular_out_count
    public native int[] modularOutShape(int idx);                  // jxl_modular_out_shape -> {width, height}
    public native void modularReadChannel(int idx, ByteBuffer dst); // jxl_modular_read_channel
    public native int modularLastLaunchCount();                    // jxl_modular_last_launch_count
    public native int modularRedoCount();                          // jxl_modular_redo_count
    /** channels: one direct buffer per encoded channel; squeezeParams: 4 ints per step. */
    public native void modularApply(ByteBuffer[] chans, int[] widths, int[] heights, int[] squeezeParams, int rctType,
        int rctBegin, ByteBuffer[] out, int[] outWidths, int[] outHeights); // jxl_modular_apply
}
