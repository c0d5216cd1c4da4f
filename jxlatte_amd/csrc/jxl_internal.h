// Internal declarations shared by the HIP translation units of libjxlatte_amd.so.
// gfx950 (MI355X) only. All device arithmetic is strict IEEE f32: the library is built with
// -ffp-contract=off (no FMA contraction), default correctly-rounded f32 division, f32
// denormals preserved -- required for bit-exact parity with the Java reference.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <cmath>
#include <stdint.h>
#include "../../include/jxlatte_amd.h"
#include "../../include/jxl_transform_types.h"
#include "plane_tiled.h"
#include "blend_ops.h"
#include "patch_compile.h"
#include "modchain_check.h"
#include "image_home.h"
#include "tone_map_ops.h"

namespace jxl {

// total floats of the cosine LUT for sizes 1..256: sum (s-1)*s
constexpr int kLutTotal = 86870;

// One varblock, frame coordinates. 16 bytes (one dwordx4 load).
struct DevBlock {
    uint16_t cy, cx;    // top-left cell (8x8 px units) in the frame
    uint32_t type;      // TransformType.type
    uint32_t cfl_zero;  // bit (ty*5+tx): CfL factors of that 64x64 tile (relative to the block's first
                        // tile) read as 0 for this block -- the reference's per-group xFactors cache has
                        // not been filled yet when this block is visited (HFCoefficients.java:159-181)
    int32_t hf_mul;     // HFMetadata.hfMultiplier of the block's first cell: carried here so that the kernels do not
                        // chain a second dependent load behind the block record
};

// One workgroup's share of a type-uniform launch.
static_assert(sizeof(DevBlock) == 16, "one dwordx4 per block record");

// One workgroup's share of a type-uniform launch.
struct WorkItem {
    uint32_t type;
    uint32_t first;  // index into the binned DevBlock array
    uint32_t count;  // blocks handled by this workgroup
};

// Device-resident view of one VarDCT frame (all pointers are device pointers).
struct DevFrame {
    int32_t no_cfl;         // chroma-subsampled frame: chroma-from-luma is skipped (HFCoefficients.java:149-151) and the
                            // geometry below is the one of the channel the launch handles
    int32_t width, height;  // padded px
    int32_t bw, bh;         // cells
    int32_t tw, th;         // 64x64 tiles
    const int32_t* coeff[3];
    const float* lf[3];     // [bh][bw]
    const float* llf[3];    // [bh][bw]: lf with the LLF coefficients of blocks larger than 8x8 (k_llf)
    const int32_t* hf_mul;  // [bh][bw]
    const int32_t* sharpness;
    const float* kx_tab;  // [th][tw]: baseCorrelationX + xFromY / colorFactor per 64x64 tile (HFCoefficients.java:177-181),
    const float* kb_tab;  //           computed once per frame on the host (same IEEE float division and addition)
    const float* weights;     // flat, reciprocal
    const float* weights_t;   // same offsets, every matrix transposed (for flip() blocks: coalesced reads)
    int32_t woffs[51];
    const float* lut;         // cosine LUT, all sizes; size s=1<<l starts at lut_off(l)
    const float* dq_tab;      // [kWg3DqTabFloats]: the dequantisation tables of the persistent launch (wg3_build_tables), per frame
    float scale_factor[3];
    float quant_bias[3];
    float quant_bias_numerator;
    float base_corr_x, base_corr_b;
    float color_factor_f;     // (float)colorFactor
};

// Layout of the quantised-coefficient planes on the device (r4): tiled by 8x8 cell. The 64 samples of cell (by, bx) of a
// plane W samples wide are consecutive, row-major, at ((by * (W / 8) + bx) * 64 -- a varblock's rows then share cache lines
// (an 8x8 block is two whole 128-byte lines instead of eight quarter lines), which is what the launches that handle one
// transform type at a time need: in a raster plane they fetched 1.5-3.7 times the bytes they used (profiles/r4_rocprof_summary).
// The C ABI still speaks raster planes; the writers (k_store2d_tiled / k_widen2d* in host.hip) do the re-tiling. Runs of up to
// 8 samples that start at a multiple of 4 (8) stay inside one cell row, so 16- and 32-byte loads are unaffected.
__host__ __device__ __forceinline__ int64_t coeff_off(int W, int py, int px) {
    return (((int64_t)(py >> 3) * (W >> 3) + (px >> 3)) << 6) + (((py & 7) << 3) | (px & 7));
}

__host__ __device__ inline int lut_off(int l) {
    // sum_{j<l} (2^j - 1) * 2^j
    int o = 0;
    for (int j = 0; j < l; j++) o += ((1 << j) - 1) << j;
    return o;
}

struct EpfParams {
    float channel_scale[3];
    float sigma_scale;   // stepMultiplier * pass scale for this iteration
    float border_sad_mul;
    float inv_sigma_modular;
};

struct XybParams {
    float sm[9];         // matrix * itScale
    float ob[3];         // opsinBias
    float cob[3];        // -cbrtOpsinBias
};

// Argument block of a merged IDCT launch (k_idct_multi): a few type-uniform segments of work items, in launch order.
struct MultiArgs {
    static constexpr int kMaxSeg = 12;
    DevFrame f;
    const DevBlock* blocks;
    const WorkItem* items;  // (no reader left: items are implicit, see below)
    int n_seg;
    int seg_b0[kMaxSeg + 1];  // first workgroup of segment k (a multiple of 8); seg_b0[n_seg] = grid size
    int seg_n[kMaxSeg];       // items in segment k
    int seg_type[kMaxSeg];    // TransformType.type of segment k
    int seg_first[kMaxSeg];   // first block of the type in `blocks`
    int seg_nblocks[kMaxSeg]; // blocks of the type
    int nch, ch0;             // channels per block group (always 1: a chroma-subsampled frame's per-channel launch), the channel
    float *o0, *o1, *o2;
};
// work items are implicit: item i of a segment = block group i of channel ch0, a group being medium_blocks_per_wg(type)
// consecutive blocks (no item table to load before the block records)
struct IdctSegment { int type, first_block, n_blocks; };

// Argument block of the persistent three-channel IDCT launch (k_idct_wg3.hip): type-uniform segments in launch order
struct Wg3Seg { int type, first_block, n_blocks, item_base; };  // item_base: index of the segment's first work item in the launch
struct Wg3Args {
    static constexpr int kMaxSeg = 21;
    DevFrame f;
    const DevBlock* blocks;
    float *o0, *o1, *o2;
    int n_seg, total_items;
    int img_floats;  // floats of the largest three-channel LDS image among the segments' types (the tables follow it)
    int llf_in_item;  // always 1: the items transform their blocks' LF patches themselves (finalizeLLF)
    // the item list: 32-byte records {type, first_block, n_blocks, geometry word (wg3_geo), weight offsets of the three channels, 0},
    // total_items of them, in the order the workgroups take them (wg3_item_table: spatial, dealt to the XCDs, cost-balanced)
    const int* items;
    Wg3Seg seg[kMaxSeg];
    int tiled; // the output planes are cell-tiled (plane_tiled.h): the 256-thread class only, pooled planes only (run_frame)
};

// The two tables the persistent launch keeps in LDS, as a function of the seven floats they depend on: [3][128] dequantised value of
// q = -64 .. 63 (entry q + 64: 0, +-quantBias[c], (float)q - quantBiasNumerator / (float)q, HFCoefficients.java:309-315), then
// [3][256] scaleFactor[c] / (float)m for hfMultiplier m = 1 .. 255 (entry 0 as m = 1; :299). Built on the host once per frame
// description with the expressions the workgroups used to evaluate themselves (correctly rounded f32 division on both sides).
constexpr int kWg3DqTabFloats = 3 * 128 + 3 * 256;
void wg3_build_tables(const float quant_bias[3], float quant_bias_numerator, const float scale_factor[3], float* out /* [kWg3DqTabFloats] */);
// the item list of one class's segments in spatial order, dealt to the XCDs in runs (host side)
void wg3_item_table(const DevBlock* host_blocks, int frame_bw, const IdctSegment* segs, int n_seg, int which, const int32_t* woffs,
                    std::vector<int>& out, int grid);
int wg3_grid_cap(bool big);  // workgroups of a single-frame launch (JXL_WG3_GRID / JXL_WG3_GRID_BIG)
bool wg3_handles(int type);  // every type but the 128/256-edge ones (frames without chroma subsampling)
bool wg3_big(int type);  // 64x32 / 32x64: the 512-thread launch (register / LDS class)
int build_wg3_args(const DevFrame& f, const DevBlock* blocks, const IdctSegment* segs, int n_seg, int which, float* const out[3],
                   Wg3Args& a, bool tiled = false);
void launch_idct_wg3(const Wg3Args& a, bool big, int grid_cap, hipStream_t s);
size_t wg3_lds_bytes(const Wg3Args& a);
void launch_idct_wg3_batch(const Wg3Args* dev_args, int n_frames, bool big, int grid_x, size_t lds, hipStream_t s);


// ---- launchers (defined in the kernel TUs) ---------------------------------------------------
// Chroma-subsampled frames: one launch per register class (0: every type up to 32x32, 1: the 64-point family) and channel ch,
// 256-thread workgroups. An item covers up to medium_blocks_per_wg(type) blocks of that channel.
int idct_class_of(int type);
void launch_idct_multi(const DevFrame& f, const DevBlock* blocks, int cls, const IdctSegment* segs, int n_seg, int ch,
                       float* const out[3], hipStream_t s);
// the special 8x8-footprint types: items of up to 64 blocks (one per lane) of one channel, WorkItem.type = TransformType.type | channel << 8
void launch_idct_special(const DevFrame& f, const DevBlock* blocks, const WorkItem* items, int n_items, float* const out[3], hipStream_t s);
int medium_blocks_per_wg(int type);
// finalizeLLF of blocks[first..first+count) (all larger than 8x8) into the llf planes
void launch_llf(const DevFrame& f, const DevBlock* blocks, int first, int count, float* const llf[3], hipStream_t s);
// large (128/256-edge) blocks: `first..first+count` of `blocks`; scratch planes same shape as out
void launch_idct_large(const DevFrame& f, const DevBlock* blocks, const DevBlock* host_blocks, int first, int count,
                       float* const out[3], float* const scratch[3], hipStream_t s, int* n_launches);
void launch_accumulate(int32_t* dst, const int32_t* src, int64_t n, hipStream_t s);

// ---- sparse coefficient feed (k_sparse.hip): lists of (position, value) entries scattered into the tiled planes ----
// One run of entries of one (group, channel), as the scatter kernel sees it: 16 bytes, so that the table of a whole 4K frame
// (1 215 runs) sits in LDS. The run's geometry (plane, origin, gw, gh) is recomputed from group / channel and SparseGeom.
struct SparseRec {
    uint32_t chunk_first;  // prefix sum: index of the run's first 16-byte chunk among the launch's chunks
    uint32_t chunk_src;    // where that chunk is: in 16-byte units from the base of source `src`
    uint32_t count_wide;   // entries of the run | wide form << 31
    uint32_t where;        // group | channel << 24 | source << 26
};
static_assert(sizeof(SparseRec) == 16, "one dwordx4 per run record");
constexpr int kSparseMaxRuns = 2048;  // run records of one launch (32 KB of LDS); longer run lists take more launches
struct SparseGeom {
    int32_t* plane[3];      // the tiled coefficient planes (coeff_off)
    int32_t W, H;           // padded frame
    int32_t sx[3], sy[3];   // jpeg upsampling shifts per channel
};
// the rectangle of `group` in channel ch's own geometry (Frame.getGroupLocation / getGroupSize, Frame.java:883-905)
struct SparseRect { int32_t W, y0, x0, gw, gh; };
__host__ __device__ inline SparseRect sparse_rect(int W, int H, int sx, int sy, int group) {
    const int grs = (W + 255) >> 8, gy = group / grs, gx = group - gy * grs;
    const int gh = H - gy * 256 < 256 ? H - gy * 256 : 256, gw = W - gx * 256 < 256 ? W - gx * 256 : 256;
    return SparseRect{W >> sx, (gy * 256) >> sy, (gx * 256) >> sx, gw >> sx, gh >> sy};
}
// entries at positions outside [0, gh) x [0, gw) (a wide entry: also any bit above the low 16 of its position word)
bool sparse_entries_valid(const uint32_t* words, int32_t n_entries, bool wide, int gw, int gh);
// n_recs <= kSparseMaxRuns records (host memory: copied into the launch's arguments when n_recs <= 3, else `recs_dev` is
// their device-visible address), total_chunks = sum of their chunks; src[k] device-visible bases of the entry words
void launch_sparse_scatter(const SparseGeom& g, const SparseRec* recs, const SparseRec* recs_dev, int n_recs, uint32_t total_chunks,
                           const void* const src[3], unsigned long long* rejected, int grid, hipStream_t s);
// zero the rectangles of `group` in the three planes (a pass-0 put over a group that has been written before)
void launch_sparse_clear(const SparseGeom& g, int group, hipStream_t s);

void launch_gab(const float* const in[3], float* const out[3], int h, int w, const float w1[3], const float w2[3],
                hipStream_t s);
void launch_epf_sigma(const int32_t* hf_mul, const int32_t* sharpness, int bh, int bw, float global_scale_f,
                      const float sharp_lut[8], float* inv_sigma, int* bad_flag, hipStream_t s);
void launch_epf_iter(const float* const in[3], float* const out[3], int h, int w, int iter, const float* inv_sigma,
                     const EpfParams& p, hipStream_t s);
void launch_xyb(float* const planes[3], int64_t n, const XybParams& p, hipStream_t s);
void launch_ycbcr(float* const planes[3], int64_t n, hipStream_t s);
// transfer + quantise: out elem size 4 (float or int32), 2 (u16), 1 (u8)
// out index = i * out_pitch + out_off (pitch 1 = planar; pitch 3, off c = pixel-interleaved)
// pq_tab: the PQ segment table of build_pq_table (device; null: the double-precision form)
void launch_transfer(const float* in, int64_t n, int transfer, int max_value, void* out, int out_elem, hipStream_t s,
                     int out_pitch = 1, int out_off = 0, const float* pq_tab = nullptr, const float* srgb8_tab = nullptr,
                     const float* pq16_thr = nullptr, const float* srgb16_tab = nullptr);
// colour management in one pass (k_color.hip): jxl_color_params as the kernels see it. All pointers are device pointers.
struct ColorArgs {
    const void* in[3];  // n_planes planes of float or int32 samples
    void* out[3];       // float, or int32 when max_value > 0; three planes when n_planes == 3, use_matrix or use_tone_map, else one
    int64_t n;
    int n_planes, in_is_int;
    float in_scale[3];  // 1.0f / in_max[c] (ImageBuffer.castToFloat0)
    int tf_in, kind_in;  // JXL_TF_*; kind_*: the exponent of a GAMMA curve is 0 no integer, 1 an even, 2 an odd integer
    double p_in;         // GAMMA: 1e7 / gamma_in
    int use_scale;
    float scale;
    int use_matrix;
    float m[9];
    int tf_out, kind_out;
    double p_out;  // GAMMA: 1e-7 * gamma_out
    int max_value;
    const float* pq_tab;      // the tables jxl_stage_transfer would use for (tf_out, max_value), or null
    const float* srgb8_tab;
    const float* pq16_thr;
    const float* srgb16_tab;
    int use_tone_map;  // tone_map_ops.h behind the matrix, instead of the scale; three planes out, as with use_matrix
    ToneMapArgs tm;
};
void launch_color_convert(const ColorArgs& a, hipStream_t s);
// determinePeak over h rows of w samples (w <= 2^30): *result, zeroed by the caller, receives an order-preserving uint32 key of
// the peak (host.hip: color_peak_value)
void launch_color_peak(const ColorArgs& a, int h, int w, uint32_t* result, hipStream_t s);
// the PNG's samples from the colour planes in one pass (k_png.hip): stages 1-6 of ColorArgs (out[], max_value and the integer
// tables are not looked at), then PNGWriter's coercion, un-premultiplication, quantisation and interleaving
struct PngArgs {
    ColorArgs c;
    const void* alpha;  // device plane of c.n float or int32 samples, or null
    int alpha_is_int;
    int alpha_coerce;   // an int32 alpha plane is cast to float first (PNGWriter.java:79-88), else clamped as it is
    float alpha_scale;  // 1.0f / maxValue(tagged depth)
    int premultiplied, bit_depth, big_endian;
    void* out;          // c.n * (n_color + (alpha != null)) samples of bit_depth / 8 bytes
};
// n_color: 3 when c.n_planes == 3, c.use_matrix or c.use_tone_map, else 1
void launch_png_samples(const PngArgs& p, int n_color, hipStream_t s);
// the image as a device tensor in one pass (k_tensor.hip): stages 1-6 and the alpha rule of PngArgs (g.bit_depth 8; g.out is not
// looked at), then un-premultiplication, normalisation and the conversion to `dtype`, stored CHW or HWC
struct TensorArgs {
    PngArgs g;
    int dtype, layout;      // JXL_TENSOR_*
    int n_out;              // output channels: n_color, + 1 when alpha is written
    int use_norm;
    float mean[4], inv_std[4];
    int wide;               // every group of a lane's 4 pixels may leave as vector stores (tensor_wide_ok); else sample by sample
    void* out;              // device memory, element-aligned: c.n * n_out elements
};
// max_workgroups > 0: a smaller grid bound than the kernel's own (tests reach the grid-stride loop at a small size)
void launch_tensor_samples(const TensorArgs& p, hipStream_t s, int max_workgroups = 0);
// the image resampled to a device tensor in one pass (k_tensor_resize.hip): stages 1-5 per source pixel, the separable filter of
// the tap tables (vertical pass first), then stage 6 and TensorArgs' tail per output pixel. t.g.c.n is the SOURCE planes' size,
// t.out holds oh * ow * n_out elements (t.wide is not looked at)
struct ResizeArgs {
    TensorArgs t;
    int src_w;                   // the planes' row pitch in samples
    int x0, y0;                  // the box's first column and row
    int oh, ow;
    int tw, th;                  // the output tile of a workgroup: tw * th <= 256, th <= 4
    int planes;                  // colour planes (n_color) + 1 when the alpha plane is read
    int lds_w;                   // floats of one (tile row, plane) line of the LDS image (tensor_resize_check.h: resize_tile_fits)
    int lds_bytes;
    int skew;                    // the LDS column of footprint column x is x + (x >> 5), else x
    int wide_in;                 // every plane row starts 16-byte aligned: 16-byte loads (resize_wide_in_ok)
    const int32_t *yfirst, *yoff, *xfirst, *xoff;  // device: first[O] relative to the box, off[O + 1]
    const float *wy, *wx;                          // device: the f32 weights, packed
};
void launch_tensor_resize(const ResizeArgs& r, hipStream_t s);
// N images in one launch (k_tensor_resize_batch.hip): items[n] with their t.out set, tile_base[n + 1] the prefix sum of their tile
// counts, counts[0] = n -- all device pointers; dtype and n_color are the batch's, lds_bytes the largest of the items'
void launch_tensor_resize_batch(const ResizeArgs* items, const int64_t* tile_base, const int32_t* counts, int dtype, int n_color,
                                unsigned grid, int lds_bytes, hipStream_t s);
// the PFM's samples from the image's planes in one pass (k_pfm.hip): cast of the int32 planes, floatToIntBits, big-endian words,
// channels interleaved, rows bottom to top (PFMWriter.java:22-49)
struct PfmArgs {
    const void* in[3];  // device planes of h * w float or int32 samples; [0, n_planes) are read
    int h, w;
    int n_planes;       // 1 or 3
    int is_int[3];      // the plane holds int32 samples
    float scale[3];     // 1.0f / max of the plane's tagged depth (int32 planes)
    void* out;          // h * w * n_planes words
};
void launch_pfm_samples(const PfmArgs& p, hipStream_t s);
// Frame.drawVarblocks (Frame.java:464-503) on three float planes, in place (k_varblocks.hip); the cell map and the factors are
// varblock_check.h's
struct VarblockArgs {
    float* pl[3];          // device planes of h * w floats
    int h, w;
    const uint8_t* map;    // cells_h * cells_w bytes: type | top-row bit | left-column bit, or 0xFF
    int cells_h, cells_w;
    const float* factors;  // 27 x 3: rFactor, gFactor, bFactor per type
};
void launch_varblocks(const VarblockArgs& p, hipStream_t s);
// The inverse Palette transform (ModularStream.java:327-378) on device planes (k_palette.hip); the arithmetic is palette_ops.h's,
// the checks palette_check.h's
constexpr int kPaletteLdsInts = 8192;      // a palette of at most this many entries (num_c * nb_colors) is staged in LDS: 32 KiB
constexpr int kPaletteChainThreads = 256;  // k_palette_chain's workgroup: that many rows of one t-front per pass
// (the fused run's budget, kPaletteRunLdsInts = 12288 entries for all palettes of a run together, and its stage / depth / output
// limits stand in modchain_check.h: the plain header that decides which runs are fused needs them without this one)
constexpr int kPaletteRunMaxGrid = 2048;   // k_palette_run's grid bound: 8 workgroups per CU, each stages the run's palettes once
struct PaletteArgs {
    const int32_t* index;     // h * w
    const int32_t* palette;   // num_c rows of nb_colors, pal_pitch apart
    int32_t pal_pitch;        // >= nb_colors (jxl_stage_palette: back to back; a plan: the palette channel's own width)
    const int32_t* pred;      // h * w, or null
    int32_t* out;             // num_c planes, plane_stride apart
    int64_t plane_stride;     // >= h * w, a multiple of 4
    int h, w;
    int num_c, nb_colors, nb_deltas, d_pred, bit_depth;
    unsigned int* delta_count;  // += the pixels with index < nb_deltas (zeroed by the caller)
};
void launch_palette_lookup(const PaletteArgs& p, hipStream_t s);
void launch_palette_chain(const PaletteArgs& p, hipStream_t s);  // only where d_pred is neither 0 nor 6 and the count is not 0
// A run of consecutive inverse Palette transforms as one launch (k_palette_run.hip); the table is modchain_check.h's
struct PaletteRunStage {
    const int32_t* palette;  // the device copy of the palette channel: num_c rows, pal_w apart
    int32_t pal_w, num_c, nb_colors, nb_deltas;
    int32_t chained;         // 1: a delta pixel of this stage needs its neighbours (d_pred neither 0 nor 6)
    int32_t lds_off;         // where the stage's num_c * nb_colors entries start in LDS
};
struct PaletteRunOut {
    int32_t* plane;                                        // n samples, 16-byte aligned
    int32_t depth;                                         // 1 .. kPalRunMaxDepth
    int32_t stage[kPalRunMaxDepth], row[kPalRunMaxDepth];  // the lookups from the source to this plane, in order
};
struct PaletteRunArgs {
    const int32_t* src;    // n samples, 16-byte aligned
    int64_t n;
    int32_t n_stage, n_out, bit_depth, lds_ints;
    unsigned int* impure;  // += the workgroups that met a delta pixel of a chained stage (zeroed by the caller)
    PaletteRunStage st[kPalRunMaxStages];
    PaletteRunOut out[kPalRunMaxOut];
};
void launch_palette_run(const PaletteRunArgs& p, hipStream_t s);
// PQ as a table of quadratic segments (jxl_fastpow.h): kPqTableFloats floats = float4 {a0 hi, a0 lo, a1, a2} per segment
constexpr int kPqTableFloats = (129 - 87) * 128 * 4;
void build_pq_table(float* out /* [kPqTableFloats] */);
constexpr int kSrgb8TableFloats = (127 - 118) * 128 * 4;
bool build_srgb8_table(float* out /* [kSrgb8TableFloats] */);  // false: a segment with more than three thresholds (never)
constexpr int kThr16Floats = 65537;                   // thresholds of a 16-bit quantiser: thr[0] = -inf .. thr[65536] = +inf
constexpr int kPq8ThrOffset = kThr16Floats;           // RestoreParams::pq16_thr: the PQ -> 8 bit thresholds follow the 16-bit ones
constexpr int kSrgb16ThrOffset = kSrgb8TableFloats;   // RestoreParams::srgb16_tab: the thresholds follow the segments
void build_pq16_thresholds(float* out /* [kThr16Floats] */);
void build_pq8_thresholds(float* out /* [257] */);
void build_srgb16_table(float* out /* [kSrgb16ThrOffset + kThr16Floats]: segments, then thresholds */);
// fused restoration + colour tile kernel (Gab -> EPF iters -> XYB -> optional transfer/quantise)
struct RestoreParams {
    int gab, epf_iters, xyb, transfer, max_value, out_elem;
    int interleaved;  // JXL_OUT_RGB8 / RGB16: out[0] holds R,G,B per pixel
    float gab_base[3], gab_adj[3], gab_diag[3];
    EpfParams epf[3];  // per iteration index 0..2
    XybParams xybp;
    float global_scale_f;
    float sharp_lut[8];
    int hf_mul_negative;  // the hf_mul map the EPF reads holds a negative entry (no bitstream does: HfMul is 1 + u32; synthetic maps may)
    const float* pq_tab;  // device: PQ segment table (null: double-precision PQ)
    const float* srgb8_tab;  // device: sRGB -> 8-bit threshold table (fp_srgb8; null: double-precision pow + quantise)
    const float* pq16_thr;   // device: the kThr16Floats thresholds of PQ -> 16 bit (fp_pq16), then (at kPq8ThrOffset) the 257 of
                             // PQ -> 8 bit (fp_pq8); null: table / f64 float result, then quantise
    const float* srgb16_tab;  // device: quadratic segments of the sRGB curve over [2^-9, 1), then (at kSrgb16ThrOffset) the
                              // kThr16Floats thresholds of sRGB -> 16 bit (fp_srgb16; null: double-precision pow + quantise)
};
// argument block of the fused kernel (one per frame; an array of them for the batched launch)
struct FusedArgs {
    const float* in[3];
    void* out[3];
    const float* inv_sigma;  // [ceil(H / 8)][bw] inverse sigma per cell (Frame.java:552-571): the frame's plane of the table arena
                             // (finalize_tables), or what k_epf_sigma made of maps handed over as device planes; null without EPF
    int W, H, bw;
    int tiled;  // in[] are cell-tiled planes (plane_tiled.h): run_frame's pooled planes only; epf_iters <= 2
    RestoreParams p;
};
// what the fused restoration kernel takes: planes of at least one cell (its mirror fix-up assumes at most one reflection within the
// halo) and, when EPF iterations run, the inverse-sigma plane of the cells. fill_restore_fused_args declines everything else; run_frame
// asks the same question before it decides where the IDCT output goes
inline bool restore_fused_covers(int h, int w, int epf_iters, const void* inv_sigma) {
    return w >= 8 && h >= 8 && (epf_iters <= 0 || inv_sigma);
}
// The fused kernel divides the EPF sums by a sum of weights it knows to lie in [1, 13] (epf_quot3.h). A weight is max(1 - x, 0),
// x = dist * border_sad_mul * sigma_scale * inv_sigma, so that needs x >= 0 or NaN, i.e. no negative factor: a parameter set with one
// (or a NaN, or a -0 that an inversion would turn into -inf) runs the instantiations that keep the plain divisions. Such a launch
// reports kRestorePlainBit (jxl_debug_last_restore_launches), and the frames of a batch launch agree on it.
inline bool epf_weights_plain(const RestoreParams& p) {
    if (p.epf_iters <= 0) return false;
    auto bad = [](float v) { return !(v >= 0.0f) || std::signbit(v); };
    bool plain = p.hf_mul_negative != 0 || bad(p.global_scale_f);
    for (int k = 0; k < 8; k++) plain = plain || bad(p.sharp_lut[k]);
    for (int i = 0; i < 3; i++) {  // (every iteration index: which of them run depends on epf_iters alone)
        plain = plain || bad(p.epf[i].sigma_scale) || bad(p.epf[i].border_sad_mul);
        for (int c = 0; c < 3; c++) plain = plain || bad(p.epf[i].channel_scale[c]);
    }
    return plain;
}
// false if the configuration is not covered by the fused kernel
bool fill_restore_fused_args(const float* const in[3], void* const out[3], int h, int w, const float* inv_sigma, const RestoreParams& p,
                             FusedArgs& a);
// (stage timing) the events the next single-frame launch of the fused restoration kernel records its own start / stop into; else null
extern thread_local hipEvent_t g_restore_kernel_ev[2];
int restore_fused_variant(const FusedArgs& a);  // which kernel instantiation the arguments select
// the non-float sinks of the fused kernel (k_restore_fused_gen.hip, k_restore_fused_q.hip): one frame (`single`) or a batch
void launch_restore_fused_gen(const FusedArgs* single, const FusedArgs* host_args, const FusedArgs* dev_args, int n, hipStream_t s);
void launch_restore_fused_q(int sink_kind, const FusedArgs* single, const FusedArgs* host_args, const FusedArgs* dev_args, int n, hipStream_t s);
void launch_restore_fused_batch(const FusedArgs* host_args, const FusedArgs* dev_args, int n, hipStream_t s);
// (test hook) epf_quot3 over arrays in device memory: out[k * count + i] = n[k * count + i] / d[i], k = 0..2
void launch_epf_quot3(const float* n, const float* d, float* out, int64_t count, hipStream_t s);
// returns false if the configuration is not covered by the fused kernel (caller falls back to stage kernels)
bool launch_restore_fused(const float* const in[3], void* const out[3], int h, int w, const float* inv_sigma, const RestoreParams& p,
                          hipStream_t s, bool tiled_in = false);
// the input layouts the fused kernel is instantiated for: cell-tiled planes feed the 4x1-patch variants without the 13-tap iteration
// (false under JXL_RESTORE_PH=2, whose 4x2-patch kernels read raster). run_frame asks before it picks the layout of a pooled set.
bool restore_fused_takes_tiled(int epf_iters);

// one inverse squeeze step over up to 8 channels in a single launch
struct SqueezeDesc {
    const int32_t* a;  // averages
    const int32_t* b;  // residuals
    int32_t* o;        // output
    int adim, rdim;    // squeezed-axis length of a and b (widths for H, heights for V)
    int other;         // the other dimension (rows for H, columns for V)
    int32_t* side;     // [nseg][other] chain state at every segment start (segmented mode), or null: one segment
    int seg, warm;     // pairs per segment and warm-up pairs in front of it (multiples of 8); 0: kSqueezeSeg / kSqueezeWarm
    int32_t* tail;     // [nseg][other] last output of every segment but the last (what side[s + 1] is checked against), or null:
                       // the check reads it from the output plane (for H steps that is one cache line per row and segment)
};
__host__ __device__ inline int squeeze_seg(const SqueezeDesc& d);
__host__ __device__ inline int squeeze_warm(const SqueezeDesc& d);
// The recurrence (left = previously output odd sample) is serial along the squeezed axis, but it forgets its start
// within a few pairs (tendency() is clamped to [0, 2(avg - nextAvg)], so every step maps all inputs to a handful of
// outputs: measured 1-2 pairs on average, 6 at most on photographic, synthetic and white-noise rows). So the axis is cut
// into segments of kSqueezeSeg pairs; the wave of segment s > 0 starts kSqueezeWarm pairs early from a guessed state,
// stores nothing for those, and records the state it has reached at its segment start in `side`. A second, tiny
// kernel compares that state with the true one (the last output of segment s-1); every segment of a row / column whose
// boundaries all match is exact by induction, and a row / column with a mismatch (constructible, not observed) is redone
// serially from its first bad boundary. Results are bit-identical to the serial walk in every case.
#ifndef JXL_SQUEEZE_SEG
#define JXL_SQUEEZE_SEG 64
#endif
#ifndef JXL_SQUEEZE_WARM
#define JXL_SQUEEZE_WARM 16
#endif
constexpr int kSqueezeSeg = JXL_SQUEEZE_SEG;
constexpr int kSqueezeWarm = JXL_SQUEEZE_WARM;
// the segment-boundary arrays of an EARLIER step, checked in the prologue of a later step's walk kernel (r4)
struct SqueezeCheck {
    const int32_t* side;  // [nseg][n]
    const int32_t* tail;  // [nseg - 1][n] (rows 0 .. nseg-2 used)
    int n, nseg;
};
struct SqueezeBatch {
    int n;
    int horizontal;
    SqueezeDesc d[8];
    // k_squeeze_verify: nullptr = repair a mismatching row / column in place (the step is then exact before the next one
    // starts); else = only report (atomicOr 1): the check runs beside / behind the following steps and the host redoes the plan
    int32_t* flag;
    // r4: the verification of the PREVIOUS segmented step rides in this step's walk launch -- every workgroup compares a slice
    // of that step's compact side / tail arrays before it starts its own walk and reports a mismatch in `flag`; a 1080p plan is
    // then 13 launches instead of 23 (the check launches were 6 us each on the chain of dependent launches that bounds it)
    int n_chk;
    SqueezeCheck chk[16];
};
constexpr int kSqueezeMaxChecks = 16;

// r5: a vertical step and the horizontal step that follows it on the same channels (ModularStream.java:229-254 applies them back
// to back: V_k, H_k produce level k of the squeeze pyramid from level k + 1) as ONE launch -- the V output lives in LDS only.
// One wave = one tile: 64 output rows (a "stripe": 32 V pairs) x one H segment of `seg` pairs, walked left to right in chunks of
// 16 H pairs (k_modular_vh.hip). Guessed states, all verified like the segmented walk's (SqueezeCheck): the H chain at a segment
// start (side_h / tail_h, [nseg][rows]), the V chain at a stripe start (side_v / tail_v, [nstripe][columns]), and the V chain at
// the three quarter boundaries inside a stripe (compared inside the wave, reported in VHBatch::flag).
constexpr int kVhPad = 30, kVhPadH = 31;  // samples in front of a plane / of a horizontal step's residual plane (host.hip, jxl_modular_begin)
struct VHDesc {
    const int32_t* va;  // V averages  [ah][w]
    const int32_t* vb;  // V residuals [rh][w]
    const int32_t* hb;  // H residuals [ah + rh][rw]
    int32_t* o;         // output      [ah + rh][w + rw]
    int w, ah, rh, rw;  // rh >= 1, rw >= 1; ah - rh and w - rw are 0 or 1
    int seg;            // H pairs per segment (a multiple of VHBatch::cw)
    int nseg, nstripe;  // max(1, ceil((rw - 1) / seg)), ceil((ah + rh) / 64)
    int tile0;          // index of this channel's first tile in the launch (tiles: [stripe][segment])
    int32_t *side_h, *tail_h;  // [nseg][ah + rh]
    int32_t *side_v, *tail_v;  // [ceil(rh / 32)][w]
};
struct VHBatch {
    int n, n_tiles;
    int cw;         // H pairs per chunk: 16 or 32 (the kernel instantiation; VHDesc::seg is a multiple of it)
    VHDesc d[8];
    int32_t* flag;  // report a mismatch (atomicOr 1); never null
    int n_chk;      // segment-boundary arrays of an EARLIER step, checked in this launch's prologue
    SqueezeCheck chk[kSqueezeMaxChecks];
};
void launch_squeeze_vh(const VHBatch& bt, hipStream_t s);
// parallel report-only comparison of segment-boundary arrays (the last step of a plan has no later launch to ride in)
void launch_squeeze_check(const SqueezeCheck* chk, int n_chk, int32_t* flag, hipStream_t s);
// Small steps are bound by the time ONE wave needs for its segment (~130 cycles per pair), large ones by bandwidth: the host
// gives steps of up to 8 Mi samples 32-pair segments with an 8-pair warm-up (measured: 1080p image 0.245 -> 0.195 ms) and
// keeps 64 + 16 beyond (8K image: 0.78 ms against 0.80 ms with 32 + 8 everywhere).
__host__ __device__ inline int squeeze_seg(const SqueezeDesc& d) { return d.seg > 0 ? d.seg : kSqueezeSeg; }
__host__ __device__ inline int squeeze_warm(const SqueezeDesc& d) { return d.seg > 0 ? d.warm : kSqueezeWarm; }
__host__ __device__ inline int squeeze_segments(const SqueezeDesc& d) {
    return d.side && d.rdim > squeeze_seg(d) ? (d.rdim + squeeze_seg(d) - 1) / squeeze_seg(d) : 1;
}
// check_stream / ev: with bt.flag set, the verification launch goes to check_stream behind an event recorded on s
void launch_squeeze_batch(const SqueezeBatch& bt, hipStream_t s, hipStream_t check_stream = nullptr, hipEvent_t ev = nullptr);
// the two halves on their own: the walk (with the fused check of an earlier step, SqueezeBatch::chk) and the verification;
// squeeze_can_fuse_check: the step is segmented and all its channels keep compact tail arrays
void launch_squeeze_walk(const SqueezeBatch& bt, hipStream_t s);
void launch_squeeze_verify(const SqueezeBatch& bt, hipStream_t s);
bool squeeze_can_fuse_check(const SqueezeBatch& bt);
// a run of small steps in one launch: dev_steps = the steps' SqueezeBatch blocks in device memory, slot i of every step by
// workgroup i (the caller has checked that slot i of a step depends on slot i of the step before only)
void launch_squeeze_chain(const SqueezeBatch* dev_steps, int n_steps, int n_slots, hipStream_t s);
void launch_inv_hsqueeze(const int32_t* avg, int aw, const int32_t* res, int rw, int h, int32_t* out, hipStream_t s);
void launch_inv_vsqueeze(const int32_t* avg, int ah, const int32_t* res, int rh, int w, int32_t* out, hipStream_t s);
void launch_rct(int32_t* v0, int32_t* v1, int32_t* v2, int64_t n, int type, hipStream_t s);
void launch_modular_to_float(const int32_t* a, const int32_t* b, int64_t n, float scale, float* out, hipStream_t s);

// LF stage (row f1): q/out device pointers; out written at out_off + y*out_stride + x
// one channel of a chroma-subsampled frame: out = q * (scaledDequant / (1 << extraPrecision)), no CfL, no smoothing
void launch_lf_dequant_plain(const int32_t* q, float* out, int H, int W, int64_t out_off, int out_stride, float scaled_dequant,
                             int extra_precision, hipStream_t s);
void launch_lf_dequant(const int32_t* const q[3], float* const out[3], int H, int W, int64_t out_off, int out_stride,
                       const float scaled_dequant[3], int extra_precision, float base_corr_x, float base_corr_b,
                       int color_factor, int x_factor_lf, int b_factor_lf, int smooth, hipStream_t s);

// rows f4 / f3 (k_post.hip); all pointers are device pointers
void launch_chroma_upsample_h(const float* in, int h, int w, float* out, hipStream_t s);
void launch_chroma_upsample_v(const float* in, int h, int w, float* out, hipStream_t s);
void launch_upsample(const float* in, int h, int w, int k, const float* weights, float* out, hipStream_t s);
void launch_noise_init(int h, int w, int group_dim, uint64_t seed0, int colors, float* const tmp[3], float* const out[3],
                       hipStream_t s);
void launch_noise_add(float* const planes[3], const float* const noise[3], int64_t n, const float lut[8], float bcx, float bcb,
                      hipStream_t s);
// the inner blend functions (k_blend's switch), blend_op and blend_needs: blend_ops.h
void launch_blend(int op, unsigned flags, void* canvas, int cw, const void* frame, int fw, const void* ref, int rw,
                  const float* frame_alpha, const float* ref_alpha, const jxl_blend_rect& r, hipStream_t s);
void launch_orient(const void* in, int h, int w, int orientation, void* out, hipStream_t s);
void launch_pack(const void* const planes[4], const jxl_pack_params& p, bool coerce, void* out, hipStream_t s);

// ---- splines (spline_host.hip: the host side; k_spline.hip: the kernel) ----
// footprint of one workgroup of k_splines, and the unit of the host's binning
constexpr int kSplineTileW = 32, kSplineTileH = 8;
constexpr int64_t kSplineMaxArcs = (int64_t)1 << 26;
static_assert(sizeof(jxl_spline_arc) == 48, "arc record");
// the arc table of jxl_spline_arcs, uncapped; JXL_OK or a status (the reason in *why)
jxl_status spline_arc_table(const jxl_spline_desc* d, int32_t height, int32_t width, std::vector<jxl_spline_arc>* out, const char** why);
// SplineBins, the binned form of an arc table: patch_compile.h (the patch stage bins its positions the same way)
// false: the lists do not fit (bad_alloc, or 2^31 entries and more)
bool spline_bin(const jxl_spline_arc* arcs, int64_t n, int32_t height, int32_t width, SplineBins* out);
void launch_splines(float* const planes[3], int h, int w, const jxl_spline_arc* arcs, const int32_t* tile, const int32_t* start,
                    const int32_t* list, int n_tiles, int tiles_x, hipStream_t s);

// ---- patches (patch_compile.h: validation, blend functions, binning -- plain C++, no device call; k_patch.hip: the kernel) ----
// PatchRec, PatchOp, PatchStage and patch_compile: patch_compile.h
// planes: device table of int64 -- frame plane pointers [n_chan], slot plane pointers [4][n_chan] (0: reads as zeros), slot
// widths [4]
void launch_patches(const int64_t* planes, int n_chan, int w, const PatchRec* rec, const PatchOp* ops, const int32_t* tile,
                    const int32_t* start, const int32_t* list, int n_tiles, int tiles_x, hipStream_t s);

// ---- device plane sets (canvas_host.hip: the sets and the jxl_canvas_* entries; k_canvas.hip: the blend kernel) ----
// one canvas channel as the kernel reads it: every pointer already stands on the rectangle's origin in its plane (patchStart,
// frameOffset, refOffset -- frameOffset for the reference plane of OP_COPY_REF); a plane the function does not read is null
struct CanvasChan {
    uint32_t* canvas;
    const uint32_t *frame, *ref, *frame_alpha, *ref_alpha;
    int32_t op, flags;  // BlendOp, JXL_BLEND_FLAG_*
};
struct CanvasArgs {
    int32_t n, h, w;      // channels, blendSize
    int32_t cw, fw, rw;   // row strides (samples) of the canvas, frame and reference planes
    int32_t c_align;      // sample index of the rectangle's origin in its canvas plane, modulo 4 (plane bases are 16-byte aligned)
    int32_t reserved;
    CanvasChan ch[JXL_CANVAS_MAX_PLANES];
};
void launch_canvas_blend(const CanvasArgs& a, hipStream_t s);
// jxl_canvas_cast_planes' kernel (k_canvas.hip): ImageBuffer.castToFloat0 of every listed plane in place, one launch. One
// workgroup converts one run of kCastRun consecutive samples of one item; first_block[i] is the first workgroup of item i
// (first_block[n] = the grid). The table travels as the kernel's argument: wave-uniform, read through scalar loads.
constexpr int kCastMaxItems = 5 * JXL_CANVAS_MAX_PLANES;
constexpr int kCastRun = 4096;
struct CastItem {
    uint32_t* base;  // h x w 4-byte samples, int32 before and float after
    int64_t n;       // h * w
    float scale;     // 1f / max
    int32_t reserved;
};
struct CastArgs {
    int32_t n, reserved;
    int32_t first_block[kCastMaxItems + 2];  // n + 1 entries in use; the even count keeps `it` 8-byte aligned without padding
    CastItem it[kCastMaxItems];
};
static_assert(sizeof(CastArgs) <= 4096, "the cast table is a kernel argument");
void launch_canvas_cast(const CastArgs& a, hipStream_t s);
// The context is host.hip's: canvas_host.hip reaches what it needs of it through these. CanvasStore: a context's sets.
struct CanvasStore;
void canvas_store_free(CanvasStore* s);  // jxl_ctx_destroy, after the stream has drained
struct CtxLink {
    hipStream_t stream;
    CanvasStore** canvas;  // the context's slot for its store (null until the first set)
    int device;            // the context's device ordinal
};
// png_args of host.hip for tensor_host.hip: the checks of the three PNG entries on one jxl_png_params, and the kernel's arguments
// (plane and output pointers are the caller's to fill in)
jxl_status ctx_png_args(jxl_ctx* c, const jxl_png_params* p, const void* const in[3], const void* alpha, const void* out, PngArgs* a,
                        int* n_color);
jxl_status ctx_link(jxl_ctx* c, CtxLink* out);                      // hipSetDevice + the fields above
jxl_status ctx_fail(jxl_ctx* c, jxl_status st, const char* msg);    // records the message (c may be null) and returns st
bool ctx_tone_map_armed(const jxl_ctx* c);                          // jxl_ctx_set_tone_map: the colour passes write three colour channels
jxl_status ctx_planes_get(jxl_ctx* c, int* h, int* w, float* p[3]);  // the resident planes, or JXL_ERR_STATE
jxl_status ctx_planes_set(jxl_ctx* c, int h, int w, float* p[3]);    // resident planes of h x w to fill (contents undefined)
// an image's home (image_home.h) for the exits: the resident planes with the host plane `alpha` (JXL_ERR_STATE without); planes
// 0 .. n_color - 1 of the set `id` and its plane alpha_plane (an unknown id and planes it has not are the home's first half)
jxl_status ctx_home_resident(jxl_ctx* c, const void* alpha, ImageHome* m);
ImageHome ctx_home_set(jxl_ctx* c, int32_t id, int32_t n_color, int32_t alpha_plane, bool has_alpha);
// the XYB stage's parameters as jxl_planes_xyb / jxl_stage_xyb make them from the header's values
XybParams ctx_make_xyb(const float matrix[9], const float opsin_bias[3], const float cbrt_opsin_bias[3], float intensity_target);
// the page-locked staging buffer of the spline and patch tables: room for `total` bytes at *host once the transfer before has read
// it, then its first `total` bytes queued to the context's table buffer (*dev) by ONE transfer on the stream
jxl_status ctx_tables_reserve(jxl_ctx* c, size_t total, char** host);
jxl_status ctx_tables_send(jxl_ctx* c, size_t total, const char** dev);
// the Modular context's result channels (device pointers), settled as jxl_modular_read_channel settles them; *ran: a plan has
// run since jxl_modular_begin
struct ModResult { const int32_t* d; int32_t h, w; };
jxl_status ctx_modular_out(jxl_ctx* c, std::vector<ModResult>* out, bool* ran);
// a set as the exits read it (CanvasView: image_home.h; canvas_host.hip): false for an unknown id
bool canvas_view(const CanvasStore* s, int32_t id, CanvasView* out);
// jxl_canvas_from_modular's kernel (k_modplanes.hip): plane i of the set from one or two result channels of one pitch
struct ModPlane {
    const int32_t *a, *b;  // b: null, or the channel added first
    uint32_t* out;         // h x w words
    int32_t pitch;         // the channels' width
    int32_t is_float;      // scale * (float)v, else the int32 sample as it is
    float scale;
    int32_t reserved;
};
struct ModPlanesArgs {
    int32_t h, w, n, reserved;
    ModPlane p[JXL_CANVAS_MAX_PLANES];
};
void launch_modplanes(const ModPlanesArgs& p, hipStream_t s);
// jxl_canvas_from_modular_up's kernel (k_modplanes.hip): plane i of the set, k*h x k*w floats, from the h x w crop of one or two
// result channels of one pitch; weights: k * k * 25 floats in device memory
struct ModUpPlane {
    const int32_t *a, *b;  // b: null, or the channel added first
    float* out;            // k*h x k*w floats
    int32_t pitch;         // the channels' width
    float scale;
};
struct ModUpArgs {
    int32_t h, w, n, reserved;  // the crop; planes
    const float* weights;
    ModUpPlane p[JXL_CANVAS_MAX_PLANES];
};
void launch_modplanes_up(const ModUpArgs& p, int k, hipStream_t s);

void launch_idct2d_single(const float* src, float* dst, int h, int w, int transposed, const float* lut, hipStream_t s);
void launch_fdct2d_single(const float* src, float* dst, int h, int w, const float* lut, hipStream_t s);

}  // namespace jxl
