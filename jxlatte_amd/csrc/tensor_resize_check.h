// The pure part of the resized tensor entries (tensor_resize_host.hip): the box, size and filter rules in 64-bit arithmetic, the
// tap tables both passes of k_tensor_resize read, the cap on a tap range, the tile picker and the rule of the kernel's 16-byte
// plane loads. Plain C++: no device call, no context; tools/native/tensor_resize_check.cpp runs it as a program of its own under
// the sanitizers. Everything about the OUTPUT tensor is tensor_check.h's, asked with the output size.
//
// Tap tables, per axis (box length L, output length O), in IEEE double -- Pillow's precompute_coeffs:
//   s = L / O, fs = max(s, 1), sup = r * fs                      r: 1 for the triangle, 0.5 for the box
//   c = (o + 0.5) * s, lo = max(0, floor(c - sup + 0.5)), hi = min(L, floor(c + sup + 0.5))
//   weight of j in [lo, hi): t = (j + 0.5 - c) / fs; triangle max(0, 1 - |t|); box 1 where -0.5 < t <= 0.5, else 0
//   divided by their sum (taken in ascending j), each then rounded to f32; trailing, then leading taps whose f32 weight is 0
//   are dropped, one tap at least is kept
// packed: first[O] (relative to the box), off[O + 1], w[off[O]].
#ifndef JXL_TENSOR_RESIZE_CHECK_H
#define JXL_TENSOR_RESIZE_CHECK_H
#include <cmath>
#include <stdint.h>
#include <vector>

#include "tensor_check.h"

namespace jxl {

constexpr int kResizeMaxTaps = 1024;       // per output sample and axis, before the trim
constexpr int kResizeLdsBytes = 64 * 1024;  // the workgroup's image of its vertical sums
constexpr int kResizeLanes = 256;

struct ResizeTaps {
    std::vector<int32_t> first, off;
    std::vector<float> w;
};

// nullptr, or why box / size / filter are refused (p: the SOURCE planes' size and the tensor's parameters)
inline const char* resize_check_params(const jxl_tensor_params* p, const jxl_resize_params* r) {
    if (!p || !r) return "tensor resized: null argument";
    if (p->height <= 0 || p->width <= 0) return "tensor samples: bad size";
    if (r->out_height <= 0 || r->out_width <= 0) return "tensor resized: bad output size";
    if (r->filter != JXL_RESIZE_TRIANGLE && r->filter != JXL_RESIZE_BOX) return "tensor resized: unknown filter";
    if (r->box_width <= 0 || r->box_height <= 0 || r->box_x0 < 0 || r->box_y0 < 0 ||
        (int64_t)r->box_x0 + r->box_width > p->width || (int64_t)r->box_y0 + r->box_height > p->height)
        return "tensor resized: the box is not inside the image";
    return nullptr;
}

// the table of one axis. nullptr, or why it is refused; the ranges it builds are inside [0, L), and first and first + count
// never decrease with o (the kernel takes a tile's footprint from its first and last sample)
inline const char* resize_build_taps(int64_t L, int64_t O, int filter, ResizeTaps* t) {
    if (L <= 0 || O <= 0 || L > INT32_MAX || O > INT32_MAX) return "tensor resized: bad size";
    const double s = (double)L / (double)O, fs = s > 1.0 ? s : 1.0, sup = (filter == JXL_RESIZE_BOX ? 0.5 : 1.0) * fs;
    t->first.assign((size_t)O, 0);
    t->off.assign((size_t)O + 1, 0);
    t->w.clear();
    std::vector<double> d;
    int64_t prev_first = 0, prev_end = 0;
    for (int64_t o = 0; o < O; o++) {
        const double c = ((double)o + 0.5) * s;
        double flo = std::floor(c - sup + 0.5), fhi = std::floor(c + sup + 0.5);
        int64_t lo = flo < 0.0 ? 0 : (int64_t)flo, hi = fhi > (double)L ? L : (int64_t)fhi;
        if (lo > L - 1) lo = L - 1;
        if (hi <= lo) hi = lo + 1;  // (never with these formulas: a range holds the sample under c)
        if (hi - lo > kResizeMaxTaps) return "tensor resized: more than 1024 taps";
        d.assign((size_t)(hi - lo), 0.0);
        double sum = 0.0;
        for (int64_t j = lo; j < hi; j++) {
            const double x = (((double)j + 0.5) - c) / fs;
            double v;
            if (filter == JXL_RESIZE_BOX) v = (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
            else v = 1.0 - std::fabs(x), v = v > 0.0 ? v : 0.0;
            d[(size_t)(j - lo)] = v;
            sum += v;
        }
        int64_t a = 0, b = hi - lo;
        std::vector<float>& w = t->w;
        const size_t base = w.size();
        for (int64_t k = 0; k < b; k++) w.push_back((float)(d[(size_t)k] / sum));
        while (b - a > 1 && w[base + (size_t)b - 1] == 0.0f) b--;
        while (b - a > 1 && w[base + (size_t)a] == 0.0f) a++;
        w.erase(w.begin() + (ptrdiff_t)(base + (size_t)b), w.end());
        w.erase(w.begin() + (ptrdiff_t)base, w.begin() + (ptrdiff_t)(base + (size_t)a));
        if (w.size() > (size_t)INT32_MAX) return "tensor resized: the tap table does not fit 31 bits";
        t->first[(size_t)o] = (int32_t)(lo + a);
        t->off[(size_t)o + 1] = (int32_t)w.size();
        if (o && (lo + a < prev_first || lo + b < prev_end)) return "tensor resized: the tap ranges are not monotone";
        prev_first = lo + a, prev_end = lo + b;
    }
    return nullptr;
}

// the 16-byte plane loads of the vertical pass: every row of every plane read starts 16-byte aligned
inline bool resize_wide_in_ok(int32_t width, const uint64_t* bases, int n_bases) {
    if (width % 4) return false;
    for (int i = 0; i < n_bases; i++)
        if (bases[i] % 16) return false;
    return true;
}

// the skewed LDS column of footprint column x (a 16-dword lane stride, the 3840 -> 240 case, then spreads over all banks)
inline int64_t resize_lds_col(int64_t x, bool skew) { return skew ? x + (x >> 5) : x; }

// the widest footprint, in columns from its start aligned down to 4 (x0: the box's first column), of a row of tw-column tiles
inline int64_t resize_footprint(const ResizeTaps& x, int64_t x0, int64_t tw) {
    const int64_t O = (int64_t)x.first.size();
    int64_t widest = 0;
    for (int64_t a = 0; a < O; a += tw) {
        const int64_t b = (a + tw < O ? a + tw : O) - 1;
        const int64_t lo = (x0 + x.first[(size_t)a]) & ~(int64_t)3;
        const int64_t hi = x0 + x.first[(size_t)b] + (x.off[(size_t)b + 1] - x.off[(size_t)b]);
        if (hi - lo > widest) widest = hi - lo;
    }
    return widest;
}

struct ResizeTile {
    int tw, th;
    int lds_w;      // floats of one (row, plane) line of the LDS image
    int lds_bytes;  // th * planes * lds_w * 4
};

inline bool resize_tile_fits(const ResizeTaps& x, int64_t x0, int planes, bool skew, int tw, int th, ResizeTile* out) {
    const int64_t fw = (resize_footprint(x, x0, tw) + 3) & ~(int64_t)3;
    const int64_t lds_w = resize_lds_col(fw, skew) + 1;
    const int64_t bytes = (int64_t)th * planes * lds_w * 4;
    if (bytes > kResizeLdsBytes) return false;
    out->tw = tw, out->th = th, out->lds_w = (int)lds_w, out->lds_bytes = (int)bytes;
    return true;
}

// the most source rows a band of th output rows spans (what one workgroup's vertical pass walks)
inline int64_t resize_band_rows(const ResizeTaps& y, int64_t th) {
    const int64_t O = (int64_t)y.first.size();
    int64_t most = 0;
    for (int64_t a = 0; a < O; a += th) {
        const int64_t b = (a + th < O ? a + th : O) - 1;
        const int64_t rows = y.first[(size_t)b] + (y.off[(size_t)b + 1] - y.off[(size_t)b]) - y.first[(size_t)a];
        if (rows > most) most = rows;
    }
    return most;
}

// The tile of a launch: among TW of 64, 32, 16, 8 and TH of 4, 2, 1 (a lane keeps TH * planes * 4 accumulators: at most 64
// registers) whose LDS image fits, the one with the least estimated time of the vertical pass,
//   ceil(tiles / slots) * chunks * rows:  slots: the workgroups the device holds at once; chunks: the 1024-column passes of the
//   lanes over the widest footprint; rows: the source rows a workgroup walks (resize_band_rows)
// -- the larger tile on a tie (fewer rows loaded twice). Measured at 3840x2160 -> 224x224 (profiles/tensor_resized.md): the
// estimate orders 64x4, 64x2, 32x2 and 32x4 as the clock does. Then, for the ranges near the cap only, one row of 4, 2 or 1
// columns: one column of 1024 taps and four planes is 17 KiB, so every pair the checks admit launches.
// planes: the colour planes + the alpha plane when read. force_tw / force_th: 0, or the tile of jxl_debug_tensor_resize_tile
// (refused when it does not fit)
inline const char* resize_pick_tile(const ResizeTaps& x, int64_t x0, const ResizeTaps& y, int planes, bool skew, int64_t slots, int force_tw,
                                    int force_th, ResizeTile* out) {
    if (force_tw || force_th) {
        const bool known = (force_tw == 64 || force_tw == 32 || force_tw == 16 || force_tw == 8 || force_tw == 4 || force_tw == 2 || force_tw == 1) &&
                           (force_th == 4 || force_th == 2 || force_th == 1);
        if (!known || force_tw * force_th > kResizeLanes) return "tensor resized: no such tile";
        return resize_tile_fits(x, x0, planes, skew, force_tw, force_th, out) ? nullptr : "tensor resized: the forced tile does not fit the LDS";
    }
    const int64_t ow = (int64_t)x.first.size(), oh = (int64_t)y.first.size();
    if (slots < 1) slots = 1;
    bool any = false;
    int64_t best = 0;
    for (int th = 4; th >= 1; th >>= 1) {
        const int64_t rows = resize_band_rows(y, th);
        for (int tw = 64; tw >= 8; tw >>= 1) {
            ResizeTile t;
            if (!resize_tile_fits(x, x0, planes, skew, tw, th, &t)) continue;
            const int64_t tiles = ((ow + tw - 1) / tw) * ((oh + th - 1) / th);
            const int64_t chunks = (resize_footprint(x, x0, tw) + 1023) / 1024;
            const int64_t cost = ((tiles + slots - 1) / slots) * chunks * rows;
            if (!any || cost < best) any = true, best = cost, *out = t;
        }
    }
    if (any) return nullptr;
    for (int tw = 4; tw >= 1; tw >>= 1)
        if (resize_tile_fits(x, x0, planes, skew, tw, 1, out)) return nullptr;
    return "tensor resized: no tile fits the LDS";  // (not reached under the cap)
}

}  // namespace jxl
#endif  // JXL_TENSOR_RESIZE_CHECK_H
