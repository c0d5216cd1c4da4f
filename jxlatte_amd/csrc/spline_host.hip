// Host side of the spline stage: the arc table of Frame.renderSplines / Spline.renderSpline (J/frame/features/spline/Spline.java)
// and its binning into the tiles of k_splines. No device code and no device call: jxl_spline_arcs works without a GPU.
// Float operations in the reference's order (the library is built with -ffp-contract=off); the double functions pow, cos,
// sqrt and log are the host libm's, as in jxlatte_amd/decoder.py, whose arc table this one equals bit for bit.
#include "sample_ops.h"

#include <cmath>
#include <limits>
#include <new>

namespace jxl {
namespace {

struct RawArc { float y, x, len; };  // SplineArc

// Spline.upsampleControlPoints (Spline.java:27-87); cp = n (y, x) pairs. Point arithmetic is Java int arithmetic (wraps)
void upsample_control_points(const int32_t* cp, int64_t n, std::vector<float>& uy, std::vector<float>& ux) {
    if (n == 1) {
        uy.assign(1, (float)cp[0]);
        ux.assign(1, (float)cp[1]);
        return;
    }
    auto ext = [&](int64_t i, int k) -> int32_t {  // extended[i], component k
        if (i == 0) return (int32_t)((uint32_t)cp[k] * 2u - (uint32_t)cp[2 + k]);
        if (i == n + 1) return (int32_t)((uint32_t)cp[2 * (n - 1) + k] * 2u - (uint32_t)cp[2 * (n - 2) + k]);
        return cp[2 * (i - 1) + k];
    };
    const int64_t total = 16 * (n - 1) + 1;
    uy.assign((size_t)total, 0.0f);
    ux.assign((size_t)total, 0.0f);
    float t[4], pY[4], pX[4], dY[3], dX[3], aY[3], aX[3], bY[2], bX[2];
    for (int64_t i = 0; i < n - 1; i++) {
        for (int k = 0; k < 4; k++) {
            pY[k] = (float)ext(i + k, 0);
            pX[k] = (float)ext(i + k, 1);
        }
        uy[(size_t)i << 4] = pY[1];
        ux[(size_t)i << 4] = pX[1];
        t[0] = 0.0f;
        for (int k = 0; k < 3; k++) {
            dY[k] = pY[k + 1] - pY[k];
            dX[k] = pX[k + 1] - pX[k];
            t[k + 1] = t[k] + (float)std::pow((double)(dY[k] * dY[k] + dX[k] * dX[k]), 0.25);
        }
        for (int step = 1; step < 16; step++) {
            const float knot = t[1] + 0.0625f * (float)step * (t[2] - t[1]);
            for (int k = 0; k < 3; k++) {
                const float f = (knot - t[k]) / (t[k + 1] - t[k]);
                aY[k] = dY[k] * f + pY[k];
                aX[k] = dX[k] * f + pX[k];
            }
            for (int k = 0; k < 2; k++) {
                const float f = (knot - t[k]) / (t[k + 2] - t[k]);
                bY[k] = (aY[k + 1] - aY[k]) * f + aY[k];
                bX[k] = (aX[k + 1] - aX[k]) * f + aX[k];
            }
            const float f = (knot - t[1]) / (t[2] - t[1]);
            uy[(size_t)(i * 16 + step)] = (bY[1] - bY[0]) * f + bY[0];
            ux[(size_t)(i * 16 + step)] = (bX[1] - bX[0]) * f + bX[0];
        }
    }
    uy[(size_t)total - 1] = (float)cp[2 * (n - 1)];
    ux[(size_t)total - 1] = (float)cp[2 * (n - 1) + 1];
}

// Spline.computeIntermediarySamples (Spline.java:89-123); false: more than kSplineMaxArcs samples
bool intermediary_samples(const std::vector<float>& uy, const std::vector<float>& ux, float rd, std::vector<RawArc>& arcs) {
    // the walk below advances by rd along the polyline of the upsampled points: a polyline longer than the cap times rd cannot
    // fit, and is turned away before the table grows (the count check in the loop stays: samples at which a float step no
    // longer moves the point end there)
    double polyline = 0.0;
    for (size_t i = 1; i < uy.size(); i++) {
        const double dy = (double)uy[i] - (double)uy[i - 1], dx = (double)ux[i] - (double)ux[i - 1];
        polyline += std::sqrt(dy * dy + dx * dx);
    }
    if (std::isfinite(polyline) && polyline > (double)kSplineMaxArcs * (double)rd) return false;  // (NaN / inf knots: the walk decides)
    float cy = uy[0], cx = ux[0];
    size_t next = 0;
    arcs.clear();
    arcs.push_back({cy, cx, rd});
    while (next < uy.size()) {
        float py = cy, px = cx, acc = 0.0f;
        for (;;) {
            if (next >= uy.size()) {
                arcs.push_back({py, px, acc});
                break;
            }
            const float ny = uy[next], nx = ux[next];
            const float dy = ny - py, dx = nx - px;
            const float to_next = (float)std::sqrt((double)(dy * dy + dx * dx));
            if (acc + to_next >= rd) {
                const float f = (rd - acc) / to_next;
                cy = dy * f + py;
                cx = dx * f + px;
                arcs.push_back({cy, cx, rd});
                break;
            }
            acc += to_next;
            py = ny;
            px = nx;
            next++;
        }
        if ((int64_t)arcs.size() > kSplineMaxArcs) return false;
    }
    return true;
}

// MathHelper.round (MathHelper.java:36-38): (int)(d + 0.5f), Java's cast
int32_t java_round(float d) { return java_f2i(d + 0.5f); }

}  // namespace

jxl_status spline_arc_table(const jxl_spline_desc* d, int32_t height, int32_t width, std::vector<jxl_spline_arc>* out, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    out->clear();
    if (!d || d->n_splines < 0 || height < 1 || width < 1) return *why = "splines: bad arguments", JXL_ERR_INVALID_ARGUMENT;
    if (d->n_splines == 0) return JXL_OK;
    if (!d->n_control || !d->control || !d->coeff) return *why = "splines: null table", JXL_ERR_INVALID_ARGUMENT;
    for (int32_t s = 0; s < d->n_splines; s++)
        if (d->n_control[s] < 1) return *why = "splines: a spline without control points", JXL_ERR_INVALID_ARGUMENT;
    try {
        // Spline.computeCoeffs (Spline.java:133-152) -- of spline 0 for every spline: the constructor drops the id (:23-25)
        const float sqrt_h = (float)std::sqrt(0.5);
        const float qa = (float)d->quant_adjust / 8.0f;
        const float inv_qa = qa >= 0 ? 1.0f / (1.0f + qa) : 1.0f - qa;
        const float y_adj = 0.106066017f * inv_qa, x_adj = 0.005939697f * inv_qa, b_adj = 0.098994949f * inv_qa,
                    s_adj = 0.47135738f * inv_qa;
        float cf[4][32];  // X, Y, B, sigma
        for (int i = 0; i < 32; i++) {
            cf[1][i] = (float)d->coeff[32 + i] * y_adj;
            cf[0][i] = (float)d->coeff[i] * x_adj + d->base_corr_x * cf[1][i];
            cf[2][i] = (float)d->coeff[64 + i] * b_adj + d->base_corr_b * cf[1][i];
            cf[3][i] = (float)d->coeff[96 + i] * s_adj;
        }
        const float log3 = (float)std::log(0.1) * 3.0f;
        const double pi32 = 3.14159265358979323846 / 32.0;  // Math.PI / 32D
        std::vector<float> uy, ux;
        std::vector<RawArc> arcs;
        const int32_t* cp = d->control;
        for (int32_t s = 0; s < d->n_splines; cp += 2 * (int64_t)d->n_control[s], s++) {
            upsample_control_points(cp, d->n_control[s], uy, ux);
            const float rd = 1.0f;
            if (!intermediary_samples(uy, ux, rd, arcs)) return *why = "splines: too many arcs", JXL_ERR_OOM;
            const float arc_len = ((float)arcs.size() - 2.0f) * rd + arcs.back().len;
            if (arc_len <= 0) continue;  // :160-161
            for (size_t i = 0; i < arcs.size(); i++) {
                const RawArc& a = arcs[i];
                const float q = ((float)i * rd) / arc_len;
                const float progress = q < 1.0f ? q : 1.0f;
                const float t = 31.0f * progress;
                // Spline.fourierICT (:125-131) of the four coefficient rows: they share the cosines
                float v[4];
                for (int r = 0; r < 4; r++) v[r] = sqrt_h * cf[r][0];
                for (int k = 1; k < 32; k++) {
                    const float c = (float)std::cos((double)k * pi32 * ((double)t + 0.5));
                    for (int r = 0; r < 4; r++) v[r] = v[r] + cf[r][k] * c;
                }
                const float values[3] = {v[0] * a.len, v[1] * a.len, v[2] * a.len};
                const float sigma = v[3];
                const float inv_sigma = 1.0f / sigma;
                float max_color = 0.01f;  // MathHelper.max(float...): the minimum (MathHelper.java:190-195)
                for (int c = 0; c < 3; c++) max_color = values[c] < max_color ? values[c] : max_color;
                const float max_dist = (float)std::sqrt((double)(-2.0f * sigma * sigma * (log3 - max_color)));
                if (!std::isfinite(max_dist)) continue;
                const int32_t x0 = std::max(0, java_round(a.x - max_dist)), x1 = std::min(width - 1, java_round(a.x + max_dist));
                const int32_t y0 = std::max(0, java_round(a.y - max_dist)), y1 = std::min(height - 1, java_round(a.y + max_dist));
                if (x0 > x1 || y0 > y1) continue;
                if ((int64_t)out->size() >= kSplineMaxArcs) return *why = "splines: too many arcs", JXL_ERR_OOM;
                jxl_spline_arc r;
                r.y = a.y;
                r.x = a.x;
                r.sigma = sigma;
                r.inv_sigma = inv_sigma;
                for (int c = 0; c < 3; c++) r.mul[c] = 0.25f * values[c] * sigma;
                r.x0 = x0, r.x1 = x1, r.y0 = y0, r.y1 = y1;
                r.reserved = 0;
                out->push_back(r);
            }
        }
    } catch (const std::bad_alloc&) {
        return *why = "splines: host allocation failed (arc table)", JXL_ERR_OOM;
    }
    return JXL_OK;
}

bool spline_bin(const jxl_spline_arc* arcs, int64_t n, int32_t height, int32_t width, SplineBins* out) {
    try {
        const int tx_n = (width + kSplineTileW - 1) / kSplineTileW, ty_n = (height + kSplineTileH - 1) / kSplineTileH;
        out->tiles_x = tx_n;
        out->tiles_y = ty_n;
        const size_t n_all = (size_t)tx_n * ty_n;
        std::vector<int64_t> count(n_all + 1, 0);
        for (int64_t i = 0; i < n; i++) {
            const jxl_spline_arc& a = arcs[i];
            for (int ty = a.y0 / kSplineTileH; ty <= a.y1 / kSplineTileH; ty++)
                for (int tx = a.x0 / kSplineTileW; tx <= a.x1 / kSplineTileW; tx++) count[(size_t)ty * tx_n + tx + 1]++;
        }
        for (size_t i = 0; i < n_all; i++) count[i + 1] += count[i];  // count[t] = first entry of tile t
        if (count[n_all] > std::numeric_limits<int32_t>::max()) return false;
        out->list.assign((size_t)count[n_all], 0);
        out->tile.clear();
        out->start.clear();
        for (size_t t = 0; t < n_all; t++)
            if (count[t + 1] > count[t]) {
                out->tile.push_back((int32_t)t);
                out->start.push_back((int32_t)count[t]);
            }
        out->start.push_back((int32_t)count[n_all]);
        // arcs visited in table order, each appended to the lists of its tiles: every list is in table order
        for (int64_t i = 0; i < n; i++) {
            const jxl_spline_arc& a = arcs[i];
            for (int ty = a.y0 / kSplineTileH; ty <= a.y1 / kSplineTileH; ty++)
                for (int tx = a.x0 / kSplineTileW; tx <= a.x1 / kSplineTileW; tx++) out->list[(size_t)count[(size_t)ty * tx_n + tx]++] = (int32_t)i;
        }
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}

}  // namespace jxl

extern "C" int64_t jxl_spline_arcs(const jxl_spline_desc* d, int32_t height, int32_t width, jxl_spline_arc* out, int64_t cap) {
    if (cap < 0 || (cap > 0 && !out)) return JXL_ERR_INVALID_ARGUMENT;
    std::vector<jxl_spline_arc> arcs;
    const jxl_status st = jxl::spline_arc_table(d, height, width, &arcs, nullptr);
    if (st != JXL_OK) return st;
    const int64_t n = (int64_t)arcs.size();
    for (int64_t i = 0; i < n && i < cap; i++) out[i] = arcs[(size_t)i];
    return n;
}

// tests/test_splines_cpu.py: the knots of Spline.upsampleControlPoints for n control points (host only), NaN / inf knots of
// repeated points included. Returns their number and writes uy[], ux[] when they fit cap; a negative status otherwise
extern "C" int64_t jxl_debug_spline_knots(const int32_t* control, int64_t n, float* uy, float* ux, int64_t cap) {
    if (!control || n < 1 || n > (1 << 20) || cap < 0 || (cap > 0 && (!uy || !ux))) return JXL_ERR_INVALID_ARGUMENT;
    try {
        std::vector<float> y, x;
        jxl::upsample_control_points(control, n, y, x);
        const int64_t total = (int64_t)y.size();
        if (total <= cap)
            for (int64_t i = 0; i < total; i++) uy[i] = y[(size_t)i], ux[i] = x[(size_t)i];
        return total;
    } catch (const std::bad_alloc&) {
        return JXL_ERR_OOM;
    }
}

// tests/test_splines_cpu.py: the tile lists of an arc table (host only). Returns the number of non-empty tiles (*n_list = the
// number of list entries) and writes tile[], start[] and list[] when they fit cap_tiles / cap_list; a negative status otherwise
extern "C" int64_t jxl_debug_spline_bins(const jxl_spline_arc* arcs, int64_t n, int32_t height, int32_t width, int32_t* tile, int32_t* start,
                                         int32_t* list, int64_t cap_tiles, int64_t cap_list, int64_t* n_list) {
    if (n < 0 || (n > 0 && !arcs) || height < 1 || width < 1 || !n_list) return JXL_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n; i++)
        if (arcs[i].x0 < 0 || arcs[i].y0 < 0 || arcs[i].x1 >= width || arcs[i].y1 >= height || arcs[i].x0 > arcs[i].x1 || arcs[i].y0 > arcs[i].y1)
            return JXL_ERR_INVALID_ARGUMENT;
    jxl::SplineBins b;
    if (!jxl::spline_bin(arcs, n, height, width, &b)) return JXL_ERR_OOM;
    *n_list = (int64_t)b.list.size();
    const int64_t nt = (int64_t)b.tile.size();
    if (tile && start && list && nt <= cap_tiles && *n_list <= cap_list) {
        for (int64_t i = 0; i < nt; i++) tile[i] = b.tile[(size_t)i];
        for (int64_t i = 0; i <= nt; i++) start[i] = b.start[(size_t)i];
        for (int64_t i = 0; i < *n_list; i++) list[i] = b.list[(size_t)i];
    }
    return nt;
}
