// The pure part of the windowed noise entries (noise_window_host.hip: jxl_planes_noise_at, jxl_stage_noise_window): what the
// arguments must satisfy before anything is allocated or queued, and the geometry both launches of k_noise_window.hip index with.
// Plain C++: no device call, no context; tools/native/noise_window_check.cpp runs it as a program of its own under the sanitizers.
//
// The planes are the window [y0, y0 + win_h) x [x0, x0 + win_w) of a frame_h x frame_w frame. The 5x5 high-pass of
// Frame.initializeNoise reads two samples around a pixel through MathHelper.mirrorCoordinate against the FRAME's size, so the raw
// noise is needed on the apron: the window grown by 2 and clipped to the frame. noise_mirror of every coordinate the convolution
// forms lies inside the apron (noise_window_apron_holds checks exactly that, exhaustively per axis); the generator runs the groups
// the apron touches and stores only the samples inside it.
#ifndef JXL_NOISE_WINDOW_CHECK_H
#define JXL_NOISE_WINDOW_CHECK_H
#include <stdint.h>

#if defined(__HIPCC__)
#define JXL_NW_HD __host__ __device__
#else
#define JXL_NW_HD
#endif

namespace jxl {

constexpr int64_t kNoiseWindowMaxPixels = (int64_t)1 << 30;  // of the frame: above any frame the front-end accepts (2^28)
constexpr int kNoiseReach = 2;                               // the 5x5 kernel's reach

// MathHelper.mirrorCoordinate (MathHelper.java:323-329)
JXL_NW_HD inline int noise_mirror(int c, int size) {
    while (c < 0 || c >= size) {
        const int tc = ~c;
        c = tc >= 0 ? tc : (size << 1) + tc;
    }
    return c;
}

struct NoiseWindowPlan {
    int32_t frame_h = 0, frame_w = 0, group_dim = 0;
    int32_t y0 = 0, x0 = 0, win_h = 0, win_w = 0;  // the window
    int32_t ay0 = 0, ax0 = 0, ah = 0, aw = 0;      // the apron: rows [ay0, ay0 + ah), columns [ax0, ax0 + aw) of the frame
    int32_t gy0 = 0, gx0 = 0, gh = 0, gw = 0;      // the groups the apron touches, in groups
    int32_t n_groups = 0;                          // gh * gw
    int64_t apron_floats = 0;                      // ah * aw, per channel
    int64_t window_floats = 0;                     // win_h * win_w, per plane
};

// nullptr, or why the arguments are refused
inline const char* noise_window_check(int32_t group_dim, const float* lut, int32_t frame_h, int32_t frame_w, int32_t y0, int32_t x0,
                                      int32_t win_h, int32_t win_w, NoiseWindowPlan* p) {
    if (!lut || !p) return "noise window: null argument";
    if (group_dim < 16 || group_dim > (1 << 16) || (group_dim & (group_dim - 1))) return "noise window: group_dim is not a power of two from 16 up";
    if (frame_h < 1 || frame_w < 1 || (int64_t)frame_h * frame_w > kNoiseWindowMaxPixels) return "noise window: the frame size is out of range";
    if (win_h < 1 || win_w < 1) return "noise window: empty window";
    if (y0 < 0 || x0 < 0 || (int64_t)y0 + win_h > frame_h || (int64_t)x0 + win_w > frame_w) return "noise window: the window is not inside the frame";
    p->frame_h = frame_h; p->frame_w = frame_w; p->group_dim = group_dim;
    p->y0 = y0; p->x0 = x0; p->win_h = win_h; p->win_w = win_w;
    const int32_t ay0 = y0 - kNoiseReach < 0 ? 0 : y0 - kNoiseReach, ax0 = x0 - kNoiseReach < 0 ? 0 : x0 - kNoiseReach;
    const int64_t ay1w = (int64_t)y0 + win_h + kNoiseReach, ax1w = (int64_t)x0 + win_w + kNoiseReach;
    const int32_t ay1 = ay1w > frame_h ? frame_h : (int32_t)ay1w, ax1 = ax1w > frame_w ? frame_w : (int32_t)ax1w;
    p->ay0 = ay0; p->ax0 = ax0; p->ah = ay1 - ay0; p->aw = ax1 - ax0;
    p->gy0 = ay0 / group_dim; p->gx0 = ax0 / group_dim;
    p->gh = (ay1 - 1) / group_dim - p->gy0 + 1;
    p->gw = (ax1 - 1) / group_dim - p->gx0 + 1;
    const int64_t n_groups = (int64_t)p->gh * p->gw;
    if (n_groups > (1 << 24)) return "noise window: too many groups";
    p->n_groups = (int32_t)n_groups;
    p->apron_floats = (int64_t)p->ah * p->aw;
    p->window_floats = (int64_t)win_h * win_w;
    return nullptr;
}

// one axis of the claim the convolution launch rests on: every coordinate c + d, c in the window, |d| <= 2, mirrors into the apron
inline bool noise_window_axis_holds(int32_t size, int32_t w0, int32_t wn, int32_t a0, int32_t an) {
    for (int32_t c = w0; c < w0 + wn; c++)
        for (int d = -kNoiseReach; d <= kNoiseReach; d++) {
            const int m = noise_mirror(c + d, size);
            if (m < a0 || m >= a0 + an) return false;
        }
    return true;
}
inline bool noise_window_apron_holds(const NoiseWindowPlan& p) {
    return noise_window_axis_holds(p.frame_h, p.y0, p.win_h, p.ay0, p.ah) && noise_window_axis_holds(p.frame_w, p.x0, p.win_w, p.ax0, p.aw);
}

}  // namespace jxl
#endif  // JXL_NOISE_WINDOW_CHECK_H
