// Where a decoded image is when it leaves the library -- host planes (jxl_stage_*), the context's three resident float planes
// (jxl_planes_*), a plane set of the canvas store (jxl_canvas_*, JXL_BATCH_SET) -- and the questions every exit (PNG, PFM, colour
// peak, tensor, resized tensor, batch) asks of it: is it there, has it the planes asked for, do the parameters describe it, and
// which planes have still to go to the device. Plain C++ (no device code, no context), so the rules can be compiled and run on
// their own. The answers are codes: each exit family has one place where a code becomes its own words.
#pragma once
#include <cstdint>

#include "../../include/jxlatte_amd.h"

namespace jxl {

// a set as the exits read it (canvas_view, canvas_host.hip)
struct CanvasView {
    int32_t n, h, w;
    int32_t type[JXL_CANVAS_MAX_PLANES];
    const uint32_t* plane[JXL_CANVAS_MAX_PLANES];
};

enum HomeKind { HOME_HOST, HOME_RESIDENT, HOME_SET };
enum HomeRefusal { HOME_OK, HOME_UNKNOWN_SET, HOME_NO_SUCH_PLANES, HOME_NOT_DESCRIBED };

struct ImageHome {
    HomeKind kind;
    HomeRefusal planes;    // the first half: the home exists and has the planes asked for
    int32_t h, w;          // 0 x 0 for host planes: the parameters are their size
    int32_t n;             // the planes it has (host planes: unknown, 0)
    const void* color[3];  // null behind the planes asked for
    bool no_array;         // host planes given as a null array
    bool color_int[3];     // int32, else float (host planes: what the parameters say)
    const void* alpha;
    bool alpha_int;
    bool alpha_on_device;
    // the colour planes as an entry's argument checks take them (they refuse a null array in their own words)
    const void* const* in() const { return no_array ? nullptr : color; }
};

inline ImageHome home_host(const void* const in[3], const void* alpha) {
    ImageHome m{};
    m.kind = HOME_HOST;
    m.no_array = !in;
    for (int i = 0; i < 3 && in; i++) m.color[i] = in[i];
    m.alpha = alpha;
    return m;
}

inline ImageHome home_resident(int32_t h, int32_t w, const void* const planes[3], const void* alpha) {
    ImageHome m{};
    m.kind = HOME_RESIDENT;
    m.h = h, m.w = w, m.n = 3;
    for (int i = 0; i < 3; i++) m.color[i] = planes[i];
    m.alpha = alpha;
    return m;
}

// planes 0 .. n_color - 1 of the set and, with has_alpha, its plane alpha_plane (else -1). v: null for an unknown id
inline ImageHome home_set(const CanvasView* v, int32_t n_color, int32_t alpha_plane, bool has_alpha) {
    ImageHome m{};
    m.kind = HOME_SET;
    m.alpha_on_device = true;
    if (!v) return m.planes = HOME_UNKNOWN_SET, m;
    m.h = v->h, m.w = v->w, m.n = v->n;
    if ((n_color != 1 && n_color != 3) || n_color > v->n || alpha_plane < -1 || alpha_plane >= v->n || has_alpha != (alpha_plane >= 0))
        return m.planes = HOME_NO_SUCH_PLANES, m;
    for (int i = 0; i < n_color; i++) m.color[i] = v->plane[i], m.color_int[i] = v->type[i] == JXL_PLANE_INT32;
    if (alpha_plane >= 0) m.alpha = v->plane[alpha_plane], m.alpha_int = v->type[alpha_plane] == JXL_PLANE_INT32;
    return m;
}

// the second half: height x width, n_color colour planes tagged is_int[i] and an alpha plane tagged alpha_is_int are what the
// home holds. Host planes are what the parameters say; an alpha plane that comes from the host is too
inline HomeRefusal home_describes(const ImageHome& m, int32_t height, int32_t width, int32_t n_color, const int32_t is_int[3], int32_t alpha_is_int) {
    if (m.kind == HOME_HOST) return HOME_OK;
    if (m.planes != HOME_OK) return m.planes;
    if (height != m.h || width != m.w) return HOME_NOT_DESCRIBED;
    if (m.kind == HOME_RESIDENT ? n_color != 3 : (n_color < 1 || n_color > 3 || n_color > m.n)) return HOME_NOT_DESCRIBED;
    for (int i = 0; i < n_color; i++)
        if ((is_int[i] != 0) != m.color_int[i]) return HOME_NOT_DESCRIBED;
    if (m.alpha && m.alpha_on_device && (alpha_is_int != 0) != m.alpha_int) return HOME_NOT_DESCRIBED;
    return HOME_OK;
}
// the same with one tag for every colour plane
inline HomeRefusal home_describes(const ImageHome& m, int32_t height, int32_t width, int32_t n_color, int32_t color_is_int, int32_t alpha_is_int) {
    const int32_t is_int[3] = {color_is_int, color_is_int, color_is_int};
    return home_describes(m, height, width, n_color, is_int, alpha_is_int);
}

// which planes have still to go to the device (whether the alpha plane is read at all is the entry's to say)
struct HomeUploads {
    bool color, alpha;
};
inline HomeUploads home_uploads(const ImageHome& m) { return HomeUploads{m.kind == HOME_HOST, !m.alpha_on_device}; }

}  // namespace jxl
