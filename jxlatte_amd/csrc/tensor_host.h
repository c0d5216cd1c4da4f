// What the tensor entries' host files (tensor_host.hip, tensor_resize_host.hip, tensor_batch_host.hip) share: the staging of
// host planes, the runtime check of out_device, the checks of one jxl_tensor_params, an image's home (image_home.h) in these
// entries' words, and -- of the resized entries -- the plan of a launch.
#ifndef JXL_TENSOR_HOST_H
#define JXL_TENSOR_HOST_H
#include "jxl_internal.h"
#include "tensor_check.h"
#include "tensor_resize_check.h"

#include <vector>

namespace jxl {

// a failed HIP call ends the entry: JXL_ERR_OOM or JXL_ERR_DEVICE with the runtime's words
#define TENSOR_HIP(c, expr)                                                                                                    \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess) return ctx_fail(c, e_ == hipErrorOutOfMemory ? JXL_ERR_OOM : JXL_ERR_DEVICE, hipGetErrorString(e_)); \
    } while (0)

// device copies of host planes, freed when the entry returns
struct Staged {
    std::vector<void*> v;
    ~Staged() { for (void* p : v) (void)hipFree(p); }
    const void* up(const void* host, size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes < 16 ? 16 : bytes) != hipSuccess) return nullptr;
        v.push_back(d);
        if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    // device memory the caller fills itself
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes < 16 ? 16 : bytes) != hipSuccess) return nullptr;
        v.push_back(d);
        return d;
    }
};

// out_device is device memory of the context's device and its allocation holds `bytes` bytes from there on
jxl_status tensor_out_check(jxl_ctx* c, const CtxLink& l, void* out, uint64_t bytes);
// every check of an entry but those of its planes' home: the kernel's arguments without the plane pointers. out_height /
// out_width: the tensor's size where it is not the planes' (the resized entries), else 0. check_out: false where the caller has
// asked tensor_out_check about an extent that holds this tensor (the batch entry: once, for all its tensors)
jxl_status tensor_args(jxl_ctx* c, const CtxLink& l, const jxl_tensor_params* p, const void* const in[3], const void* alpha, void* out,
                       TensorArgs* t, TensorLayout* lay, int32_t out_height = 0, int32_t out_width = 0, bool check_out = true);
// the alpha plane is read only where it is written or divides the colours
inline bool tensor_alpha_read(const jxl_tensor_params* p) { return p->has_alpha && (p->write_alpha || p->premultiplied); }

// ---- an image's home (image_home.h) in the tensor entries' words; host planes are home_host, resident ones ctx_home_resident ----
// a set's planes 0 .. n_planes - 1 and its plane alpha_plane: the first half (the set, a null p, the planes asked for)
jxl_status tensor_home_set(jxl_ctx* c, int32_t id, int32_t alpha_plane, const jxl_tensor_params* p, ImageHome* m);
// the second half, behind tensor_args / resize_args: the parameters describe the home
jxl_status tensor_home_fits(jxl_ctx* c, const ImageHome& m, const jxl_tensor_params* p);
// the plane pointers of g: planes on the device as they are, the others uploaded (the alpha plane only where it is read)
jxl_status tensor_place(jxl_ctx* c, const ImageHome& m, const jxl_tensor_params* p, PngArgs* g, Staged* s);

// ---- the resized entries (tensor_resize_host.hip), one image at a time or many (tensor_batch_host.hip) ----
// the workgroups the device holds at once: two per compute unit (the kernel's registers allow two waves per SIMD)
int64_t resize_slots(const CtxLink& l);
// the checks every resized entry makes first: the pure ones of the resize, then tensor_args with the tensor's size
jxl_status resize_args(jxl_ctx* c, const CtxLink& l, const jxl_tensor_params* p, const jxl_resize_params* rz, const void* const in[3],
                       const void* alpha, void* out, ResizeArgs* r, TensorLayout* lay, bool check_out = true);
// the tile (for `slots` workgroups at once, under the debug hooks' tile and skew) and the descriptor's geometry into r; the
// table and plane pointers of r are the caller's to set
jxl_status resize_plan(jxl_ctx* c, const jxl_tensor_params* p, const jxl_resize_params* rz, const TensorLayout& lay, const ResizeTaps& x,
                       const ResizeTaps& y, int64_t slots, ResizeArgs* r);
// r->wide_in from the plane pointers of r->t (resize_wide_in_ok)
void resize_set_wide_in(ResizeArgs* r);

}  // namespace jxl
#endif  // JXL_TENSOR_HOST_H
