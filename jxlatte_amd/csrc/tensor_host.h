// What the tensor entries' two host files (tensor_host.hip, tensor_resize_host.hip) share: the staging of host planes, the
// runtime check of out_device and the checks of one jxl_tensor_params.
#ifndef JXL_TENSOR_HOST_H
#define JXL_TENSOR_HOST_H
#include "jxl_internal.h"
#include "tensor_check.h"

#include <vector>

namespace jxl {

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
};

// out_device is device memory of the context's device and its allocation holds `bytes` bytes from there on
jxl_status tensor_out_check(jxl_ctx* c, const CtxLink& l, void* out, uint64_t bytes);
// every check of an entry but those of its planes' home: the kernel's arguments without the plane pointers. out_height /
// out_width: the tensor's size where it is not the planes' (the resized entries), else 0
jxl_status tensor_args(jxl_ctx* c, const CtxLink& l, const jxl_tensor_params* p, const void* const in[3], const void* alpha, void* out,
                       TensorArgs* t, TensorLayout* lay, int32_t out_height = 0, int32_t out_width = 0);
// the alpha plane is read only where it is written or divides the colours
inline bool tensor_alpha_read(const jxl_tensor_params* p) { return p->has_alpha && (p->write_alpha || p->premultiplied); }

}  // namespace jxl
#endif  // JXL_TENSOR_HOST_H
