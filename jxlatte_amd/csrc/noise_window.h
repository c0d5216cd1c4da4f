// k_noise_window.hip's launch (noise_window_host.hip calls it): the geometry is noise_window_check.h's plan, passed by value.
#pragma once
#include <hip/hip_runtime.h>

#include "noise_window_check.h"

namespace jxl {

// apron: three device planes of plan.apron_floats floats (scratch: the raw noise); planes: the window's three planes of
// plan.window_floats floats, updated in place. Two launches on s; nothing is waited for
void launch_noise_window(const NoiseWindowPlan& p, uint64_t seed0, float* const apron[3], float* const planes[3], const float lut[8],
                         float bcx, float bcb, hipStream_t s);

}  // namespace jxl
