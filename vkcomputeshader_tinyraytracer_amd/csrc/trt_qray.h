// trt_qray.h — the one validity predicate of a ray query record (abi.h trt_qray), shared by the
// host checker (trt_check_rays, trt_trace_rays with host pointers) and the query kernel
// (ray_query_kernel, which cannot be checked on the host when the records live on the device).
//
// A valid ray has six finite floats and a direction whose squared length
//   s = (dx * dx + dy * dy) + dz * dz        (FP32, the project's dot order, no contraction)
// lies in [TRT_QRAY_MIN_LEN2, TRT_QRAY_MAX_LEN2]: then 1 / sqrt(s) is a normal number, the
// shader's normalize (normalize3: d * (1 / sqrt(s))) is finite and of unit length, and s stays
// inside the fast domain of trt_math.h's square root.  Both translation units compile with
// -ffp-contract=off, so the host and the device compute the same s bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/trt/abi.h"

namespace trt {

__host__ __device__ inline bool qray_finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; } // false for NaN

__host__ __device__ inline bool qray_valid(float ox, float oy, float oz, float dx, float dy, float dz) {
    const float s = (dx * dx + dy * dy) + dz * dz;
    return qray_finite(ox) && qray_finite(oy) && qray_finite(oz) && qray_finite(dx) && qray_finite(dy) &&
           qray_finite(dz) && s >= TRT_QRAY_MIN_LEN2 && s <= TRT_QRAY_MAX_LEN2;
}

// A segment of an occlusion query (abi.h trt_qseg; trt_check_segs, trt_occluded with host pointers
// and occlusion_query_kernel): a valid ray cut off at 0 < tmax <= TRT_QSEG_MAX_T.  Both comparisons
// are false for a NaN; a subnormal tmax is positive on both sides (denormals are kept).
__host__ __device__ inline bool qseg_valid(float ox, float oy, float oz, float dx, float dy, float dz, float tmax) {
    return qray_valid(ox, oy, oz, dx, dy, dz) && tmax > 0.0f && tmax <= TRT_QSEG_MAX_T;
}

} // namespace trt
