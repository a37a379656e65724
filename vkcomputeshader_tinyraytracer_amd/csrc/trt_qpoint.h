// trt_qpoint.h — the arithmetic of a visibility query (abi.h trt_visibility) that the host and the
// kernel must agree on bit for bit: the validity predicate of a point record (abi.h trt_qpoint) and
// the one function that forms segment (i, k) from point i and set entry k.  Shared by
// visibility_query_kernel, trt_check_points, trt_point_segments and trt_visibility's host-pointer
// path; both translation units compile with -ffp-contract=off, so every product and sum below is
// rounded on its own on both sides.
//
// The square root of a TARGETS length is correctly rounded on both sides: sqrtf on the host,
// trt_math.h's sqrt_rn on the device (exact over every fp32 input, tests/test_gpu_fastmath.py).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/trt/abi.h"
#include "trt_qray.h"
#ifdef __HIP_DEVICE_COMPILE__
#include "trt_math.h"
#else
#include <cmath>
#endif

namespace trt {

// A valid point, in either mode: pos and n finite, 0 < tmax <= TRT_QSEG_MAX_T (false for a NaN; a
// subnormal tmax is positive on both sides).  n only chooses a side: any finite n will do.
__host__ __device__ inline bool qpoint_valid(float px, float py, float pz, float tmax, float nx, float ny, float nz) {
    return qray_finite(px) && qray_finite(py) && qray_finite(pz) && qray_finite(nx) && qray_finite(ny) &&
           qray_finite(nz) && tmax > 0.0f && tmax <= TRT_QSEG_MAX_T;
}

// A valid set entry: a valid ray direction for TRT_VIS_DIRS (qray_valid's length range), a finite
// point for TRT_VIS_TARGETS.  Host only in practice (the set is always a host array).
__host__ __device__ inline bool qset_entry_valid(uint32_t mode, float ex, float ey, float ez) {
    return mode == TRT_VIS_DIRS ? qray_valid(0.0f, 0.0f, 0.0f, ex, ey, ez)
                                : qray_finite(ex) && qray_finite(ey) && qray_finite(ez);
}

struct QPointSeg { float dx, dy, dz, tmax; }; // the origin is the point's pos

// Segment (i, k) of a visibility query: the direction and cut-off the kernel hands to the any-hit
// walk for point (p, ptmax, n) and set entry e.
//   DIRS:    s = (e.x n.x + e.y n.y) + e.z n.z;  dir = s < 0 ? -e : e (zero, -0.0 and n = 0 keep e);
//            tmax = the point's.
//   TARGETS: dir = e - p;  len = sqrt((dx dx + dy dy) + dz dz), scene.segments_between's bits;
//            tmax = min(len, the point's): the point's tmax is a range cap.  n is not read.
// A TARGETS segment may fail qseg_valid (a point on its target, or too far from it): it is formed
// as computed here and not traced.
__host__ __device__ inline QPointSeg qpoint_segment(uint32_t mode, float px, float py, float pz, float ptmax, float nx,
                                                    float ny, float nz, float ex, float ey, float ez) {
    if (mode == TRT_VIS_DIRS) {
        const float s = (ex * nx + ey * ny) + ez * nz;
        const bool flip = s < 0.0f;
        return QPointSeg{flip ? -ex : ex, flip ? -ey : ey, flip ? -ez : ez, ptmax};
    }
    const float dx = ex - px, dy = ey - py, dz = ez - pz;
    const float s = (dx * dx + dy * dy) + dz * dz;
#ifdef __HIP_DEVICE_COMPILE__
    const float len = sqrt_rn(s);
#else
    const float len = std::sqrt(s);
#endif
    return QPointSeg{dx, dy, dz, __builtin_fminf(len, ptmax)};
}

} // namespace trt
