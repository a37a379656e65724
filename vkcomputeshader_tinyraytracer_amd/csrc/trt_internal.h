// trt_internal.h — what trt_runtime.cpp, trt_scene_upload.cpp and trt_diag.cpp share.
#pragma once

#include <string>

#include "trt_ctx.h"

#pragma GCC visibility push(hidden) // internal to libtrt.so: none of this is exported
namespace trt {
hipError_t launch_trace(const KArgs& A, hipStream_t stream, bool count);
hipError_t launch_envp(const uint32_t* env, uint2* out, uint32_t W, uint32_t H, hipStream_t stream);
hipError_t launch_sky(const KArgs& A, uint32_t* out, hipStream_t stream);
hipError_t launch_shadow_batch(const KArgs& A, const float4* rays, uint32_t n, uint32_t* occ, hipStream_t stream);
hipError_t launch_ray_query(const KArgs& A, const float4* rays, uint32_t n, uint32_t* out8, float4* out32, uint4* hits,
                            bool count, hipStream_t stream);
hipError_t launch_occlusion_query(const KArgs& A, const float4* segs, uint32_t n, uint8_t* out, hipStream_t stream);
hipError_t launch_all_hits(const KArgs& A, const float4* segs, uint32_t n, uint32_t max_hits, uint4* hits, uint32_t* counts,
                           hipStream_t stream);
hipError_t launch_visibility_query(const KArgs& A, const float4* pts, uint32_t npts, const float4* set, uint32_t nset,
                                   uint32_t mode, bool coop, uint64_t* out, hipStream_t stream);
namespace jpeg { struct Image; const Image* image_of(const trt_jpeg* j); }

int fail(trt_ctx* c, int code, const std::string& msg);
int hip_fail(trt_ctx* c, hipError_t e, const char* what);
#define HIP_TRY(ctx, expr)                                            \
    do {                                                              \
        hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) return trt::hip_fail((ctx), e_, #expr); \
    } while (0)
int ensure(trt_ctx* c, void** p, size_t* cap, size_t bytes, const char* what);
void free_scene(trt_ctx* c);
int check_params(trt_ctx* c, const trt_params* p);
void fill_args(trt_ctx* c, const trt_params* p, KArgs& A);
int ensure_envp(trt_ctx* c, const trt_params* p, hipStream_t stream);
uint32_t floor_lit(uint32_t flags, const float (*light)[3]);
} // namespace trt
#pragma GCC visibility pop
