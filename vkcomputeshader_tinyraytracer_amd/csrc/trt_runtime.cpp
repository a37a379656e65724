// trt_runtime.cpp — the C-ABI (include/trt/abi.h) over the HIP runtime: the context's lifecycle,
// the setters and the render and query entry points.
//
// Replaces the reference's Vulkan compute plumbing: createShaderStorageBuffers() /
// createUniformBuffers() / the background texture upload (main.cpp:928-1111, 1494-1664)
// become trt_upload_scene() (trt_scene_upload.cpp); updateUniformBuffer() (main.cpp:2165-2179)
// becomes trt_update_ubo(); recordComputeCommandBuffer() + vkQueueSubmit (main.cpp:2108-2131,
// 2181-2205) become trt_render().  No exception crosses the ABI; failures set the context's
// last error and return a negative TRT_ERR_* code (the reference throws std::runtime_error
// and exits, main.cpp:2565-2573).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "jpeg.h"
#include "scene_pack.h"
#include "trt_bands.h"
#include "trt_internal.h"
#include "trt_qpoint.h"
#include "trt_qray.h"

namespace trt {
// HIP creates a stream's hardware queue at its first submission, which costs ~0.1 ms: every
// stream the library creates gets a 4-byte fill of scratch memory (then a sync) right away, so
// that cost never lands in a frame loop.
hipError_t touch_stream(hipStream_t s, void* scratch) {
    hipError_t e = hipMemsetAsync(scratch, 0, 4, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

int fail(trt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int hip_fail(trt_ctx* c, hipError_t e, const char* what) {
    // an allocation failure is reported through the return code; its sticky last-error state
    // must not surface in the caller's next HIP call (a torch launch check)
    if (e == hipErrorOutOfMemory) (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? TRT_ERR_OOM : TRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Grow-only device scratch buffer.
int ensure(trt_ctx* c, void** p, size_t* cap, size_t bytes, const char* what) {
    if (bytes <= *cap && *p) return TRT_OK;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return hip_fail(c, e, what);
    *cap = bytes;
    return TRT_OK;
}
} // namespace trt

using namespace trt;

namespace {

// Failure injection (tests only, with TRT_ENABLE_TEST_HOOKS=1): TRT_TEST_FAIL_DEFER_SLOT=k makes
// the deferred-frame scratch allocation of in-flight slot k report out-of-memory.
int test_fail_defer_slot() {
    const char* on = std::getenv("TRT_ENABLE_TEST_HOOKS");
    const char* e = std::getenv("TRT_TEST_FAIL_DEFER_SLOT");
    return (on && std::atoi(on) == 1 && e) ? std::atoi(e) : -1;
}

void fill_ubo_args(KArgs& A, const trt_ubo& u) {
    const trt_sphere* s[4] = {&u.sphere0, &u.sphere1, &u.sphere2, &u.sphere3};
    for (int i = 0; i < 4; ++i) {
        std::memcpy(A.sph[i].c, &s[i]->center_radius, sizeof(A.sph[i].c)); // x, y, z
        A.sph[i].r = s[i]->center_radius.w;
        A.sph[i].m = to_mat(s[i]->material);
    }
    const trt_vec4* l[3] = {&u.light0, &u.light1, &u.light2};
    for (int i = 0; i < 3; ++i) std::memcpy(A.light[i], l[i], sizeof(A.light[i])); // x, y, z
}

void fill_frame(trt::FrameRec& f, const trt_ubo& u, uint8_t* out8, bool in_place) {
    std::memcpy(f.cam, &u.camPos, sizeof(f.cam)); // x, y, z
    f.in_place = in_place ? 1u : 0u;
    f.out8 = reinterpret_cast<uint32_t*>(out8);
}

// Views (abi.h trt_view).  The reference camera's 36 bytes are "no view": such a frame is not
// oriented and runs what it ran before there were views.
const trt_view kViewIdentity{{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
bool view_is_identity(const trt_view& v) { return std::memcmp(&v, &kViewIdentity, sizeof(trt_view)) == 0; }
bool view_is_finite(const trt_view& v) {
    const float* f = v.right; // right, up, back: nine consecutive floats
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(f[i])) return false;
    return true;
}
// Frame f's basis of an oriented launch (KArgs::view): right[3], up[3], back[3].
void fill_view(KArgs& A, uint32_t f, const trt_view& v) {
    static_assert(sizeof(trt_view) == sizeof(A.view[0]), "a view is nine floats");
    std::memcpy(A.view[f], &v, sizeof(trt_view));
}

// dir_z = -1.0 * (HEIGHT / (2.0 * tan(fov / 2.0))) in double, main.cpp:1503: the one expression
// behind KArgs::dz (fill_args), trt_view_rays and trt_pixel_ray.
float view_dz(const trt_params* p) { return (float)(-1.0 * ((double)p->height / (2.0 * std::tan((double)p->fov / 2.0)))); }
// Steps 1 and 2 of the view contract (abi.h trt_view) for one pixel at spp 1: primary_dir's spp-1
// arithmetic, operation for operation (this file compiles with -ffp-contract=off).
void view_pixel_dir(const trt_params* p, const trt_view& V, float dz, uint32_t x, uint32_t y, float w[3]) {
    const uint32_t W = p->width, H = p->height;
    const uint32_t row = ((p->flags & TRT_FLAG_ROW_QUIRK) && x + 1u == W) ? y + 1u : y;
    const float dx = ((float)x + 0.5f) - (float)W * 0.5f;
    const float dy = -((float)row + 0.5f) + (float)H * 0.5f;
    const float inv = 1.0f / std::sqrt((dx * dx + dy * dy) + dz * dz);
    const float cx = dx * inv, cy = dy * inv, cz = dz * inv;
    for (int a = 0; a < 3; ++a) w[a] = (cx * V.right[a] + cy * V.up[a]) + cz * V.back[a];
}

// Frames that may share a launch: every UBO field but camPos equal (byte-wise).
bool same_but_camera(const trt_ubo& a, const trt_ubo& b) {
    constexpr size_t cam = offsetof(trt_ubo, camPos);
    return std::memcmp(&a, &b, cam) == 0 &&
           std::memcmp(reinterpret_cast<const char*>(&a) + cam + sizeof(trt_vec4),
                       reinterpret_cast<const char*>(&b) + cam + sizeof(trt_vec4),
                       sizeof(trt_ubo) - cam - sizeof(trt_vec4)) == 0;
}

// trt_check_rays / trt_check_segs: TRT_OK, or TRT_ERR_INVALID with the first record that fails.
template <class R, class Valid>
int first_invalid(const R* recs, uint32_t n, uint32_t* first_bad, Valid valid) {
    if (first_bad) *first_bad = 0;
    if (n && !recs) return TRT_ERR_INVALID;
    for (uint32_t i = 0; i < n; ++i) {
        if (valid(recs[i])) continue;
        if (first_bad) *first_bad = i;
        return TRT_ERR_INVALID;
    }
    return TRT_OK;
}

// The direction or target set of a visibility query (trt_visibility, trt_point_segments): a known
// mode, 1..TRT_VIS_MAX_SET entries, each valid for the mode.  *bad (may be null): the first entry
// that fails, or nset when the mode, the count or a null array is at fault.
int check_vis_set(const float* set, uint32_t nset, uint32_t mode, uint32_t* bad) {
    if (bad) *bad = nset;
    if ((mode != TRT_VIS_DIRS && mode != TRT_VIS_TARGETS) || nset < 1u || nset > TRT_VIS_MAX_SET || !set) return TRT_ERR_INVALID;
    for (uint32_t k = 0; k < nset; ++k) {
        if (trt::qset_entry_valid(mode, set[4 * k], set[4 * k + 1], set[4 * k + 2])) continue;
        if (bad) *bad = k;
        return TRT_ERR_INVALID;
    }
    return TRT_OK;
}

// A new context's knobs; the per-call ones, which tests change between calls, are read per call.
void read_env_knobs(trt_ctx* c) {
    if (const char* e = std::getenv("TRT_BVH_WAVES4")) c->bvh_waves4 = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = std::getenv("TRT_SPP_LANES")) c->spp_lanes = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_VIS_COOP")) c->vis_coop = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_DEFER_PPW")) { // pass-A pixels per wave: 64, 32, 16 or 8
        const int ppw = std::atoi(e);
        c->defer_sub = ppw == 8 ? 8u : ppw == 16 ? 4u : ppw == 32 ? 2u : ppw == 64 ? 1u : 0u;
    }
    if (const char* e = std::getenv("GPU_MAX_HW_QUEUES")) c->hw_queues = (uint32_t)std::max(1, std::atoi(e));
    if (const char* e = std::getenv("TRT_DEFER_INTER")) c->defer_inter = (uint32_t)std::min(2, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("TRT_DEFER_GROUP"))
        c->defer_group = (uint32_t)std::min((int)trt::kMaxLaunchFrames, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("TRT_DEFER_IN_FLIGHT")) {
        c->defer_in_flight = (uint32_t)std::min((int)TRT_BUILD_MAX_IN_FLIGHT, std::max(1, std::atoi(e)));
        c->defer_in_flight_set = true;
    }
    if (const char* e = std::getenv("TRT_XCD_ROT")) c->xcd_rot = (uint32_t)std::min(8, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("TRT_XCD_SKEW")) c->xcd_skew = (uint32_t)std::min(7, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("TRT_XCD_INTER")) c->xcd_inter = (uint32_t)std::min(2, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("TRT_FRAME_GROUP")) c->frame_group = std::min(2, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("TRT_SKY_TABLE")) c->sky_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_SKY_SPANS")) c->span_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_SKY_SPAN_FRAMES")) c->span_frames = (uint32_t)std::min(64, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("TRT_SHADOW_MASK")) c->smask_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_FLOOR_CLASS")) c->floor_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_FLOOR_LIT")) c->floor_lit_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("TRT_SHADOW_MASK_CELL")) { // floor cell edge; the build clamps it
        const float v = (float)std::atof(e);
        if (v > 0.0f) c->smask_cell = v;
    }
}

} // namespace

extern "C" {

#define TRT_STR2(x) #x
#define TRT_STR(x) TRT_STR2(x)
const char* trt_version(void) { return "trt-mi355x 0.2 (gfx950, abi " TRT_STR(TRT_ABI_VERSION) ")"; }

int trt_set_view(trt_ctx* c, const trt_view* v) {
    if (!c) return TRT_ERR_INVALID;
    if (v && !view_is_finite(*v)) return fail(c, TRT_ERR_INVALID, "trt_set_view: the view is not finite");
    c->view = v ? *v : kViewIdentity;
    c->view_on = !view_is_identity(c->view);
    return TRT_OK;
}

int trt_view_look(trt_view* out, const float front[3], const float world_up[3]) {
    if (!out || !front || !world_up) return TRT_ERR_INVALID;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(front[a]) || !std::isfinite(world_up[a])) return TRT_ERR_INVALID;
    const float fl = std::sqrt((front[0] * front[0] + front[1] * front[1]) + front[2] * front[2]);
    if (!(fl > 0.0f) || !std::isfinite(fl)) return TRT_ERR_INVALID;
    const float f[3] = {front[0] / fl, front[1] / fl, front[2] / fl};
    // cross(front, up): the right vector processInput walks along (main.cpp:391-403)
    float r[3] = {f[1] * world_up[2] - world_up[1] * f[2], f[2] * world_up[0] - world_up[2] * f[0],
                  f[0] * world_up[1] - world_up[0] * f[1]};
    const float rl = std::sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const float ul = std::sqrt((world_up[0] * world_up[0] + world_up[1] * world_up[1]) + world_up[2] * world_up[2]);
    if (!std::isfinite(rl) || !std::isfinite(ul) || !(rl > 1e-6f * ul)) return TRT_ERR_INVALID; // zero up, or front || up
    for (int a = 0; a < 3; ++a) r[a] = r[a] / rl;
    const float u[3] = {r[1] * f[2] - f[1] * r[2], r[2] * f[0] - f[2] * r[0], r[0] * f[1] - f[0] * r[1]};
    for (int a = 0; a < 3; ++a) {
        out->right[a] = r[a] + 0.0f; // -0.0 -> +0.0: the reference's vectors give the identity bytes
        out->up[a] = u[a] + 0.0f;
        out->back[a] = -f[a] + 0.0f;
    }
    return TRT_OK;
}

int trt_view_rays(const trt_params* p, const trt_view* v, trt_ray* out) {
    if (!p || !out || p->width == 0 || p->height == 0 || p->width > 65536 || p->height > 65536) return TRT_ERR_INVALID;
    const trt_view& V = v ? *v : kViewIdentity;
    const uint32_t W = p->width, H = p->height;
    const float dz = view_dz(p);
    for (uint32_t y = 0; y < H; ++y) {
        for (uint32_t x = 0; x < W; ++x) {
            trt_ray& r = out[(size_t)y * W + x];
            std::memset(&r, 0, sizeof(r));
            float w[3];
            view_pixel_dir(p, V, dz, x, y, w);
            r.dir = {w[0], w[1], w[2], 1.0f};
        }
    }
    return TRT_OK;
}

int trt_pixel_ray(const trt_params* p, const trt_view* v, const float cam[3], uint32_t x, uint32_t y, trt_qray* out) {
    if (!p || !cam || !out || p->width == 0 || p->height == 0 || p->width > 65536 || p->height > 65536) return TRT_ERR_INVALID;
    if (x >= p->width || y >= p->height) return TRT_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    view_pixel_dir(p, v ? *v : kViewIdentity, view_dz(p), x, y, out->dir);
    for (int a = 0; a < 3; ++a) out->org[a] = cam[a];
    return TRT_OK;
}

int trt_check_rays(const trt_qray* rays, uint32_t n, uint32_t* first_bad) {
    return first_invalid(rays, n, first_bad, [](const trt_qray& r) {
        return trt::qray_valid(r.org[0], r.org[1], r.org[2], r.dir[0], r.dir[1], r.dir[2]);
    });
}

int trt_check_segs(const trt_qseg* segs, uint32_t n, uint32_t* first_bad) {
    return first_invalid(segs, n, first_bad, [](const trt_qseg& s) {
        return trt::qseg_valid(s.org[0], s.org[1], s.org[2], s.dir[0], s.dir[1], s.dir[2], s.tmax);
    });
}

int trt_check_points(const trt_qpoint* pts, uint32_t n, uint32_t* first_bad) {
    return first_invalid(pts, n, first_bad, [](const trt_qpoint& q) {
        return trt::qpoint_valid(q.pos[0], q.pos[1], q.pos[2], q.tmax, q.n[0], q.n[1], q.n[2]);
    });
}

int trt_point_segments(const trt_qpoint* pts, uint32_t npts, const float* set, uint32_t nset, uint32_t mode, trt_qseg* out) {
    if (check_vis_set(set, nset, mode, nullptr) != TRT_OK) return TRT_ERR_INVALID;
    if (trt_check_points(pts, npts, nullptr) != TRT_OK || (npts && !out)) return TRT_ERR_INVALID;
    for (uint32_t i = 0; i < npts; ++i) {
        const trt_qpoint& q = pts[i];
        for (uint32_t k = 0; k < nset; ++k) {
            const float* e = set + 4 * (size_t)k;
            const trt::QPointSeg s =
                trt::qpoint_segment(mode, q.pos[0], q.pos[1], q.pos[2], q.tmax, q.n[0], q.n[1], q.n[2], e[0], e[1], e[2]);
            out[(size_t)i * nset + k] = trt_qseg{{q.pos[0], q.pos[1], q.pos[2]}, s.tmax, {s.dx, s.dy, s.dz}, 0.0f};
        }
    }
    return TRT_OK;
}

void trt_params_default(trt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->width = 1024;  // main.cpp:35
    p->height = 768;  // main.cpp:36
    p->max_depth = 20; // shader.comp:75
    p->spp = 1;
    p->fov = 1.05f; // main.cpp:1498
    p->flags = TRT_FLAGS_REFERENCE;
}

uint32_t trt_output_rows(const trt_params* p) {
    if (!p) return 0;
    if (p->band_rows == 0 || p->band_count <= 1) return p->height;
    if (p->band_index >= p->band_count) return 0;
    return trt::band_group_rows(p->height, p->band_rows, p->band_count, p->band_index);
}

int trt_create(trt_ctx** out, int hip_device) {
    if (!out) return TRT_ERR_INVALID;
    *out = nullptr;
    trt_ctx* c = new (std::nothrow) trt_ctx();
    if (!c) return TRT_ERR_OOM;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || hip_device < 0 || hip_device >= n) {
        delete c;
        return TRT_ERR_HIP;
    }
    c->device = hip_device;
    if (hipSetDevice(hip_device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc((void**)&c->d_counters, 32 * sizeof(unsigned long long)) != hipSuccess) {
        trt_destroy(c);
        return TRT_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0)
        c->num_cus = (uint32_t)prop.multiProcessorCount;
    c->stream = c->own_stream;
    if (trt::touch_stream(c->own_stream, c->d_counters) != hipSuccess) {
        trt_destroy(c);
        return TRT_ERR_HIP;
    }
    read_env_knobs(c);
    *out = c;
    return TRT_OK;
}

int trt_destroy(trt_ctx* c) {
    if (!c) return TRT_ERR_INVALID;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
    // frames of earlier trt_render calls may still run on other streams (render_slot): every
    // buffer below may be in use until the device drains
    (void)hipDeviceSynchronize();
    free_scene(c);
    for (void* p : {(void*)c->d_envp, (void*)c->d_sky, (void*)c->d_smask, c->d_out8, c->d_out32, c->d_rays, c->d_qrays,
                    c->d_qhits, c->d_visset, (void*)c->d_counters})
        (void)hipFree(p);
    for (hipEvent_t e : c->fev) (void)hipEventDestroy(e);
    for (auto& b : c->split) {
        for (void* p : {(void*)b.q[0], (void*)b.q[1], (void*)b.qlink[0], (void*)b.qlink[1], (void*)b.acc, (void*)b.spilled,
                        (void*)b.ctr, (void*)b.ev, (void*)b.shq, (void*)b.px_ev, (void*)b.fb, (void*)b.dctr})
            (void)hipFree(p);
        if (b.done) (void)hipEventDestroy(b.done);
    }
    for (hipStream_t s : c->aux) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    for (hipEvent_t e : c->aux_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->fork_ev, c->ev0, c->ev1})
        if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return TRT_OK;
}

const char* trt_last_error(const trt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int trt_set_stream(trt_ctx* c, void* s) {
    if (!c) return TRT_ERR_INVALID;
    c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
    return TRT_OK;
}

int trt_set_frames_in_flight(trt_ctx* c, uint32_t n) {
    if (!c) return TRT_ERR_INVALID;
    if (n > TRT_BUILD_MAX_IN_FLIGHT)
        return fail(c, TRT_ERR_INVALID, "trt_set_frames_in_flight: n must be 0 (auto) or in [1, TRT_MAX_FRAMES_IN_FLIGHT]");
    c->frames_in_flight = n;
    return TRT_OK;
}

int trt_set_subtree_split(trt_ctx* c, int window) {
    if (!c) return TRT_ERR_INVALID;
    if (window != TRT_SPLIT_AUTO && window != TRT_SPLIT_OFF && (window < 2 || window > 5))
        return fail(c, TRT_ERR_INVALID, "trt_set_subtree_split: window must be 0 (auto), 1 (off) or 2..5");
    c->subtree_split = window;
    return TRT_OK;
}

int trt_set_deferred_shadows(trt_ctx* c, int mode) {
    if (!c) return TRT_ERR_INVALID;
    if (mode != TRT_DEFER_AUTO && mode != TRT_DEFER_OFF && mode != TRT_DEFER_ON)
        return fail(c, TRT_ERR_INVALID, "trt_set_deferred_shadows: mode must be TRT_DEFER_AUTO, _OFF or _ON");
    c->deferred_shadows = mode;
    return TRT_OK;
}

int trt_defer_stats(trt_ctx* c, uint32_t slot, uint64_t out[5]) {
    if (!c || !out) return TRT_ERR_INVALID;
    if (slot >= TRT_BUILD_MAX_IN_FLIGHT) return fail(c, TRT_ERR_INVALID, "trt_defer_stats: slot out of range");
    const auto& b = c->split[slot];
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!b.dctr) return TRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (b.last && b.done) HIP_TRY(c, hipEventSynchronize(b.done));
    trt::DeferCtr d{};
    HIP_TRY(c, hipMemcpy(&d, b.dctr, sizeof(d), hipMemcpyDeviceToHost));
    // taken = min(requested, the stripe capacity the slot's last frame ran with: its own size or
    // a test hook's, not the slot's allocation, which may be larger)
    const size_t ev_s = b.used_ev_cap, q_s = b.used_shq_cap;
    for (uint32_t s = 0; s < trt::kDeferStripes; ++s) {
        out[0] += std::min<size_t>(d.chunks[s * trt::kCtrStride], ev_s);
        out[1] += std::min<size_t>(d.nq[s * trt::kCtrStride], q_s);
    }
    out[2] = d.nfb;
    out[3] = b.ev_chunks;
    out[4] = b.shq_cap;
    return TRT_OK;
}

int trt_synchronize(trt_ctx* c) {
    if (!c) return TRT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return TRT_OK;
}

int trt_update_ubo(trt_ctx* c, const trt_ubo* ubo) {
    if (!c || !ubo) return fail(c, TRT_ERR_INVALID, "trt_update_ubo: null argument");
    c->ubo = *ubo;
    return TRT_OK;
}

} // extern "C"

namespace trt {

// Builds the envmap pair rows (KArgs::envp) on `stream` when d_env changed since the last
// build.  Without them (TRT_ENV_PAIRROWS=0 in the environment) env_fetch reads d_env directly.
int ensure_envp(trt_ctx* c, const trt_params* p, hipStream_t stream) {
    if (!(p->flags & TRT_FLAG_ENVMAP) || !c->d_env || c->envp_ok) return TRT_OK;
    if (const char* e = std::getenv("TRT_ENV_PAIRROWS"))
        if (std::atoi(e) == 0) return TRT_OK;
    const size_t bytes = ((size_t)c->env_h + 2) * ((size_t)c->env_w + 3) * sizeof(uint2);
    if (bytes > c->envp_cap) {
        HIP_TRY(c, hipStreamSynchronize(stream));
        (void)hipFree(c->d_envp);
        c->d_envp = nullptr;
        c->envp_cap = 0;
        HIP_TRY(c, hipMalloc((void**)&c->d_envp, bytes));
        c->envp_cap = bytes;
    }
    HIP_TRY(c, trt::launch_envp(c->d_env, c->d_envp, c->env_w, c->env_h, stream));
    // once per envmap upload: wait for the build, since later frames may run on streams not
    // ordered after `stream` (trt_multi's two batch slots fork before the first batch builds)
    HIP_TRY(c, hipStreamSynchronize(stream));
    c->envp_ok = true;
    return TRT_OK;
}

// attach_floor_class's floor_lit (kFloorLit beside the class bit, sky_trace_kernel_floor_lit): the
// floor's three channels are one value and every light shines on its upper side, which floor_frame LIT relies on.
// Not under TRT_FLOOR_LIT=0: the launch then runs sky_trace_kernel_floor as before.
uint32_t floor_lit(uint32_t flags, const float (*light)[3]) {
    if (flags & TRT_FLAG_CHECKER) return 0u;
    for (int i = 0; i < 3; ++i)
        if (!(light[i][1] + 4.0f > trt::kFloorLitPad)) return 0u; // NaN too
    return 1u;
}

int check_params(trt_ctx* c, const trt_params* p) {
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_render: null params");
    if (!c->have_scene) return fail(c, TRT_ERR_NOSCENE, "trt_render: no scene uploaded");
    if (p->width == 0 || p->height == 0 || p->width > 65536 || p->height > 65536)
        return fail(c, TRT_ERR_INVALID, "trt_render: image size out of range");
    if (p->max_depth < 1 || p->max_depth > TRT_MAX_DEPTH_LIMIT)
        return fail(c, TRT_ERR_INVALID, "trt_render: max_depth must be 1..20");
    if (p->spp > 4096) return fail(c, TRT_ERR_INVALID, "trt_render: spp must be <= 4096");
    if (p->band_rows && p->band_count > 1 && p->band_index >= p->band_count)
        return fail(c, TRT_ERR_INVALID, "trt_render: band_index >= band_count");
    if ((p->flags & TRT_FLAG_BAND_IN_PLACE) && !(p->flags & TRT_FLAG_DEVICE_PTRS))
        return fail(c, TRT_ERR_INVALID, "trt_render: TRT_FLAG_BAND_IN_PLACE needs TRT_FLAG_DEVICE_PTRS");
    if ((p->flags & TRT_FLAG_ENVMAP) && !c->d_env)
        return fail(c, TRT_ERR_INVALID, "trt_render: TRT_FLAG_ENVMAP without an uploaded envmap");
    return TRT_OK;
}

// Everything of KArgs that does not depend on the UBO or the output pointers.
void fill_args(trt_ctx* c, const trt_params* p, KArgs& A) {
    std::memset(&A, 0, sizeof(A));
    A.width = p->width;
    A.height = p->height;
    A.rows = trt_output_rows(p);
    A.band_rows = p->band_rows;
    A.band_count = p->band_count;
    A.band_index = p->band_index;
    A.max_depth = p->max_depth;
    A.spp = p->spp ? p->spp : 1;
    // spp a power of two in [2, 64] and no replayed rays: one lane per sample (trace_samples;
    // TRT_SPP_LANES=0 keeps the per-pixel sample loop)
    A.spp_lanes = (A.spp >= 2u && A.spp <= 64u && (A.spp & (A.spp - 1u)) == 0u && !p->rays_in && c->spp_lanes) ? 1u : 0u;
    A.seed = p->seed;
    A.flags = p->flags;
    A.dz = view_dz(p);
    A.nbatch = c->nbatch;
    fill_ubo_args(A, c->ubo);
    A.nframes = 1;
    fill_frame(A.fr[0], c->ubo, nullptr, (p->flags & TRT_FLAG_BAND_IN_PLACE) != 0);
    // the context's view (trt_set_view); replayed rays are the caller's directions and win
    A.view_on = (c->view_on && !p->rays_in) ? 1u : 0u;
    if (A.view_on) fill_view(A, 0, c->view);
    A.batches = c->d_batches;
    A.geo = c->d_geo;
    A.shade = c->d_shade;
    A.mats = c->d_mats;
    A.env = c->d_env;
    A.envp = c->envp_ok ? c->d_envp : nullptr;
    A.env_w = c->env_w;
    A.env_h = c->env_h;
    A.counters = c->d_counters;
    A.nodes = c->d_nodes;
    A.bvh = c->d_bvh;
    A.bvh4 = c->d_bvh4;
    A.bvh4q = c->d_bvh4q;
    A.diag = reinterpret_cast<float4*>(c->diag);
    A.bvh_tris = c->d_bvh_tris;
    A.top = c->top;
    std::memcpy(A.node_off, c->node_off, sizeof(A.node_off));
    A.ntx = (A.width + 7u) / 8u;
    A.ntiles = A.ntx * ((A.rows + 7u) / 8u);
    // The BVH walk at 4 waves per SIMD (GEOM 3: <= 128 VGPRs, 16-entry LDS stack, quantized
    // nodes) hides more of the node-fetch latency than the 3-wave build.  Round 1 measured it
    // for large scenes only (C4 -13 %, C3 / shipped frame +1 %, profiles/r01_ab_occupancy.log);
    // since the traversal stack's index left scratch memory (round 3) it is ahead or equal
    // everywhere: C4 2.90 vs 3.38 ms, C3 -9 %, shipped frame and README scene within 1 %
    // (profiles/r03_ab_waves4_after_stack_fix.log), so it is the default for every BVH scene.
    // GEOM 3 kernels walk only the quantized nodes (trt_kernel.hip g3_quant_only): a scene whose
    // nodes did not quantize (or whose 4-wide stack would not fit) takes the GEOM 2 kernels.
    A.bvh_waves4 = c->d_bvh4q ? (c->bvh_waves4 >= 0 ? (uint32_t)c->bvh_waves4 : 1u) : 0u;
    A.xcd_rot = c->xcd_rot;
    A.xcd_skew = c->xcd_skew;
    A.xcd_inter = c->xcd_inter;
    {   // xcd_inter 2: a multiplier near 0.618 of the dealt chunk count, coprime to it (a
        // golden-ratio step spreads each XCD's chunks evenly over the image)
        const uint32_t tyn = (A.rows + 7u) / 8u;
        const uint32_t nfull = ((A.ntx / 2u) * (tyn / 2u) / 8u) * 8u;
        uint32_t m = nfull ? (uint32_t)(0.6180339887 * nfull) | 1u : 1u;
        auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
        while (nfull && gcd(m, nfull) != 1u) m += 2u;
        A.xcd_mult = nfull ? m % nfull : 1u;
        if (A.xcd_mult == 0u || nfull >= 65536u) A.xcd_mult = 1u; // the kernel's k * mult stays in 32 bits
    }
    // Frame groups (trace_kernel): triangle-free frames (C2) 14.8 -> 13.85 us per frame at
    // 20-frame launches with pairs; mesh frames lose (C4 +2.5 %, C3 +10 %: their tiles' costs
    // vary more from frame to frame and a pair doubles the longest wave),
    // profiles/r03_ab_frame_pair.log
    A.frame_group = c->frame_group > 0 ? (uint32_t)c->frame_group : (c->nbatch == 0 ? 2u : 1u);
    // the dealing constants of a single frame; prepare_launch writes those of the launch's frames
    trt::fill_deal(A.deal, A.ntx, A.ntiles, 1u);
}

} // namespace trt

namespace {

// The sky table of a frame's arguments (KArgs::sky), or null when the frame does not use one.
// The table serves triangle-free plain frames at spp 1 that neither replay rays (rays_in) nor
// write rayOut (out32) nor count; A carries all of that (fill_args, then the caller's rays_in /
// out32).  It is rebuilt on `stream` when anything sky_kernel reads has changed: the image
// size, dz, the flags that shape a primary ray or the pack, or the envmap.  Frames of earlier
// calls may still read the old table on other streams (frames in flight, trt_render on
// alternating streams), so a rebuild first drains the device; like ensure_envp it then waits
// for the build, since later frames may run on streams not ordered after `stream`.  Both happen
// once per change, never in a frame loop.  The drain is of the whole device, not only of this
// context's slot streams: trt_render may have been given any stream of the caller's
// (trt_set_stream), which the context does not keep.  A context holds ONE table: a caller that
// alternates two keys on it (two resolutions, sRGB on and off) rebuilds on every switch, a
// drain and one small kernel each time; such a caller uses one context per key or switches the
// table off (TRT_SKY_TABLE=0).  Without device memory for the table the frames run without it.
int attach_sky(trt_ctx* c, KArgs& A, bool count, hipStream_t stream) {
    A.sky = nullptr;
    if (!c->sky_on || c->nbatch != 0 || A.spp > 1 || A.rays_in || A.out32 || count) return TRT_OK;
    // an oriented launch: the table (and the spans, masks and floor class, which all need it)
    // holds the fixed basis's primary misses
    if (A.view_on) return TRT_OK;
    if ((A.flags & TRT_FLAG_ENVMAP) && !c->d_env) return TRT_OK;
    const uint32_t kflags = A.flags & (TRT_FLAG_ROW_QUIRK | TRT_FLAG_SRGB_OUT | TRT_FLAG_ENVMAP);
    const trt_ctx::SkyKey key{A.width, A.height, kflags, A.dz, (A.flags & TRT_FLAG_ENVMAP) ? c->env_gen : 0u};
    const trt_ctx::SkyKey& k = c->sky_key;
    const bool same = c->sky_ok && k.width == key.width && k.height == key.height && k.flags == key.flags &&
                      std::memcmp(&k.dz, &key.dz, sizeof(float)) == 0 && k.env_gen == key.env_gen;
    if (!same) {
        c->sky_ok = false;
        HIP_TRY(c, hipDeviceSynchronize());
        const size_t bytes = (size_t)A.width * A.height * sizeof(uint32_t);
        if (bytes > c->sky_cap || !c->d_sky) {
            (void)hipFree(c->d_sky);
            c->d_sky = nullptr;
            c->sky_cap = 0;
            const hipError_t e = hipMalloc((void**)&c->d_sky, bytes);
            if (e == hipErrorOutOfMemory) {
                (void)hipGetLastError(); // not the next launch's error
                c->d_sky = nullptr;
                c->sky_key = key; // frames of this key run without a table: no retry per call
                c->sky_ok = true;
                return TRT_OK;
            }
            HIP_TRY(c, e);
            c->sky_cap = bytes;
        }
        HIP_TRY(c, trt::launch_sky(A, c->d_sky, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
        c->sky_key = key;
        c->sky_ok = true;
    }
    A.sky = c->d_sky;
    return TRT_OK;
}

// The sky spans of a launch (KArgs::span), from what the launch's arguments already hold: the
// frames' cameras (fill_frame), the UBO's spheres (fill_ubo_args) and the sky table (attach_sky).
// Unset wherever there is no table, and under TRT_SKY_SPANS=0.
void fill_spans(trt_ctx* c, KArgs& A) {
    A.span_tables = 0;
    A.floor_class = 0;
    if (!A.sky || !c->span_on || A.out32 || A.spp > 1) return;
    trt::SpanIn in{};
    in.width = A.width;
    in.height = A.height;
    in.dz = A.dz;
    in.flags = A.flags;
    in.band_rows = A.band_rows;
    in.band_count = A.band_count;
    in.band_index = A.band_index;
    in.rays_in = A.rays_in != nullptr;
    for (int i = 0; i < 4; ++i) {
        for (int a = 0; a < 3; ++a) in.sph[i][a] = A.sph[i].c[a];
        in.sph[i][3] = A.sph[i].r;
    }
    float cams[3 * trt::kMaxLaunchFrames];
    const uint32_t n = std::min(A.nframes, trt::kMaxLaunchFrames);
    for (uint32_t f = 0; f < n; ++f)
        for (int a = 0; a < 3; ++a) cams[3 * f + a] = A.fr[f].cam[a];
    uint32_t ntr = 0, shift = 0;
    const uint32_t T = trt::sky_spans(in, cams, n, c->span_frames, A.span, &ntr, &shift, c->floor_on && A.nframes > 1u ? c->sph_span : nullptr);
    if (T == 0 || A.ntx == 0 || ntr != A.ntiles / A.ntx) return; // the kernel indexes by tile / ntx
    A.span_tables = T;
    A.span_shift = shift;
    A.span_ntr = ntr;
}

// The shadow occluder masks of a launch (KArgs::smask, shadow_mask.h), for every launch that has
// sky spans (the only kernel that reads them is sky_trace_kernel_smask), or null: the launch then
// runs the kernel without masks, which tests every sphere.  The key is the bytes the build
// reads, taken from the launch's own arguments (fill_ubo_args): the spheres' centres and radii,
// the lights and the spheres flag.  A frame loop only compares the key; a change builds the masks
// on the host (tools/shadow_mask_host_cost.cpp), drains the device (frames of earlier calls may
// still read the old table on other streams, as with the sky table), uploads on `stream` and
// waits.  A context holds ONE table.  No masks: TRT_SHADOW_MASK=0, every fallback of the build
// (all ones), a launch with a camera outside the build's error bound (beyond kShadowCamMax, or
// not finite), and no device memory for the table.
int attach_smask(trt_ctx* c, KArgs& A, hipStream_t stream) {
    A.smask = nullptr;
    if (!A.sky || !A.span_tables || !c->smask_on) return TRT_OK;
    trt::ShadowMaskIn key{};
    for (int j = 0; j < 4; ++j) {
        for (int a = 0; a < 3; ++a) key.sph[j][a] = A.sph[j].c[a];
        key.sph[j][3] = A.sph[j].r;
    }
    std::memcpy(key.light, A.light, sizeof(key.light));
    key.flags = A.flags & TRT_FLAG_SPHERES;
    if (!c->smask_ok || std::memcmp(&key, &c->smask_key, sizeof(key)) != 0) {
        c->smask_ok = false;
        trt::ShadowMask m;
        trt::shadow_mask(key, c->smask_cell, true, m);
        constexpr size_t kCells = 200u * 250u; // kShadowCellMin over the 20 x 25 floor
        if (m.cells.size() > kCells) trt::shadow_mask(key, c->smask_cell, false, m); // cannot happen: all ones
        if (!m.fallback) {
            HIP_TRY(c, hipDeviceSynchronize());
            if (!c->d_smask) {
                const hipError_t e = hipMalloc((void**)&c->d_smask, kCells * sizeof(uint16_t));
                if (e == hipErrorOutOfMemory) {
                    (void)hipGetLastError(); // not the next launch's error
                    c->d_smask = nullptr;    // frames of this key run without masks: no retry per call
                } else {
                    HIP_TRY(c, e);
                }
            }
            if (c->d_smask) {
                HIP_TRY(c, hipMemcpyAsync(c->d_smask, m.cells.data(), m.cells.size() * sizeof(uint16_t),
                                          hipMemcpyHostToDevice, stream));
                HIP_TRY(c, hipStreamSynchronize(stream));
            }
        }
        c->smask_nx = m.nx;
        c->smask_nz = m.nz;
        c->smask_inv = m.inv_cell;
        c->smask_rows[0] = m.rows[0] | (m.rows[1] << 16);
        c->smask_rows[1] = m.rows[2] | (m.rows[3] << 16);
        c->smask_fallback = m.fallback;
        c->smask_key = key;
        c->smask_ok = true;
    }
    if (!c->d_smask || c->smask_fallback) return TRT_OK;
    for (uint32_t f = 0; f < A.nframes && f < trt::kMaxLaunchFrames; ++f)
        for (int a = 0; a < 3; ++a)
            if (!(std::fabs(A.fr[f].cam[a]) <= trt::kShadowCamMax)) return TRT_OK; // NaN too
    A.smask = c->d_smask;
    A.smask_nx = c->smask_nx;
    A.smask_nz = c->smask_nz;
    A.smask_inv = c->smask_inv;
    A.smask_rows[0] = c->smask_rows[0];
    A.smask_rows[1] = c->smask_rows[1];
    return TRT_OK;
}

// The floor class of a launch (KArgs::floor_class, sky_trace_kernel_floor): for every launch that
// has spans (fill_spans, which left the rows' sphere intervals in c->sph_span) and masks
// (attach_smask), both scene parts on and tile rows that fit the packed word, A.span is repacked
// with the sphere interval beside the span.  Any other launch, and every launch under
// TRT_FLOOR_CLASS=0, keeps its span words and runs the kernel it ran before.  So does a launch of
// one frame: frames launched one by one were 1.5-2.2 % slower with the class than without
// (profiles/floor_class_ab_summary.txt), so they neither compute the intervals nor change kernel.
void attach_floor_class(const trt_ctx* c, KArgs& A) {
    A.floor_class = 0;
    if (!c->floor_on || A.nframes < 2u || !A.span_tables || !A.smask || A.ntx > trt::kFloorPackMaxNtx) return;
    if (!(A.flags & TRT_FLAG_FLOOR) || !(A.flags & TRT_FLAG_SPHERES)) return;
    const uint32_t words = A.span_tables * A.span_ntr;
    for (uint32_t i = 0; i < words; ++i) A.span[i] = trt::floor_pack(A.span[i], c->sph_span[i]);
    A.floor_class = 1;
    if (c->floor_lit_on && floor_lit(A.flags, A.light)) A.floor_class |= trt::kFloorLit;
}

// The dealing constants of a launch (KArgs::deal, trt_deal.h), once its frames are set: the frames
// or pairs its kernel interleaves.
void attach_deal(KArgs& A) {
    trt::fill_deal(A.deal, A.ntx, A.ntiles, trt::deal_frames(A.nframes, A.xcd_inter, A.frame_group, A.nbatch == 0));
}

// Launch preparation, once the frames, the UBO, A.sky and A.view_on are set.  The order is a
// correctness condition: the floor class needs the masks and repacks A.span in place from
// c->sph_span, which fill_spans left behind; the bases of an oriented launch (views[f], null: the
// identity; views null: fill_args wrote the one basis) share their bytes with the span words, so
// they come last (an oriented launch has no table, hence no span words).
int prepare_launch(trt_ctx* c, KArgs& A, hipStream_t stream, const trt_view* const* views) {
    fill_spans(c, A);
    const int rc = attach_smask(c, A, stream);
    if (rc != TRT_OK) return rc;
    attach_floor_class(c, A);
    attach_deal(A);
    if (A.view_on && views)
        for (uint32_t f = 0; f < A.nframes; ++f) fill_view(A, f, views[f] ? *views[f] : kViewIdentity);
    return TRT_OK;
}

// Does this frame run deferred shadows?  Auto: mesh scenes with max_depth >= 8, whose deep
// refraction trees leave most lanes of a wave idle while a few trace their shadow rays.
// COUNT frames (the reference's counters) and spp > 1 frames run the per-pixel loop.
bool defer_frame(const trt_ctx* c, const trt_params* p, bool ignore_count = false) {
    if (p->spp > 1 || c->deferred_shadows == TRT_DEFER_OFF) return false;
    if ((p->flags & TRT_FLAG_COUNT) && !ignore_count) return false;
    if (c->deferred_shadows == TRT_DEFER_ON) return true;
    return c->nbatch > 0 && p->max_depth >= 8;
}

// The subtree-split window of a frame: 0 = off.  Auto: scenes with meshes (whose deep
// refraction trees make a few tiles run for milliseconds) with max_depth above the window.
uint32_t split_window(const trt_ctx* c, const trt_params* p) {
    const uint32_t D = p->max_depth;
    if ((p->spp > 1) || c->subtree_split == TRT_SPLIT_OFF) return 0;
    if ((size_t)trt_output_rows(p) * p->width >= (1u << (32 - trt::kTaskDepthBits))) return 0;
    uint32_t w;
    // experiment: a deferred frame traced one depth per launch (TRT_DEFER_WAVEFRONT=1)
    if (const char* e = std::getenv("TRT_DEFER_WAVEFRONT"))
        if (std::atoi(e) != 0 && defer_frame(c, p) && D > 1) return 1u;
    if (c->subtree_split == TRT_SPLIT_AUTO) {
        // measured (profiles/r01_split_sweep.log): -10..-16 % on the shipped depth-20 frame with
        // w = 4; +0..+25 % on depth-4 mesh frames (C3/C4) for any window, so only deep trees.
        // Deferred-shadow frames are not split: their trees hold no shadow rays, and a split
        // (exact, through LINK events) measured +11..+29 % on the shipped frame and +38..+69 %
        // on the README scene for windows 2..5 (profiles/r02_ab_defer_split.log).
        if (c->nbatch == 0 || D < 8 || defer_frame(c, p)) return 0;
        w = 4u;
    } else {
        w = (uint32_t)c->subtree_split;
    }
    return w < D ? w : 0u;
}

size_t env_cap(const char* name, size_t v) {
    if (const char* e = std::getenv(name)) return std::min<size_t>(v, (size_t)std::strtoull(e, nullptr, 10));
    return v;
}

// ---- deferred-frame scratch (one set per frames-in-flight slot) ----------------------------

// Deferred-frame sizes: event chunks (per tile:
// ceil((2^D - 1) / kEvRows) at depth <= 4, else 4 on average, at least 128 per stripe) and
// shadow queries (6 per pixel on average), both split into kDeferStripes equal stripes (tile t
// uses stripe hash(t)); ~1.2 KB per pixel at depth >= 5 (16 events of 64 B + 6 queries of 32 B).
// Every lane of a pool wave takes an event slot on every step of the wave's shared segment pool
// (idle lanes too, so the lanes stay on one row of one chunk), so a tile's event count is set by
// the pool's schedule, not bounded by 2^D - 1 per pixel; a tile that runs out re-traces its
// pixels in place (defer_fallback: the image stays exact, only slower).  Slot ids
// (chunk * kEvRows + row) * 64 + lane travel in 30 bits of a query.
constexpr size_t kPoolEvBytes = trt::kEvRows * 4 * 64 * sizeof(float4); // one chunk
size_t pool_chunks(size_t ntiles, uint32_t D) {
    const size_t per_tile = D <= 4 ? ((1u << D) - 1u + trt::kEvRows - 1u) / trt::kEvRows : 4u;
    constexpr size_t S = trt::kDeferStripes;
    const size_t tiles_per_stripe = (ntiles + S - 1) / S;
    return S * std::min<size_t>(std::max<size_t>(tiles_per_stripe * per_tile, D <= 4 ? 16u : 128u),
                                (1u << 30) / (trt::kEvRows * 64u) / S);
}
size_t shadow_qcap(size_t ntiles) {
    constexpr size_t S = trt::kDeferStripes;
    const size_t tiles_per_stripe = (ntiles + S - 1) / S;
    return S * std::min<size_t>(std::max<size_t>(6 * tiles_per_stripe * 64u, 1u << 12), 0xFFFFFFFFu / S);
}
struct DeferSizes {
    size_t chunks = 0, qcap = 0; // event chunks and shadow queries
    size_t bytes = 0;
};
DeferSizes defer_sizes(size_t ntiles, uint32_t D, size_t npx) {
    DeferSizes z;
    z.chunks = pool_chunks(ntiles, D);
    z.qcap = shadow_qcap(ntiles);
    z.bytes = z.chunks * kPoolEvBytes + z.qcap * 2 * sizeof(float4) + npx * (sizeof(uint2) + sizeof(uint32_t)) +
              sizeof(trt::DeferCtr);
    return z;
}

// A slot holds the scratch of `dframes` frames (a deferred launch group), each of the per-frame
// capacities below.
bool defer_bufs_fit(const trt_ctx::SplitBufs& b, const DeferSizes& z, size_t npx, uint32_t frames) {
    return z.chunks <= b.ev_chunks && z.qcap <= b.shq_cap && npx <= b.dnpx && frames <= b.dframes;
}

// Deferred frame loop shape: `group` frames per launch sequence on each of `slots` in-flight
// slots.  Explicit: TRT_DEFER_GROUP, or trt_set_frames_in_flight (then groups of 1, the
// reference's pacing when it is 2).  Auto, with the group's frames dealt block by block
// (defer_inter): with at least 16 hardware queues 8 slots of 3 frames (24 in flight: the shipped
// frame 320 -> 311 us, the README scene 155 -> 149 us against 16 slots of 1, at half the frame
// latency; profiles/r06t_ab_defer_shape_32q.jsonl); with fewer, defer_in_flight (16) frames over
// at most half the queues — a stream per slot, and slots sharing a queue serialise: with HIP's
// default 4 queues 2 slots of 8 frames (the shipped frame through the C++ host 0.82 -> 0.51 ms
// per frame; 2 x 12 and 6 x 4 within 2 %, profiles/r06t_shape_q4.log).  An explicit
// TRT_DEFER_IN_FLIGHT keeps the second rule at every queue count.
void defer_shape(const trt_ctx* c, uint32_t& group, uint32_t& slots) {
    const uint32_t T = std::max(c->defer_in_flight, 1u);
    if (c->frames_in_flight) {
        slots = c->frames_in_flight;
        group = c->defer_group ? c->defer_group : 1u;
        return;
    }
    if (c->defer_group) {
        group = c->defer_group;
        slots = std::max(1u, (T + group - 1) / group);
        return;
    }
    if (c->hw_queues >= 16u && !c->defer_in_flight_set) {
        slots = 8u;
        group = 3u;
        return;
    }
    slots = std::min(T, std::max(2u, c->hw_queues / 2u));
    group = (T + slots - 1) / slots;
}

// Device bytes one frames-in-flight slot needs for a group of `frames` deferred frames of these
// params (0 when the slot already holds enough).
size_t defer_slot_bytes(const trt_ctx* c, const trt_params* p, uint32_t slot, uint32_t frames) {
    const size_t npx = (size_t)trt_output_rows(p) * p->width;
    const size_t ntiles = ((p->width + 7u) / 8u) * ((trt_output_rows(p) + 7u) / 8u);
    const DeferSizes z = defer_sizes(ntiles * std::max(1u, c->defer_sub / 2u), p->max_depth, npx); // as prepare_defer
    return defer_bufs_fit(c->split[slot], z, npx, frames) ? 0 : z.bytes * frames;
}

// The automatic frames-in-flight count of a deferred loop, bounded by device memory: each slot
// holds its own scratch (defer_sizes: the shipped 1024x768 frame ~1 GB per slot), and the slots that would still need allocating may take
// at most half of the free device memory.
uint32_t fit_defer_slots(const trt_ctx* c, const trt_params* p, uint32_t want, uint32_t frames) {
    size_t freeb = 0, total = 0;
    if (hipMemGetInfo(&freeb, &total) != hipSuccess) return want;
    size_t need = 0;
    uint32_t n = 0;
    for (; n < want && n < TRT_BUILD_MAX_IN_FLIGHT; ++n) {
        need += defer_slot_bytes(c, p, n, frames);
        if (n > 0 && need > freeb / 2) break;
    }
    return std::max(1u, n);
}

void free_defer_bufs(trt_ctx::SplitBufs& b) {
    for (void** q : {(void**)&b.ev, (void**)&b.shq, (void**)&b.px_ev, (void**)&b.fb, (void**)&b.dctr})
        (void)hipFree(*q), *q = nullptr;
    b.ev_chunks = b.shq_cap = b.dnpx = 0;
    b.dframes = 0;
}

// Allocates slot `slot`'s deferred-frame scratch for this frame and fills
// A's defer fields.
int prepare_defer(trt_ctx* c, const trt_params* p, KArgs& A, uint32_t slot) {
    auto& b = c->split[slot];
    const size_t npx = (size_t)trt_output_rows(p) * p->width;
    const uint32_t G = std::max(A.nframes, 1u); // frames of this launch, each with its own scratch
    // pass-A waves per tile (pool design): explicit (TRT_DEFER_PPW), else by the frames that
    // overlap: with few frames in flight a frame's latency — its deepest tiles' chains of walks —
    // sets the rate, and more waves per tile spread a deep tile's pixels (the shipped frame at 2
    // in flight: 1 wave 1.09, 2 waves 0.82 ms, profiles/r05j_ab_defer_ppw.jsonl; 4 waves a
    // further -2 % on both deep scenes at 2 in flight, 8 waves +12 % / -10 %, and at 4 in flight
    // 2 waves stay best, profiles/r06zb_ab_pass_a_waves_per_tile.jsonl); with many, the idle
    // lanes of the cheap tiles cost more than the overlap hides (at 16 in flight 0.32 -> 0.40 ms)
    const uint32_t ov = c->cur_in_flight * G;
    const uint32_t Sd = c->defer_sub ? c->defer_sub : ov <= 2u ? 4u : ov <= 4u ? 2u : 1u;
    // every pass-A wave takes its own event chunks (a row of 64 lanes per step, idle lanes'
    // slots unused): four waves per tile need twice the chunks of two (the shipped frame at two
    // waves peaks at 60 % of the capacity, profiles/r06z_defer_probe.jsonl)
    const DeferSizes z = defer_sizes(A.ntiles * std::max(1u, Sd / 2u), p->max_depth, npx);
    if (!defer_bufs_fit(b, z, npx, G)) {
        free_defer_bufs(b);
        hipError_t e = hipSuccess;
        auto alloc = [&](void** q, size_t bytes) {
            if (e == hipSuccess && bytes) e = hipMalloc(q, bytes);
        };
        if ((int)slot == test_fail_defer_slot()) e = hipErrorOutOfMemory;
        alloc((void**)&b.ev, G * z.chunks * kPoolEvBytes);
        alloc((void**)&b.shq, G * z.qcap * 2 * sizeof(float4));
        alloc((void**)&b.px_ev, G * npx * sizeof(uint2));
        alloc((void**)&b.fb, G * npx * sizeof(uint32_t));
        alloc((void**)&b.dctr, G * sizeof(trt::DeferCtr));
        if (e != hipSuccess) {
            free_defer_bufs(b);
            return hip_fail(c, e, "alloc deferred-frame buffers");
        }
        b.ev_chunks = z.chunks;
        b.shq_cap = z.qcap;
        b.dnpx = npx;
        b.dframes = G;
    }
    A.defer = 1;
    A.defer_sub = Sd;
    A.defer_inter = c->defer_inter;
    // test hooks: tiny capacities exercise the in-place fallback (tests/test_gpu_defer.py)
    A.ev_cap = (uint32_t)env_cap("TRT_DEFER_EVCAP", z.chunks / trt::kDeferStripes);
    A.shq_cap = (uint32_t)env_cap("TRT_DEFER_QCAP", z.qcap / trt::kDeferStripes);
    A.ev = b.ev;
    A.shq = b.shq;
    A.px_ev = b.px_ev;
    A.fb = b.fb;
    A.dctr = b.dctr;
    A.dframes = G;
    A.ev_fstride = b.ev_chunks * (kPoolEvBytes / sizeof(float4));
    A.shq_fstride = b.shq_cap * 2;
    A.px_fstride = (uint32_t)b.dnpx;
    b.used_ev_cap = A.ev_cap;
    b.used_shq_cap = A.shq_cap;
    return TRT_OK;
}

// Allocates slot `slot`'s split (or deferred-shadow) scratch for this frame size and fills A's
// split / defer fields; a frame on `stream` waits for the slot's previous frame when that ran
// on another stream.
int prepare_split(trt_ctx* c, const trt_params* p, KArgs& A, uint32_t slot, hipStream_t stream) {
    A.split_w = 0;
    A.split_d1 = A.max_depth;
    A.num_cus = c->num_cus;
    A.defer = 0;
    const bool defer = defer_frame(c, p);
    // A COUNT frame of a scene whose frames run deferred is traced unsplit, so its image is the
    // deferred frame's bit for bit (both are the reference's single running sum; a deferred
    // frame's subtree split keeps that order through LINK events).
    if (defer || !defer_frame(c, p, true)) A.split_w = split_window(c, p);
    if (!A.split_w && !defer) return TRT_OK;
    auto& b = c->split[slot];
    if (b.last && b.last != stream) HIP_TRY(c, hipStreamWaitEvent(stream, b.done, 0));
    if (defer) {
        const int rc = prepare_defer(c, p, A, slot);
        if (rc != TRT_OK) return rc;
    }
    if (!A.split_w) return TRT_OK;
    const size_t npx = (size_t)trt_output_rows(p) * p->width;
    if (npx > b.npx) {
        // queue capacity: 4 tasks per pixel per window edge (a full queue is not an error: the
        // child is traced in place, SplitCtr::overflow counts it; a deferred frame re-traces
        // the pixel in place)
        const size_t cap = std::min<size_t>(std::max<size_t>(4 * npx, 1u << 16), 1u << 28);
        auto drop = [&] {
            for (void** q : {(void**)&b.q[0], (void**)&b.q[1], (void**)&b.qlink[0], (void**)&b.qlink[1], (void**)&b.acc,
                             (void**)&b.spilled})
                (void)hipFree(*q), *q = nullptr;
            b.npx = 0;
            b.cap = 0;
        };
        drop();
        hipError_t e = hipMalloc((void**)&b.q[0], cap * sizeof(trt::Task));
        if (e == hipSuccess) e = hipMalloc((void**)&b.q[1], cap * sizeof(trt::Task));
        if (e == hipSuccess) e = hipMalloc((void**)&b.qlink[0], cap * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&b.qlink[1], cap * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&b.acc, npx * 4 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc((void**)&b.spilled, npx * sizeof(uint32_t));
        if (e == hipSuccess && !b.ctr) e = hipMalloc((void**)&b.ctr, sizeof(trt::SplitCtr));
        if (e != hipSuccess) {
            drop();
            return hip_fail(c, e, "alloc subtree-split buffers");
        }
        b.npx = npx;
        b.cap = (uint32_t)cap;
    }
    A.q_link_buf[0] = b.qlink[0];
    A.q_link_buf[1] = b.qlink[1];
    A.q_buf[0] = b.q[0];
    A.q_buf[1] = b.q[1];
    A.q_cap = b.cap;
    // test hook: a tiny queue exercises the in-place fallback (tests/test_gpu_split.py)
    if (const char* e = std::getenv("TRT_SPLIT_QCAP")) A.q_cap = std::min<uint32_t>(A.q_cap, (uint32_t)std::strtoul(e, nullptr, 10));
    A.acc = b.acc;
    A.spilled = b.spilled;
    A.ctr = b.ctr;
    return TRT_OK;
}

// After a split frame's launches on `stream`: the slot's fence.
int fence_split(trt_ctx* c, const KArgs& A, uint32_t slot, hipStream_t stream) {
    if (!A.split_w && !A.defer) return TRT_OK;
    auto& b = c->split[slot];
    if (!b.done) HIP_TRY(c, hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(b.done, stream));
    b.last = stream;
    return TRT_OK;
}

// trt_stats from the device counters, in KArgs::counters order (kernel_ms is the caller's).
void stats_from_counters(trt_stats* st, const unsigned long long* cnt) {
    static uint64_t trt_stats::*const field[20] = {
        &trt_stats::primary_rays, &trt_stats::secondary_rays, &trt_stats::shadow_rays, &trt_stats::misses,
        &trt_stats::tri_nearest, &trt_stats::sphere_tests, &trt_stats::batch_tests, &trt_stats::batch_hits,
        &trt_stats::tri_tests, &trt_stats::node_tests, &trt_stats::tri_past_a, &trt_stats::tri_past_u,
        &trt_stats::tri_past_v, &trt_stats::shadow_skipped, &trt_stats::skipped_sphere_tests,
        &trt_stats::skipped_box_tests, &trt_stats::skipped_tri_tests, &trt_stats::skipped_tri_past_a,
        &trt_stats::skipped_tri_past_u, &trt_stats::skipped_tri_past_v};
    for (int i = 0; i < 20; ++i) st->*field[i] = cnt[i];
}

// trt_render's split slot: one per distinct stream among the last TRT_BUILD_MAX_IN_FLIGHT
// (so renders alternating between streams overlap), reused least recently first.
uint32_t render_slot(trt_ctx* c, hipStream_t s) {
    for (uint32_t k = 0; k < TRT_BUILD_MAX_IN_FLIGHT; ++k)
        if (c->render_slot_stream[k] == s) return k;
    const uint32_t k = c->render_slot_next;
    c->render_slot_next = (k + 1) % TRT_BUILD_MAX_IN_FLIGHT;
    c->render_slot_stream[k] = s;
    return k;
}

// Before the launch of trt_render, trt_trace_rays and trt_occluded; finish_call after it.
int begin_call(trt_ctx* c, bool count, bool timing) {
    if (count) HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, 32 * sizeof(unsigned long long), c->stream));
    if (timing) HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    return TRT_OK;
}

// A host array staged through a grow-only buffer of the context: `in`, when given, is copied to
// it; *dev is the array's device twin (finish_call copies outputs back).
template <class T>
int stage(trt_ctx* c, void** buf, size_t* cap, size_t bytes, const char* what, const void* in, T** dev) {
    const int rc = ensure(c, buf, cap, bytes, what);
    if (rc != TRT_OK) return rc;
    if (in) HIP_TRY(c, hipMemcpyAsync(*buf, in, bytes, hipMemcpyHostToDevice, c->stream));
    *dev = static_cast<T*>(*buf);
    return TRT_OK;
}
struct StagedOut { void* host; const void* dev; size_t bytes; }; // host null: not asked for
// The stream is synchronised when the caller reads anything on return.
int finish_call(trt_ctx* c, bool dev, bool count, bool timing, trt_stats* st, std::initializer_list<StagedOut> outs) {
    if (timing) HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (!dev)
        for (const StagedOut& o : outs)
            if (o.host) HIP_TRY(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
    unsigned long long cnt[32] = {0};
    if (count) HIP_TRY(c, hipMemcpyAsync(cnt, c->d_counters, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    if (!dev || count || timing) HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st) {
        stats_from_counters(st, cnt);
        st->kernel_ms = 0.0;
        if (timing) {
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
            st->kernel_ms = ms;
        }
    }
    return TRT_OK;
}

// What a query reads of p, as frame params for fill_args: 64 x 1 pixels that reach no kernel.
trt_params query_params(const trt_params* p, uint32_t max_depth, uint32_t flag_mask) {
    trt_params q;
    trt_params_default(&q);
    q.width = 64;
    q.height = 1;
    q.max_depth = max_depth;
    q.flags = p->flags & flag_mask;
    return q;
}

// The shape of a frame loop: `want` in-flight slots and `per_launch` frames per launch.
// Plain frames (no subtree split, no deferred shadows: the same decision prepare_split
// makes) go out several per launch; the others one per launch (per-slot scratch).
// Frames in flight (main.cpp:45, MAX_FRAMES_IN_FLIGHT): launch j runs on slot j % n.  Slot 0
// is the context's stream, slots 1..n-1 are context-owned streams forked from it and joined
// back into it, so to the caller all frames complete on its stream.  A
// plain loop needs no second slot: one multi-frame launch keeps the GPU full from its first frame
// to its last, so a 20-frame loop is one launch and drains once (C2 at 20 frames: 20.5 us per
// frame against 25.0 with one launch per frame on 4 slots; at 1000 frames 15.6 vs 15.9,
// profiles/r03_ab_frame_batch.log); with n slots set explicitly the frames are spread over
// n launches.  Per-frame launch sequences (split / deferred-shadow frames) keep the slots
// busy instead: auto 4, or defer_in_flight (16) for deferred-shadow frames (8 vs 16 in round
// 4: the shipped frame 0.42 -> 0.35 ms, the README scene 0.24 -> 0.17 ms,
// profiles/r04z_ab_deferred_in_flight.jsonl; round 2: the shipped frame 1.45 -> 0.56 ms at
// 8, profiles/r02_ab_queues_deep.log).
uint32_t loop_shape(const trt_ctx* c, const trt_params* p, uint32_t nframes, uint32_t& want) {
    const bool defer = defer_frame(c, p);
    const bool split = (defer || !defer_frame(c, p, true)) && split_window(c, p) != 0;
    const bool plain = !defer && !split;
    want = c->frames_in_flight ? c->frames_in_flight : plain ? 1u : defer ? c->defer_in_flight : 4u;
    // auto: no more deferred slots than device memory holds (each slot owns its scratch)
    // deferred frames (not split) go out in groups of frames per launch sequence (defer_shape)
    uint32_t group = 1;
    if (defer && !split) {
        uint32_t slots = want;
        defer_shape(c, group, slots);
        group = std::min(group, trt::kMaxLaunchFrames);
        want = slots;
    }
    if (!c->frames_in_flight && defer) want = fit_defer_slots(c, p, want, group);
    const uint32_t cap = plain ? (c->frame_batch ? c->frame_batch : trt::kMaxLaunchFrames) : group;
    return std::max(1u, std::min(cap, (nframes + want - 1) / want));
}

// launches: runs of consecutive frames sharing every UBO field but camPos; run j is frames
// [first[j], first[j + 1]).  Views do not split launches; a launch with an oriented frame holds
// at most kMaxViewFrames frames (one basis each in KArgs::view), so a run breaks where it would
// outgrow that
template <class ViewOf, class UboOf>
std::vector<uint32_t> launch_runs(ViewOf view_of, UboOf ubo_of, uint32_t nframes, uint32_t per_launch) {
    std::vector<uint32_t> first{0};
    bool run_oriented = view_of(0) != nullptr;
    for (uint32_t i = 1; i < nframes; ++i) {
        const bool o = view_of(i) != nullptr;
        const uint32_t len = i - first.back();
        const bool cut = len >= per_launch || !same_but_camera(ubo_of(i), ubo_of(first.back())) ||
                         ((run_oriented || o) && len >= trt::kMaxViewFrames);
        if (cut) first.push_back(i);
        run_oriented = o || (run_oriented && !cut);
    }
    first.push_back(nframes);
    return first;
}

// The streams of slots 0..nfl-1 into sv, slots 1.. forked from the context's stream.
int fork_slots(trt_ctx* c, uint32_t want, uint32_t nfl, std::vector<hipStream_t>& sv) {
    sv.assign(1, c->stream);
    // every slot's stream is made on first use of the in-flight count, not only the ones this
    // call needs: creating a stream takes milliseconds and must not land in a later, longer
    // call (a timed loop after a short warmup)
    while (c->aux.size() + 1 < want) {
        hipStream_t s;
        HIP_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_TRY(c, trt::touch_stream(s, c->d_counters)); // its hardware queue exists from now on
        c->aux.push_back(s);
        hipEvent_t e;
        HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->aux_ev.push_back(e);
    }
    if (nfl > 1) {
        if (!c->fork_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->fork_ev, c->stream));
        for (uint32_t k = 0; k + 1 < nfl; ++k) {
            HIP_TRY(c, hipStreamWaitEvent(c->aux[k], c->fork_ev, 0));
            sv.push_back(c->aux[k]);
        }
    }
    return TRT_OK;
}

int join_slots(trt_ctx* c, uint32_t nfl) {
    for (uint32_t k = 0; k + 1 < nfl; ++k) {
        HIP_TRY(c, hipEventRecord(c->aux_ev[k], c->aux[k]));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->aux_ev[k], 0));
    }
    return TRT_OK;
}

} // namespace

namespace trt {

int render_frame_list(trt_ctx* c, const trt_params* p, const FrameOut* frames, uint32_t nframes,
                      uint32_t time_every) {
    if (!c) return TRT_ERR_INVALID;
    int rc = check_params(c, p);
    if (rc != TRT_OK) return rc;
    if (!(p->flags & TRT_FLAG_DEVICE_PTRS))
        return fail(c, TRT_ERR_INVALID, "trt_render_frames: needs TRT_FLAG_DEVICE_PTRS");
    if (p->flags & TRT_FLAG_COUNT)
        return fail(c, TRT_ERR_INVALID, "trt_render_frames: COUNT is a per-frame trt_render flag");
    if (nframes && !frames) return fail(c, TRT_ERR_INVALID, "trt_render_frames: null frame list");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool timing = time_every > 0;
    const uint32_t every = timing ? time_every : 1u;
    c->fev_frames = 0;
    c->fev_nframes.clear();
    if ((rc = ensure_envp(c, p, c->stream)) != TRT_OK) return rc;
    KArgs A;
    fill_args(c, p, A);
    A.rays_in = reinterpret_cast<const float*>(p->rays_in);
    // a frame's view: its own, else the context's; null for the reference camera's bytes and
    // under replayed rays (such a frame is not oriented)
    auto view_of = [&](uint32_t i) -> const trt_view* {
        if (p->rays_in) return nullptr;
        const trt_view* v = frames[i].view ? frames[i].view : (c->view_on ? &c->view : nullptr);
        return (v && !view_is_identity(*v)) ? v : nullptr;
    };
    auto ubo_of = [&](uint32_t i) -> const trt_ubo& { return frames[i].ubo ? *frames[i].ubo : c->ubo; };
    bool any_plain_view = false;
    for (uint32_t i = 0; i < nframes; ++i) {
        if (frames[i].view && !view_is_finite(*frames[i].view))
            return fail(c, TRT_ERR_INVALID, "trt_render_frames_view: a view is not finite");
        if (!view_of(i)) any_plain_view = true;
    }
    // the sky table serves the launches without an oriented frame (set per launch below)
    A.view_on = any_plain_view ? 0u : 1u;
    if (A.rows != 0 && nframes != 0 && (rc = attach_sky(c, A, false, c->stream)) != TRT_OK) return rc;
    const uint32_t* const sky = A.sky;
    if (A.rows == 0 || nframes == 0) {
        if (nframes) c->ubo = ubo_of(nframes - 1);
        return TRT_OK;
    }
    uint32_t want;
    const uint32_t per_launch = loop_shape(c, p, nframes, want);
    const std::vector<uint32_t> first = launch_runs(view_of, ubo_of, nframes, per_launch);
    const uint32_t nl = (uint32_t)first.size() - 1;
    if (timing) {
        const uint32_t ntimed = (nl + every - 1) / every; // launches 0, every, 2*every, ...
        while (c->fev.size() < 2 * (size_t)ntimed) {
            hipEvent_t e;
            HIP_TRY(c, hipEventCreate(&e));
            c->fev.push_back(e);
        }
    }
    uint32_t nfl = std::min(want, nl);
    c->cur_in_flight = nfl;
    std::vector<hipStream_t> sv;
    if ((rc = fork_slots(c, want, nfl, sv)) != TRT_OK) return rc;
    for (uint32_t j = 0; j < nl; ++j) {
        const uint32_t i0 = first[j], n = first[j + 1] - i0;
        c->ubo = ubo_of(i0);
        fill_ubo_args(A, c->ubo);
        A.nframes = n;
        for (uint32_t k = 0; k < n; ++k) fill_frame(A.fr[k], ubo_of(i0 + k), frames[i0 + k].out8, frames[i0 + k].in_place);
        // an oriented launch: no sky table (so no spans, masks or floor class), and every
        // frame's basis, the identity for its frames of the reference camera
        const trt_view* views[trt::kMaxLaunchFrames];
        A.view_on = 0;
        for (uint32_t k = 0; k < n; ++k)
            if ((views[k] = view_of(i0 + k))) A.view_on = 1;
        A.sky = A.view_on ? nullptr : sky;
        if (A.view_on && n > trt::kMaxViewFrames) return fail(c, TRT_ERR_INVALID, "trt_render_frames: oriented launch too long");
        if ((rc = prepare_launch(c, A, c->stream, views)) != TRT_OK) return rc;
        uint32_t slot = j % nfl;
        if ((rc = prepare_split(c, p, A, slot, sv[slot])) != TRT_OK) {
            // auto count: a slot whose scratch does not fit in device memory is dropped, with the
            // slots after it, and the launch goes to a slot that has its scratch; any other
            // failure is the caller's
            if (c->frames_in_flight || slot == 0 || rc != TRT_ERR_OOM) return rc;
            (void)hipGetLastError(); // the failed hipMalloc's sticky error: not the next launch's
            c->err.clear();
            nfl = slot;
            c->cur_in_flight = nfl;
            slot = j % nfl;
            if ((rc = prepare_split(c, p, A, slot, sv[slot])) != TRT_OK) return rc;
        }
        hipStream_t st = sv[slot];
        const bool timed = timing && j % every == 0;
        const size_t k = 2 * (size_t)(j / every);
        if (timed) HIP_TRY(c, hipEventRecord(c->fev[k], st));
        HIP_TRY(c, trt::launch_trace(A, st, false));
        if ((rc = fence_split(c, A, slot, st)) != TRT_OK) return rc;
        if (timed) {
            HIP_TRY(c, hipEventRecord(c->fev[k + 1], st));
            c->fev_nframes.push_back(n);
            c->fev_frames = j / every + 1;
        }
    }
    c->ubo = ubo_of(nframes - 1);
    return join_slots(c, nfl);
}

} // namespace trt

extern "C" int trt_render_frames_view(trt_ctx* c, const trt_params* p, const trt_ubo* ubos, const trt_view* views,
                                      uint32_t nframes, uint8_t* out8, size_t frame_stride, uint32_t time_every) {
    if (!c) return TRT_ERR_INVALID;
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_render_frames: null params");
    std::vector<trt::FrameOut> fl(nframes);
    const bool in_place = (p->flags & TRT_FLAG_BAND_IN_PLACE) != 0;
    for (uint32_t i = 0; i < nframes; ++i)
        fl[i] = trt::FrameOut{ubos ? &ubos[i] : nullptr, out8 ? out8 + (size_t)i * frame_stride : nullptr, in_place,
                              views ? &views[i] : nullptr};
    // TRT_FLAG_TIMING: events around every time_every-th launch (0 or 1: every launch)
    return trt::render_frame_list(c, p, fl.data(), nframes, (p->flags & TRT_FLAG_TIMING) ? std::max(time_every, 1u) : 0u);
}

extern "C" int trt_render_frames(trt_ctx* c, const trt_params* p, const trt_ubo* ubos, uint32_t nframes,
                                 uint8_t* out8, size_t frame_stride, uint32_t time_every) {
    return trt_render_frames_view(c, p, ubos, nullptr, nframes, out8, frame_stride, time_every);
}

extern "C" int trt_set_frame_batch(trt_ctx* c, uint32_t n) {
    if (!c) return TRT_ERR_INVALID;
    if (n > TRT_MAX_FRAME_BATCH)
        return fail(c, TRT_ERR_INVALID, "trt_set_frame_batch: n must be 0 (auto) or in [1, TRT_MAX_FRAME_BATCH]");
    c->frame_batch = n;
    return TRT_OK;
}

extern "C" int trt_frame_times(trt_ctx* c, float* ms, uint32_t n) {
    if (!c || (!ms && n)) return TRT_ERR_INVALID;
    if (n > c->fev_frames) return fail(c, TRT_ERR_INVALID, "trt_frame_times: more launches than were timed");
    HIP_TRY(c, hipSetDevice(c->device));
    for (uint32_t i = 0; i < n; ++i) {
        HIP_TRY(c, hipEventSynchronize(c->fev[2 * i + 1]));
        HIP_TRY(c, hipEventElapsedTime(&ms[i], c->fev[2 * i], c->fev[2 * i + 1]));
        ms[i] /= (float)std::max(c->fev_nframes[i], 1u);
    }
    return TRT_OK;
}

extern "C" uint32_t trt_timed_launches(trt_ctx* c, uint32_t* frames_out, uint32_t cap) {
    if (!c) return 0;
    for (uint32_t i = 0; frames_out && i < cap && i < c->fev_frames; ++i) frames_out[i] = c->fev_nframes[i];
    return c->fev_frames;
}

extern "C" {

int trt_render(trt_ctx* c, const trt_params* p, uint8_t* out8, float* out32, trt_stats* st) {
    if (!c) return TRT_ERR_INVALID;
    int rc = check_params(c, p);
    if (rc != TRT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));

    const bool dev = (p->flags & TRT_FLAG_DEVICE_PTRS) != 0;
    const bool count = (p->flags & TRT_FLAG_COUNT) != 0 && st;
    const bool timing = (p->flags & TRT_FLAG_TIMING) != 0 && st;
    const uint32_t rows = trt_output_rows(p);
    const size_t npx = (size_t)rows * p->width;

    if ((rc = ensure_envp(c, p, c->stream)) != TRT_OK) return rc;
    KArgs A;
    fill_args(c, p, A);

    const float* d_rays = reinterpret_cast<const float*>(p->rays_in);
    uint32_t* d8 = reinterpret_cast<uint32_t*>(out8);
    float* d32 = out32;
    if (!dev) {
        if (p->rays_in && (rc = stage(c, &c->d_rays, &c->caprays, sizeof(trt_ray) * (size_t)p->width * p->height,
                                      "alloc rays", p->rays_in, &d_rays)) != TRT_OK)
            return rc;
        if (out8 && (rc = stage(c, &c->d_out8, &c->cap8, npx * 4, "alloc rgba8", nullptr, &d8)) != TRT_OK) return rc;
        if (out32 && (rc = stage(c, &c->d_out32, &c->cap32, npx * 16, "alloc rgba32f", nullptr, &d32)) != TRT_OK) return rc;
    }
    A.rays_in = d_rays;
    A.fr[0].out8 = d8;
    A.out32 = d32;
    if (npx > 0 && (rc = attach_sky(c, A, count, c->stream)) != TRT_OK) return rc;
    if ((rc = prepare_launch(c, A, c->stream, nullptr)) != TRT_OK) return rc;
    const uint32_t slot = render_slot(c, c->stream);
    c->cur_in_flight = 1u; // one frame: its latency is the rate
    if ((rc = prepare_split(c, p, A, slot, c->stream)) != TRT_OK) return rc;
    if ((rc = begin_call(c, count, timing)) != TRT_OK) return rc;
    if (npx > 0) HIP_TRY(c, trt::launch_trace(A, c->stream, count));
    if ((rc = fence_split(c, A, slot, c->stream)) != TRT_OK) return rc;
    return finish_call(c, dev, count, timing, st, {{out8, d8, npx * 4}, {out32, d32, npx * 16}});
}

// Ray queries (abi.h): the caller's rays through ray_query_kernel.  Nothing of the context that a
// frame depends on is written: the launch reads the scene bindings and the UBO's spheres and
// lights through fill_args and takes no sky table, spans, masks, view or frame slot.
int trt_trace_rays(trt_ctx* c, const trt_params* p, const trt_qray* rays, uint32_t nrays, uint8_t* out8, float* out32,
                   trt_qhit* hits, trt_stats* st) {
    if (!c) return TRT_ERR_INVALID;
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_trace_rays: null params");
    if (!c->have_scene) return fail(c, TRT_ERR_NOSCENE, "trt_trace_rays: no scene uploaded");
    if (p->max_depth < 1 || p->max_depth > TRT_MAX_DEPTH_LIMIT)
        return fail(c, TRT_ERR_INVALID, "trt_trace_rays: max_depth must be 1..20");
    if (!out8 && !out32 && !hits) return fail(c, TRT_ERR_INVALID, "trt_trace_rays: no output requested");
    const bool shade = out8 || out32;
    if ((p->flags & TRT_FLAG_COUNT) && !shade)
        return fail(c, TRT_ERR_INVALID, "trt_trace_rays: TRT_FLAG_COUNT needs a colour output");
    if ((p->flags & TRT_FLAG_ENVMAP) && !c->d_env)
        return fail(c, TRT_ERR_INVALID, "trt_trace_rays: TRT_FLAG_ENVMAP without an uploaded envmap");
    if (nrays > TRT_QRAY_MAX_RAYS) return fail(c, TRT_ERR_INVALID, "trt_trace_rays: more than 2^28 rays");
    if (nrays && !rays) return fail(c, TRT_ERR_INVALID, "trt_trace_rays: null rays");
    const bool dev = (p->flags & TRT_FLAG_DEVICE_PTRS) != 0;
    // the kernel moves a ray, a hit and a rayOut entry as 16-byte vectors, straight from and to the
    // caller's device arrays (host arrays are staged)
    if (dev && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(hits) |
                 reinterpret_cast<uintptr_t>(out32)) & 15u))
        return fail(c, TRT_ERR_INVALID, "trt_trace_rays: device rays, hits and out_rgba32f must be 16-byte aligned");
    if (dev && (reinterpret_cast<uintptr_t>(out8) & 3u))
        return fail(c, TRT_ERR_INVALID, "trt_trace_rays: device out_rgba8 must be 4-byte aligned");
    const bool count = (p->flags & TRT_FLAG_COUNT) != 0 && st;
    const bool timing = (p->flags & TRT_FLAG_TIMING) != 0 && st;
    if (st) std::memset(st, 0, sizeof(*st));
    if (nrays == 0) return TRT_OK;
    if (!dev) { // a device array cannot be read here: the kernel applies the same predicate
        uint32_t bad = 0;
        if (trt_check_rays(rays, nrays, &bad) != TRT_OK)
            return fail(c, TRT_ERR_INVALID, "trt_trace_rays: ray " + std::to_string(bad) +
                                                " is not valid (non-finite, or direction length out of range)");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    const trt_params q = query_params(p, p->max_depth,
                                      TRT_FLAG_SPHERES | TRT_FLAG_FLOOR | TRT_FLAG_CHECKER | TRT_FLAG_ENVMAP | TRT_FLAG_BATCH_WALK |
                                          TRT_FLAG_SRGB_OUT | TRT_FLAG_DEVICE_PTRS | TRT_FLAG_COUNT | TRT_FLAG_TIMING);
    int rc;
    if ((rc = ensure_envp(c, &q, c->stream)) != TRT_OK) return rc;
    KArgs A;
    fill_args(c, &q, A);
    A.view_on = 0; // the rays are the caller's

    const float4* d_rays = reinterpret_cast<const float4*>(rays);
    uint32_t* d8 = reinterpret_cast<uint32_t*>(out8);
    float4* d32 = reinterpret_cast<float4*>(out32);
    uint4* dh = reinterpret_cast<uint4*>(hits);
    const size_t n = nrays;
    if (!dev) {
        if ((rc = stage(c, &c->d_qrays, &c->capqrays, n * sizeof(trt_qray), "alloc query rays", rays, &d_rays)) != TRT_OK) return rc;
        if (out8 && (rc = stage(c, &c->d_out8, &c->cap8, n * 4, "alloc rgba8", nullptr, &d8)) != TRT_OK) return rc;
        if (out32 && (rc = stage(c, &c->d_out32, &c->cap32, n * 16, "alloc rgba32f", nullptr, &d32)) != TRT_OK) return rc;
        if (hits && (rc = stage(c, &c->d_qhits, &c->capqhits, n * sizeof(trt_qhit), "alloc query hits", nullptr, &dh)) != TRT_OK) return rc;
    }
    if ((rc = begin_call(c, count, timing)) != TRT_OK) return rc;
    HIP_TRY(c, trt::launch_ray_query(A, d_rays, nrays, d8, d32, dh, count, c->stream));
    return finish_call(c, dev, count, timing, st, {{out8, d8, n * 4}, {out32, d32, n * 16}, {hits, dh, n * sizeof(trt_qhit)}});
}

// Occlusion queries (abi.h): the caller's segments through occlusion_query_kernel, one byte each.
// Like trt_trace_rays it writes nothing of the context that a frame or a ray query depends on; host
// arrays stage through the ray-query record buffer and the RGBA8 buffer (both only grow).
int trt_occluded(trt_ctx* c, const trt_params* p, const trt_qseg* segs, uint32_t nsegs, uint8_t* out, trt_stats* st) {
    if (!c) return TRT_ERR_INVALID;
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_occluded: null params");
    if (!c->have_scene) return fail(c, TRT_ERR_NOSCENE, "trt_occluded: no scene uploaded");
    if (p->flags & TRT_FLAG_COUNT)
        return fail(c, TRT_ERR_INVALID, "trt_occluded: TRT_FLAG_COUNT is not offered (any-hit counters depend on the walk order)");
    if ((p->flags & TRT_FLAG_TIMING) && !st) return fail(c, TRT_ERR_INVALID, "trt_occluded: TRT_FLAG_TIMING needs stats");
    if (nsegs > TRT_QRAY_MAX_RAYS) return fail(c, TRT_ERR_INVALID, "trt_occluded: more than 2^28 segments");
    if (nsegs && !segs) return fail(c, TRT_ERR_INVALID, "trt_occluded: null segs");
    if (nsegs && !out) return fail(c, TRT_ERR_INVALID, "trt_occluded: null out");
    const bool dev = (p->flags & TRT_FLAG_DEVICE_PTRS) != 0;
    // the kernel reads a segment as two 16-byte vectors straight from the caller's device array
    // and stores single bytes (host arrays are staged)
    if (dev && (reinterpret_cast<uintptr_t>(segs) & 15u))
        return fail(c, TRT_ERR_INVALID, "trt_occluded: device segs must be 16-byte aligned");
    const bool timing = (p->flags & TRT_FLAG_TIMING) != 0;
    if (st) std::memset(st, 0, sizeof(*st));
    if (nsegs == 0) return TRT_OK;
    if (!dev) { // a device array cannot be read here: the kernel applies the same predicate
        uint32_t bad = 0;
        if (trt_check_segs(segs, nsegs, &bad) != TRT_OK)
            return fail(c, TRT_ERR_INVALID, "trt_occluded: segment " + std::to_string(bad) +
                                                " is not valid (non-finite, direction length or tmax out of range)");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    const trt_params q = query_params(p, 1, TRT_FLAG_SPHERES | TRT_FLAG_FLOOR | TRT_FLAG_BATCH_WALK | TRT_FLAG_DEVICE_PTRS | TRT_FLAG_TIMING);
    int rc;
    KArgs A;
    fill_args(c, &q, A);
    A.view_on = 0;

    const float4* d_segs = reinterpret_cast<const float4*>(segs);
    uint8_t* d_out = out;
    const size_t n = nsegs;
    if (!dev) {
        if ((rc = stage(c, &c->d_qrays, &c->capqrays, n * sizeof(trt_qseg), "alloc query segments", segs, &d_segs)) != TRT_OK) return rc;
        if ((rc = stage(c, &c->d_out8, &c->cap8, n, "alloc occlusion bytes", nullptr, &d_out)) != TRT_OK) return rc;
    }
    if ((rc = begin_call(c, false, timing)) != TRT_OK) return rc;
    HIP_TRY(c, trt::launch_occlusion_query(A, d_segs, nsegs, d_out, c->stream));
    return finish_call(c, dev, false, timing, st, {{out, d_out, n}});
}

// Visibility masks (abi.h): the gather form of trt_occluded through visibility_query_kernel, which
// forms the npts * nset segments itself.  The set, always a host array, is checked here and copied
// stream-ordered into a small buffer of the context; host points stage through the ray-query record
// buffer and the masks through the RGBA8 buffer (hipMalloc's alignment serves both).  Like
// trt_occluded it writes nothing of the context that a frame or a query depends on.
int trt_visibility(trt_ctx* c, const trt_params* p, const trt_qpoint* pts, uint32_t npts, const float* set, uint32_t nset,
                   uint32_t mode, uint64_t* out, trt_stats* st) {
    if (!c) return TRT_ERR_INVALID;
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_visibility: null params");
    if (!c->have_scene) return fail(c, TRT_ERR_NOSCENE, "trt_visibility: no scene uploaded");
    if (p->flags & TRT_FLAG_COUNT)
        return fail(c, TRT_ERR_INVALID, "trt_visibility: TRT_FLAG_COUNT is not offered (any-hit counters depend on the walk order)");
    if ((p->flags & TRT_FLAG_TIMING) && !st) return fail(c, TRT_ERR_INVALID, "trt_visibility: TRT_FLAG_TIMING needs stats");
    if (mode != TRT_VIS_DIRS && mode != TRT_VIS_TARGETS) return fail(c, TRT_ERR_INVALID, "trt_visibility: unknown mode");
    if (nset < 1u || nset > TRT_VIS_MAX_SET) return fail(c, TRT_ERR_INVALID, "trt_visibility: a set holds 1..63 entries");
    if ((uint64_t)npts * nset > TRT_QRAY_MAX_RAYS) return fail(c, TRT_ERR_INVALID, "trt_visibility: more than 2^28 segments");
    if (npts && !pts) return fail(c, TRT_ERR_INVALID, "trt_visibility: null pts");
    if (npts && !set) return fail(c, TRT_ERR_INVALID, "trt_visibility: null set");
    if (npts && !out) return fail(c, TRT_ERR_INVALID, "trt_visibility: null out_masks");
    const bool dev = (p->flags & TRT_FLAG_DEVICE_PTRS) != 0;
    // the kernel reads a point as two 16-byte vectors straight from the caller's device array and
    // stores whole 8-byte masks (host arrays are staged)
    if (dev && (reinterpret_cast<uintptr_t>(pts) & 15u))
        return fail(c, TRT_ERR_INVALID, "trt_visibility: device pts must be 16-byte aligned");
    if (dev && (reinterpret_cast<uintptr_t>(out) & 7u))
        return fail(c, TRT_ERR_INVALID, "trt_visibility: device out_masks must be 8-byte aligned");
    if (set) {
        uint32_t bad = 0;
        if (check_vis_set(set, nset, mode, &bad) != TRT_OK)
            return fail(c, TRT_ERR_INVALID, "trt_visibility: set entry " + std::to_string(bad) +
                                                (mode == TRT_VIS_DIRS ? " is not a valid direction (non-finite, or length out of range)"
                                                                      : " is not finite"));
    }
    const bool timing = (p->flags & TRT_FLAG_TIMING) != 0;
    if (st) std::memset(st, 0, sizeof(*st));
    if (npts == 0) return TRT_OK;
    if (!dev) { // a device array cannot be read here: the kernel applies the same predicate
        uint32_t bad = 0;
        if (trt_check_points(pts, npts, &bad) != TRT_OK)
            return fail(c, TRT_ERR_INVALID, "trt_visibility: point " + std::to_string(bad) +
                                                " is not valid (non-finite pos or n, or tmax out of range)");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    const trt_params q = query_params(p, 1, TRT_FLAG_SPHERES | TRT_FLAG_FLOOR | TRT_FLAG_BATCH_WALK | TRT_FLAG_DEVICE_PTRS | TRT_FLAG_TIMING);
    int rc;
    KArgs A;
    fill_args(c, &q, A);
    A.view_on = 0;

    const float4* d_pts = reinterpret_cast<const float4*>(pts);
    uint64_t* d_out = out;
    const size_t n = npts;
    // the buffer holds a whole 64-entry set whatever nset is; the copy is ordered on the stream
    // behind an earlier query's kernel, which may still be reading the buffer
    if ((rc = ensure(c, &c->d_visset, &c->capvisset, 64 * 4 * sizeof(float), "alloc visibility set")) != TRT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_visset, set, (size_t)nset * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const float4* d_set = static_cast<const float4*>(c->d_visset);
    if (!dev) {
        if ((rc = stage(c, &c->d_qrays, &c->capqrays, n * sizeof(trt_qpoint), "alloc query points", pts, &d_pts)) != TRT_OK) return rc;
        if ((rc = stage(c, &c->d_out8, &c->cap8, n * sizeof(uint64_t), "alloc visibility masks", nullptr, &d_out)) != TRT_OK) return rc;
    }
    if ((rc = begin_call(c, false, timing)) != TRT_OK) return rc;
    HIP_TRY(c, trt::launch_visibility_query(A, d_pts, npts, d_set, nset, mode, c->vis_coop, d_out, c->stream));
    return finish_call(c, dev, false, timing, st, {{out, d_out, n * sizeof(uint64_t)}});
}

// All-hits queries (abi.h): the caller's segments through all_hits_kernel, up to max_hits records
// and one count each.  Shaped like trt_occluded; host segments stage through the ray-query record
// buffer, the records through the hit-record buffer and the counts through the RGBA8 buffer.
int trt_trace_all(trt_ctx* c, const trt_params* p, const trt_qseg* segs, uint32_t nsegs, uint32_t max_hits, trt_qhit* hits,
                  uint32_t* counts, trt_stats* st) {
    if (!c) return TRT_ERR_INVALID;
    if (!p) return fail(c, TRT_ERR_INVALID, "trt_trace_all: null params");
    if (!c->have_scene) return fail(c, TRT_ERR_NOSCENE, "trt_trace_all: no scene uploaded");
    if (p->flags & TRT_FLAG_COUNT) return fail(c, TRT_ERR_INVALID, "trt_trace_all: TRT_FLAG_COUNT is not offered");
    if ((p->flags & TRT_FLAG_TIMING) && !st) return fail(c, TRT_ERR_INVALID, "trt_trace_all: TRT_FLAG_TIMING needs stats");
    if (max_hits < 1u || max_hits > TRT_ALLHITS_MAX) return fail(c, TRT_ERR_INVALID, "trt_trace_all: max_hits must be 1..32");
    if ((uint64_t)nsegs * max_hits > TRT_QRAY_MAX_RAYS) return fail(c, TRT_ERR_INVALID, "trt_trace_all: more than 2^28 hit slots");
    if (nsegs && !segs) return fail(c, TRT_ERR_INVALID, "trt_trace_all: null segs");
    if (nsegs && !counts) return fail(c, TRT_ERR_INVALID, "trt_trace_all: null counts");
    const bool dev = (p->flags & TRT_FLAG_DEVICE_PTRS) != 0;
    // the kernel moves a segment and a hit record as 16-byte vectors and a count as one word,
    // straight from and to the caller's device arrays (host arrays are staged)
    if (dev && ((reinterpret_cast<uintptr_t>(segs) | reinterpret_cast<uintptr_t>(hits)) & 15u))
        return fail(c, TRT_ERR_INVALID, "trt_trace_all: device segs and hits must be 16-byte aligned");
    if (dev && (reinterpret_cast<uintptr_t>(counts) & 3u))
        return fail(c, TRT_ERR_INVALID, "trt_trace_all: device counts must be 4-byte aligned");
    const bool timing = (p->flags & TRT_FLAG_TIMING) != 0;
    if (st) std::memset(st, 0, sizeof(*st));
    if (nsegs == 0) return TRT_OK;
    if (!dev) { // a device array cannot be read here: the kernel applies the same predicate
        uint32_t bad = 0;
        if (trt_check_segs(segs, nsegs, &bad) != TRT_OK)
            return fail(c, TRT_ERR_INVALID, "trt_trace_all: segment " + std::to_string(bad) +
                                                " is not valid (non-finite, direction length or tmax out of range)");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    const trt_params q = query_params(p, 1, TRT_FLAG_SPHERES | TRT_FLAG_FLOOR | TRT_FLAG_BATCH_WALK | TRT_FLAG_DEVICE_PTRS | TRT_FLAG_TIMING);
    int rc;
    KArgs A;
    fill_args(c, &q, A);
    A.view_on = 0;

    const float4* d_segs = reinterpret_cast<const float4*>(segs);
    uint4* dh = reinterpret_cast<uint4*>(hits);
    uint32_t* d_counts = counts;
    const size_t n = nsegs, nh = n * max_hits;
    if (!dev) {
        if ((rc = stage(c, &c->d_qrays, &c->capqrays, n * sizeof(trt_qseg), "alloc query segments", segs, &d_segs)) != TRT_OK) return rc;
        if (hits && (rc = stage(c, &c->d_qhits, &c->capqhits, nh * sizeof(trt_qhit), "alloc all-hits records", nullptr, &dh)) != TRT_OK) return rc;
        if ((rc = stage(c, &c->d_out8, &c->cap8, n * sizeof(uint32_t), "alloc all-hits counts", nullptr, &d_counts)) != TRT_OK) return rc;
    }
    if ((rc = begin_call(c, false, timing)) != TRT_OK) return rc;
    HIP_TRY(c, trt::launch_all_hits(A, d_segs, nsegs, max_hits, dh, d_counts, c->stream));
    return finish_call(c, dev, false, timing, st, {{hits, dh, nh * sizeof(trt_qhit)}, {counts, d_counts, n * sizeof(uint32_t)}});
}

} // extern "C"

// ---- envmap JPEG: host entropy decode + GPU reconstruction ----------------

extern "C" int trt_jpeg_decode(trt_ctx* c, const trt_jpeg* j, uint8_t* out, uint32_t flags) {
    if (!c) return TRT_ERR_INVALID;
    const trt::jpeg::Image* im = trt::jpeg::image_of(j);
    if (!im) return fail(c, TRT_ERR_INVALID, "trt_jpeg_decode: nothing parsed");
    if (!out) return fail(c, TRT_ERR_INVALID, "trt_jpeg_decode: null output");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)im->width * im->height * 4;
    const bool dev = (flags & TRT_FLAG_DEVICE_PTRS) != 0;
    uint8_t* dst = out;
    if (!dev) {
        const int rc = stage(c, &c->d_out8, &c->cap8, bytes, "jpeg output", nullptr, &dst);
        if (rc != TRT_OK) return rc;
    }
    HIP_TRY(c, trt::jpeg::reconstruct(*im, dst, c->stream));
    return finish_call(c, dev, false, false, nullptr, {{out, dst, bytes}});
}

