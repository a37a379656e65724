// trt_scene_upload.cpp — the scene bindings of a context: trt_upload_scene, the envmap JPEG
// upload, and the header and adoption behind trt_multi.cpp's scene broadcast.
#include <cstring>

#include "jpeg.h"
#include "scene_pack.h"
#include "trt_internal.h"

namespace trt {

void** scene_buf(trt_ctx* c, int k) {
    switch (k) {
    case kSceneBatches: return reinterpret_cast<void**>(&c->d_batches);
    case kSceneNodes: return reinterpret_cast<void**>(&c->d_nodes);
    case kSceneBvh: return reinterpret_cast<void**>(&c->d_bvh);
    case kSceneBvh4: return reinterpret_cast<void**>(&c->d_bvh4);
    case kSceneBvhTris: return reinterpret_cast<void**>(&c->d_bvh_tris);
    case kSceneGeo: return reinterpret_cast<void**>(&c->d_geo);
    case kSceneShade: return reinterpret_cast<void**>(&c->d_shade);
    case kSceneMats: return reinterpret_cast<void**>(&c->d_mats);
    case kSceneBvh4Q: return reinterpret_cast<void**>(&c->d_bvh4q);
    default: return reinterpret_cast<void**>(&c->d_env);
    }
}

void free_scene(trt_ctx* c) {
    for (int k = 0; k < kSceneBufs; ++k) {
        void** p = scene_buf(c, k);
        (void)hipFree(*p);
        *p = nullptr;
    }
    c->top = 0;
    c->envp_ok = false;
    ++c->env_gen;
    c->nbatch = c->ntri = c->nmat = c->env_w = c->env_h = 0;
    std::memset(c->scene_bytes, 0, sizeof(c->scene_bytes));
    c->have_scene = false;
}

namespace {

// Binding k takes the device buffer d of `bytes` bytes; what it held is freed.
void scene_set(trt_ctx* c, int k, void* d, size_t bytes) {
    void** p = scene_buf(c, k);
    (void)hipFree(*p);
    *p = d;
    c->scene_bytes[k] = bytes;
}

// ... a new buffer, filled from src when given.  On failure the scene is dropped.
int scene_alloc(trt_ctx* c, int k, const void* src, size_t bytes, const char* what) {
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess && src) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    scene_set(c, k, d, bytes);
    if (e == hipSuccess) return TRT_OK;
    free_scene(c);
    return hip_fail(c, e, what);
}

} // namespace

// What a scene has besides its buffers, between a context and a header (the members' names agree).
template <class D, class S>
void copy_scene_scalars(D& d, const S& s) {
    d.nbatch = s.nbatch;
    d.ntri = s.ntri;
    d.nmat = s.nmat;
    d.env_w = s.env_w;
    d.env_h = s.env_h;
    d.top = s.top;
    std::memcpy(d.node_off, s.node_off, sizeof(d.node_off));
    d.ubo = s.ubo;
}

void scene_header(const trt_ctx* c, SceneHeader& h) {
    std::memset(&h, 0, sizeof(h));
    h.magic = kSceneMagic;
    copy_scene_scalars(h, *c);
    for (int k = 0; k < kSceneBufs; ++k) h.bytes[k] = c->scene_bytes[k];
}

int scene_adopt(trt_ctx* c, const SceneHeader& h) {
    if (h.magic != kSceneMagic) return fail(c, TRT_ERR_INVALID, "scene broadcast: bad header");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_scene(c);
    for (int k = 0; k < kSceneBufs; ++k) {
        if (!h.bytes[k]) continue;
        const int rc = scene_alloc(c, k, nullptr, h.bytes[k], "scene broadcast: alloc");
        if (rc != TRT_OK) return rc;
    }
    copy_scene_scalars(*c, h);
    c->have_scene = true;
    return TRT_OK;
}

} // namespace trt

using namespace trt;

extern "C" int trt_upload_scene(trt_ctx* c, const trt_ubo* ubo, const trt_triangle* tris, uint32_t ntri,
                                const trt_model* models, uint32_t nmodel, const uint8_t* env,
                                uint32_t env_w, uint32_t env_h) {
    if (!c) return TRT_ERR_INVALID;
    if (!ubo) return fail(c, TRT_ERR_INVALID, "trt_upload_scene: null ubo");
    if (ntri && !tris) return fail(c, TRT_ERR_INVALID, "trt_upload_scene: null triangles");
    if (nmodel && !models) return fail(c, TRT_ERR_INVALID, "trt_upload_scene: null models");
    if (env && (env_w == 0 || env_h == 0))
        return fail(c, TRT_ERR_INVALID, "trt_upload_scene: zero-size envmap");
    const int64_t bad = first_bad_model(models, nmodel, ntri);
    if (bad >= 0)
        return fail(c, TRT_ERR_INVALID,
                    "trt_upload_scene: model " + std::to_string(bad) + " triangle range outside the triangle buffer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_scene(c);

    PackedScene s;
    pack_scene(tris, ntri, models, nmodel, s);
    // in upload order; `always`: never bind a null buffer (an empty array gets 16 bytes, no copy)
    const struct { int k; const void* src; size_t bytes; bool always; const char* what; } up[] = {
        {kSceneBatches, s.batches.data(), sizeof(BatchRec) * s.batches.size(), true, "upload batches"},
        {kSceneGeo, s.geo.data(), sizeof(TriGeo) * s.geo.size(), true, "upload triangle geometry"},
        {kSceneShade, s.shade.data(), sizeof(TriShade) * s.shade.size(), true, "upload triangle shading"},
        {kSceneMats, s.mats.data(), sizeof(Mat) * s.mats.size(), true, "upload materials"},
        {kSceneNodes, s.nodes.data(), sizeof(float4) * s.nodes.size(), true, "upload batch hierarchy"},
        {kSceneBvh4Q, s.bvh4q.data(), sizeof(Bvh4QNode) * s.bvh4q.size(), false, "upload quantized bvh4"},
        {kSceneBvh, s.bvh.data(), sizeof(BvhNode) * s.bvh.size(), false, "upload bvh"},
        {kSceneBvh4, s.bvh4.data(), sizeof(Bvh4Node) * s.bvh4.size(), false, "upload bvh4"},
        {kSceneBvhTris, s.bvh_tris.data(), sizeof(TriGeo) * s.bvh_tris.size(), false, "upload bvh triangles"},
        {kSceneEnv, env, env ? (size_t)env_w * env_h * 4 : 0, false, "upload envmap"},
    };
    static_assert(sizeof(up) / sizeof(up[0]) == kSceneBufs, "one upload entry per scene binding");
    for (const auto& b : up) {
        if (!b.bytes && !b.always) continue;
        const int rc = scene_alloc(c, b.k, b.bytes ? b.src : nullptr, b.bytes ? b.bytes : 16, b.what);
        if (rc != TRT_OK) return rc;
    }
    if (env) {
        c->env_w = env_w;
        c->env_h = env_h;
    }
    c->nbatch = nmodel;
    c->top = s.top;
    std::memcpy(c->node_off, s.node_off, sizeof(s.node_off));
    c->ntri = ntri;
    c->nmat = (uint32_t)s.mats.size();
    c->ubo = *ubo;
    c->have_scene = true;
    return TRT_OK;
}

extern "C" int trt_upload_envmap_jpeg(trt_ctx* c, const uint8_t* data, size_t len) {
    if (!c) return TRT_ERR_INVALID;
    trt_jpeg* j = nullptr;
    int rc = trt_jpeg_create(&j);
    if (rc != TRT_OK) return fail(c, rc, "trt_upload_envmap_jpeg: out of memory");
    rc = trt_jpeg_parse(j, data, len);
    if (rc != TRT_OK) {
        std::string msg = std::string("trt_upload_envmap_jpeg: ") + trt_jpeg_last_error(j);
        trt_jpeg_destroy(j);
        return fail(c, rc, msg);
    }
    const trt::jpeg::Image* im = trt::jpeg::image_of(j);
    hipError_t e = hipSetDevice(c->device);
    uint32_t* d = nullptr;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d), (size_t)im->width * im->height * 4);
    if (e == hipSuccess) e = trt::jpeg::reconstruct(*im, reinterpret_cast<uint8_t*>(d), c->stream);
    if (e != hipSuccess) {
        (void)hipFree(d);
        trt_jpeg_destroy(j);
        return hip_fail(c, e, "trt_upload_envmap_jpeg");
    }
    scene_set(c, kSceneEnv, d, (size_t)im->width * im->height * 4);
    c->envp_ok = false;
    ++c->env_gen;
    c->env_w = (uint32_t)im->width;
    c->env_h = (uint32_t)im->height;
    trt_jpeg_destroy(j);
    return TRT_OK;
}
