// trt_diag.cpp — diagnostic entries (not part of include/trt/abi.h) for tests/ and tools/.
#include <cstring>

#include "scene_pack.h"
#include "trt_internal.h"

using namespace trt;

// diagnostic: the first 16 words of slot `slot`'s deferred-frame counters (nfb + pad, where
// defer_resolve records a log it could not finish)
extern "C" int trt_diag_defer_pad(trt_ctx* c, uint32_t slot, uint32_t* out16) {
    if (!c || !out16 || slot >= TRT_BUILD_MAX_IN_FLIGHT || !c->split[slot].dctr) return TRT_ERR_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out16, c->split[slot].dctr, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TRT_OK;
}

// Ray-dump buffer of TRT_DIAG_DUMP_SHADOW builds (device pointer, or NULL; tools/shadow_exp.py).
extern "C" int trt_diag_set_buffer(trt_ctx* c, void* dev_ptr) {
    if (!c) return TRT_ERR_INVALID;
    c->diag = dev_ptr;
    return TRT_OK;
}

// attach_floor_class's floor_lit conditions on a launch's flags and its three lights (x, y, z
// each), without the knob: 1 or 0 (tests/test_floor_lit.py, no GPU).
extern "C" int trt_diag_floor_lit(uint32_t flags, const float* lights) {
    if (!lights) return 0;
    return (int)floor_lit(flags, reinterpret_cast<const float(*)[3]>(lights));
}

// counters[k] of the last counting pass (k < 32).
extern "C" unsigned long long trt_diag_counter(trt_ctx* c, uint32_t k) {
    unsigned long long v = 0;
    if (!c || k >= 32 || hipSetDevice(c->device) != hipSuccess) return 0;
    if (hipMemcpy(&v, c->d_counters + k, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return v;
}

// Traces n shadow queries (2 float4 each, device) into occ (device, one uint32 each) on the
// context's stream with the frame params' traversal (BVH build, waves).
extern "C" int trt_diag_shadow_batch(trt_ctx* c, const trt_params* p, const void* rays, uint32_t n, void* occ) {
    if (!c) return TRT_ERR_INVALID;
    int rc = check_params(c, p);
    if (rc != TRT_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_envp(c, p, c->stream)) != TRT_OK) return rc;
    KArgs A;
    fill_args(c, p, A);
    HIP_TRY(c, trt::launch_shadow_batch(A, static_cast<const float4*>(rays), n, static_cast<uint32_t*>(occ), c->stream));
    return TRT_OK;
}

// Diagnostic (tests/test_deal_order.py), host only: the (tile, frame) of every block of a launch
// shape, by the kernels' own dealing functions (trt_deal.h) over fill_deal's constants.
// inter 0: block vb is xcd_tile(vb % ntiles, vb / ntiles) (F frames one after the other; F 1: a
// single frame); inter 1, 2: inter_tile over F frames or pairs.  tile_out, frame_out: ntiles * F
// words each.
extern "C" int trt_diag_deal_map(uint32_t ntx, uint32_t ntiles, uint32_t F, uint32_t xcd_rot, uint32_t xcd_skew,
                                 uint32_t xcd_inter, uint32_t xcd_mult, uint32_t* tile_out, uint32_t* frame_out) {
    if (!ntx || !ntiles || ntiles % ntx || !F || !tile_out || !frame_out) return TRT_ERR_INVALID;
    Deal D;
    fill_deal(D, ntx, ntiles, xcd_inter ? F : 1u);
    const DealKnobs K{xcd_rot, xcd_skew, xcd_inter, xcd_mult};
    for (uint32_t vb = 0; vb < ntiles * F; ++vb) {
        uint32_t f = 0, tile;
        if (xcd_inter) {
            tile = inter_tile(D, K, vb, f);
        } else {
            f = vb / ntiles;
            tile = xcd_tile(D, K, vb - f * ntiles, f);
        }
        tile_out[vb] = tile;
        frame_out[vb] = f;
    }
    return TRT_OK;
}

// Diagnostic, host only: the kernels' division by a launch divisor (trt_deal.h deal_div over
// deal_magic's multiplier).  trt_diag_deal_div: out[i] = n[i] / d by deal_div; trt_diag_deal_div_range:
// the number of n in [n0, n1) for which deal_div differs from n / d.
extern "C" void trt_diag_deal_div(uint32_t d, const uint32_t* n, uint32_t count, uint32_t* out) {
    Deal D{};
    uint32_t s;
    deal_magic(d, D.magic[kDivNl], s);
    D.shifts = s << (6u * kDivNl);
    for (uint32_t i = 0; i < count; ++i) out[i] = deal_div(D, kDivNl, n[i]);
}
extern "C" uint64_t trt_diag_deal_div_range(uint32_t d, uint64_t n0, uint64_t n1) {
    if (!d || n1 > (1ull << 32)) return UINT64_MAX;
    Deal D{};
    uint32_t s;
    deal_magic(d, D.magic[kDivNtx], s);
    D.shifts = s;
    uint64_t bad = 0;
    for (uint64_t n = n0; n < n1; ++n) bad += deal_div(D, kDivNtx, (uint32_t)n) != (uint32_t)n / d;
    return bad;
}

namespace {
// The upload's BVH step, 4-wide nodes kept whatever their stack.  False: bad arguments or no BVH.
bool diag_bvh(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel, const void* out,
              PackedScene& s) {
    if (!out || (ntri && !tris) || (nmodel && !models)) return false;
    return pack_bvh(tris, ntri, models, nmodel, UINT32_MAX, s);
}

template <class T>
void copy_out(T* dst, uint32_t cap, const std::vector<T>& v) {
    if (dst && v.size() <= cap) std::memcpy(dst, v.data(), v.size() * sizeof(T));
}

uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 0x100000001b3ull;
    return h;
}
} // namespace

// Diagnostic (tests/test_bvh_layout.py): the BVH2 the upload builds — nodes and the BVH-ordered
// leaf triangle records (meta: triangle, batch, ni) — copied out when the capacities suffice;
// counts[0] = nodes, counts[1] = leaf references.
extern "C" int trt_diag_bvh_export(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel,
                                   trt::BvhNode* nodes_out, uint32_t cap_nodes, TriGeo* tris_out, uint32_t cap_tris,
                                   uint64_t counts[2]) {
    PackedScene s;
    if (!diag_bvh(tris, ntri, models, nmodel, counts, s)) return TRT_ERR_INVALID;
    counts[0] = s.bvh.size();
    counts[1] = s.bvh_tris.size();
    copy_out(nodes_out, cap_nodes, s.bvh);
    copy_out(tris_out, cap_tris, s.bvh_tris);
    return TRT_OK;
}

// Diagnostic (tests/test_mesh_cases.py), host only: the 4-wide nodes collapse_bvh4 makes of that
// BVH2 (child refs index these nodes or the leaf references of trt_diag_bvh_export), copied out
// when the capacity suffices; counts[0] = 4-wide nodes, counts[1] = their worst-case stack (the
// upload keeps them only when it is <= kBvhStack).
extern "C" int trt_diag_bvh4_export(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel,
                                    trt::Bvh4Node* nodes_out, uint32_t cap_nodes, uint64_t counts[2]) {
    PackedScene s;
    if (!diag_bvh(tris, ntri, models, nmodel, counts, s)) return TRT_ERR_INVALID;
    counts[1] = s.bvh4_stack;
    counts[0] = s.bvh4.size();
    copy_out(nodes_out, cap_nodes, s.bvh4);
    return TRT_OK;
}

// Host-only check of the BVH pipeline of trt_upload_scene (no GPU): BVH2 build, 4-wide
// collapse and quantization.  out[0] BVH2 nodes, out[1] BVH4 nodes, out[2] quantized (0/1),
// out[3] BVH2 depth (levels of the deepest leaf, root = 1), out[4] worst-case BVH4 stack,
// out[5] leaf triangles.  Returns TRT_ERR_INVALID when no BVH is built (overlapping batch ranges).
extern "C" int trt_diag_bvh_build(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel,
                                  uint64_t out[6]) {
    if (!out || (ntri && !tris) || (nmodel && !models)) return TRT_ERR_INVALID;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    PackedScene s;
    if (!diag_bvh(tris, ntri, models, nmodel, out, s)) return TRT_ERR_INVALID;
    out[0] = s.bvh.size();
    out[4] = s.bvh4_stack;
    out[1] = s.bvh4.size();
    out[2] = s.bvh4q.empty() ? 0 : 1;
    out[3] = trt::bvh_depth(s.bvh);
    out[5] = s.bvh_tris.size();
    return TRT_OK;
}

// Diagnostic (tests/test_scene_pack.py), host only: what pack_scene makes of a scene.  out[0] =
// top, out[1..11] = node_off, then the element count and the 64-bit FNV-1a hash of the bytes of
// each packed array: batches, nodes, geo, shade, mats, bvh, bvh4, bvh4q, bvh_tris (out[12..29]);
// out[30] = the collapse's worst-case stack (0: no BVH).  TRT_ERR_INVALID for what
// trt_upload_scene rejects.
extern "C" int trt_diag_scene_pack(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel,
                                   uint64_t out[31]) {
    if (!out || (ntri && !tris) || (nmodel && !models) || first_bad_model(models, nmodel, ntri) >= 0) return TRT_ERR_INVALID;
    PackedScene s;
    pack_scene(tris, ntri, models, nmodel, s);
    out[0] = s.top;
    for (int i = 0; i < 11; ++i) out[1 + i] = s.node_off[i];
    uint64_t* o = out + 12;
    auto put = [&o](const auto& v) {
        *o++ = v.size();
        *o++ = fnv1a(v.data(), v.size() * sizeof(v[0]));
    };
    put(s.batches), put(s.nodes), put(s.geo), put(s.shade), put(s.mats), put(s.bvh), put(s.bvh4), put(s.bvh4q), put(s.bvh_tris);
    *o = s.bvh4_stack;
    return TRT_OK;
}
