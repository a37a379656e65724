// scene_pack.cpp — the host packing of a scene (scene_pack.h).  Pure host arithmetic:
// trt_scene_upload.cpp uploads what it makes.
#include "scene_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <string>

namespace trt {
Mat to_mat(const trt_material& m) {
    const trt_vec4 &a = m.albedo, &d = m.diffuse_specular;
    return Mat{{a.x, a.y, a.z, a.w}, {d.x, d.y, d.z}, d.w, m.refractive.x, {}};
}

int64_t first_bad_model(const trt_model* models, uint32_t nmodel, uint32_t ntri) {
    for (uint32_t i = 0; i < nmodel; ++i) {
        const int64_t s = models[i].params0.x, n = models[i].params0.y;
        if (s < 0 || n < 0 || s + n > (int64_t)ntri) return i;
    }
    return -1;
}

void pack_scene(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel, PackedScene& ps) {
    ps = PackedScene{};
    // Repack binding 6 (Model) and binding 5 (Triangle) for the wave-uniform walks.
    std::vector<BatchRec>& batches = ps.batches;
    batches.resize(nmodel);
    for (uint32_t i = 0; i < nmodel; ++i) {
        const trt_model& m = models[i];
        BatchRec& b = batches[i];
        std::memcpy(b.bmin, &m.bboxMin, sizeof(b.bmin)); // x, y, z
        std::memcpy(b.bmax, &m.bboxMax, sizeof(b.bmax));
        b.start = m.params0.x;
        b.count_ni = (m.params0.y & 0x7fffffff) | (m.params0.z != 0 ? (int32_t)0x80000000 : 0);
    }
    // Implicit 8-ary range hierarchy: node k of level L is the exact union of the boxes of
    // batches [k*8^L, (k+1)*8^L).  A NaN coordinate anywhere below makes the node infinite
    // (always entered), so culling stays conservative for degenerate input.
    std::vector<float4>& nodes = ps.nodes;
    uint32_t* node_off = ps.node_off;
    uint32_t& top = ps.top;
    while (top < 10 && (1ull << (3 * top)) < (unsigned long long)nmodel) ++top;
    {
        std::vector<float4> prev_lo(nmodel), prev_hi(nmodel);
        for (uint32_t i = 0; i < nmodel; ++i) {
            const BatchRec& b = batches[i];
            prev_lo[i] = make_float4(b.bmin[0], b.bmin[1], b.bmin[2], 0.0f);
            prev_hi[i] = make_float4(b.bmax[0], b.bmax[1], b.bmax[2], 0.0f);
        }
        const float inf = std::numeric_limits<float>::infinity();
        for (uint32_t L = 1; L <= top; ++L) {
            const size_t n = (prev_lo.size() + 7) / 8;
            node_off[L] = (uint32_t)(nodes.size() / 2);
            std::vector<float4> lo(n), hi(n);
            for (size_t k = 0; k < n; ++k) {
                float4 a = make_float4(inf, inf, inf, 0.0f), z = make_float4(-inf, -inf, -inf, 0.0f);
                bool bad = false;
                for (size_t j = 8 * k; j < std::min(prev_lo.size(), 8 * k + 8); ++j) {
                    const float4 &pl = prev_lo[j], &ph = prev_hi[j];
                    bad |= std::isnan(pl.x) || std::isnan(pl.y) || std::isnan(pl.z) || std::isnan(ph.x) ||
                           std::isnan(ph.y) || std::isnan(ph.z);
                    // the reference's slab test takes min / max of the two planes per axis, so a
                    // batch box with bboxMin > bboxMax on an axis (a caller's, or the builder's
                    // untouched FLT_MAX / -FLT_MAX sentinels when every vertex is NaN there) is the
                    // slab between the planes, not an empty one: the union orders the planes first
                    const float4 l = make_float4(std::min(pl.x, ph.x), std::min(pl.y, ph.y), std::min(pl.z, ph.z), 0.0f);
                    const float4 h = make_float4(std::max(pl.x, ph.x), std::max(pl.y, ph.y), std::max(pl.z, ph.z), 0.0f);
                    a.x = std::min(a.x, l.x); a.y = std::min(a.y, l.y); a.z = std::min(a.z, l.z);
                    z.x = std::max(z.x, h.x); z.y = std::max(z.y, h.y); z.z = std::max(z.z, h.z);
                }
                if (bad) {
                    a = make_float4(-inf, -inf, -inf, 0.0f);
                    z = make_float4(inf, inf, inf, 0.0f);
                }
                lo[k] = a;
                hi[k] = z;
                nodes.push_back(a);
                nodes.push_back(z);
            }
            prev_lo.swap(lo);
            prev_hi.swap(hi);
        }
    }
    std::vector<TriGeo>& geo = ps.geo;
    std::vector<TriShade>& shade = ps.shade;
    std::vector<Mat>& mats = ps.mats;
    geo.resize(ntri);
    shade.resize(ntri);
    std::map<std::string, uint32_t> mat_index;
    for (uint32_t j = 0; j < ntri; ++j) {
        const trt_triangle& t = tris[j];
        TriGeo& g = geo[j];
        std::memcpy(g.v0, &t.v0, sizeof(g.v0)); // x, y, z
        // edge1 = v1 - v0, edge2 = v2 - v0 (shader.comp:230-231): same float subtraction
        g.e1[0] = t.v1.x - t.v0.x;
        g.e1[1] = t.v1.y - t.v0.y;
        g.e1[2] = t.v1.z - t.v0.z;
        g.e2[0] = t.v2.x - t.v0.x;
        g.e2[1] = t.v2.y - t.v0.y;
        g.e2[2] = t.v2.z - t.v0.z;
        g.pad[0] = g.pad[1] = g.pad[2] = 0.0f;
        TriShade& s = shade[j];
        std::memcpy(s.n0, &t.v0_norm, sizeof(s.n0)); // x, y, z
        std::memcpy(s.n1, &t.v1_norm, sizeof(s.n1));
        std::memcpy(s.n2, &t.v2_norm, sizeof(s.n2));
        std::string key(reinterpret_cast<const char*>(&t.material), sizeof(trt_material));
        auto it = mat_index.find(key);
        if (it == mat_index.end()) {
            it = mat_index.emplace(key, (uint32_t)mats.size()).first;
            mats.push_back(to_mat(t.material));
        }
        s.material = it->second;
        s.pad[0] = s.pad[1] = 0;
    }
    if (mats.empty()) mats.push_back(Mat{});

    pack_bvh(tris, ntri, models, nmodel, (uint32_t)kBvhStack, ps);
}

bool pack_bvh(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel, uint32_t max_stack,
              PackedScene& ps) {
    ps.bvh4.clear();
    ps.bvh4q.clear();
    ps.bvh4_stack = 0;
    if (!nmodel || !build_bvh(tris, ntri, models, nmodel, ps.bvh, ps.bvh_tris)) {
        ps.bvh.clear();
        ps.bvh_tris.clear();
        return false;
    }
    // the 4-wide walk only when its worst-case stack fits (else the BVH2 walk: <= depth)
    ps.bvh4_stack = collapse_bvh4(ps.bvh, ps.bvh4);
    if (ps.bvh4_stack > max_stack) ps.bvh4.clear();
    if (ps.bvh4.empty() || !quantize_bvh4(ps.bvh4, ps.bvh4q)) ps.bvh4q.clear();
    return true;
}

} // namespace trt
