// scene_pack.h — what trt_upload_scene computes on the host before it touches the device: the
// arrays behind the scene bindings (trt_ctx.h SceneBuf), as plain vectors.  No HIP runtime call.
#pragma once

#include <vector>

#include "../../include/trt/abi.h"
#include "trt_device.h"

#pragma GCC visibility push(hidden) // internal to libtrt.so
namespace trt {

struct PackedScene {
    std::vector<BatchRec> batches;
    std::vector<float4> nodes; // the implicit 8-ary hierarchy: (lo, hi) per node, level by level
    std::vector<TriGeo> geo;
    std::vector<TriShade> shade;
    std::vector<Mat> mats;
    // pack_bvh: empty when no BVH is built; bvh4 also when its stack does not fit; bvh4q with it
    std::vector<BvhNode> bvh;
    std::vector<Bvh4Node> bvh4;
    std::vector<Bvh4QNode> bvh4q;
    std::vector<TriGeo> bvh_tris;
    uint32_t bvh4_stack = 0; // collapse_bvh4's worst-case stack, whether or not bvh4 was kept
    uint32_t top = 0;
    uint32_t node_off[11] = {0};
};

// bvh_build.cpp
bool build_bvh(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel,
               std::vector<BvhNode>& nodes, std::vector<TriGeo>& leaf_tris);
uint32_t collapse_bvh4(const std::vector<BvhNode>& b2, std::vector<Bvh4Node>& b4);
bool quantize_bvh4(const std::vector<Bvh4Node>& b4, std::vector<Bvh4QNode>& out);
uint32_t bvh_depth(const std::vector<BvhNode>& b2);

Mat to_mat(const trt_material& m);
// The first model whose triangle range lies outside [0, ntri), or -1.
int64_t first_bad_model(const trt_model* models, uint32_t nmodel, uint32_t ntri);
// BVH2 build, 4-wide collapse, quantization.  False (and no nodes) when no BVH is built.  The
// 4-wide nodes are dropped when their stack exceeds max_stack (the upload's is kBvhStack).
bool pack_bvh(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel, uint32_t max_stack,
              PackedScene& ps);
// Everything of a scene but the envmap.  The caller has checked first_bad_model.
void pack_scene(const trt_triangle* tris, uint32_t ntri, const trt_model* models, uint32_t nmodel, PackedScene& ps);
} // namespace trt
#pragma GCC visibility pop
