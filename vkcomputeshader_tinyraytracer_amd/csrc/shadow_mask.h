// shadow_mask.h — per launch, which spheres can occlude which lights from where (host only, no
// HIP).
//
// Spheres and lights are per-launch constants, so whether sphere j can shadow a point from
// light i depends on the point alone: not on the camera, the frame or the ray that found it.
// Bit 4 * i + j of a mask means "sphere j may occlude light i"; a clear bit is a proof that
// shadow_intersect's test of sphere j cannot return an accepted hit for a query towards light i
// from any point the mask serves, so sky_trace_kernel skips the test when the bit is clear in
// every active lane of the wave.
#pragma once

#include <stdint.h>

#include <vector>

namespace trt {

constexpr uint32_t kShadowAll = 0x0FFFu;      // 3 lights x 4 spheres
constexpr float kShadowCellDefault = 0.25f;   // floor cell edge (TRT_SHADOW_MASK_CELL)
constexpr float kShadowCellMin = 0.1f, kShadowCellMax = 25.0f; // 200 x 250 cells at most
// The floor rectangle of scene_intersect (shader.comp:302-320): |x| < 10, -30 < z < -5, y = -4.
constexpr double kFloorX0 = -10.0, kFloorX1 = 10.0, kFloorZ0 = -30.0, kFloorZ1 = -5.0, kFloorY = -4.0;
// The error bound of the construction assumes every ray origin of the launch within this of the
// origin on each axis: the runtime checks the launch's cameras against it (all-ones masks
// otherwise), and a scene reaching further than this is bounded by its own extent.
constexpr float kShadowCamMax = 64.0f;

struct ShadowMaskIn {
    float sph[4][4];   // centre, radius of the UBO's spheres
    float light[3][3]; // the UBO's lights
    uint32_t flags;    // TRT_FLAG_SPHERES is read
};

struct ShadowMask {
    uint32_t nx = 1, nz = 1;    // floor cells along x and z; cell (ix, iz) at cells[iz * nx + ix]
    float inv_cell = 0.0f;      // ix = clamp(int((x + 10) * inv_cell)), iz = clamp(int((z + 30) * inv_cell))
    uint32_t rows[4] = {kShadowAll, kShadowAll, kShadowAll, kShadowAll}; // per hit sphere
    std::vector<uint16_t> cells{(uint16_t)kShadowAll};
    bool fallback = true;       // all ones: 1 x 1 cells, inv_cell 0
};

// The masks of a launch.  `on` false (TRT_SHADOW_MASK=0), spheres off, a non-finite or absurd
// input, a light inside a padded sphere or within the pad of the floor plane: all ones.
void shadow_mask(const ShadowMaskIn& in, float cell, bool on, ShadowMask& out);

} // namespace trt
