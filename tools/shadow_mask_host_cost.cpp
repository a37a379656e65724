// Host cost of the shadow occluder masks of one scene (csrc/shadow_mask.cpp), timed with
// std::chrono: the reference spheres and lights at floor cells of 0.5, 0.25 and 0.125.  The
// runtime pays it when the key (spheres, lights, spheres flag) changes, never per launch.
//   g++ -O2 -std=c++17 -o shadow_mask_host_cost tools/shadow_mask_host_cost.cpp vkcomputeshader_tinyraytracer_amd/csrc/shadow_mask.cpp
#include <chrono>
#include <cstdio>
#include <initializer_list>

#include "../include/trt/abi.h"
#include "../vkcomputeshader_tinyraytracer_amd/csrc/shadow_mask.h"

int main() {
    trt::ShadowMaskIn in{};
    const float sph[4][4] = {{-3, 0, -16, 2}, {-1, -1.5f, -12, 2}, {1.5f, -0.5f, -18, 3}, {7, 5, -18, 4}};
    const float lts[3][3] = {{-20, 20, 20}, {30, 50, -25}, {30, 20, 30}};
    for (int i = 0; i < 4; ++i)
        for (int a = 0; a < 4; ++a) in.sph[i][a] = sph[i][a];
    for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) in.light[i][a] = lts[i][a];
    in.flags = TRT_FLAG_SPHERES | TRT_FLAG_FLOOR;
    uint32_t sink = 0;
    for (float cell : {0.5f, 0.25f, 0.125f}) {
        const int reps = 200;
        trt::ShadowMask m;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r) {
            trt::shadow_mask(in, cell, true, m);
            sink += m.cells[r % m.cells.size()];
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
        uint64_t set = 0;
        for (uint16_t c : m.cells) set += (uint64_t)__builtin_popcount(c);
        int rows = 0;
        for (uint32_t r : m.rows) rows += __builtin_popcount(r);
        std::printf("cell %.3f  %3u x %3u cells  %6zu B  host %7.1f us per build  bits set %.2f %%  row bits %d of 48\n", cell, m.nx,
                    m.nz, m.cells.size() * 2, us, 100.0 * (double)set / (12.0 * m.cells.size()), rows);
    }
    return sink == 0xdeadbeef;
}
