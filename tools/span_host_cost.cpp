// Host cost of the sky spans of one launch (csrc/sky_spans.cpp), timed with std::chrono: the
// bench's walk (speed 0.02 along +x and -z from the origin) at 1024x768 for 20- and 64-frame
// launches, one table per 16 frames and one table per launch; with and without the second
// interval per row (the sphere intervals of the floor class), and the class's share.
//   g++ -O2 -std=c++17 -o span_host_cost tools/span_host_cost.cpp vkcomputeshader_tinyraytracer_amd/csrc/sky_spans.cpp
#include <chrono>
#include <cstdio>
#include <initializer_list>

#include "../include/trt/abi.h"
#include "../vkcomputeshader_tinyraytracer_amd/csrc/sky_spans.h"

int main() {
    trt::SpanIn in{};
    in.width = 1024;
    in.height = 768;
    in.dz = -663.1f; // 768 / (2 tan(1.05 / 2))
    in.flags = TRT_FLAG_SPHERES | TRT_FLAG_FLOOR | TRT_FLAG_ENVMAP | TRT_FLAG_ROW_QUIRK;
    const float sph[4][4] = {{-3, 0, -16, 2}, {-1, -1.5f, -12, 2}, {1.5f, -0.5f, -18, 3}, {7, 5, -18, 4}};
    for (int i = 0; i < 4; ++i)
        for (int a = 0; a < 4; ++a) in.sph[i][a] = sph[i][a];
    float cams[3 * 64];
    for (int k = 0; k < 64; ++k) {
        cams[3 * k] = 0.02f * k;
        cams[3 * k + 1] = 0.0f;
        cams[3 * k + 2] = -0.02f * k;
    }
    uint32_t out[trt::kSpanWords], sph_out[trt::kSpanWords], ntr, shift, sink = 0;
    for (uint32_t n : {20u, 64u})
        for (uint32_t group : {16u, 0u})
          for (uint32_t* sph : {(uint32_t*)nullptr, sph_out}) {
            const int reps = 20000;
            const auto t0 = std::chrono::steady_clock::now();
            uint32_t T = 0;
            for (int r = 0; r < reps; ++r) {
                T = trt::sky_spans(in, cams, n, group, out, &ntr, &shift, sph);
                sink += out[r % (T * ntr)] + (sph ? sph[r % (T * ntr)] : 0u);
            }
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
            uint64_t in_span = 0, in_sph = 0;
            for (uint32_t g = 0; g < T; ++g) {
                const uint32_t frames = (g + 1u) << shift <= n ? 1u << shift : n - (g << shift);
                for (uint32_t r = 0; r < ntr; ++r) {
                    in_span += (uint64_t)frames * ((out[g * ntr + r] >> 16) - (out[g * ntr + r] & 0xffffu));
                    if (sph) in_sph += (uint64_t)frames * ((sph[g * ntr + r] >> 16) - (sph[g * ntr + r] & 0xffffu));
                }
            }
            const double all = (double)n * ntr * 128;
            std::printf("frames %2u  frames per table %2u  tables %u  %s  host %.2f us per launch (%.3f us per frame)  culled %.1f %%", n,
                        group ? group : n, T, sph ? "spans + sphere intervals" : "spans only              ", us, us / n,
                        100.0 - 100.0 * (double)in_span / all);
            if (sph) std::printf("  may hit a sphere %.1f %%  floor class %.1f %%", 100.0 * (double)in_sph / all, 100.0 * (double)(in_span - in_sph) / all);
            std::printf("\n");
        }
    return sink == 0xdeadbeef;
}
