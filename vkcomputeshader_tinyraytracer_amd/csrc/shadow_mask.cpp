// shadow_mask.cpp — the shadow occluder masks of a launch (shadow_mask.h), in double precision.
//
// The proof behind a clear bit.  A shadow query of cast_seg starts at so = p +- n * TRT_EPS for a
// hit point p, runs along ld = normalize(L - p) and accepts a hit of sphere j only at
// TRT_EPS < t < |L - p| (shadow_intersect, sphere_hit).  Every point of that stretch is
// (so - p) + (1 - u) p + u L with 0 <= u <= 1, so it lies within |so - p| + |p - q| of the point
// (1 - u) q + u L of the segment q -> L for any q: the stretch stays within TRT_EPS + |p - q| of
// the segment q -> L.  sphere_hit passes its first branch when its FP32 d2 <= r2; with
// d2 = |Lc|^2 - tca^2 formed from Lc = centre - so, the rounding of the three products, their sum,
// tca, its square, the difference and of the normalised direction is below kD2Err * |Lc|^2, so
// the true distance of the centre from the query's line is then at most sqrt(r^2 + E), E =
// kD2Err * |Lc|^2.  The same bound holds for a hit point: |p - centre|^2 = d2_true + thc^2 =
// r^2 + (d2_true - d2) differs from r^2 by at most E of the ray that found it.  So with
//   test_j = sqrt(r_j^2 + E_test_j) - r_j   (query origins lie on the floor or a sphere)
//   hit_k  = sqrt(r_k^2 + E_hit_k) - r_k    (the ray that found p starts at a camera or a surface)
// sphere j cannot be hit from light i's query
//   * of a floor hit in a cell of centre q and half-diagonal h unless
//       dist(centre_j, segment q -> L_i) <= r_j (1 + 1e-4) + test_j + h + kPad,
//   * of a hit on sphere k (from outside or inside) unless
//       dist(centre_j, segment centre_k -> L_i) <= r_j (1 + 1e-4) + test_j + r_k + hit_k + kPad.
// kPad = 1e-2 covers TRT_EPS (1e-3), the FP32 rounding of p, so and L - p at these coordinates
// (below 1e-4: every coordinate is bounded by kShadowCamMax or kSceneMax), the floor hit's
// distance from the plane y = -4 (the rounding of o.y + d.y * t, below 1e-4), and a point that
// the kernel's FP32 index arithmetic assigns to the neighbouring cell (below 1e-4 of the border).
#include "shadow_mask.h"

#include <algorithm>
#include <cmath>

#include "../../include/trt/abi.h"

namespace trt {

namespace {

constexpr double kPad = 1e-2;
constexpr double kRelR = 1e-4;
constexpr double kD2Err = 32.0 / 16777216.0; // 32 * 2^-24: twice the 17 roundings counted above
constexpr double kSceneMax = 1e3;            // |centre| + r beyond this: all ones
constexpr double kLightMax = 1e6;

struct V3 {
    double x, y, z;
};
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Distance of c from the segment a -> b.
inline double seg_dist(V3 c, V3 a, V3 b) {
    const V3 d = b - a, w = c - a;
    const double dd = dot(d, d);
    double u = dd > 0.0 ? dot(w, d) / dd : 0.0;
    u = std::min(1.0, std::max(0.0, u));
    const V3 e{w.x - u * d.x, w.y - u * d.y, w.z - u * d.z};
    return std::sqrt(dot(e, e));
}

void all_ones(ShadowMask& out) {
    out.nx = out.nz = 1;
    out.inv_cell = 0.0f;
    for (uint32_t& r : out.rows) r = kShadowAll;
    out.cells.assign(1, (uint16_t)kShadowAll);
    out.fallback = true;
}

} // namespace

void shadow_mask(const ShadowMaskIn& in, float cell_in, bool on, ShadowMask& out) {
    all_ones(out);
    if (!on || !(in.flags & TRT_FLAG_SPHERES)) return;
    if (!std::isfinite(cell_in)) return;
    const float cellf = std::min(kShadowCellMax, std::max(kShadowCellMin, cell_in));
    V3 c[4], L[3];
    double r[4], cmax[4];
    double S = 30.0; // the floor rectangle's furthest coordinate
    for (int j = 0; j < 4; ++j) {
        for (int a = 0; a < 4; ++a)
            if (!std::isfinite(in.sph[j][a])) return;
        c[j] = {in.sph[j][0], in.sph[j][1], in.sph[j][2]};
        r[j] = std::fabs((double)in.sph[j][3]); // sphere_hit squares the radius
        cmax[j] = std::max(std::fabs(c[j].x), std::max(std::fabs(c[j].y), std::fabs(c[j].z)));
        if (cmax[j] + r[j] > kSceneMax) return;
        S = std::max(S, cmax[j] + r[j]);
    }
    for (int i = 0; i < 3; ++i) {
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(in.light[i][a]) || std::fabs((double)in.light[i][a]) > kLightMax) return;
        L[i] = {in.light[i][0], in.light[i][1], in.light[i][2]};
        if (std::fabs(L[i].y - kFloorY) <= kPad) return;
    }
    // ray origins: shadow queries start on a surface (within 1 of the scene's extent, checked
    // below), the rays that find hits at a camera (kShadowCamMax, checked per launch) or a surface
    const double o_test = S + 1.0, o_hit = std::max((double)kShadowCamMax, S + 1.0);
    double test[4], hit[4];
    for (int j = 0; j < 4; ++j) {
        const double e_test = kD2Err * 3.0 * (cmax[j] + o_test) * (cmax[j] + o_test);
        const double e_hit = kD2Err * 3.0 * (cmax[j] + o_hit) * (cmax[j] + o_hit);
        test[j] = std::sqrt(r[j] * r[j] + e_test) - r[j];
        hit[j] = std::sqrt(r[j] * r[j] + e_hit) - r[j];
        if (!(hit[j] + kPad < 1.0)) return;
        for (int i = 0; i < 3; ++i) {
            const V3 d = L[i] - c[j];
            if (std::sqrt(dot(d, d)) <= r[j] * (1.0 + kRelR) + hit[j] + kPad) return; // light inside
        }
    }
    // sphere rows
    for (int k = 0; k < 4; ++k) {
        uint32_t m = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                const bool may = j == k || seg_dist(c[j], c[k], L[i]) <=
                                               r[j] * (1.0 + kRelR) + test[j] + r[k] + hit[k] + kPad;
                m |= (may ? 1u : 0u) << (4 * i + j);
            }
        out.rows[k] = m;
    }
    // floor cells
    const double cell = (double)cellf;
    out.nx = (uint32_t)std::ceil((kFloorX1 - kFloorX0) / cell);
    out.nz = (uint32_t)std::ceil((kFloorZ1 - kFloorZ0) / cell);
    out.inv_cell = (float)(1.0 / cell);
    // the kernel's cell is int((x + 10) * inv_cell) with the FP32 inv_cell: measure the cells in
    // its unit, so that a cell's centre is where the kernel's index puts it
    const double ucell = 1.0 / (double)out.inv_cell;
    const double h = ucell * std::sqrt(2.0) * 0.5;
    out.cells.assign((size_t)out.nx * out.nz, 0);
    double thr2[4];
    for (int j = 0; j < 4; ++j) {
        const double t = r[j] * (1.0 + kRelR) + test[j] + h + kPad;
        thr2[j] = t * t;
    }
    // seg_dist(c_j, q, L_i) <= thr_j with the segment's terms shared by the four spheres and the
    // distances compared squared (|L_i - q| > 0: the light is off the floor plane)
    for (uint32_t iz = 0; iz < out.nz; ++iz)
        for (uint32_t ix = 0; ix < out.nx; ++ix) {
            const V3 q{kFloorX0 + (ix + 0.5) * ucell, kFloorY, kFloorZ0 + (iz + 0.5) * ucell};
            uint32_t m = 0;
            for (int i = 0; i < 3; ++i) {
                const V3 d = L[i] - q;
                const double inv_dd = 1.0 / dot(d, d);
                for (int j = 0; j < 4; ++j) {
                    const V3 w = c[j] - q;
                    const double u = std::min(1.0, std::max(0.0, dot(w, d) * inv_dd));
                    const V3 e{w.x - u * d.x, w.y - u * d.y, w.z - u * d.z};
                    m |= (dot(e, e) <= thr2[j] ? 1u : 0u) << (4 * i + j);
                }
            }
            out.cells[(size_t)iz * out.nx + ix] = (uint16_t)m;
        }
    out.fallback = false;
}

} // namespace trt

// Diagnostic entry (include/trt/abi.h): the masks of one launch, computed without a context or a
// GPU.  `spheres`: 4 x (centre, radius); `lights`: 3 x 3 floats; `cell`: the floor cell edge
// (<= 0: the default).  Writes nx * nz cell masks to out_cells (room for `cap`), the grid to
// nx / nz and the four sphere rows to out_rows.  Returns 1 when the masks are the all-ones
// fallback (nx = nz = 1), 0 otherwise, -1 on a null argument or when the cells do not fit `cap`.
extern "C" int trt_diag_shadow_mask(const float* spheres, const float* lights, uint32_t flags, float cell,
                                    uint16_t* out_cells, uint32_t cap, uint32_t* nx, uint32_t* nz,
                                    uint32_t* out_rows) {
    if (!spheres || !lights || !out_cells || !nx || !nz || !out_rows) return -1;
    trt::ShadowMaskIn in{};
    for (int j = 0; j < 4; ++j)
        for (int a = 0; a < 4; ++a) in.sph[j][a] = spheres[4 * j + a];
    for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) in.light[i][a] = lights[3 * i + a];
    in.flags = flags;
    trt::ShadowMask m;
    trt::shadow_mask(in, cell > 0.0f ? cell : trt::kShadowCellDefault, true, m);
    if (m.cells.size() > cap) return -1;
    std::copy(m.cells.begin(), m.cells.end(), out_cells);
    *nx = m.nx;
    *nz = m.nz;
    for (int k = 0; k < 4; ++k) out_rows[k] = m.rows[k];
    return m.fallback ? 1 : 0;
}
