// sky_spans.cpp — see sky_spans.h and DESIGN §4 item 19.
//
// Construction.  Let o_c be the centre of a group's camera positions and rho the largest
// distance of a camera from it.  A ray from camera o that hits a point P at parameter t has a
// parallel ray from o_c that hits P + (o_c - o) at the same t, a point within rho of P.  So
// every direction that hits anything from any camera of the group hits, from o_c, a sphere of
// radius r + rho or the box [-10 - rho, 10 + rho] x [-4 - rho, -4 + rho] x [-30 - rho, -5 + rho]
// around the floor rectangle (scene_intersect, shader.comp:302-335).  Both are convex, so their
// images in the plane z = dz of the unnormalised pixel directions (dx, dy, dz) are convex, and
// the extent in dx over a strip of dy is reached on the outline: at the strip's two edges, or
// at the outline's own extreme where that lies inside the strip.  All in double; the result is
// padded by one whole tile on every side, ~1.2e-2 rad at 1024x768 against the ~1e-5 of the
// kernel's FP32 tests.
#include "sky_spans.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "../../include/trt/abi.h"
#include "trt_bands.h"

namespace trt {
namespace {

struct Range {
    double lo = 1e300, hi = -1e300;
    void add(double v) {
        lo = std::min(lo, v);
        hi = std::max(hi, v);
    }
};

// The image of a ball (centre q relative to o_c, radius R) that lies wholly in front of the
// camera: the directions v = (dx, dy, dz) with (q.v)^2 >= K |v|^2, K = |q|^2 - R^2 > 0, an
// ellipse in the plane z = dz.
struct Ball {
    double qx, qy, qz, R, K, dz;
    double ex[2], ey[2]; // the ellipse's extremes in dx and the dy where they are reached
    double ylo, yhi;     // its extent in dy
    double a, inv_a;     // f = a dx^2 + 2 b dx + c along a line of constant dy; a < 0
    void prepare() {
        // f as a quadratic in dy has a real root where (qx dx + qz dz)^2 + a2 (dx^2 + dz^2) >= 0,
        // a2 = R^2 - qx^2 - qz^2: the tangents in the xz plane
        const double A = R * R - qz * qz, B = qx * qz * dz, C = (R * R - qx * qx) * dz * dz;
        const double s = std::sqrt(std::max(0.0, B * B - A * C));
        const double a2 = R * R - qx * qx - qz * qz;
        ex[0] = (-B + s) / A; // A < 0: the smaller root
        ex[1] = (-B - s) / A;
        for (int i = 0; i < 2; ++i) ey[i] = -qy * (qx * ex[i] + qz * dz) / a2;
        // and the same in the yz plane, for the rows the ellipse does not reach
        const double By = qy * qz * dz, Cy = (R * R - qy * qy) * dz * dz;
        const double sy = std::sqrt(std::max(0.0, By * By - A * Cy));
        ylo = (-By + sy) / A;
        yhi = (-By - sy) / A;
        a = R * R - qy * qy - qz * qz;
        inv_a = 1.0 / a;
    }
    void extent(double dy_lo, double dy_hi, Range& r) const {
        if (!(yhi >= dy_lo && ylo <= dy_hi)) return;
        for (int i = 0; i < 2; ++i)
            if (ey[i] >= dy_lo && ey[i] <= dy_hi) r.add(ex[i]);
        for (const double dy : {dy_lo, dy_hi}) {
            const double u = qy * dy + qz * dz;
            const double b = qx * u, c = u * u - K * (dy * dy + dz * dz);
            const double disc = b * b - a * c;
            if (disc < 0.0) continue;
            const double s = std::sqrt(disc);
            r.add((-b + s) * inv_a);
            r.add((-b - s) * inv_a);
        }
    }
};

struct Seg2 {
    double x0, y0, x1, y1;
    double inv_dy; // 1 / (y1 - y0), or 0 for a segment of constant dy
};

// What one group's cameras can hit: balls, the floor box's projected edges, or "anything".
struct Group {
    bool full = false;
    int nball = 0, nseg = 0;
    Ball ball[4];
    Seg2 seg[12];
};

constexpr double kHuge = 1e6;

// std::floor / std::ceil of a double, value for value (but for the sign of a zero result), without
// the library call: a row takes eight of them, once the sphere interval is rounded beside the span.
inline double floor_d(double x) {
    if (!(std::fabs(x) < 4e15)) return std::floor(x); // already an integer, or not finite
    const double t = (double)(int64_t)x;
    return t > x ? t - 1.0 : t;
}
inline double ceil_d(double x) {
    if (!(std::fabs(x) < 4e15)) return std::ceil(x);
    const double t = (double)(int64_t)x;
    return t < x ? t + 1.0 : t;
}

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

void prepare_group(const SpanIn& in, const float* cams, uint32_t n, Group& G) {
    const double dz = (double)in.dz;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t f = 0; f < n; ++f) {
        if (!finite3(cams + 3 * f)) {
            G.full = true;
            return;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], (double)cams[3 * f + a]);
            hi[a] = std::max(hi[a], (double)cams[3 * f + a]);
        }
    }
    const double oc[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    double rho = 0.0;
    for (uint32_t f = 0; f < n; ++f) {
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) d2 += ((double)cams[3 * f + a] - oc[a]) * ((double)cams[3 * f + a] - oc[a]);
        rho = std::max(rho, std::sqrt(d2));
    }
    // magnitudes far beyond any scene would overflow the products below: nothing is culled
    if (!(rho < kHuge) || !(std::fabs(oc[0]) < kHuge) || !(std::fabs(oc[1]) < kHuge) || !(std::fabs(oc[2]) < kHuge)) {
        G.full = true;
        return;
    }
    rho = rho * (1.0 + 1e-6) + 1e-6;
    if (in.flags & TRT_FLAG_SPHERES) {
        for (int i = 0; i < 4; ++i) {
            const float* s = in.sph[i];
            if (!finite3(s) || !(std::fabs((double)s[3]) < kHuge)) {
                G.full = true;
                return;
            }
            Ball b;
            b.qx = (double)s[0] - oc[0];
            b.qy = (double)s[1] - oc[1];
            b.qz = (double)s[2] - oc[2];
            b.R = (std::fabs((double)s[3]) + rho) * (1.0 + 1e-4) + 1e-6;
            b.dz = dz;
            const double q2 = b.qx * b.qx + b.qy * b.qy + b.qz * b.qz;
            b.K = q2 - b.R * b.R;
            if (!(b.K > 0.0)) { // a camera within the padded radius
                G.full = true;
                return;
            }
            if (b.qz - b.R > 0.0) continue; // wholly behind the camera plane: no ray reaches it
            if (!(b.qz + b.R < -1e-9 * (1.0 + b.R))) { // straddles it: its image is unbounded
                G.full = true;
                return;
            }
            b.prepare();
            if (!std::isfinite(b.ex[0]) || !std::isfinite(b.ex[1]) || !std::isfinite(b.ey[0]) || !std::isfinite(b.ey[1]) ||
                !std::isfinite(b.ylo) || !std::isfinite(b.yhi) || !std::isfinite(b.inv_a)) {
                G.full = true;
                return;
            }
            G.ball[G.nball++] = b;
        }
    }
    if (in.flags & TRT_FLAG_FLOOR) {
        const double h = oc[1] - (-4.0 + rho); // height above the padded slab
        if (!(h > 1e-3)) {
            G.full = true;
            return;
        }
        const double bl[3] = {-10.0 - rho - oc[0], -4.0 - rho - oc[1], -30.0 - rho - oc[2]};
        const double bh[3] = {10.0 + rho - oc[0], -4.0 + rho - oc[1], -5.0 + rho - oc[2]};
        // Points of the box with -delta < z < 0 lie at y <= -h, so they project to
        // dy = y dz / z <= -h |dz| / delta = -2 H: below every pixel row.  Points at z >= 0 are
        // behind every ray.  So the box clipped to z <= -delta has the same image on the screen.
        const double delta = h * std::fabs(dz) / (2.0 * (double)in.height + 32.0);
        for (int e = 0; e < 12; ++e) {
            const int axis = e / 4, u = (axis + 1) % 3, v = (axis + 2) % 3;
            double p[3], q[3];
            p[u] = q[u] = (e & 1) ? bh[u] : bl[u];
            p[v] = q[v] = (e & 2) ? bh[v] : bl[v];
            p[axis] = bl[axis];
            q[axis] = bh[axis];
            if (p[2] > -delta && q[2] > -delta) continue;
            if (p[2] > -delta || q[2] > -delta) { // clip the end behind the plane z = -delta
                double* far = p[2] > -delta ? p : q;
                const double* near = p[2] > -delta ? q : p;
                const double t = (-delta - near[2]) / (far[2] - near[2]);
                for (int a = 0; a < 3; ++a) far[a] = near[a] + t * (far[a] - near[a]);
                far[2] = -delta;
            }
            Seg2 sg{p[0] * dz / p[2], p[1] * dz / p[2], q[0] * dz / q[2], q[1] * dz / q[2], 0.0};
            if (sg.y1 != sg.y0) sg.inv_dy = 1.0 / (sg.y1 - sg.y0);
            G.seg[G.nseg++] = sg;
        }
    }
}

void seg_extent(const Seg2& s, double dy_lo, double dy_hi, Range& r) {
    if (std::max(s.y0, s.y1) < dy_lo || std::min(s.y0, s.y1) > dy_hi) return;
    double t0 = 0.0, t1 = 1.0;
    if (s.inv_dy != 0.0) {
        double ta = (dy_lo - s.y0) * s.inv_dy, tb = (dy_hi - s.y0) * s.inv_dy;
        if (ta > tb) std::swap(ta, tb);
        t0 = std::max(t0, ta);
        t1 = std::min(t1, tb);
        if (t0 > t1) return;
    }
    r.add(s.x0 + t0 * (s.x1 - s.x0));
    r.add(s.x0 + t1 * (s.x1 - s.x0));
}

} // namespace

uint32_t sky_spans(const SpanIn& in, const float* cams, uint32_t nframes, uint32_t group_frames, uint32_t* out,
                   uint32_t* ntr_out, uint32_t* shift_out, uint32_t* sph_out) {
    *ntr_out = 0;
    *shift_out = 0;
    const bool banded = in.band_rows != 0 && in.band_count > 1;
    if (in.rays_in || nframes == 0 || in.width == 0 || in.height == 0) return 0;
    if (banded && (in.band_rows % 8u != 0 || in.band_index >= in.band_count)) return 0;
    const uint32_t rows = banded ? band_group_rows(in.height, in.band_rows, in.band_count, in.band_index) : in.height;
    const uint32_t ntr = (rows + 7u) / 8u, ntx = (in.width + 7u) / 8u;
    if (ntr == 0 || ntr > kSpanWords) return 0;
    uint32_t shift = 1;
    while ((1u << shift) < group_frames && shift < 16) ++shift;
    if (group_frames == 0) shift = 16;
    auto tables = [&](uint32_t s) { return (nframes + (1u << s) - 1u) >> s; };
    while (tables(shift) > kSpanMaxTables || tables(shift) * ntr > kSpanWords) ++shift;
    const uint32_t T = tables(shift);
    *ntr_out = ntr;
    *shift_out = shift;

    const bool sane = in.dz < 0.0f && in.dz > -1e9f; // not NaN
    const double W = (double)in.width, H = (double)in.height;
    for (uint32_t g = 0; g < T; ++g) {
        uint32_t* tab = out + (size_t)g * ntr;
        uint32_t* stab = sph_out ? sph_out + (size_t)g * ntr : nullptr;
        const uint32_t f0 = g << shift, n = std::min(nframes - f0, 1u << shift);
        Group G;
        if (sane) prepare_group(in, cams + 3 * (size_t)f0, n, G);
        else G.full = true;
        for (uint32_t tr = 0; tr < ntr; ++tr) {
            if (G.full) {
                tab[tr] = kSpanFull;
                if (stab) stab[tr] = kSpanFull;
                continue;
            }
            const uint32_t k0 = tr * 8u, k1 = std::min(k0 + 7u, rows - 1u);
            // band_rows is a multiple of 8, so a tile row's compact rows are consecutive frame rows
            const uint32_t y0 = banded ? band_frame_row(k0, in.band_rows, in.band_count, in.band_index) : k0;
            const uint32_t y1 = y0 + (k1 - k0);
            // the rows' dy = H / 2 - (row + 0.5) from pixel edge to pixel edge, the row below for
            // the last column under ROW_QUIRK, and one tile of padding
            const double dy_hi = H * 0.5 - (double)y0 + 8.0;
            const double dy_lo = H * 0.5 - (double)(y1 + 1u) - ((in.flags & TRT_FLAG_ROW_QUIRK) ? 1.0 : 0.0) - 8.0;
            // the balls alone first (the sphere interval), then the floor box's edges on top
            Range rb;
            for (int i = 0; i < G.nball; ++i) G.ball[i].extent(dy_lo, dy_hi, rb);
            Range r = rb;
            for (int i = 0; i < G.nseg; ++i) seg_extent(G.seg[i], dy_lo, dy_hi, r);
            // dx = x + 0.5 - W / 2; the pixel columns the extent touches, then one tile of padding
            auto word = [&](const Range& e) -> uint32_t {
                if (!(e.lo <= e.hi)) return (e.lo == 1e300 && e.hi == -1e300) ? 0u : kSpanFull; // empty, or NaN: full
                const double x0 = floor_d(e.lo + W * 0.5 - 0.5), x1 = ceil_d(e.hi + W * 0.5 - 0.5);
                const double c0 = std::max(0.0, floor_d(x0 * 0.125) - 1.0);
                const double c1 = std::min((double)ntx, floor_d(x1 * 0.125) + 2.0);
                return c0 < c1 ? ((uint32_t)c0 | ((uint32_t)c1 << 16)) : 0u;
            };
            tab[tr] = word(r);
            if (stab) {
                // rb lies inside r, so the interval lies inside the span; a full interval beside a
                // span that is not full cannot arise, and would be cut to the span (still a proof).
                // A row the floor box adds nothing to has the span's own word.
                const uint32_t w = (rb.lo == r.lo && rb.hi == r.hi) ? tab[tr] : word(rb);
                stab[tr] = (w == kSpanFull && tab[tr] != kSpanFull) ? tab[tr] : w;
            }
        }
    }
    return T;
}

} // namespace trt

// Diagnostic entries (not in include/trt/abi.h, like trt_diag_set_buffer): the span tables, or the
// sphere intervals, of one launch, computed without a context or a GPU.  `spheres`: 4 x (centre,
// radius); `cams`: 3 floats per frame; `out`: room for out_cap words.  Return the number of tables
// (0: spans off), or -1 when they do not fit out_cap.
static int diag_spans(bool sphere, uint32_t width, uint32_t height, float fov, uint32_t flags, uint32_t band_rows,
                      uint32_t band_count, uint32_t band_index, int rays_in, const float* spheres, const float* cams,
                      uint32_t nframes, uint32_t group_frames, uint32_t* out, uint32_t out_cap, uint32_t* ntr,
                      uint32_t* shift) {
    if (!spheres || !cams || !out || !ntr || !shift) return -1;
    trt::SpanIn in{};
    in.width = width;
    in.height = height;
    in.dz = (float)(-1.0 * ((double)height / (2.0 * std::tan((double)fov / 2.0)))); // as fill_args
    in.flags = flags;
    in.band_rows = band_rows;
    in.band_count = band_count;
    in.band_index = band_index;
    in.rays_in = rays_in != 0;
    for (int i = 0; i < 4; ++i)
        for (int a = 0; a < 4; ++a) in.sph[i][a] = spheres[4 * i + a];
    uint32_t tmp[trt::kSpanWords], stmp[trt::kSpanWords];
    const uint32_t T = trt::sky_spans(in, cams, nframes, group_frames, tmp, ntr, shift, stmp);
    if ((size_t)T * *ntr > out_cap) return -1;
    const uint32_t* src = sphere ? stmp : tmp;
    std::copy(src, src + (size_t)T * *ntr, out);
    return (int)T;
}

extern "C" int trt_diag_sky_spans(uint32_t width, uint32_t height, float fov, uint32_t flags, uint32_t band_rows,
                                  uint32_t band_count, uint32_t band_index, int rays_in, const float* spheres,
                                  const float* cams, uint32_t nframes, uint32_t group_frames, uint32_t* out,
                                  uint32_t out_cap, uint32_t* ntr, uint32_t* shift) {
    return diag_spans(false, width, height, fov, flags, band_rows, band_count, band_index, rays_in, spheres, cams, nframes,
                      group_frames, out, out_cap, ntr, shift);
}

// The sphere intervals (sky_spans' sph_out) in the span words' format, s0 | s1 << 16.
extern "C" int trt_diag_sphere_spans(uint32_t width, uint32_t height, float fov, uint32_t flags, uint32_t band_rows,
                                     uint32_t band_count, uint32_t band_index, int rays_in, const float* spheres,
                                     const float* cams, uint32_t nframes, uint32_t group_frames, uint32_t* out,
                                     uint32_t out_cap, uint32_t* ntr, uint32_t* shift) {
    return diag_spans(true, width, height, fov, flags, band_rows, band_count, band_index, rays_in, spheres, cams, nframes,
                      group_frames, out, out_cap, ntr, shift);
}
