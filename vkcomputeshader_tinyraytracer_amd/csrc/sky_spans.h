// sky_spans.h — per tile row of a launch, the tile columns outside which no primary ray of any
// of the launch's frames can hit the floor or a sphere (host only, no HIP).
//
// Which screen regions a primary ray can hit depends on the UBOs alone, and the host holds the
// UBO of every frame of a launch before it enqueues it.  sky_trace_kernel reads the row's
// interval with a scalar load and stores a tile outside it straight from the sky table, without
// generating or intersecting its primary rays.  A second interval per row,
// of the spheres alone, marks the tiles inside the span that can only hit the floor (item 21).
#pragma once

#include <stdint.h>

namespace trt {

// Span words of a launch (KArgs::span): one uint32 per tile row and table, c0 | c1 << 16 for
// the half-open interval [c0, c1) of tile columns that may hit; every tile of the row outside
// it is all sky in every frame of the table's group.
constexpr uint32_t kSpanWords = 384;
constexpr uint32_t kSpanMaxTables = 4;
constexpr uint32_t kSpanFull = 0xffff0000u; // [0, 65535): every column may hit

struct SpanIn {
    uint32_t width, height;
    float dz;                  // KArgs::dz (negative)
    uint32_t flags;            // TRT_FLAG_FLOOR | TRT_FLAG_SPHERES | TRT_FLAG_ROW_QUIRK are read
    uint32_t band_rows, band_count, band_index;
    bool rays_in;              // replayed rays: the directions are not the camera's
    float sph[4][4];           // centre, radius of the UBO's spheres
};

// Fills `out` with T tables of `ntr` words (table g at out + g * ntr) and returns T; table g
// serves frames [g << shift, (g + 1) << shift) of the launch.  `cams`: 3 floats per frame.
// `group_frames`: frames per table wanted (rounded up to a power of two >= 2, and further until
// the tables fit kSpanWords and kSpanMaxTables).  Returns 0 — spans off, the kernel's path of a
// launch without them — for replayed rays, band_rows that are no multiple of 8 and more tile
// rows than fit.  A group whose cameras are not finite, inside a padded sphere or not above the
// padded floor slab gets full rows.
//
// `sph_out` (optional, laid out like `out`): the sphere interval of each row, s0 | s1 << 16 — the
// same construction over the inflated balls alone, without the floor box.  Outside [s0, s1) no
// primary ray of any frame of the table's group passes sphere_hit for any sphere, so a tile inside
// the span and outside the interval can only hit the floor (the floor class).
// [s0, s1) lies inside [c0, c1); it is kSpanFull wherever the span is, and empty (0) with
// TRT_FLAG_SPHERES clear.
uint32_t sky_spans(const SpanIn& in, const float* cams, uint32_t nframes, uint32_t group_frames, uint32_t* out,
                   uint32_t* ntr, uint32_t* shift, uint32_t* sph_out = nullptr);

// The floor-class kernel's span word (KArgs::span of a launch with KArgs::floor_class set; tile
// rows of at most 255 tiles): c0 | c1 << 8 | s0 << 16 | s1 << 24.
constexpr uint32_t kFloorPackMaxNtx = 255;
constexpr uint32_t kFloorPackFull = 0xff00ff00u; // [0, 255) twice: every column may hit a sphere
inline uint32_t floor_pack(uint32_t span, uint32_t sph) {
    auto b = [](uint32_t v) { return v < 255u ? v : 255u; };
    return b(span & 0xffffu) | b(span >> 16) << 8 | b(sph & 0xffffu) << 16 | b(sph >> 16) << 24;
}

} // namespace trt
