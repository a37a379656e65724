// sky_spans.h — per tile row of a launch, the tile columns outside which no primary ray of any
// of the launch's frames can hit the floor or a sphere (host only, no HIP).
//
// Which screen regions a primary ray can hit depends on the UBOs alone, and the host holds the
// UBO of every frame of a launch before it enqueues it.  sky_trace_kernel reads the row's
// interval with a scalar load and stores a tile outside it straight from the sky table, without
// generating or intersecting its primary rays.
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
uint32_t sky_spans(const SpanIn& in, const float* cams, uint32_t nframes, uint32_t group_frames, uint32_t* out,
                   uint32_t* ntr, uint32_t* shift);

} // namespace trt
