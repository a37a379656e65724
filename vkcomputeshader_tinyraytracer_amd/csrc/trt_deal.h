// trt_deal.h — which tile (and frame) a workgroup of a trace launch renders: the dealing of blocks
// to 2x2-tile chunks and XCDs, as host and device functions over a small block of per-launch
// constants (Deal, KArgs::deal).  Everything here that depends only on the launch's shape is
// computed once on the host (fill_deal); the kernels divide by the launch's divisors with a
// multiply-high and two shifts instead of the 20-instruction integer division sequence.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRT_HD __host__ __device__ __forceinline__
#else
#define TRT_HD inline
#endif

namespace trt {

// Frame pairs (TRT_FRAME_GROUP=2) for mesh frames: compiled only on request (measured slower
// for meshes: C4 +2.5 %, C3 +10 %, profiles/r03_ab_frame_pair.log)
#ifndef TRT_MESH_PAIRS
#define TRT_MESH_PAIRS 0
#endif

// Whether a plain launch of more than one frame deals its blocks as frame pairs.  Triangle-free
// frames only unless TRT_MESH_PAIRS: mesh kernels do not compile the pair path.
TRT_HD bool deal_pairs(uint32_t xcd_inter, uint32_t frame_group, bool triangle_free) {
    return xcd_inter && frame_group > 1u && (triangle_free || TRT_MESH_PAIRS);
}
// Deal::F of a plain launch of nframes frames: what its kernel passes through inter_tile.
TRT_HD uint32_t deal_frames(uint32_t nframes, uint32_t xcd_inter, uint32_t frame_group, bool triangle_free) {
    if (nframes <= 1u || !xcd_inter) return 1u;
    return deal_pairs(xcd_inter, frame_group, triangle_free) ? (nframes + 1u) / 2u : nframes;
}

// The divisors of a launch that the kernels divide by (Deal::magic, Deal::shifts).
enum DealDiv : uint32_t { kDivNtx = 0, kDivCw, kDivF, kDivNl, kDealDivs };

// Per-launch dealing constants: one 64-byte, 16-byte-aligned block of the kernel arguments, so a
// wave fetches it in a few wide scalar loads.  With tyn = ntiles / ntx tile rows:
struct alignas(16) Deal {
    uint32_t ntx;      // 8x8 tiles per row
    uint32_t cw, ch;   // whole 2x2-tile chunks per row (ntx / 2) and per column (tyn / 2)
    uint32_t nfull;    // chunks dealt evenly to the XCDs: (cw * ch / 8) * 8
    uint32_t per;      // blocks of a frame in whole chunk groups: nfull * 4
    uint32_t F;        // frames (or frame pairs) that inter_tile interleaves; 1 for a single frame
    uint32_t Fper;     // F * per
    uint32_t nl;       // leftover tiles of a frame: ntiles - per
    uint32_t nc;       // ... of which in the last cw * ch % 8 chunks: (cw * ch - nfull) * 4
    uint32_t shifts;   // per divisor i, bits [6 i, 6 i + 6): sh1 | sh2 << 1 (deal_div)
    uint32_t magic[kDealDivs]; // per divisor: the multiplier (ntx, cw, F, nl)
    uint32_t pad[2];
};
static_assert(sizeof(Deal) == 64, "Deal is one 64-byte block");

TRT_HD uint32_t deal_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// n / d for the launch's divisor `which`: exact for every 32-bit n and every d >= 1 (Granlund and
// Montgomery's round-up multiplier m = floor(2^32 (2^l - d) / d) + 1 with l = ceil(log2 d):
// n / d = (t + ((n - t) >> sh1)) >> sh2, t = mulhi(n, m), sh1 = min(l, 1), sh2 = max(l, 1) - 1).
// A divisor of 0 (no leftover tiles) has magic 0 and is never divided by.
TRT_HD uint32_t deal_div(const Deal& D, uint32_t which, uint32_t n) {
    const uint32_t s = D.shifts >> (6u * which);
    const uint32_t t = deal_mulhi(n, D.magic[which]);
    return (t + ((n - t) >> (s & 1u))) >> ((s >> 1) & 31u);
}

inline void deal_magic(uint32_t d, uint32_t& magic, uint32_t& shift6) {
    magic = 0;
    shift6 = 0;
    if (d == 0u) return;
    uint32_t l = 0;
    while (l < 32u && (1ull << l) < d) ++l;
    magic = (uint32_t)((((1ull << l) - d) << 32) / d + 1ull);
    const uint32_t sh1 = l < 1u ? l : 1u, sh2 = (l > 1u ? l : 1u) - 1u;
    shift6 = sh1 | (sh2 << 1);
}

// The launch's constants.  F: the frames (or pairs) the launch interleaves (inter_tile), 1 for a
// single frame.
inline void fill_deal(Deal& D, uint32_t ntx, uint32_t ntiles, uint32_t F) {
    const uint32_t tyn = ntx ? ntiles / ntx : 0u;
    D.ntx = ntx;
    D.cw = ntx / 2u;
    D.ch = tyn / 2u;
    const uint32_t nchunk = D.cw * D.ch;
    D.nfull = (nchunk / 8u) * 8u;
    D.per = D.nfull * 4u;
    D.F = F ? F : 1u;
    D.Fper = D.F * D.per;
    D.nl = ntiles - D.per;
    D.nc = (nchunk - D.nfull) * 4u;
    D.pad[0] = D.pad[1] = 0;
    const uint32_t d[kDealDivs] = {D.ntx, D.cw, D.F, D.nl};
    D.shifts = 0;
    for (uint32_t i = 0; i < kDealDivs; ++i) {
        uint32_t s;
        deal_magic(d[i], D.magic[i], s);
        D.shifts |= s << (6u * i);
    }
}

// What of KArgs the dealing reads besides Deal (the XCD knobs, trt_ctx).
struct DealKnobs {
    uint32_t rot, skew, inter, mult;
};

// Blocks b and b+8 share an XCD (round-robin dispatch, MI355X_MICROARCH.md): give each XCD
// 2x2-tile chunks (16x16 px) so neighbouring pixels' envmap texels and batch records hit
// the same XCD L2.  Chunk c of XCD x is global chunk c*8+x; chunks are row-major over the
// image in 2x2 tile units.  Bijective on [0, ntiles) (tail tiles map to themselves).
//
// Frame f of a multi-frame launch can deal the chunk classes rotated (xcd_rot: class
// (x + f / 2^(xcd_rot - 1)) mod 8 to XCD x) and skewed per chunk row (xcd_skew: row cy's chunk
// columns shifted by xcd_skew * cy, diagonal classes).  Both are bijections of the chunks, so
// every tile is traced once; they only move work between XCDs.  Why: the hardware deals blocks
// to the XCDs round-robin, statically, so an XCD whose chunk class is costlier (the glass
// spheres' stripes) finishes its share of a launch later than the others.
// perm (xcd_inter 2): chunk k of the evenly dealt ones is chunk (k * xcd_mult) mod nfull, a
// bijection (xcd_mult is coprime to nfull) that makes each XCD's chunks a 2-D lattice spread over
// the whole image instead of every 8th chunk column.
TRT_HD uint32_t xcd_deal(const Deal& D, const DealKnobs& K, uint32_t b, uint32_t roff, bool perm = false) {
    auto chunk_tile = [&](uint32_t chunk, uint32_t sub) {
        const uint32_t cy = deal_div(D, kDivCw, chunk);
        uint32_t cx = chunk - cy * D.cw;
        if (K.skew) {
            cx += K.skew * cy;
            cx -= deal_div(D, kDivCw, cx) * D.cw;
        }
        return (cy * 2u + sub / 2u) * D.ntx + cx * 2u + (sub % 2u);
    };
    if (b < D.per) {
        const uint32_t j = b / 8u; // j-th block of XCD x
        uint32_t x = b % 8u;
        x = (x + roff) & 7u;
        uint32_t k = (j / 4u) * 8u + x;
        if (perm) k = (k * K.mult) % D.nfull; // fits 32 bits: the host keeps xcd_mult 1 for >= 65536 chunks
        return chunk_tile(k, j % 4u);
    }
    // leftovers: the last nchunk % 8 chunks, then the odd right column, then the odd bottom row
    uint32_t r = b - D.per;
    if (r < D.nc) return chunk_tile(D.nfull + r / 4u, r % 4u);
    r -= D.nc;
    const uint32_t na = (D.ntx & 1u) ? D.ch * 2u : 0u;
    if (r < na) return r * D.ntx + (D.ntx - 1u);
    r -= na;
    return (D.ch * 2u) * D.ntx + r; // tile rows odd: the last tile row
}

// Block b's tile with the chunk classes rotated for frame f of this launch (xcd_rot: by
// f / 2^(xcd_rot - 1)).  Successive single-frame launches keep one dealing: rotating them too
// (a per-launch offset) cost the shipped frame's 8 in-flight deferred frames +5 % (consecutive
// frames' tiles on one XCD share its L2) for README -2 %, profiles/r03_ab_launch_off.log.
TRT_HD uint32_t xcd_tile(const Deal& D, const DealKnobs& K, uint32_t b, uint32_t f = 0) {
    return xcd_deal(D, K, b, K.rot ? (f >> (K.rot - 1u)) : 0u);
}
// the unrotated dealing
TRT_HD uint32_t xcd_tile_base(const Deal& D, const DealKnobs& K, uint32_t b) { return xcd_deal(D, K, b, 0u); }

// Frame-interleaved dealing of a multi-frame launch (xcd_inter): the launch walks the chunk
// groups once, and each XCD traces chunk group g of every frame before group g + 1 (frame f's
// chunk of group g rotated by f, so every XCD sees every chunk class).  All frames advance
// together, so the launch ends on the last chunk groups of all frames instead of on the last
// frame's whole tile order (whose costliest tiles then start near the end).  Sets f; tiles
// outside whole chunk groups (leftovers) are dealt frame by frame after them.
// D.F: the launch's frames (or frame pairs, frame_group).
// xcd_inter 2: no rotation — chunk group g's chunk on XCD x is the same in every frame of the
// launch, so that XCD traces that chunk in all frames back to back and the texels its primary
// rays miss into (the same directions in every frame while the camera only translates) stay in its L2;
// the permuted classes (xcd_deal perm) keep the XCDs balanced without the rotation.
TRT_HD uint32_t inter_tile(const Deal& D, const DealKnobs& K, uint32_t vb, uint32_t& f) {
    if (vb < D.Fper) {
        const uint32_t x = vb % 8u, i = vb / 8u, q = i / 4u;
        const uint32_t g = deal_div(D, kDivF, q); // chunk group: chunks g * 8 .. g * 8 + 7
        f = q - g * D.F;
        // block (g * 8 + ((x + f) & 7)) * 4 + i % 4 of frame f, in xcd_tile's unrotated dealing
        const bool fixed = K.inter == 2u;
        const uint32_t c = fixed ? x : (x + f) & 7u;
        return xcd_deal(D, K, (g * 4u + i % 4u) * 8u + c, 0u, fixed);
    }
    const uint32_t r = vb - D.Fper;
    f = deal_div(D, kDivNl, r);
    return xcd_tile_base(D, K, D.per + (r - f * D.nl));
}

} // namespace trt
