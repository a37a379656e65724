/*
 * trt/abi.h — the C-ABI drop-in for the reference's compute-shader hot path.
 *
 * The reference's "operator boundary" is a Vulkan descriptor set with seven bindings
 * (main.cpp:1218-1274) plus one vkCmdDispatch per frame (main.cpp:2108-2131).  Each
 * entry point below replaces one piece of that boundary:
 *
 *   trt_create / trt_destroy   <- device + pipeline setup (main.cpp:547-725, 1394-1427)
 *                                 and teardown (main.cpp:440-526)
 *   trt_upload_scene           <- createShaderStorageBuffers() (main.cpp:1494-1647:
 *                                 binding 5 triangles, binding 6 models), createUniformBuffers()
 *                                 (main.cpp:1650-1664, binding 0) and the background texture
 *                                 upload + sampler (main.cpp:928-1111, binding 4)
 *   trt_update_ubo             <- updateUniformBuffer() (main.cpp:2165-2179)
 *   trt_render                 <- recordComputeCommandBuffer() + vkQueueSubmit
 *                                 (main.cpp:2108-2131, 2181-2205); binding 1 (rayIn) is
 *                                 trt_params.rays_in, binding 2 (rayOut.resultColor) is
 *                                 out_rgba32f, binding 3 (storage image) is out_rgba8.
 *
 * Conventions: every function returns 0 (TRT_OK) or a negative TRT_ERR_* code and never
 * throws; trt_last_error() returns the message of the last failure on that context.  The
 * caller owns every host array (copied during the call).  The context owns its device
 * buffers until trt_destroy().  Calls on one context are serialised by the caller; use one
 * context per GPU.
 */
#ifndef TRT_ABI_H
#define TRT_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "scene_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRT_ABI_VERSION 5

/* status codes */
#define TRT_OK 0
#define TRT_ERR_INVALID (-1) /* bad argument (null pointer, size, depth, band) */
#define TRT_ERR_HIP (-2)     /* HIP runtime failure (no device, launch, copy) */
#define TRT_ERR_NOSCENE (-3) /* trt_render before trt_upload_scene */
#define TRT_ERR_OOM (-4)     /* host or device allocation failed */
#define TRT_ERR_IO (-5)      /* file could not be read or parsed */

/* trt_params.flags */
#define TRT_FLAG_SPHERES (1u << 0)     /* draw_sphere, shader.comp:83 (false in the shipped shader) */
#define TRT_FLAG_FLOOR (1u << 1)       /* draw_floor, shader.comp:84 */
#define TRT_FLAG_CHECKER (1u << 2)     /* checker floor colour, shader.comp:312 (commented out upstream) */
#define TRT_FLAG_ENVMAP (1u << 3)      /* miss -> envmap, shader.comp:455-456; else BACKGROUND_COLOR :77 */
#define TRT_FLAG_ROW_QUIRK (1u << 4)   /* the pix++ off-by-one of main.cpp:1501-1502 */
#define TRT_FLAG_DEVICE_PTRS (1u << 5) /* out_rgba8 / out_rgba32f / rays_in are device pointers */
#define TRT_FLAG_COUNT (1u << 6)       /* fill trt_stats ray counters */
#define TRT_FLAG_TIMING (1u << 7)      /* fill trt_stats.kernel_ms (waits for the frame) */
#define TRT_FLAG_BATCH_WALK (1u << 8)  /* trace meshes by walking the batch list in the reference's
                                          order (shader.comp:338) instead of the per-ray BVH; same
                                          image, and batch/triangle work counters equal the
                                          reference's */
#define TRT_FLAG_SRGB_OUT (1u << 9)    /* out_rgba8 = the frame as displayed: sRGB-encoded
                                          (the B8G8R8A8_SRGB swapchain, main.cpp:2341, that
                                          shader.frag writes the sampled image to); out_rgba32f
                                          stays rayOut */
#define TRT_FLAG_BAND_IN_PLACE (1u << 10) /* with band params: each rendered row is written at its
                                          row of a full width*height image instead of compactly
                                          (several bands render into one frame); needs
                                          TRT_FLAG_DEVICE_PTRS */

/* The shipped shader: floor on, spheres off, envmap background, host ray quirk. */
#define TRT_FLAGS_REFERENCE (TRT_FLAG_FLOOR | TRT_FLAG_ENVMAP | TRT_FLAG_ROW_QUIRK)

#define TRT_MAX_DEPTH_LIMIT 20u /* MAX_DEPTH of shader.comp:75 */

typedef struct trt_params {
    uint32_t width, height; /* image size; WIDTH/HEIGHT of main.cpp:35-36 & shader.comp:79-80 */
    uint32_t max_depth;     /* MAX_DEPTH (shader.comp:75): segments of depth 0..max_depth-1; 1..20 */
    uint32_t spp;           /* samples per pixel; 1 = the reference's pixel-centre rays */
    uint32_t seed;          /* jitter seed (spp > 1 only) */
    uint32_t flags;         /* TRT_FLAG_* */
    float fov;              /* vertical field of view in radians (main.cpp:1498: 1.05f) */
    uint32_t band_rows;     /* row-band sharding: 0 = whole image; else rows r with */
    uint32_t band_count;    /*   (r / band_rows) % band_count == band_index are rendered and */
    uint32_t band_index;    /*   written compactly, in row order */
    const trt_ray* rays_in; /* optional binding-1 replay (width*height rays), or NULL */
} trt_params;

typedef struct trt_stats {
    uint64_t primary_rays;   /* root segments traced (W*H*spp over the rendered rows) */
    uint64_t secondary_rays; /* reflection/refraction/TIR segments that reach scene_intersect */
    uint64_t shadow_rays;    /* shadow_intersect calls */
    /* Per-stage work, the units of the algorithmic-byte roofline: */
    uint64_t misses;         /* segments with no hit (background lookups) */
    uint64_t tri_nearest;    /* segments whose closest hit is a triangle */
    uint64_t sphere_tests;   /* ray_sphere_intersect calls (scene + shadow) */
    uint64_t batch_tests;    /* ray_aabb_intersect calls (scene + shadow) */
    uint64_t batch_hits;     /* ... that passed */
    uint64_t tri_tests;      /* ray_triangle_intersect calls (scene + shadow) */
    uint64_t node_tests;     /* hierarchy-node box tests in front of the batch tests (0 in the
                                reference's linear loop; batch_tests then counts only the batch
                                boxes actually reached) */
    double kernel_ms;        /* device time of the frame (TRT_FLAG_TIMING) */
    /* Moller-Trumbore stages reached (shader.comp:223-270; the per-stage FP32 work of the VALU
     * roofline, SURVEY §8d: 22 / 34 / 52 / 59 flops at exit after a / u / v / t): */
    uint64_t tri_past_a;     /* triangle tests past the parallel test (u computed) */
    uint64_t tri_past_u;     /* ... past the u test (v computed) */
    uint64_t tri_past_v;     /* ... past the v test (t computed) */
    /* Shadow queries a frame does not trace: the light's diffuse and specular terms both vanish
     * from the colour (zero term or zero albedo weight), so lit or shadowed it adds exactly
     * nothing (shader.comp:495-505).  The counting pass traces them (every counter above is the
     * reference's work) and reports them and the work inside them here: */
    uint64_t shadow_skipped;
    uint64_t skipped_sphere_tests, skipped_box_tests, skipped_tri_tests;
    uint64_t skipped_tri_past_a, skipped_tri_past_u, skipped_tri_past_v;
} trt_stats;

typedef struct trt_ctx trt_ctx;

const char* trt_version(void);

/* Creates a context on HIP device `hip_device` (a fresh non-blocking stream). */
int trt_create(trt_ctx** out, int hip_device);
int trt_destroy(trt_ctx* ctx);
const char* trt_last_error(const trt_ctx* ctx);

/* Launch subsequent work on an external hipStream_t (e.g. a torch.cuda.Stream); NULL
 * restores the context's own stream (the legacy null stream cannot be selected). */
int trt_set_stream(trt_ctx* ctx, void* hip_stream);

/* Uploads the bindings of one scene.  ntri/nmodel may be 0 (the reference cannot bind a
 * zero-size SSBO; this boundary can), env may be NULL when TRT_FLAG_ENVMAP is never set.
 * Triangle materials are kept per triangle as in binding 5. */
int trt_upload_scene(trt_ctx* ctx, const trt_ubo* ubo, const trt_triangle* tris, uint32_t ntri,
                     const trt_model* models, uint32_t nmodel, const uint8_t* env_rgba8,
                     uint32_t env_w, uint32_t env_h);

/* Per-frame UBO update (spheres, lights, camera). */
int trt_update_ubo(trt_ctx* ctx, const trt_ubo* ubo);

/* Renders one frame.  out_rgba8: rows*width*4 bytes (RGBA8 = floor(255*c + 0.5), a = 255);
 * out_rgba32f: rows*width*4 floats (rayOut.resultColor = (c, 1)).  Either may be NULL.
 * rows = trt_output_rows(p).  Host pointers unless TRT_FLAG_DEVICE_PTRS; with device
 * pointers and no COUNT/TIMING flag the call only enqueues work on the stream. */
int trt_render(trt_ctx* ctx, const trt_params* p, uint8_t* out_rgba8, float* out_rgba32f,
               trt_stats* st);

/* Frames in flight of trt_render_frames (the reference's MAX_FRAMES_IN_FLIGHT = 2,
 * main.cpp:45: per-frame command buffers, UBOs and rayOut buffers, main.cpp:1518-1664, with
 * no barrier between consecutive compute submissions).  Frame i of a trt_render_frames call
 * runs on in-flight slot i % n: slot 0 is the context's stream, slots 1..n-1 are streams the
 * context owns, forked from and joined back into its stream inside the call, so frame i+1's
 * workgroups fill the GPU while frame i's slowest tiles finish.  n in [1, 32], or 0 = auto
 * (the default): 4, or for deferred-shadow frames, whose depth-20 trees leave the longest
 * tails, a shape by the hardware queues (below; measured: profiles/r02_ab_queues_*.log,
 * profiles/r04z_ab_deferred_in_flight.jsonl, profiles/r06t_ab_defer_shape_32q.jsonl).  With n
 * set, deferred frames go one per launch on the n slots.  Each slot is a HIP stream, so the process
 * needs as many hardware queues: the library leaves GPU_MAX_HW_QUEUES to the host (HIP's
 * default is 4; the Python package and bench.py raise it to 32 before HIP initialises, see
 * INTEGRATION.md) and only reads it: with auto in-flight, a deferred loop runs slots tracing
 * launch groups of several consecutive frames each, on at most half the queues: 8 slots x 3
 * frames with >= 16 queues, 2 x 8 with HIP's default 4. */
#define TRT_FRAMES_IN_FLIGHT_DEFAULT 0u
#define TRT_FRAMES_IN_FLIGHT_AUTO 0u
/* Fixed by the ABI (a host cannot change it): the upper bound of n.  The library's own slot
 * count is the private build-time TRT_BUILD_MAX_IN_FLIGHT (csrc/trt_ctx.h, default and maximum:
 * this value); its range checks use that count. */
#define TRT_MAX_FRAMES_IN_FLIGHT 32u
int trt_set_frames_in_flight(trt_ctx* ctx, uint32_t n);

/* Frames per launch of trt_render_frames.  The reference records one vkCmdDispatch per frame
 * (main.cpp:2122-2124).  Here consecutive frames of a plain frame loop (no subtree split, no
 * deferred shadows) whose UBOs differ only in camPos — the reference's interactive loop moves
 * only the camera, main.cpp:391-403 — are traced by ONE launch of ntiles x n workgroups: frame
 * k of the launch owns blocks [k * ntiles, (k + 1) * ntiles), so a frame's slowest tiles overlap
 * the next frame's tiles inside one grid and the GPU drains once per launch instead of once per
 * frame.  n in [1, TRT_MAX_FRAME_BATCH]: 1 = one launch per frame (the reference's dispatch per
 * frame); 0 = auto (the default): up to TRT_MAX_FRAME_BATCH frames per launch.  Split frames
 * launch one frame at a time; deferred-shadow frames in launch groups of their own (above),
 * each frame of a group with its own scratch. */
#define TRT_FRAME_BATCH_AUTO 0u
#define TRT_MAX_FRAME_BATCH 64u
int trt_set_frame_batch(trt_ctx* ctx, uint32_t n);

/* Subtree split (load balance of deep refraction trees).  The reference traces a pixel's whole
 * Whitted tree depth-first in one invocation (shader.comp:423-583); in mesh scenes at depth 20
 * a few pixels' trees hold hundreds of segments and one 8x8 tile then runs for milliseconds
 * while the rest of the GPU idles.  With a window of w depths the frame is traced in depth
 * windows: a segment at depth k*w is handed to a task queue and traced by any lane of the
 * next launch.  Rays, hits and counters are unchanged; the colour of a split pixel is the
 * sum of its subtrees' colours (each summed in the reference's pop order) added in 32.32
 * fixed point — deterministic, and within a few ulp of the reference's single running sum
 * (well inside the RGBA8 +-1 bar).  Pixels whose tree stays within the first window are
 * bit-identical to the unsplit frame.  spp > 1 frames are never split.
 * window: TRT_SPLIT_AUTO (default: w = 4 for mesh scenes with max_depth >= 8, else off),
 * TRT_SPLIT_OFF, or 2..5. */
#define TRT_SPLIT_AUTO 0
#define TRT_SPLIT_OFF 1
int trt_set_subtree_split(trt_ctx* ctx, int window);

/* Deferred shadow rays (the reference traces a hit's three shadow rays in place inside the
 * pixel's DFS, shader.comp:483-507).  A deferred frame runs in three passes: (A) every pixel's
 * Whitted tree without shadow rays, logging one colour event per segment in the reference's
 * pop order, with the shadow queries appended to one dense queue; (B) the queue traced with
 * every lane of every wave busy (in the per-pixel loop a wave runs the shadow rays of only the
 * lanes that sit at a hit); (C) each pixel's events summed in logged order with the shader's
 * own arithmetic.  The image is bit-identical to the per-pixel loop without subtree split (the
 * reference's single running sum), rays and counters are unchanged, and a pixel whose log does
 * not fit the scratch is re-traced in place.  With an explicit subtree-split window (above) a
 * deferred frame's subtrees are traced by other lanes into logs of their own, reached through
 * LINK events at the place of their events, so the sum keeps the reference order (no
 * fixed-point sums); TRT_SPLIT_AUTO does not split deferred frames.  COUNT and spp > 1 frames
 * always run the per-pixel loop (a COUNT frame of a scene that would defer runs unsplit, so its
 * image equals the deferred frame's).
 * mode: TRT_DEFER_AUTO (default: mesh scenes with max_depth >= 8, unless a subtree-split
 * window 2..5 was set explicitly), TRT_DEFER_OFF, TRT_DEFER_ON. */
#define TRT_DEFER_AUTO 0
#define TRT_DEFER_OFF 1
#define TRT_DEFER_ON 2
int trt_set_deferred_shadows(trt_ctx* ctx, int mode);

/* Counters of the last deferred frame rendered on `slot` (0 .. TRT_MAX_FRAMES_IN_FLIGHT-1;
 * trt_render uses one slot per stream): out[0] event chunks taken, out[1] shadow queries
 * appended, out[2] pixels re-traced in place, out[3] chunk capacity, out[4] query capacity (of
 * the slot's allocation).  Waits for the context's stream. */
int trt_defer_stats(trt_ctx* ctx, uint32_t slot, uint64_t out[5]);

/* The reference's frame loop (mainLoop -> drawFrame, main.cpp:405-438, 2181-2205) in one
 * call: for each of `nframes` frames, updateUniformBuffer with ubos[i] (or the current UBO
 * when ubos is NULL) and trace the frame into out_rgba8 + i * frame_stride bytes.  Plain
 * frames are traced several per launch (trt_set_frame_batch); launches rotate over the
 * frames-in-flight streams (trt_set_frames_in_flight), so frames may run concurrently: give
 * concurrent frames distinct images (frame_stride >= rows*width*4) unless they are identical —
 * frame_stride 0 makes every frame write the same image, like the reference's single storage
 * image (binding 3, main.cpp:865-926).  Requires TRT_FLAG_DEVICE_PTRS; only enqueues; all
 * frames have completed on the context's stream when work enqueued after the call runs.  With
 * TRT_FLAG_TIMING a HIP event pair brackets every `time_every`-th launch (0 or 1: every
 * launch) on its stream (the span includes any overlap with launches on the other streams);
 * trt_frame_times() reads them. */
int trt_render_frames(trt_ctx* ctx, const trt_params* p, const trt_ubo* ubos, uint32_t nframes,
                      uint8_t* out_rgba8, size_t frame_stride, uint32_t time_every);

/* ---- camera orientation: a view basis for the primary rays --------------------------------
 * The reference keeps cameraFront / cameraUp (main.cpp:342-344) but only moves camPos with them:
 * its ray table is built once for a camera looking down -z (main.cpp:1496-1506).  A view turns
 * the camera: `right`, `up`, `back` are the columns of the camera-to-world rotation (back =
 * -front); the reference camera is right (1,0,0), up (0,1,0), back (0,0,1).  A pixel's (and, at
 * spp > 1, a sample's) direction under a view is, in this order,
 *   1. c = normalize(dx, dy, dz), the host direction of main.cpp:1504 (row quirk and jitter as
 *      without a view);
 *   2. w[a] = (c.x * right[a] + c.y * up[a]) + c.z * back[a], a = 0, 1, 2 — every product and sum
 *      rounded to FP32 on its own, no FMA: what a host would store into binding 1;
 *   3. d = normalize(w), the shader's own normalize (shader.comp:593).
 * The basis need not be orthonormal, only finite (step 3 fixes the length).  trt_params.rays_in,
 * when set, wins over a view (the directions are the caller's).  A view whose 36 bytes equal the
 * reference camera's (+0.0 and 1.0) is no view: the frame runs exactly the code it runs without
 * one.  Any other view is generated in the kernel from the launch's arguments (one basis per
 * frame of a launch), and its launch runs without the sky table and what rides on it (sky
 * spans, shadow occluder masks, floor class): those are proofs about the fixed basis, so an
 * oriented triangle-free frame takes the general trace kernel (what TRT_SKY_TABLE=0 runs).
 * Oriented frames share launches, up to TRT_MAX_VIEW_FRAMES frames each with its own view. */
typedef struct trt_view { float right[3], up[3], back[3]; } trt_view; /* 36 B */
#define TRT_MAX_VIEW_FRAMES 32u

/* host only: right = normalize(cross(front, world_up)), up = cross(right, front),
 * back = -normalize(front); the reference's front (0,0,-1), up (0,1,0) give the identity bytes.
 * TRT_ERR_INVALID for a null, non-finite, zero or parallel input. */
int trt_view_look(trt_view* out, const float front[3], const float world_up[3]);

/* host only, no context: the width*height Ray records (dir = w of step 2, .w = 1, resultColor 0)
 * a host would bind as binding 1 for this view at spp 1; v NULL = the reference camera. */
int trt_view_rays(const trt_params* p, const trt_view* v, trt_ray* out);

/* the context's view for trt_render, trt_render_frames and the multi-GPU calls;
 * NULL restores the reference camera.  Copied.  TRT_ERR_INVALID if not finite (the view in
 * force stays). */
int trt_set_view(trt_ctx* ctx, const trt_view* v);

/* trt_render_frames with one view per frame; views NULL = the context's view for every frame.
 * Views do not split launches (only the TRT_MAX_VIEW_FRAMES clamp of a launch with an oriented
 * frame does); a call whose views are all the reference camera enqueues what trt_render_frames
 * enqueues.  TRT_ERR_INVALID if a view is not finite. */
int trt_render_frames_view(trt_ctx* ctx, const trt_params* p, const trt_ubo* ubos, const trt_view* views,
                           uint32_t nframes, uint8_t* out_rgba8, size_t frame_stride, uint32_t time_every);

/* ---- ray queries: caller rays with their own origins, with hit records --------------------
 * trt_render answers one question: what does the pinhole camera at camPos see.  A ray query
 * traces `nrays` rays the caller made — picking, a panorama or stereo camera, rays leaving a
 * surface — and can return, per ray, the colour and the nearest hit.
 *
 * What ray i is: the primary ray main() of the shader would trace from origin `org` in direction
 * d = normalize(dir), the shader's own normalize (shader.comp:593) — exactly what the kernel does
 * to a binding-1 direction.  The scene, UBO spheres and lights are the context's; camPos and the
 * context's view are not read.
 *
 * Read from p: max_depth (1..20) and flags, of which SPHERES, FLOOR, CHECKER, ENVMAP, BATCH_WALK,
 * SRGB_OUT, DEVICE_PTRS, COUNT and TIMING are honoured.  Every other field and flag is ignored.
 *
 * Outputs, any of which may be NULL (all three NULL: TRT_ERR_INVALID):
 *   out_rgba8[i]        the storage-image word of the ray (RGBA8 = floor(255 * c + 0.5), a = 255);
 *   out_rgba32f[4i..]   rayOut.resultColor = (gamma(c), 1);
 *   hits[i]             the result of scene_intersect for the ray (shader.comp:295-362): t, what
 *                       was hit and, for a triangle, the Moller-Trumbore weights u, v of v1, v2
 *                       (the point is (1 - u - v) v0 + u v1 + v v2) and the caller's index into
 *                       the binding-5 array; n is the shading normal before any facing flip:
 *                       (0, 1, 0) for the floor, normalize(p - centre) for a sphere, the flat or
 *                       interpolated normal for a triangle.  A miss is t = 1e10 (the shader's
 *                       initial nearest distance), kind TRT_HIT_NONE, the rest 0.
 * With both colour outputs NULL nothing is shaded: a pure nearest-hit query, max_depth unused
 * (still range-checked).  TRT_FLAG_COUNT without a colour output is TRT_ERR_INVALID.
 *
 * A valid ray: all six floats finite, and s = (dx * dx + dy * dy) + dz * dz, in FP32 in that
 * order, within [TRT_QRAY_MIN_LEN2, TRT_QRAY_MAX_LEN2], so the normalized direction is finite
 * and of unit length.  The host checker and the kernel share one predicate.  A host-pointer call
 * validates every ray before anything is launched: a bad ray returns TRT_ERR_INVALID with its
 * index in trt_last_error and the outputs untouched.  A device-pointer call cannot be checked on
 * the host, so the kernel treats a bad ray as inactive: it traces nothing and counts nothing,
 * and writes RGBA8 word 0 (alpha 0), float4 0 and kind TRT_HIT_BAD_RAY with zeros elsewhere;
 * the other rays of its wave are unaffected.
 *
 * Counting (TRT_FLAG_COUNT): the counters are those of cast_ray alone — the hit record's own
 * intersection is not counted — and primary_rays is the number of valid rays.
 *
 * Stream and buffers as trt_render: with device pointers and no COUNT / TIMING the call only
 * enqueues on the context's stream (trt_set_stream applies); host pointers are synchronous and
 * go through context-owned staging buffers that only grow.  Device arrays are read and written
 * as 16-byte vectors: with TRT_FLAG_DEVICE_PTRS `rays`, `hits` and `out_rgba32f` must be 16-byte
 * aligned and `out_rgba8` 4-byte aligned, else TRT_ERR_INVALID (host arrays need only the
 * alignment of their C types).  nrays == 0 is TRT_OK and launches
 * nothing; nrays > TRT_QRAY_MAX_RAYS is TRT_ERR_INVALID.  Meshes are traced by the path
 * trt_render takes for the scene (the BVH walk, or the batch walk with TRT_FLAG_BATCH_WALK).
 * The call changes nothing a later trt_render depends on. */
typedef struct trt_qray { float org[3]; float pad0; float dir[3]; float pad1; } trt_qray;  /* 32 B */
typedef struct trt_qhit { float t; uint32_t kind; uint32_t index; float u, v; float n[3]; } trt_qhit; /* 32 B */
#define TRT_HIT_NONE 0u      /* t = 1e10 (the shader's initial nearest), the rest 0 */
#define TRT_HIT_FLOOR 1u
#define TRT_HIT_SPHERE 2u    /* index 0..3 */
#define TRT_HIT_TRIANGLE 3u  /* index into the caller's binding-5 array, u/v the Moller-Trumbore weights of v1/v2 */
#define TRT_HIT_BAD_RAY 0xffffffffu
#define TRT_QRAY_MIN_LEN2 1e-30f
#define TRT_QRAY_MAX_LEN2 1e30f
#define TRT_QRAY_MAX_RAYS (1u << 28)
#ifdef __cplusplus
static_assert(sizeof(trt_qray) == 32 && sizeof(trt_qhit) == 32, "query records are 32 B");
#else
_Static_assert(sizeof(trt_qray) == 32 && sizeof(trt_qhit) == 32, "query records are 32 B");
#endif

int trt_trace_rays(trt_ctx* ctx, const trt_params* p, const trt_qray* rays, uint32_t nrays,
                   uint8_t* out_rgba8, float* out_rgba32f, trt_qhit* hits, trt_stats* st);
/* host only, no context: TRT_OK when every ray is valid, else TRT_ERR_INVALID with the lowest bad
 * index in *first_bad (may be NULL).  rays NULL with n > 0 is TRT_ERR_INVALID (*first_bad = 0). */
int trt_check_rays(const trt_qray* rays, uint32_t n, uint32_t* first_bad);
/* host only, no context: steps 1 and 2 of the view contract above for pixel (x, y) at spp 1, row
 * quirk honoured, v NULL = the reference camera: out->dir = w, out->org = cam, pads 0.  The
 * single-pixel twin of trt_view_rays, bit for bit.  TRT_ERR_INVALID for a null argument, a bad
 * image size or a pixel outside the image. */
int trt_pixel_ray(const trt_params* p, const trt_view* v, const float cam[3],
                  uint32_t x, uint32_t y, trt_qray* out);

/* ---- occlusion queries: any hit over caller segments, one byte each --------------------------
 * trt_trace_rays answers "what does this ray hit first"; an occlusion query answers the other
 * half: does ANYTHING lie between this point and that one — light visibility, ambient occlusion,
 * line of sight, form-factor sampling.  It is the shader's any-hit walk (shadow_intersect,
 * shader.comp:364-399) over the caller's segments, and it returns one byte per segment instead of
 * a 32-byte hit record.
 *
 * What segment i is: the ray from `org` in direction d = normalize(dir), the shader's own
 * normalize (shader.comp:593), exactly as trt_trace_rays treats a ray, cut off at distance tmax.
 *   out[i] = TRT_OCC_OCCLUDED  iff  scene_intersect(org, d) finds something at a distance t < tmax,
 * else TRT_OCC_VISIBLE: the strict `<` and the MIN_EPSILON lower bound (t > 1e-4) the shader uses
 * everywhere (shader.comp:305, 349, 372, 389).  t and tmax are in world units along d: the t that
 * trt_qhit.t reports.  So for any valid ray
 *   occluded(ray, tmax) == (hit.t < tmax),   hit = the ray's trt_trace_rays record,
 * and since a miss is t = 1e10, tmax = TRT_QSEG_MAX_T ("a whole ray") never reports a miss as
 * occluded.  A tmax at or below MIN_EPSILON is valid and always visible.
 *
 * Read from p: flags only.  TRT_FLAG_FLOOR: the floor occludes, by scene_intersect's floor test
 * (shader.comp:302-320).  Without TRT_FLAG_FLOOR the query is exactly the shader's
 * shadow_intersect, which leaves the floor out: a caller reproducing the shader's shadow rays
 * clears the flag.  SPHERES, BATCH_WALK, DEVICE_PTRS and TIMING are honoured as by trt_trace_rays.
 * TRT_FLAG_COUNT is TRT_ERR_INVALID (any-hit counters depend on the walk order).  Every other
 * field of p, max_depth included, and every other flag is ignored.  st may be NULL unless
 * TRT_FLAG_TIMING is set (then st->kernel_ms is filled and the rest zeroed).
 *
 * A valid segment: a valid ray (above: six finite floats, direction length in range) with
 * 0 < tmax <= TRT_QSEG_MAX_T; a NaN tmax is not valid.  The host checker and the kernel share one
 * predicate.  A host-pointer call validates every segment before anything is launched: a bad one
 * returns TRT_ERR_INVALID with the lowest bad index in trt_last_error and `out` untouched.  A
 * device-pointer call cannot be checked on the host, so the kernel writes TRT_OCC_BAD_SEG for a bad
 * record and traces nothing for it; the other segments of its wave are unaffected.
 *
 * Sizes, stream and buffers as trt_trace_rays: nsegs == 0 is TRT_OK and launches nothing; nsegs >
 * TRT_QRAY_MAX_RAYS, or a NULL segs or out with nsegs > 0, is TRT_ERR_INVALID; a call before
 * trt_upload_scene is TRT_ERR_NOSCENE.  With TRT_FLAG_DEVICE_PTRS `segs` must be 16-byte aligned
 * (else TRT_ERR_INVALID; `out` needs no alignment), and without TIMING the call only enqueues on
 * the context's stream (trt_set_stream applies).  Host pointers are synchronous and go through
 * context-owned staging buffers that only grow.  Meshes are traced by the path trt_render takes
 * for the scene.  The call changes nothing a later trt_render or trt_trace_rays depends on. */
typedef struct trt_qseg { float org[3]; float tmax; float dir[3]; float pad; } trt_qseg; /* 32 B */
#define TRT_OCC_VISIBLE 0u
#define TRT_OCC_OCCLUDED 1u
#define TRT_OCC_BAD_SEG 0xffu
#define TRT_QSEG_MAX_T 1e10f /* the shader's initial nearest distance: "a whole ray" */
#ifdef __cplusplus
static_assert(sizeof(trt_qseg) == 32, "segment records are 32 B");
#else
_Static_assert(sizeof(trt_qseg) == 32, "segment records are 32 B");
#endif

int trt_occluded(trt_ctx* ctx, const trt_params* p, const trt_qseg* segs, uint32_t nsegs,
                 uint8_t* out, trt_stats* st);
/* host only, no context: TRT_OK when every segment is valid, else TRT_ERR_INVALID with the lowest
 * bad index in *first_bad (may be NULL).  segs NULL with n > 0 is TRT_ERR_INVALID (*first_bad = 0). */
int trt_check_segs(const trt_qseg* segs, uint32_t n, uint32_t* first_bad);

/* ---- visibility masks: any hit over a direction or target set per point ----------------------
 * The gather form of the occlusion query.  Ambient occlusion, light visibility and form-factor
 * sampling come as POINTS that each ask the same K questions: K hemisphere directions from a
 * surface point, or the scene's lights from every hit.  Through trt_occluded the caller expands
 * every point into K 32-byte segments and reads K bytes back; here the points go in (32 B each),
 * the set of K <= TRT_VIS_MAX_SET directions or targets is shared by all of them, the segments are
 * made in the kernel, and one 64-bit mask per point comes out: bit k = segment (i, k) is occluded.
 *
 * `set` is always a HOST array of nset entries of 4 floats each (the 4th is ignored), copied during
 * the call; 1 <= nset <= TRT_VIS_MAX_SET.  Segment (i, k) is built from point i and entry e =
 * set[k], all in FP32, every product and sum rounded on its own, in the project's dot order, no FMA:
 *   TRT_VIS_DIRS:     s = (e.x * n.x + e.y * n.y) + e.z * n.z;  dir = s < 0 ? -e : e (zero, -0.0 and
 *                     n = (0,0,0) keep e: a zero normal means "the whole sphere, no flip");  org =
 *                     pos;  tmax = the point's.  n only chooses a side and need not be normalized.
 *   TRT_VIS_TARGETS:  dir = e.xyz - pos, componentwise;  len = sqrt((dx*dx + dy*dy) + dz*dz),
 *                     correctly rounded;  tmax = fminf(len, the point's tmax): the point's tmax is a
 *                     range cap.  n is not read.
 * Bit k of out_masks[i] is 1 iff trt_occluded would report TRT_OCC_OCCLUDED for that segment under
 * the same flags; bits >= nset are 0.  trt_point_segments emits the records exactly as the kernel
 * forms them, so   mask bit == trt_occluded(trt_point_segments(...))[i * nset + k].
 * In TARGETS mode a segment that is not a valid trt_qseg is not traced and reads 0: a point
 * coincident with a target, or farther from it than the direction length range allows, sees the
 * target (host and device arrays alike).
 *
 * Read from p: flags only; FLOOR, SPHERES, BATCH_WALK, DEVICE_PTRS and TIMING as by trt_occluded,
 * TRT_FLAG_COUNT is TRT_ERR_INVALID, everything else is ignored.  With TRT_FLAG_DEVICE_PTRS `pts`
 * and `out_masks` are device pointers (`set` stays a host array).
 *
 * A valid point: pos and n finite, 0 < tmax <= TRT_QSEG_MAX_T, in both modes.  A valid set entry:
 * a valid ray direction (trt_qray's length range) for DIRS, finite for TARGETS.  The set is always
 * checked on the host (TRT_ERR_INVALID, the entry's index in trt_last_error).  Host points are
 * checked before anything runs: a bad one returns TRT_ERR_INVALID with the lowest bad index in
 * trt_last_error and out_masks untouched.  In a device array a bad point reads TRT_VIS_BAD_POINT
 * and traces nothing; the other points, those that share its wave included, are unaffected (with
 * nset <= 63 a mask never equals the marker).
 *
 * Sizes, stream and buffers as trt_occluded: npts == 0 is TRT_OK and launches nothing; npts * nset >
 * TRT_QRAY_MAX_RAYS, nset of 0 or above TRT_VIS_MAX_SET, an unknown mode, or a NULL pts, set or
 * out_masks with npts > 0 is TRT_ERR_INVALID; a call before trt_upload_scene is TRT_ERR_NOSCENE.
 * Device `pts` must be 16-byte aligned and device `out_masks` 8-byte aligned.  A device-pointer call
 * without TIMING only enqueues on the context's stream; host arrays stage through context-owned
 * buffers that only grow.  The call changes nothing a later frame or query depends on. */
typedef struct trt_qpoint { float pos[3]; float tmax; float n[3]; float pad; } trt_qpoint; /* 32 B */
#define TRT_VIS_DIRS 0u
#define TRT_VIS_TARGETS 1u
#define TRT_VIS_MAX_SET 63u
#define TRT_VIS_BAD_POINT 0xffffffffffffffffull
#ifdef __cplusplus
static_assert(sizeof(trt_qpoint) == 32, "point records are 32 B");
#else
_Static_assert(sizeof(trt_qpoint) == 32, "point records are 32 B");
#endif

int trt_visibility(trt_ctx* ctx, const trt_params* p, const trt_qpoint* pts, uint32_t npts,
                   const float* set, uint32_t nset, uint32_t mode, uint64_t* out_masks, trt_stats* st);
/* host only, no context: TRT_OK when every point is valid, else TRT_ERR_INVALID with the lowest bad
 * index in *first_bad (may be NULL).  pts NULL with n > 0 is TRT_ERR_INVALID (*first_bad = 0). */
int trt_check_points(const trt_qpoint* pts, uint32_t n, uint32_t* first_bad);
/* host only, no context: the npts * nset segments of a visibility query, out[i * nset + k] = segment
 * (i, k) exactly as the kernel forms it (pad 0).  A degenerate TARGETS segment is emitted as
 * computed and fails trt_check_segs.  TRT_ERR_INVALID for a bad point or set entry, an nset outside
 * 1..TRT_VIS_MAX_SET, an unknown mode or a null array. */
int trt_point_segments(const trt_qpoint* pts, uint32_t npts, const float* set, uint32_t nset,
                       uint32_t mode, trt_qseg* out /* npts * nset, out[i * nset + k] */);

/* ---- all-hits queries: every surface crossing of a segment, in order ---------------------------
 * trt_trace_rays reports the first surface of a ray and trt_occluded whether a segment meets any;
 * trt_trace_all reports EVERYTHING a segment crosses, nearest first, and how many crossings there
 * are: thickness along a ray, absorption, X-ray views, inside / outside by parity.
 *
 * Segment i is a trt_qseg exactly as trt_occluded reads it: org, d = normalize(dir) by the shader's
 * own normalize, cut off at tmax; the same valid-record predicate.
 *
 * Its hits are the shader's own primitive tests, each kept iff MIN_EPSILON < t < tmax (both strict):
 *   floor     with TRT_FLAG_FLOOR, scene_intersect's floor test: at most one hit;
 *   sphere i  with TRT_FLAG_SPHERES, both roots of ray_sphere_intersect's terms, t0 = tca - thc then
 *             t1 = tca + thc, each if > MIN_EPSILON; t1 is dropped when it equals a kept t0 (a
 *             tangent ray gives one hit).  The first root reported is the t trt_trace_rays reports;
 *   triangle  one candidate per (batch, triangle) pair of the reference's loop: the batch passes
 *             ray_aabb_intersect and Moller-Trumbore passes, exactly as a nearest-hit query tests.
 *             A triangle the BVH references twice (a spatial split) is still one candidate.
 * They are ordered by the key (t, class, a, b): class 0 the floor, 1 a sphere (a = its index), 2 a
 * triangle (a = batch index, b = the caller's triangle index): the order in which scene_intersect
 * resolves ties (floor before sphere before triangle at equal t, lower sphere index first, then
 * (batch, triangle)).
 *
 * hits[i * max_hits + j] is the j-th hit in that order, a trt_qhit with the field meanings of
 * trt_trace_rays (n before any facing flip; u, v for triangles).  With m = min(total, max_hits),
 * slots j >= m receive the miss record (t = 1e10, TRT_HIT_NONE, zeros), and
 *   counts[i] = m | (TRT_ALLHITS_MORE if an (m + 1)-th hit exists inside tmax).
 * hits may be NULL: only the counts are produced, and max_hits still bounds them.
 * For every valid segment: (counts[i] & 0x7fffffff) > 0 equals trt_occluded's byte; record 0 equals
 * the trt_trace_rays record of the same ray, bit for bit, whenever that record's t < tmax; and the
 * answer for max_hits = K is the first K records of the answer for any larger value.
 *
 * Read from p: flags only; FLOOR, SPHERES, BATCH_WALK, DEVICE_PTRS and TIMING as by trt_occluded,
 * TRT_FLAG_COUNT is TRT_ERR_INVALID, everything else is ignored.  max_hits outside
 * 1..TRT_ALLHITS_MAX, nsegs * max_hits > TRT_QRAY_MAX_RAYS, or a NULL segs or counts with nsegs > 0
 * is TRT_ERR_INVALID; nsegs == 0 is TRT_OK and launches nothing; a call before trt_upload_scene is
 * TRT_ERR_NOSCENE.  Host arrays are validated first: a bad record returns TRT_ERR_INVALID with the
 * lowest bad index in trt_last_error and the outputs untouched; they then stage through
 * context-owned buffers that only grow.  In a device array a bad record traces nothing: its count
 * reads TRT_ALLHITS_BAD_SEG and every one of its slots kind TRT_HIT_BAD_RAY with zeros elsewhere;
 * the other segments of its wave are unaffected.  Device `segs` and `hits` must be 16-byte aligned
 * and `counts` 4-byte aligned.  A device-pointer call without TIMING only enqueues on the
 * context's stream.  The cost is one nearest-hit walk per reported hit plus one (the searches
 * restart from the root).  The call changes nothing a later frame or query depends on. */
#define TRT_ALLHITS_MAX 32u              /* max_hits in 1..32 */
#define TRT_ALLHITS_MORE 0x80000000u     /* in counts[i]: further hits exist inside tmax */
#define TRT_ALLHITS_BAD_SEG 0xffffffffu  /* counts[i] of a bad record in a device array */
int trt_trace_all(trt_ctx* ctx, const trt_params* p, const trt_qseg* segs, uint32_t nsegs,
                  uint32_t max_hits, trt_qhit* hits /* nsegs * max_hits, or NULL */,
                  uint32_t* counts /* nsegs */, trt_stats* st);

/* Device time per frame (ms) of each launch timed by the last timed trt_render_frames call:
 * the launch's event span divided by the frames it traced (waits for them); n <= the number
 * of timed launches, trt_timed_launches(). */
int trt_frame_times(trt_ctx* ctx, float* ms, uint32_t n);
/* Launches timed by the last timed trt_render_frames call, and (frames_out, may be NULL) the
 * frames each traced. */
uint32_t trt_timed_launches(trt_ctx* ctx, uint32_t* frames_out, uint32_t cap);

/* Waits for all work enqueued on the context's stream. */
int trt_synchronize(trt_ctx* ctx);

/* Rows written by trt_render for these params (H, or the band's share). */
uint32_t trt_output_rows(const trt_params* p);

/* Fills `p` with the reference defaults: 1024x768, depth 20, spp 1, fov 1.05,
 * TRT_FLAGS_REFERENCE. */
void trt_params_default(trt_params* p);

/* ---- multi-GPU frame tiling over RCCL (SURVEY §8(b) trt_render_multi, §8(e)) ----------
 * Replaces the single-queue dispatch + submit (main.cpp:2108-2131, 2181-2205) with one frame
 * row-tiled over the GPUs of a node: rows are dealt in interleaved bands of `band_rows` rows
 * to ranks * groups_per_rank band groups (row y -> group (y / band_rows) % (ranks * groups);
 * group g is rendered by rank g / groups_per_rank), every device renders its groups with the
 * single-GPU kernel into compact RGBA8 buffers, one grouped ncclSend / ncclRecv moves them to
 * the frame's root device over xGMI, and a re-interleave kernel assembles the frame there.
 * The result is bit-identical to trt_render of the whole frame.  The scene is built once, on
 * rank 0, and its device bindings are broadcast (ncclBroadcast) to the other devices.
 * Output arrays `out_rgba8` have one entry per device of THIS process (trt_multi_local_count);
 * only the root's entry is written (the others may be NULL). */
typedef struct trt_multi trt_multi;

#define TRT_MULTI_ID_BYTES 128 /* ncclUniqueId */
#define TRT_ROOT_ROTATE (-1)   /* root of frame i = rank i % ranks (every device's xGMI links
                                  ingest frames at once) */

/* One process drives `ndev` devices (ncclCommInitAll); rank i = devices[i]. */
int trt_multi_create(trt_multi** out, const int* devices, uint32_t ndev);
/* One process per GPU: every rank passes the same id (made by trt_multi_unique_id on one rank
 * and exchanged out of band, e.g. MPI or torch.distributed), ncclCommInitRank. */
int trt_multi_unique_id(uint8_t* id /* TRT_MULTI_ID_BYTES */);
int trt_multi_create_rank(trt_multi** out, int hip_device, uint32_t nranks, uint32_t rank, const uint8_t* id);
int trt_multi_destroy(trt_multi* m);
const char* trt_multi_last_error(const trt_multi* m);
uint32_t trt_multi_ranks(const trt_multi* m);       /* world size */
uint32_t trt_multi_local_count(const trt_multi* m); /* devices driven by this process */
/* The per-device context of local device i (its stream, split and frames-in-flight knobs). */
trt_ctx* trt_multi_context(trt_multi* m, uint32_t local);
/* Band groups per rank (default 1); more groups = finer interleave of the image over ranks. */
int trt_multi_set_band_groups(trt_multi* m, uint32_t groups_per_rank);
/* trt_upload_scene on rank 0 + broadcast of its device bindings; on the other ranks of a
 * one-process-per-GPU run the arrays are ignored (may be NULL).  Collective. */
int trt_multi_upload_scene(trt_multi* m, const trt_ubo* ubo, const trt_triangle* tris, uint32_t ntri,
                           const trt_model* models, uint32_t nmodel, const uint8_t* env_rgba8,
                           uint32_t env_w, uint32_t env_h);
int trt_multi_update_ubo(trt_multi* m, const trt_ubo* ubo);
/* One frame (p describes the whole frame; band_* must be 0) gathered on rank `root` (or
 * TRT_ROOT_ROTATE).  out_rgba8[i]: width*height*4 bytes, a device pointer on local device i
 * with TRT_FLAG_DEVICE_PTRS (then the call only enqueues on each context's stream), else a
 * host pointer (synchronous).  TRT_FLAG_COUNT: st = counters summed over all ranks (a
 * separate counting pass).  Collective. */
int trt_render_multi(trt_multi* m, const trt_params* p, uint32_t band_rows, int root,
                     uint8_t* const* out_rgba8, trt_stats* st);
/* The frame loop of trt_render_frames, tiled: frames i = 0..nframes-1 (UBO ubos[i], or the
 * current one) in batches of `frames_per_gather` frames.  Each device traces its band groups of
 * a batch's frames (multi-frame launches, trt_set_frame_batch), then ONE grouped ncclSend /
 * ncclRecv moves every frame's bands to that frame's root (trt_band_plan) and each root
 * re-interleaves its frames: frame i lands at out_rgba8[local index of its root] + i *
 * frame_stride on rank trt_frame_root(i, ranks, root) — with TRT_ROOT_ROTATE frame i goes to rank
 * i % ranks, so every device ingests at once and every rank's entry must be set; with a fixed
 * root only the root's entry is written.  Two batches are in flight: a batch's gather +
 * re-interleave overlaps the next batch's render.  Requires TRT_FLAG_DEVICE_PTRS; only
 * enqueues (complete on each context's stream).  Collective. */
int trt_render_multi_frames(trt_multi* m, const trt_params* p, const trt_ubo* ubos, uint32_t nframes,
                            uint32_t band_rows, int root, uint32_t frames_per_gather,
                            uint8_t* const* out_rgba8, size_t frame_stride);
/* trt_set_view on every local context of m: trt_render_multi and trt_render_multi_frames use each
 * context's view (per-frame views of the tiled loop are not offered). */
int trt_multi_set_view(trt_multi* m, const trt_view* v);
/* Waits for every context stream of this process. */
int trt_multi_synchronize(trt_multi* m);
/* Test / diagnostic: with on != 0 the root's own band groups also travel through the gather
 * (an ncclSend to itself and the re-interleave) instead of being rendered in place, so the
 * whole exchange runs on a one-GPU communicator.  Same image; slower. */
int trt_multi_set_self_gather(trt_multi* m, int on);

/* ---- the exchange plan of a tiled batch ---------------------------------------------------
 * The data movement trt_render_multi_frames performs for a batch of `nframes` frames starting
 * at frame `first_frame` of the call, as a list of transfers, so a host with its own transport
 * (MPI, torch.distributed, ...) can run the same exchange; trt_multi.cpp executes exactly this
 * plan over RCCL (ncclSend / ncclRecv in list order on both ends, one group).  Frame i's root is
 * trt_frame_root(i, nranks, root): `root`, or i % nranks for TRT_ROOT_ROTATE.  Rank q renders
 * band groups q * G .. q * G + G - 1 (G = groups_per_rank) of every frame.  One transfer per
 * (sender, root) pair carries all of the batch's frames that root owns:
 *   - the batch frames are ordered by root; rank r's J_r frames (batch order) start at frame
 *     slot off_r = the number of batch frames rooted by ranks < r;
 *   - a sender stores group v of the j-th frame of root r at ((off_r + j) * G + v) * block_bytes
 *     of its batch buffer, so the J_r * G blocks for root r are contiguous;
 *   - root r receives sender q's blocks at (q * J_r * G) * block_bytes of its gather buffer, i.e.
 *     group v of its j-th frame at ((q * J_r + j) * G + v) * block_bytes;
 *   - compact row k of band group g is frame row trt_band_frame_row(k, band_rows, groups, g).
 * Blocks are block_bytes each (padded to the largest group).  Without TRT_PLAN_SELF_GATHER the
 * root's own groups do not travel (it renders them in place).  Pure host arithmetic. */
typedef struct trt_band_layout {
    uint32_t groups;       /* band groups NG = nranks * groups_per_rank */
    uint32_t max_rows;     /* compact rows of the largest group */
    uint64_t block_bytes;  /* one compact group buffer: max_rows * width * 4 */
    uint64_t local_bytes;  /* a rank's batch buffer: nframes * groups_per_rank * block_bytes */
    uint64_t gather_bytes; /* the largest gather buffer of a root: frames rooted * groups * block_bytes */
} trt_band_layout;
typedef struct trt_band_xfer {
    uint32_t src, dst;   /* sending rank, receiving rank (the root of the carried frames) */
    uint32_t frames;     /* J_dst: the batch frames dst roots (all of them travel together) */
    uint32_t groups;     /* band groups per frame (groups_per_rank) */
    uint32_t first_slot; /* off_dst: their first frame slot in the sender's buffer */
    uint32_t pad;
    uint64_t src_offset; /* bytes into the sender's batch buffer: off_dst * G * block_bytes */
    uint64_t dst_offset; /* bytes into the root's gather buffer: src * J_dst * G * block_bytes */
    uint64_t bytes;      /* J_dst * G * block_bytes */
} trt_band_xfer;
#define TRT_PLAN_SELF_GATHER 1u
uint32_t trt_frame_root(uint32_t frame, uint32_t nranks, int root);
uint32_t trt_band_frame_row(uint32_t k, uint32_t band_rows, uint32_t groups, uint32_t g);
/* Fills *layout and up to `cap` transfers (xfers may be NULL to count them); *count = the
 * number of transfers of the plan. */
int trt_band_plan(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t nranks, uint32_t groups_per_rank,
                  uint32_t first_frame, uint32_t nframes, int root, uint32_t flags, trt_band_layout* layout,
                  trt_band_xfer* xfers, uint32_t cap, uint32_t* count);

/* ---- diagnostic: the shadow occluder masks of a launch --------------------------------------
 * Plain triangle-free frames skip a shadow query's test of sphere j for light i wherever the
 * launch's masks prove it cannot be hit: bit 4 * i + j of a mask = "sphere j may occlude light
 * i".  This returns the masks the runtime would build for a UBO, computed on the host (no context,
 * no GPU).  spheres: 4 x (centre xyz, radius); lights: 3 x xyz; flags: TRT_FLAG_SPHERES is read;
 * cell: edge of a floor cell (<= 0: the default, 0.25).  out_cells receives *nx * *nz masks, cell
 * (ix, iz) at [iz * *nx + ix], covering floor x in [-10 + ix * cell, ...), z in [-30 + iz * cell,
 * ...) at y = -4 (room for `cap` masks); out_rows receives the 4 masks of hits on spheres 0..3.
 * Returns 0, or 1 when the masks are the all-ones fallback (*nx = *nz = 1: spheres off, a
 * non-finite or absurd input, a light inside a sphere or on the floor plane), or -1 on a null
 * argument or when the cells do not fit `cap`. */
int trt_diag_shadow_mask(const float* spheres, const float* lights, uint32_t flags, float cell,
                         uint16_t* out_cells, uint32_t cap, uint32_t* nx, uint32_t* nz, uint32_t* out_rows);

/* ---- host scene build (main.cpp:192-252, 1529-1580, 2290-2335) -------------------- */

typedef struct trt_scene trt_scene;

int trt_scene_create(trt_scene** out);
void trt_scene_destroy(trt_scene* s);
const char* trt_scene_last_error(const trt_scene* s);

/* Triangles per AABB batch (main.cpp:1549: 64). */
int trt_scene_set_batch_size(trt_scene* s, uint32_t batch_size);

/* One modelList entry (config.hpp:97-101) from an already-triangulated mesh: positions
 * (xyz floats, nverts) and indices (3 per triangle, file order).  Applies
 * M = T * Rz * Ry * Rx * S (transformTriangles, main.cpp:192-216), smooth vertex
 * normals when normal_interp == 1 (computeVertexNormals, main.cpp:218-252), then splits
 * into batches with AABBs (main.cpp:1548-1566). */
int trt_scene_add_mesh(trt_scene* s, const float* positions, uint32_t nverts,
                       const uint32_t* indices, uint32_t ntris, const trt_material* mat,
                       const float scale[3], const float rotation_deg[3],
                       const float translation[3], int normal_interp);

/* The same from an OBJ file (loadObjAsTriangles, main.cpp:2290-2335, with tinyobjloader's
 * triangulation rules). */
int trt_scene_add_obj(trt_scene* s, const char* path, const trt_material* mat,
                      const float scale[3], const float rotation_deg[3],
                      const float translation[3], int normal_interp);

uint32_t trt_scene_triangle_count(const trt_scene* s);
uint32_t trt_scene_model_count(const trt_scene* s);
const trt_triangle* trt_scene_triangles(const trt_scene* s);
const trt_model* trt_scene_models(const trt_scene* s);

/* ---- envmap JPEG ---------------------------------------------------------
 * The reference reads its envmap with stb_image v2.22, stbi_load(path, ..., STBI_rgb_alpha)
 * (main.cpp:928-949), then uploads it as binding 4.  This path decodes the same files to the
 * same RGBA8 bytes: the entropy decode (Huffman, baseline and progressive scans) runs on the
 * host into coefficient planes (trt_jpeg_*), and dequantisation, IDCT, chroma upsampling and
 * colour conversion run on the GPU (trt_jpeg_decode), straight into device memory. */

/* colour model of the RGBA output (stb's load_jpeg_image) */
#define TRT_JPEG_GRAY 0
#define TRT_JPEG_YCBCR 1
#define TRT_JPEG_RGB 2  /* component ids 'R','G','B', or Adobe transform 0 without JFIF */
#define TRT_JPEG_CMYK 3 /* 4 components, Adobe transform 0 */
#define TRT_JPEG_YCCK 4 /* 4 components, Adobe transform 2 */

typedef struct trt_jpeg trt_jpeg;

typedef struct trt_jpeg_info {
    uint32_t width, height;
    uint32_t components;  /* 1, 3 or 4 */
    uint32_t progressive; /* SOF2 */
    int32_t color;        /* TRT_JPEG_* */
    uint32_t hmax, vmax;  /* largest sampling factors */
    uint32_t h[4], v[4];  /* per-component sampling factors */
    uint32_t blocks_w[4], blocks_h[4]; /* MCU-padded block grid of each coefficient plane */
} trt_jpeg_info;

int trt_jpeg_create(trt_jpeg** out);
void trt_jpeg_destroy(trt_jpeg* j);
const char* trt_jpeg_last_error(const trt_jpeg* j);

/* Parses `len` bytes of a JPEG file and entropy-decodes every scan (host). */
int trt_jpeg_parse(trt_jpeg* j, const uint8_t* data, size_t len);
int trt_jpeg_get_info(const trt_jpeg* j, trt_jpeg_info* info);

/* Raw (not dequantised) coefficients of component c: blocks_w * blocks_h blocks of 64
 * int16 in natural (row-major) order; and its 64-entry quantisation table.  NULL if c is
 * out of range or nothing was parsed. */
const int16_t* trt_jpeg_coefficients(const trt_jpeg* j, uint32_t c);
const uint16_t* trt_jpeg_quant(const trt_jpeg* j, uint32_t c);

/* GPU reconstruction of a parsed JPEG into width * height * 4 bytes of RGBA8 (alpha 255), the
 * buffer stbi_load(..., STBI_rgb_alpha) returns.  Host pointer unless TRT_FLAG_DEVICE_PTRS.
 * Synchronous. */
int trt_jpeg_decode(trt_ctx* ctx, const trt_jpeg* j, uint8_t* out_rgba8, uint32_t flags);

/* Binding 4 from JPEG bytes (the reference's stbi_load + texture upload, main.cpp:928-1111):
 * replaces the context's envmap.  Call after trt_upload_scene (which replaces every
 * binding). */
int trt_upload_envmap_jpeg(trt_ctx* ctx, const uint8_t* data, size_t len);

/* ---- frame files (the reference only presents, main.cpp:2181-2205) ------- */

/* Binary PPM (P6, RGB; alpha dropped) of a host RGBA8 frame, e.g. trt_render's out_rgba8. */
int trt_write_ppm(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* 8-bit RGBA PNG (zlib deflate) of a host RGBA8 frame. */
int trt_write_png(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* TRT_ABI_H */
