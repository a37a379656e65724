"""Host-side mirror of the reference's compute path, over the C-ABI.

The reference's ComputeShaderApplication drives the hot path as
  createShaderStorageBuffers() + createUniformBuffers()  -> Renderer.upload_scene()
  updateUniformBuffer()                                  -> Renderer.update_ubo()
  recordComputeCommandBuffer() + vkQueueSubmit()         -> Renderer.draw_frame()
(main.cpp:1494-1664, 2108-2205).  Output pointers may be numpy arrays (host) or torch CUDA
tensors (device, rendered in place on the context's stream).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import types as T
from ._lib import TrtError, lib
from .scene import Scene


def _is_torch_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


class Renderer:
    def __init__(self, device: int = 0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.trt_create(ctypes.byref(h), int(device))
        if rc != 0:
            raise TrtError(rc, f"trt_create(device={device}) failed: no usable HIP device")
        self._h = h
        self.device = device
        self.scene: Scene | None = None
        # the camera position and the view in force, for pixel_ray / pick
        self._cam = np.zeros(3, np.float32)
        self._view: np.ndarray | None = None

    # -- errors ----------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise TrtError(rc, self._L.trt_last_error(self._h).decode())

    # -- bindings --------------------------------------------------------------------------
    def upload_scene(self, scene: Scene) -> None:
        ubo = np.ascontiguousarray(scene.ubo)
        tris = np.ascontiguousarray(scene.tris, T.TRIANGLE)
        models = np.ascontiguousarray(scene.models, T.MODEL)
        env = None if scene.env is None else np.ascontiguousarray(scene.env, np.uint8)
        self._check(self._L.trt_upload_scene(
            self._h, ubo.ctypes.data, tris.ctypes.data if len(tris) else None, len(tris),
            models.ctypes.data if len(models) else None, len(models),
            env.ctypes.data if env is not None else None,
            0 if env is None else env.shape[1], 0 if env is None else env.shape[0]))
        self.scene = scene
        self._cam = np.array(ubo["camPos"], np.float32).reshape(-1)[:3]

    def update_ubo(self, ubo: np.ndarray) -> None:
        u = np.ascontiguousarray(ubo)
        self._check(self._L.trt_update_ubo(self._h, u.ctypes.data))
        self._cam = np.array(u["camPos"], np.float32).reshape(-1)[:3]

    def _walked(self, ubos, nframes: int) -> None:
        # a frame loop leaves the context's UBO at its last frame's (trt_render_frames): keep the
        # camera pixel_ray / pick read in step with it
        if ubos is not None and nframes > 0:
            self._cam = np.array(ubos[nframes - 1]["camPos"], np.float32).reshape(-1)[:3]

    def set_view(self, view) -> None:
        """The context's view (trt_set_view): a T.VIEW record (scene.view_look / view_ypr), or None
        for the reference camera.  Every later draw_frame and every render_frames frame without
        a view of its own is generated in this basis; rays_in, where given, wins."""
        if view is None:
            self._check(self._L.trt_set_view(self._h, None))
            self._view = None
            return
        v = np.ascontiguousarray(view, T.VIEW)
        self._check(self._L.trt_set_view(self._h, v.ctypes.data))
        self._view = v.copy()

    @staticmethod
    def _views(views, nframes: int):
        if views is None:
            return None
        v = np.ascontiguousarray(views, T.VIEW).reshape(-1)
        if v.shape[0] < nframes:
            raise ValueError(f"{v.shape[0]} views for {nframes} frames")
        return v

    def set_frames_in_flight(self, n: int) -> None:
        """Frames of render_frames that may run concurrently (trt_set_frames_in_flight; the
        reference's MAX_FRAMES_IN_FLIGHT = 2, main.cpp:45): 1..32, or 0 = auto (4; 16 for
        deferred-shadow frames)."""
        self._check(self._L.trt_set_frames_in_flight(self._h, int(n)))

    def set_frame_batch(self, n: int) -> None:
        """Frames per launch of render_frames (trt_set_frame_batch): 0 = auto (up to 64 plain
        frames per launch), 1 = one launch per frame (the reference's dispatch per frame),
        2..64."""
        self._check(self._L.trt_set_frame_batch(self._h, int(n)))

    def set_subtree_split(self, window: int) -> None:
        """trt_set_subtree_split: 0 = auto (default), 1 = off, 2..5 = depth window."""
        self._check(self._L.trt_set_subtree_split(self._h, int(window)))

    def set_deferred_shadows(self, mode: int) -> None:
        """trt_set_deferred_shadows: 0 = auto (default: mesh scenes at max_depth >= 8), 1 = off,
        2 = on."""
        self._check(self._L.trt_set_deferred_shadows(self._h, int(mode)))

    def defer_stats(self, slot: int = 0) -> dict:
        """trt_defer_stats of in-flight slot `slot` (waits for the context's stream): event
        chunks taken / shadow queries appended, pixels re-traced in place, and the slot's
        capacities."""
        out = (ctypes.c_uint64 * 5)()
        self._check(self._L.trt_defer_stats(self._h, int(slot), out))
        return {"chunks": out[0], "queries": out[1], "fallback_pixels": out[2], "chunk_cap": out[3],
                "query_cap": out[4]}

    def set_stream(self, stream) -> None:
        """`stream`: a torch.cuda.Stream (not the legacy default stream), a raw hipStream_t
        int, or None (the context's own stream)."""
        if stream is None:
            self._check(self._L.trt_set_stream(self._h, None))
            return
        s = getattr(stream, "cuda_stream", stream)
        if not s:
            raise ValueError("the legacy null stream cannot be selected; use a torch.cuda.Stream()")
        self._check(self._L.trt_set_stream(self._h, ctypes.c_void_p(s)))

    def synchronize(self) -> None:
        self._check(self._L.trt_synchronize(self._h))

    # -- frames ----------------------------------------------------------------------------
    def draw_frame(self, params: T.Params, out8=None, out32=None, rays_in=None, count: bool = False,
                   timing: bool = False, want8: bool = True, want32: bool = False):
        """Renders one frame.  With numpy/None outputs returns host arrays
        (rows, W, 4) uint8 / float32; with torch CUDA tensors renders into them in place.
        Returns (rgba8, rgba32f, stats_dict)."""
        p = T.Params.from_buffer_copy(params)
        rows = int(self._L.trt_output_rows(ctypes.byref(p)))
        if p.flags & T.FLAG_BAND_IN_PLACE:  # bands written at their frame rows: full-size outputs
            rows = p.height
        dev = _is_torch_cuda(out8) or _is_torch_cuda(out32) or _is_torch_cuda(rays_in)
        if dev:
            p.flags |= T.FLAG_DEVICE_PTRS
            for x in (out8, out32, rays_in):
                if x is not None and not _is_torch_cuda(x):
                    raise ValueError("mixing host and device pointers in one draw_frame call")
            if out8 is not None:
                assert out8.is_contiguous() and out8.numel() >= rows * p.width * 4
            if out32 is not None:
                assert out32.is_contiguous() and out32.numel() >= rows * p.width * 4
            o8 = out8.data_ptr() if out8 is not None else None
            o32 = out32.data_ptr() if out32 is not None else None
            if rays_in is not None:
                p.rays_in = rays_in.data_ptr()
        else:
            if out8 is None and want8:
                out8 = np.empty((rows, p.width, 4), np.uint8)
            if out32 is None and want32:
                out32 = np.empty((rows, p.width, 4), np.float32)
            if out8 is not None:
                assert out8.flags["C_CONTIGUOUS"] and out8.size >= rows * p.width * 4
            if out32 is not None:
                assert out32.flags["C_CONTIGUOUS"] and out32.size >= rows * p.width * 4
            o8 = out8.ctypes.data if out8 is not None else None
            o32 = out32.ctypes.data if out32 is not None else None
            if rays_in is not None:
                rays_in = np.ascontiguousarray(rays_in, T.RAY)
                assert rays_in.size >= p.width * p.height
                p.rays_in = rays_in.ctypes.data
        if count:
            p.flags |= T.FLAG_COUNT
        if timing:
            p.flags |= T.FLAG_TIMING
        st = T.Stats()
        self._check(self._L.trt_render(self._h, ctypes.byref(p), o8, o32, ctypes.byref(st)))
        return out8, out32, st.as_dict()

    # -- ray queries -------------------------------------------------------------------------
    def trace_rays(self, rays, params: T.Params, *, count: bool = False, want8: bool = True, want32: bool = False,
                   want_hits: bool = False, timing: bool = False, out8=None, out32=None, hits=None,
                   nrays: int | None = None):
        """Traces the caller's rays (trt_trace_rays): `rays` is a numpy array of T.QRAY (host,
        synchronous, every ray validated first) or a torch CUDA tensor holding such records
        (device pointers, only enqueued on the context's stream unless count / timing; a ray that
        is not valid gets word 0, float4 0 and kind T.HIT_BAD_RAY).  Of `params` only max_depth
        and the scene flags are read.  Outputs are made on the side of the rays unless given
        (numpy arrays, or torch CUDA tensors with device rays; they may be longer than the query):
        rgba8 (n, 4) uint8, rgba32f (n, 4) float32, hits (n,) T.QHIT — on the device an (n, 32)
        uint8 tensor of the same bytes; device rays, hits and rgba32f must be 16-byte aligned (torch's
        own allocations are; an offset view may not be: TrtError).  `nrays` limits the query to the
        first rays.
        Returns (rgba8, rgba32f, hits, stats_dict)."""
        p = T.Params.from_buffer_copy(params)
        p.rays_in = None
        dev = _is_torch_cuda(rays)
        if dev:
            import torch

            if not rays.is_contiguous():
                raise ValueError("rays must be a contiguous device tensor of T.QRAY records")
            have = rays.numel() * rays.element_size() // T.QRAY.itemsize
            n = have if nrays is None else int(nrays)
            if n > have:
                raise ValueError(f"{n} rays asked of a tensor that holds {have}")
            p.flags |= T.FLAG_DEVICE_PTRS

            def made(x, want, shape, dtype, words):
                if x is None and want:
                    x = torch.empty(shape, dtype=dtype, device=rays.device)
                if x is not None and not (_is_torch_cuda(x) and x.is_contiguous() and x.numel() * x.element_size() >= n * words):
                    raise ValueError("outputs of a device query are contiguous device tensors that hold every ray")
                return x

            out8 = made(out8, want8, (n, 4), torch.uint8, 4)
            out32 = made(out32, want32, (n, 4), torch.float32, 16)
            hits = made(hits, want_hits, (n, T.QHIT.itemsize), torch.uint8, T.QHIT.itemsize)
            ptrs = [rays.data_ptr()] + [x.data_ptr() if x is not None else None for x in (out8, out32, hits)]
        else:
            p.flags &= ~T.FLAG_DEVICE_PTRS
            r = None if rays is None else np.ascontiguousarray(rays, T.QRAY).reshape(-1)
            n = (0 if r is None else r.shape[0]) if nrays is None else int(nrays)
            if r is not None and n > r.shape[0]:
                raise ValueError(f"{n} rays asked of an array that holds {r.shape[0]}")

            def made(x, want, shape, dtype):
                if x is None and want:
                    x = np.empty(shape, dtype)
                if x is not None and not (isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == dtype
                                          and x.size >= int(np.prod(shape))):
                    raise ValueError("outputs of a host query are C-contiguous numpy arrays that hold every ray")
                return x

            out8 = made(out8, want8, (n, 4), np.uint8)
            out32 = made(out32, want32, (n, 4), np.float32)
            hits = made(hits, want_hits, (n,), T.QHIT)
            ptrs = [None if r is None else r.ctypes.data] + [x.ctypes.data if x is not None else None
                                                              for x in (out8, out32, hits)]
        if count:
            p.flags |= T.FLAG_COUNT
        else:
            p.flags &= ~T.FLAG_COUNT
        if timing:
            p.flags |= T.FLAG_TIMING
        else:
            p.flags &= ~T.FLAG_TIMING
        st = T.Stats()
        self._check(self._L.trt_trace_rays(self._h, ctypes.byref(p), ptrs[0], n, ptrs[1], ptrs[2], ptrs[3],
                                           ctypes.byref(st)))
        return out8, out32, hits, st.as_dict()

    # -- occlusion queries -------------------------------------------------------------------
    def occluded(self, segs, params: T.Params, *, out=None, timing: bool = False, nsegs: int | None = None):
        """Any-hit over the caller's segments (trt_occluded): is anything nearer than `tmax` along
        normalize(dir) from `org`?  `segs` is a numpy array of T.QSEG (host, synchronous, every
        segment validated first: a bad one raises TrtError and leaves `out` untouched) or a
        contiguous torch CUDA tensor holding such records (device pointers, 16-byte aligned, only
        enqueued on the context's stream unless timing; a segment that is not valid reads
        T.OCC_BAD_SEG).  Of `params` only the flags are read: FLOOR (the floor occludes; clear it
        for the shader's own shadow rays), SPHERES, BATCH_WALK; FLAG_COUNT is refused
        (T.TRT_ERR_INVALID).  `out` is made on the side of the segments unless given (it may be
        longer than the query; bytes past it are untouched); `nsegs` limits the query to the first
        segments.
        Returns the (n,) uint8 array or tensor of T.OCC_VISIBLE / T.OCC_OCCLUDED, or with `timing`
        the pair (bytes, stats_dict)."""
        p = T.Params.from_buffer_copy(params)
        p.rays_in = None
        if _is_torch_cuda(segs):
            import torch

            if not segs.is_contiguous():
                raise ValueError("segs must be a contiguous device tensor of T.QSEG records")
            have = segs.numel() * segs.element_size() // T.QSEG.itemsize
            n = have if nsegs is None else int(nsegs)
            if n > have:
                raise ValueError(f"{n} segments asked of a tensor that holds {have}")
            p.flags |= T.FLAG_DEVICE_PTRS
            if out is None:
                out = torch.empty((n,), dtype=torch.uint8, device=segs.device)
            if not (_is_torch_cuda(out) and out.is_contiguous() and out.numel() * out.element_size() >= n):
                raise ValueError("the output of a device query is a contiguous device tensor that holds every segment")
            ptrs = (segs.data_ptr(), out.data_ptr())
        else:
            p.flags &= ~T.FLAG_DEVICE_PTRS
            s = None if segs is None else np.ascontiguousarray(segs, T.QSEG).reshape(-1)
            n = (0 if s is None else s.shape[0]) if nsegs is None else int(nsegs)
            if s is not None and n > s.shape[0]:
                raise ValueError(f"{n} segments asked of an array that holds {s.shape[0]}")
            if out is None:
                out = np.empty((n,), np.uint8)
            if not (isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"] and out.dtype == np.uint8 and out.size >= n):
                raise ValueError("the output of a host query is a C-contiguous uint8 numpy array that holds every segment")
            ptrs = (None if s is None or not len(s) else s.ctypes.data, out.ctypes.data)
        if timing:
            p.flags |= T.FLAG_TIMING
        else:
            p.flags &= ~T.FLAG_TIMING
        st = T.Stats()
        self._check(self._L.trt_occluded(self._h, ctypes.byref(p), ptrs[0], n, ptrs[1], ctypes.byref(st)))
        return (out, st.as_dict()) if timing else out

    # -- all-hits queries --------------------------------------------------------------------
    def trace_all(self, segs, params: T.Params, max_hits: int = 8, *, want_hits: bool = True, hits=None, counts=None,
                  timing: bool = False, nsegs: int | None = None):
        """Every surface crossing of the caller's segments, nearest first (trt_trace_all): up to
        `max_hits` (1..T.ALLHITS_MAX) T.QHIT records per segment in the order (t, floor < sphere <
        triangle, index), and a count.  counts[i] & 0x7fffffff is the number of records, bit
        T.ALLHITS_MORE says further hits exist inside tmax; slots past the count hold the miss
        record.  `segs`, the flags of `params` and the host / device conventions are those of
        `occluded`: a numpy array of T.QSEG (validated first; a bad one raises TrtError and leaves
        the outputs untouched) or a contiguous torch CUDA tensor (16-byte aligned, only enqueued
        unless timing; a segment that is not valid reads T.ALLHITS_BAD_SEG and kind T.HIT_BAD_RAY
        in every slot).  Outputs are made on the side of the segments unless given and may be
        longer than the query; on the device hits are an (n, K, 32) uint8 tensor and counts
        torch.int32 (the same bits).  With want_hits false (and no `hits`) only the counts are
        produced; max_hits still bounds them.
        Returns (hits (n, K) or None, counts (n,) uint32), with `timing` also the stats_dict."""
        p = T.Params.from_buffer_copy(params)
        p.rays_in = None
        K = int(max_hits)
        if _is_torch_cuda(segs):
            import torch

            if not segs.is_contiguous():
                raise ValueError("segs must be a contiguous device tensor of T.QSEG records")
            have = segs.numel() * segs.element_size() // T.QSEG.itemsize
            n = have if nsegs is None else int(nsegs)
            if n > have:
                raise ValueError(f"{n} segments asked of a tensor that holds {have}")
            p.flags |= T.FLAG_DEVICE_PTRS
            if hits is None and want_hits:
                hits = torch.empty((n, max(K, 0), T.QHIT.itemsize), dtype=torch.uint8, device=segs.device)
            if counts is None:
                counts = torch.empty((n,), dtype=torch.int32, device=segs.device)
            for x, need in ((hits, n * K * T.QHIT.itemsize), (counts, n * 4)):
                if x is not None and not (_is_torch_cuda(x) and x.is_contiguous() and x.numel() * x.element_size() >= need):
                    raise ValueError("outputs of a device query are contiguous device tensors that hold every segment")
            ptrs = (segs.data_ptr(), None if hits is None else hits.data_ptr(), counts.data_ptr())
        else:
            p.flags &= ~T.FLAG_DEVICE_PTRS
            s = None if segs is None else np.ascontiguousarray(segs, T.QSEG).reshape(-1)
            n = (0 if s is None else s.shape[0]) if nsegs is None else int(nsegs)
            if s is not None and n > s.shape[0]:
                raise ValueError(f"{n} segments asked of an array that holds {s.shape[0]}")
            if hits is None and want_hits:
                hits = np.empty((n, max(K, 0)), T.QHIT)
            if counts is None:
                counts = np.empty((n,), np.uint32)
            for x, dtype, need in ((hits, T.QHIT, n * K), (counts, np.uint32, n)):
                if x is not None and not (isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == dtype
                                          and x.size >= need):
                    raise ValueError("outputs of a host query are C-contiguous numpy arrays that hold every segment")
            ptrs = (None if s is None or not len(s) else s.ctypes.data, None if hits is None else hits.ctypes.data,
                    counts.ctypes.data)
        if timing:
            p.flags |= T.FLAG_TIMING
        else:
            p.flags &= ~T.FLAG_TIMING
        st = T.Stats()
        self._check(self._L.trt_trace_all(self._h, ctypes.byref(p), ptrs[0], n, K & 0xFFFFFFFF, ptrs[1], ptrs[2],
                                          ctypes.byref(st)))
        return (hits, counts, st.as_dict()) if timing else (hits, counts)

    def contains(self, points, params: T.Params, direction=(0.3, 1.0, 0.2)) -> np.ndarray:
        """Which of the (n, 3) host `points` lie inside the scene's closed meshes: one whole-ray,
        count-only `trace_all` per point along `direction`, with the floor and the spheres cleared;
        inside means an odd number of crossings.  Raises if any ray crosses more than
        T.ALLHITS_MAX surfaces.  The usual caveat of parity tests applies: a ray through an edge or
        a vertex shared by two triangles may count that crossing twice or not at all (the
        Moller-Trumbore test is inclusive on the edges), a ray grazing a surface tangentially
        counts a touch as a crossing, and an open or self-intersecting mesh has no inside; choose
        a direction that is not aligned with the mesh, or vote over several.
        Returns an (n,) bool array."""
        from .scene import crossing_parity

        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        segs = np.zeros(len(pts), T.QSEG)
        segs["org"] = pts
        segs["dir"] = np.asarray(direction, np.float32)
        segs["tmax"] = T.QSEG_MAX_T
        p = T.Params.from_buffer_copy(params)
        p.flags &= ~(T.FLAG_FLOOR | T.FLAG_SPHERES)
        _, counts = self.trace_all(segs, p, T.ALLHITS_MAX, want_hits=False)
        odd, truncated = crossing_parity(counts)
        if truncated.any():
            raise ValueError(f"contains: {int(truncated.sum())} rays cross more than {T.ALLHITS_MAX} surfaces")
        return odd

    # -- visibility masks --------------------------------------------------------------------
    def visibility(self, points, params: T.Params, *, dirs=None, targets=None, out=None, timing: bool = False,
                   npoints: int | None = None):
        """The gather form of `occluded` (trt_visibility): every point asks the same K <=
        T.VIS_MAX_SET questions and gets one 64-bit mask back, bit k set = occluded.  Exactly one of
        `dirs` (directions, each turned into the hemisphere of the point's n; tmax cuts them off)
        and `targets` (points such as the lights; tmax caps the range) is a (K, 3) or (K, 4) host
        array.  The segments are made in the kernel: bit k of mask i is
        occluded(scene.point_segments(points, ...)[i, k]).  `points` is a numpy array of T.QPOINT
        (host, synchronous, every point validated first: a bad one raises TrtError and leaves `out`
        untouched) and gives a (n,) uint64 array, or a contiguous torch CUDA tensor holding such
        records (16-byte aligned, only enqueued on the context's stream unless timing) and gives a
        torch.int64 tensor in which a point that is not valid reads -1 (T.VIS_BAD_POINT).  Flags
        of `params` as for `occluded`; `out` may be longer than the query; `npoints` limits the
        query to the first points.
        Returns the masks, or with `timing` the pair (masks, stats_dict)."""
        from .scene import visibility_set

        mode, e = visibility_set(dirs, targets)
        p = T.Params.from_buffer_copy(params)
        p.rays_in = None
        if _is_torch_cuda(points):
            import torch

            if not points.is_contiguous():
                raise ValueError("points must be a contiguous device tensor of T.QPOINT records")
            have = points.numel() * points.element_size() // T.QPOINT.itemsize
            n = have if npoints is None else int(npoints)
            if n > have:
                raise ValueError(f"{n} points asked of a tensor that holds {have}")
            p.flags |= T.FLAG_DEVICE_PTRS
            if out is None:
                out = torch.empty((n,), dtype=torch.int64, device=points.device)
            if not (_is_torch_cuda(out) and out.is_contiguous() and out.numel() * out.element_size() >= n * 8):
                raise ValueError("the output of a device query is a contiguous device tensor that holds every mask")
            ptrs = (points.data_ptr(), out.data_ptr())
        else:
            p.flags &= ~T.FLAG_DEVICE_PTRS
            s = None if points is None else np.ascontiguousarray(points, T.QPOINT).reshape(-1)
            n = (0 if s is None else s.shape[0]) if npoints is None else int(npoints)
            if s is not None and n > s.shape[0]:
                raise ValueError(f"{n} points asked of an array that holds {s.shape[0]}")
            if out is None:
                out = np.empty((n,), np.uint64)
            if not (isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"] and out.dtype == np.uint64 and out.size >= n):
                raise ValueError("the output of a host query is a C-contiguous uint64 numpy array that holds every mask")
            ptrs = (None if s is None or not len(s) else s.ctypes.data, out.ctypes.data)
        if timing:
            p.flags |= T.FLAG_TIMING
        else:
            p.flags &= ~T.FLAG_TIMING
        st = T.Stats()
        self._check(self._L.trt_visibility(self._h, ctypes.byref(p), ptrs[0], n, e.ctypes.data if len(e) else None,
                                           len(e), mode, ptrs[1], ctypes.byref(st)))
        return (out, st.as_dict()) if timing else out

    def pixel_ray(self, params: T.Params, x: int, y: int) -> np.ndarray:
        """The T.QRAY of pixel (x, y)'s primary ray at spp 1 under the context's current UBO
        (camPos) and view (trt_pixel_ray)."""
        p = T.Params.from_buffer_copy(params)
        out = np.zeros(1, T.QRAY)
        cam = (ctypes.c_float * 3)(*[float(v) for v in self._cam])
        v = self._view
        rc = self._L.trt_pixel_ray(ctypes.byref(p), None if v is None else v.ctypes.data, cam, int(x), int(y),
                                   out.ctypes.data)
        if rc != 0:
            raise TrtError(rc, f"trt_pixel_ray: pixel ({x}, {y}) is outside the {p.width}x{p.height} image")
        return out

    def pick(self, params: T.Params, x: int, y: int) -> np.ndarray:
        """What is under pixel (x, y): the T.QHIT record of that pixel's primary ray under the
        context's current UBO and view — one trt_pixel_ray and a one-ray hits-only query."""
        return self.trace_rays(self.pixel_ray(params, x, y), params, want8=False, want_hits=True)[2][0]

    def render_frames(self, params: T.Params, out8, nframes: int, ubos: np.ndarray | None = None,
                      frame_stride: int = 0, timing: bool = False, time_every: int = 1, views=None) -> int:
        """Native frame loop (trt_render_frames): `nframes` frames enqueued on the context's
        stream into the device tensor `out8` (+ i * frame_stride bytes); plain frames go out
        several per launch (set_frame_batch).  `views`: one T.VIEW per frame
        (trt_render_frames_view; scene.camera_orbit), or None = the context's view for all.

        With `timing`, launches 0, time_every, 2*time_every, ... are bracketed by HIP events;
        returns how many were (read them with frame_times / launch_frames)."""
        if not _is_torch_cuda(out8):
            raise ValueError("render_frames renders into a device (torch CUDA) tensor")
        p = T.Params.from_buffer_copy(params)
        p.flags |= T.FLAG_DEVICE_PTRS
        p.flags &= ~T.FLAG_COUNT
        if timing:
            p.flags |= T.FLAG_TIMING
        else:
            p.flags &= ~T.FLAG_TIMING
        rows = p.height if p.flags & T.FLAG_BAND_IN_PLACE else int(self._L.trt_output_rows(ctypes.byref(p)))
        need = rows * p.width * 4 + max(nframes - 1, 0) * frame_stride
        if not out8.is_contiguous() or out8.dtype.itemsize != 1 or out8.numel() < need:
            raise ValueError(f"out8 must be a contiguous uint8 tensor of >= {need} bytes")
        u = None
        if ubos is not None:
            u = np.ascontiguousarray(ubos, T.UBO)
            if u.shape[0] < nframes:
                raise ValueError(f"{u.shape[0]} UBOs for {nframes} frames")
        v = self._views(views, nframes)
        up = u.ctypes.data if u is not None else None
        if v is None:
            self._check(self._L.trt_render_frames(self._h, ctypes.byref(p), up, nframes, out8.data_ptr(),
                                                  frame_stride, time_every))
        else:
            self._check(self._L.trt_render_frames_view(self._h, ctypes.byref(p), up, v.ctypes.data, nframes,
                                                       out8.data_ptr(), frame_stride, time_every))
        self._walked(u, nframes)
        return int(self._L.trt_timed_launches(self._h, None, 0)) if timing else 0

    def frames_call(self, params: T.Params, out8, nframes: int, ubos: np.ndarray | None = None,
                    frame_stride: int = 0, views=None):
        """render_frames(params, out8, nframes, ubos, frame_stride) with its argument checks and
        conversions done once: returns a zero-argument callable that only enqueues the frames
        (one trt_render_frames call), for host loops that re-issue the same frame list."""
        if not _is_torch_cuda(out8):
            raise ValueError("render_frames renders into a device (torch CUDA) tensor")
        p = T.Params.from_buffer_copy(params)
        p.flags |= T.FLAG_DEVICE_PTRS
        p.flags &= ~(T.FLAG_COUNT | T.FLAG_TIMING)
        rows = p.height if p.flags & T.FLAG_BAND_IN_PLACE else int(self._L.trt_output_rows(ctypes.byref(p)))
        need = rows * p.width * 4 + max(nframes - 1, 0) * frame_stride
        if not out8.is_contiguous() or out8.dtype.itemsize != 1 or out8.numel() < need:
            raise ValueError(f"out8 must be a contiguous uint8 tensor of >= {need} bytes")
        u = None
        if ubos is not None:
            u = np.ascontiguousarray(ubos, T.UBO)
            if u.shape[0] < nframes:
                raise ValueError(f"{u.shape[0]} UBOs for {nframes} frames")
        fn, h, pp = self._L.trt_render_frames, self._h, ctypes.byref(p)
        up, op = (u.ctypes.data if u is not None else None), out8.data_ptr()
        v = self._views(views, nframes)
        keep = (p, u, out8, v)  # alive as long as the callable

        if v is not None:  # one view per frame (trt_render_frames_view)
            fnv, vp = self._L.trt_render_frames_view, v.ctypes.data

            def call() -> None:
                rc = fnv(h, pp, up, vp, nframes, op, frame_stride, 0)
                if rc:
                    self._check(rc)
                self._walked(u, nframes)
            call.keep = keep
            return call

        def call() -> None:
            rc = fn(h, pp, up, nframes, op, frame_stride, 0)
            if rc:
                self._check(rc)
            self._walked(u, nframes)
        call.keep = keep
        return call

    def frame_times(self, n: int) -> np.ndarray:
        """Device ms per frame of each of the first n timed launches (span / frames traced)."""
        ms = (ctypes.c_float * n)()
        self._check(self._L.trt_frame_times(self._h, ms, n))
        return np.frombuffer(ms, np.float32).copy()

    def launch_frames(self) -> np.ndarray:
        """Frames traced by each launch timed by the last timed render_frames call."""
        n = int(self._L.trt_timed_launches(self._h, None, 0))
        out = (ctypes.c_uint32 * max(n, 1))()
        self._L.trt_timed_launches(self._h, out, n)
        return np.frombuffer(out, np.uint32)[:n].copy()

    # -- envmap JPEG -----------------------------------------------------------
    def decode_jpeg(self, jpeg, out=None):
        """stbi_load(..., STBI_rgb_alpha) of a JPEG (bytes, path or JpegFile): host entropy
        decode + GPU reconstruction.  Returns an (H, W, 4) uint8 numpy array, or renders into
        `out` when it is a torch CUDA tensor."""
        from .jpeg import JpegFile

        jf = jpeg if isinstance(jpeg, JpegFile) else JpegFile(jpeg)
        h, w = jf.shape
        if _is_torch_cuda(out):
            assert out.is_contiguous() and out.numel() >= h * w * 4
            self._check(self._L.trt_jpeg_decode(self._h, jf.handle, out.data_ptr(), T.FLAG_DEVICE_PTRS))
            return out
        img = np.empty((h, w, 4), np.uint8)
        self._check(self._L.trt_jpeg_decode(self._h, jf.handle, img.ctypes.data, 0))
        return img

    def upload_envmap_jpeg(self, data) -> None:
        """Binding 4 from JPEG bytes or a path (after upload_scene)."""
        if isinstance(data, (str, os.PathLike)):
            with open(data, "rb") as f:
                data = f.read()
        buf = bytes(data)
        self._check(self._L.trt_upload_envmap_jpeg(self._h, buf, len(buf)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.trt_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render(scene: Scene, device: int = 0, **kw):
    """One-shot convenience: upload + one frame with the scene's own settings."""
    with Renderer(device) as r:
        r.upload_scene(scene)
        return r.draw_frame(scene.params(), **kw)


def write_image(path, rgba8) -> None:
    """Writes an (H, W, 4) uint8 frame (numpy, or a torch tensor) as .png or .ppm through the
    C-ABI writers (trt_write_png / trt_write_ppm)."""
    if hasattr(rgba8, "detach"):
        rgba8 = rgba8.detach().cpu().numpy()
    a = np.ascontiguousarray(rgba8, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected (H, W, 4) RGBA8, got {a.shape}")
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    fn = {".png": "trt_write_png", ".ppm": "trt_write_ppm"}.get(ext)
    if fn is None:
        raise ValueError(f"unsupported image extension {ext!r} (.png or .ppm)")
    rc = getattr(lib(), fn)(path.encode(), a.ctypes.data, a.shape[1], a.shape[0])
    if rc != 0:
        raise TrtError(rc, f"{fn}({path!r}) failed")
