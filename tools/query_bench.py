#!/usr/bin/env python3
"""What a ray query costs next to the closest existing path: for C2 (1024x768, depth 4) and C3,
in one process and after a settle, the device time (HIP events, TRT_FLAG_TIMING) of

  rays_in     trt_render with rays_in = the pinhole rays, device pointers (the general trace_kernel);
  query_row   trt_trace_rays of the same rays in row-major order;
  query_tile  ... reordered so that each run of 64 rays is one 8x8 tile (a frame's wave shape);
  hits_tile   the hits-only query of the tile-ordered rays.

The variants take turns (one call each per round), so a clock drift lands on all of them alike.
One JSON line per configuration: per-call median / min / max and the quartile spread in
microseconds, nanoseconds per ray, and each median's ratio to the rays_in frame.

  python tools/query_bench.py [--configs C2,C3] [--rounds 40] [--settle-ms 300]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def tile_order(w: int, h: int):
    """Pixel indices such that each run of 64 is one 8x8 tile, tiles row-major (w, h multiples of 8)."""
    import numpy as np

    idx = np.arange(w * h, dtype=np.int64).reshape(h // 8, 8, w // 8, 8)
    return idx.transpose(0, 2, 1, 3).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    a = ap.parse_args()
    import numpy as np
    import torch

    import vkcomputeshader_tinyraytracer_amd as trt
    from vkcomputeshader_tinyraytracer_amd import scene as S

    r = trt.Renderer(0)
    for name in a.configs.split(","):
        sc = S.CONFIGS[name]()
        p = sc.params()
        w, h, n = p.width, p.height, p.width * p.height
        assert w % 8 == 0 and h % 8 == 0
        r.upload_scene(sc)
        ray_recs = S.view_rays(p)
        qrays = S.pinhole_qrays(p).reshape(-1)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, 32)).cuda()
        d_in, d_row, d_tile = dev(ray_recs.reshape(-1)), dev(qrays), dev(qrays[tile_order(w, h)])
        out8 = torch.empty((n, 4), dtype=torch.uint8, device="cuda")
        hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        variants = {
            "rays_in": lambda: r.draw_frame(p, out8=out8, rays_in=d_in, timing=True)[2]["kernel_ms"],
            "query_row": lambda: r.trace_rays(d_row, p, out8=out8, timing=True)[3]["kernel_ms"],
            "query_tile": lambda: r.trace_rays(d_tile, p, out8=out8, timing=True)[3]["kernel_ms"],
            "hits_tile": lambda: r.trace_rays(d_tile, p, want8=False, hits=hits, timing=True)[3]["kernel_ms"],
        }
        # the query is the frame: same words, pixel for pixel
        frame = out8.clone()
        torch.cuda.synchronize()
        r.draw_frame(p, out8=frame, rays_in=d_in, timing=True)
        r.trace_rays(d_row, p, out8=out8, timing=True)
        assert torch.equal(frame, out8), "row-major query differs from the rays_in frame"
        t_end = time.perf_counter() + a.settle_ms / 1e3
        while time.perf_counter() < t_end:
            for fn in variants.values():
                fn()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(fn())
        res = {"config": name, "size": [w, h], "depth": p.max_depth, "rays": n, "rounds": a.rounds}
        base = float(np.median(ms["rays_in"]))
        for k, v in ms.items():
            v = np.asarray(v) * 1e3
            q1, med, q3 = np.percentile(v, [25, 50, 75])
            res[k] = {"med_us": round(float(med), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2),
                      "iqr_us": round(float(q3 - q1), 2), "ns_per_ray": round(float(med) * 1e3 / n, 4),
                      "ratio_to_rays_in": round(float(med) / (base * 1e3), 4)}
        print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    main()
