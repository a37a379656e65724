#!/usr/bin/env python3
"""What an oriented frame costs: C2 frames through one prepared render_frames call (a ring of
per-frame images), once with camera_orbit's views (the camera turns while it walks: oriented
launches, no sky table, spans, masks or floor class), once as the same walk in the reference
camera, and once more in the reference camera under TRT_SKY_TABLE=0 (the kernel the oriented
frames run, without the view's nine VALU).  Device events around each call, alternating rounds.

  python tools/view_orbit.py [--frames 1000] [--rounds 5] [--width 1024 --height 768]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) <= 4:  # as the library (frames in flight = streams)
    os.environ["GPU_MAX_HW_QUEUES"] = "32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--ring", type=int, default=64, help="distinct output images (and camera positions / views)")
    ap.add_argument("--settle-ms", type=float, default=50.0, help="untimed frames first for this long (clock ramp)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import vkcomputeshader_tinyraytracer_amd as trt
    from vkcomputeshader_tinyraytracer_amd import scene as S

    sc = S.config_c2(a.width, a.height)
    p = sc.params()
    n, ring = a.frames, min(a.ring, a.frames)
    # a mouse look that sweeps +-16 degrees of yaw and +-4 of pitch over the ring, back and forth
    ubos_r, views_r = S.camera_orbit(sc.ubo, ring, yaw_step=0.5, pitch_step=-0.125, yaw0=-16.0, pitch0=4.0)
    idx = np.arange(n) % ring
    ubos, views = ubos_r[idx], views_r[idx]
    fb = p.height * p.width * 4
    out = torch.empty((ring, p.height, p.width, 4), dtype=torch.uint8, device="cuda")

    def context(env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            r = trt.Renderer(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        r.upload_scene(sc)
        return r

    stream = torch.cuda.Stream()
    arms = {}
    for name, env, vw in (("oriented", {}, views), ("reference_camera", {}, None),
                          ("reference_camera_TRT_SKY_TABLE_0", {"TRT_SKY_TABLE": "0"}, None)):
        r = context(env)
        r.set_stream(stream)
        # frame i of the call writes ring image i % ring: calls of `ring` frames, stride fb
        calls = [r.frames_call(p, out, min(ring, n - i0), ubos=ubos[i0:i0 + ring], frame_stride=fb,
                               views=None if vw is None else vw[i0:i0 + ring]) for i0 in range(0, n, ring)]
        arms[name] = (r, calls)

    def run(calls):
        for c in calls:
            c()

    t_end = time.perf_counter() + a.settle_ms / 1e3
    while time.perf_counter() < t_end:
        for _, calls in arms.values():
            run(calls)
        torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(a.rounds):
        for name, (_, calls) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            run(calls)
            e1.record(stream)
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / n)
    for name, v in us.items():
        print(json.dumps({"arm": name, "config": "C2", "size": [p.width, p.height], "frames": n, "ring": ring,
                          "us_per_frame_median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                          "max": round(max(v), 3), "rounds": len(v)}), flush=True)
    for r, _ in arms.values():
        r.close()


if __name__ == "__main__":
    main()
