#!/usr/bin/env python3
"""What a visibility query costs next to the same question asked through trt_occluded.

On the C4 mesh scene (20 icospheres, 102,400 triangles): 2^14 surface points — points_on_hits of
the 1024 x 512 pinhole frame's rays, every hit's point, thinned evenly to 2^14 — each asking the 63
directions of scene.sphere_dirs(63) turned into its hemisphere (ambient occlusion), cut off at tmax =
2.0 and at tmax = 1e10.  In one process, device pointers, after a warm-up, the variants taking turns
round by round so that a drift lands on all of them alike:

  visibility_t2, visibility_t1e10   trt_visibility: 32 B per point in, the 63-entry set, 8 B per
                                    point out; the segments are made in the kernel; every lane
                                    walks alone (the default);
  visibility_coop_t2, ..._t1e10     the same through a TRT_VIS_COOP=1 context: a wave is one point,
                                    one origin, and takes the wave-cooperative shadow walk;
  occluded_t2, occluded_t1e10       trt_occluded over the same 2^14 x 63 segments, expanded on the
                                    host (scene.point_segments) and already resident on the device.
                                    The expansion and its upload are NOT timed: they are the traffic
                                    the visibility form removes (2,016 B in and 63 B out per point
                                    against 32 B and 8 B), reported as bytes.

Each call is bracketed by events on the context's stream; per variant the median, min, max and
quartile spread of the timed repeats in microseconds, and nanoseconds per segment.  The answers are
compared first: every mask equals the occlusion bytes of its point, packed.  One JSON line, printed
and appended to --out.

  python tools/vis_bench.py [--rounds 20] [--settle-ms 300] [--out profiles/visibility_query.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    ap.add_argument("--size", default="1024x512", help="the pinhole frame whose hits give the points")
    ap.add_argument("--points", type=int, default=1 << 14)
    ap.add_argument("--dirs", type=int, default=63)
    ap.add_argument("--level", type=int, default=4, help="icosphere level of C4 (4: 102,400 triangles)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 10, "at least 10 timed repeats"
    import numpy as np
    import torch

    import vkcomputeshader_tinyraytracer_amd as trt
    from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

    if not torch.cuda.is_available():
        sys.exit("vis_bench: no GPU; a timing needs one")
    w, h = (int(v) for v in a.size.split("x"))
    sc = S.config_c4(w, h, env_size=(1024, 512), level=a.level)
    p = sc.params()
    os.environ.pop("TRT_VIS_COOP", None)
    r = trt.Renderer(0)
    r.upload_scene(sc)
    os.environ["TRT_VIS_COOP"] = "1"  # read when a context is created
    rc = trt.Renderer(0)
    del os.environ["TRT_VIS_COOP"]
    rc.upload_scene(sc)
    rays = S.pinhole_qrays(p).reshape(-1)
    _, _, hits, _ = r.trace_rays(rays, p, want8=False, want_hits=True)
    every, _ = S.points_on_hits(rays, hits)
    assert len(every) >= a.points, f"the frame has {len(every)} hits"
    pts = every[np.linspace(0, len(every) - 1, a.points).astype(np.int64)]
    n, k = len(pts), a.dirs
    dirs = S.sphere_dirs(k)
    tmaxes = {"t2": np.float32(2.0), "t1e10": T.QSEG_MAX_T}

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1, 32)).cuda()

    d_pts, d_segs, masks, occ = {}, {}, {}, {}
    for tag, tm in tmaxes.items():
        q = pts.copy()
        q["tmax"] = tm
        d_pts[tag] = dev(q)
        d_segs[tag] = dev(S.point_segments(q, dirs=dirs).reshape(-1))  # the expansion the caller would make
        masks[tag] = torch.empty(n, dtype=torch.int64, device="cuda")
        masks["coop_" + tag] = torch.empty(n, dtype=torch.int64, device="cuda")
        occ[tag] = torch.empty(n * k, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.set_stream(s)
    rc.set_stream(s)
    variants = {}
    for tag in tmaxes:
        variants[f"visibility_{tag}"] = lambda tag=tag: r.visibility(d_pts[tag], p, dirs=dirs, out=masks[tag])
        variants[f"visibility_coop_{tag}"] = lambda tag=tag: rc.visibility(d_pts[tag], p, dirs=dirs, out=masks["coop_" + tag])
        variants[f"occluded_{tag}"] = lambda tag=tag: r.occluded(d_segs[tag], p, out=occ[tag])

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    for fn in variants.values():  # the first launch of each kernel loads its code
        timed(fn)
    frac = {}
    for tag in tmaxes:
        o = occ[tag].cpu().numpy().reshape(n, k)
        assert np.isin(o, (T.OCC_VISIBLE, T.OCC_OCCLUDED)).all()
        want = np.bitwise_or.reduce((o == T.OCC_OCCLUDED).astype(np.uint64) << np.arange(k, dtype=np.uint64)[None], axis=1)
        for m in (tag, "coop_" + tag):
            assert masks[m].cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), f"masks differ from occluded ({m})"
        frac[tag] = round(float(o.mean()), 4)
    t_end = time.perf_counter() + a.settle_ms / 1e3
    while time.perf_counter() < t_end:
        for fn in variants.values():
            timed(fn)
    us = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            us[name].append(timed(fn))
    r.set_stream(None)
    rc.set_stream(None)
    res = {"scene": "C4", "triangles": int(len(sc.tris)), "points": n, "dirs": k, "segments": n * k, "rounds": a.rounds,
           "occluded_frac": frac,
           "bytes_visibility": {"in": n * 32 + k * 16, "out": n * 8},
           "bytes_occluded": {"in": n * k * 32, "out": n * k}}
    for name, v in us.items():
        v = np.asarray(v)
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        res[name] = {"med_us": round(float(med), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2),
                     "iqr_us": round(float(q3 - q1), 2), "ns_per_segment": round(float(med) * 1e3 / (n * k), 4)}
    for tag in tmaxes:
        res[f"visibility_over_occluded_{tag}"] = round(res[f"visibility_{tag}"]["med_us"] / res[f"occluded_{tag}"]["med_us"], 4)
        res[f"visibility_coop_over_occluded_{tag}"] = round(res[f"visibility_coop_{tag}"]["med_us"] / res[f"occluded_{tag}"]["med_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    rc.close()
    r.close()


if __name__ == "__main__":
    main()
