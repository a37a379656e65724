#!/usr/bin/env python3
"""What an all-hits query costs next to one nearest-hit walk and next to the host loop it replaces.

The scene and the records of tools/occl_bench.py: the C4 mesh scene (20 icospheres, 102,400
triangles) at 1024 x 512, 2^20 whole-ray records — half the pinhole primary rays of the frame, half
free rays — in one process, device pointers, after a warm-up, the variants taking turns round by
round so that a drift lands on all of them alike:

  all_k4, all_k8      trt_trace_all with records, max_hits 4 and 8;
  count_k4, count_k8  the same, counts only (hits = NULL);
  hits                trt_trace_rays, hits only, over the same rays: ONE nearest-hit walk, the floor of
                      what an all-hits query can cost;
  loop_k4, loop_k8    the caller's way today: max_hits + 1 rounds (the depth the kernel's loop is
                      bounded by) of hits-only trt_trace_rays, the origins advanced on the device by
                      torch to 1e-3 past each hit.  NOT an equal answer (it loses crossings nearer
                      than the step and may repeat a surface): the price of the workaround.

Each call is bracketed by events on the context's stream; per variant the median, min, max and
quartile spread of the timed repeats in microseconds and nanoseconds per record; next to them the
mean number of next-hit searches per segment (records found + 1) and the bytes written.  One JSON
line, printed and appended to --out.

  python tools/allhits_bench.py [--rounds 20] [--settle-ms 300] [--out profiles/all_hits_query.jsonl]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tools.occl_bench import free_rays  # noqa: E402

STEP = 1e-3  # how far past a hit the host loop restarts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    ap.add_argument("--size", default="1024x512", help="frame of the pinhole half (and as many free rays)")
    ap.add_argument("--level", type=int, default=4, help="icosphere level of C4 (4: 102,400 triangles)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds >= 10, "at least 10 timed repeats"
    import numpy as np
    import torch

    import vkcomputeshader_tinyraytracer_amd as trt
    from vkcomputeshader_tinyraytracer_amd import scene as S, types as T

    if not torch.cuda.is_available():
        sys.exit("allhits_bench: no GPU; a timing needs one")
    w, h = (int(v) for v in a.size.split("x"))
    sc = S.config_c4(w, h, env_size=(1024, 512), level=a.level)
    p = sc.params()
    rays = np.concatenate([S.pinhole_qrays(p).reshape(-1), free_rays(w * h, 2026)])
    n = len(rays)
    segs = S.segments_from_rays(rays)  # tmax = 1e10

    r = trt.Renderer(0)
    r.upload_scene(sc)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(n, 32)).cuda()
    d_rays, d_segs = dev(rays), dev(segs)
    KS = (4, 8)
    rec = {k: torch.empty((n, k, 32), dtype=torch.uint8, device="cuda") for k in KS}
    cnt = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in KS}
    cnt_only = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in KS}
    hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    # the host loop's state: the working rays as floats (org 0:3, dir 4:7), their unit directions
    work = torch.empty_like(d_rays)
    wf, hf = work.view(torch.float32), hits.view(torch.float32)
    unit = torch.nn.functional.normalize(d_rays.view(torch.float32)[:, 4:7].double(), dim=1).float()
    kind = hits.view(torch.int32)[:, 1]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.set_stream(s)

    def loop(k):
        with torch.cuda.stream(s):
            work.copy_(d_rays)
            for _ in range(k + 1):
                r.trace_rays(work, p, want8=False, hits=hits)
                step = torch.where(kind != T.HIT_NONE, hf[:, 0] + STEP, torch.zeros_like(hf[:, 0]))
                wf[:, 0:3] += unit * step[:, None]

    variants = {"hits": lambda: r.trace_rays(d_rays, p, want8=False, hits=hits)}
    for k in KS:
        variants[f"all_k{k}"] = lambda k=k: r.trace_all(d_segs, p, k, hits=rec[k], counts=cnt[k])
        variants[f"count_k{k}"] = lambda k=k: r.trace_all(d_segs, p, k, want_hits=False, counts=cnt_only[k])
        variants[f"loop_k{k}"] = lambda k=k: loop(k)

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    for fn in variants.values():  # the first launch of each kernel loads its code
        timed(fn)
    timed(variants["hits"])  # the loop overwrote `hits`
    # the answers first: counts-only equals the records' counts, record 0 is the ray's own record
    first = hits.cpu().numpy().view(T.QHIT).reshape(-1)
    counts = {}
    for k in KS:
        counts[k] = cnt[k].cpu().numpy().view(np.uint32)
        assert counts[k].tobytes() == cnt_only[k].cpu().numpy().tobytes(), "counts-only differs"
        got0 = np.ascontiguousarray(rec[k].cpu().numpy()[:, 0]).view(T.QHIT).reshape(-1)
        assert got0.tobytes() == first.tobytes(), "record 0 differs from trace_rays"
    t_end = time.perf_counter() + a.settle_ms / 1e3
    while time.perf_counter() < t_end:
        for fn in variants.values():
            timed(fn)
    us = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            us[k].append(timed(fn))
    r.set_stream(None)
    res = {"scene": "C4", "triangles": int(len(sc.tris)), "records": n, "pinhole": [w, h], "rounds": a.rounds,
           "loop_step": STEP}
    for k in KS:
        m = counts[k] & 0x7FFFFFFF
        res[f"k{k}"] = {"mean_records": round(float(m.mean()), 4), "mean_searches": round(float(m.mean()) + 1.0, 4),
                        "truncated_frac": round(float(((counts[k] & T.ALLHITS_MORE) != 0).mean()), 4),
                        "bytes_records": n * k * 32 + n * 4, "bytes_counts_only": n * 4,
                        "loop_traces": k + 1, "loop_bytes_hits": (k + 1) * n * 32}
    for k, v in us.items():
        v = np.asarray(v)
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        res[k] = {"med_us": round(float(med), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2),
                  "iqr_us": round(float(q3 - q1), 2), "ns_per_record": round(float(med) * 1e3 / n, 4)}
    for k in KS:
        res[f"all_k{k}_over_hits"] = round(res[f"all_k{k}"]["med_us"] / res["hits"]["med_us"], 4)
        res[f"all_k{k}_over_loop"] = round(res[f"all_k{k}"]["med_us"] / res[f"loop_k{k}"]["med_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
