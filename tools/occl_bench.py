#!/usr/bin/env python3
"""What an occlusion query costs next to the two existing ways to ask the same question.

On the C4 mesh scene (20 icospheres, 102,400 triangles) at 1024 x 512, over the same 2^20 records —
half the pinhole primary rays of the frame, half free rays (origins uniform in the scene's box,
directions uniform on the sphere times a length in [0.1, 10], as the tests' random_rays) — in one
process, device pointers, after a warm-up, the variants taking turns round by round so that a
drift lands on all of them alike:

  occluded        trt_occluded, tmax = 1e10, the scene's flags (the floor occludes);
  occluded_nofl   trt_occluded without TRT_FLAG_FLOOR: exactly the shader's shadow_intersect;
  hits            trt_trace_rays, hits only (the nearest-hit walk a caller pays today, 32 B back);
  shadow_batch    trt_diag_shadow_batch on the same records normalised on the host (the existing
                  dense any-hit kernel: no validation, no normalize, no floor, one word per query);
  *_pinhole, *_free   occluded, occluded_nofl and hits over each half of the records on its own.

Each call is bracketed by events on the context's stream; per variant the median, min, max and
quartile spread of the timed repeats in microseconds, and nanoseconds per record.  The answers are
compared first: occluded == (hits.t < 1e10), occluded_nofl == shadow_batch.  One JSON line, printed
and appended to --out.

  python tools/occl_bench.py [--rounds 20] [--settle-ms 300] [--out profiles/occlusion_query.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def free_rays(n: int, seed: int):
    import numpy as np

    from vkcomputeshader_tinyraytracer_amd import types as T

    rng = np.random.default_rng(seed)
    q = np.zeros(n, T.QRAY)
    q["org"] = rng.uniform((-8, -3, -28), (8, 6, 2), size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q["dir"] = (d * rng.uniform(0.1, 10.0, size=(n, 1))).astype(np.float32)
    return q


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
    from vkcomputeshader_tinyraytracer_amd import lib, scene as S, types as T

    if not torch.cuda.is_available():
        sys.exit("occl_bench: no GPU; a timing needs one")
    f32 = np.float32
    w, h = (int(v) for v in a.size.split("x"))
    sc = S.config_c4(w, h, env_size=(1024, 512), level=a.level)
    p = sc.params()
    rays = np.concatenate([S.pinhole_qrays(p).reshape(-1), free_rays(w * h, 2026)])
    n = len(rays)
    segs = S.segments_from_rays(rays)  # tmax = 1e10
    d = rays["dir"]
    inv = f32(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    pre = np.zeros((n, 2, 4), f32)  # shadow_batch_kernel's record: origin + max distance, unit direction
    pre[:, 0, :3], pre[:, 0, 3], pre[:, 1, :3] = rays["org"], T.QSEG_MAX_T, d * inv[:, None]

    L = lib()
    L.trt_diag_shadow_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(T.Params), ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_void_p]
    r = trt.Renderer(0)
    r.upload_scene(sc)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(n, 32)).cuda()
    d_rays, d_segs, d_pre = dev(rays), dev(segs), dev(pre)
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    occ_nf = torch.empty(n, dtype=torch.uint8, device="cuda")
    hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    p_nf = sc.params(flags=sc.flags & ~T.FLAG_FLOOR)
    pd = T.Params.from_buffer_copy(p)
    pd.flags |= T.FLAG_DEVICE_PTRS
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    r.set_stream(s)
    variants = {
        "occluded": lambda: r.occluded(d_segs, p, out=occ),
        "occluded_nofl": lambda: r.occluded(d_segs, p_nf, out=occ_nf),
        "hits": lambda: r.trace_rays(d_rays, p, want8=False, hits=hits),
        "shadow_batch": lambda: L.trt_diag_shadow_batch(r._h, ctypes.byref(pd), d_pre.data_ptr(), n, words.data_ptr()),
    }
    # the two halves on their own (same bytes out): where the time of the whole set goes
    m = n // 2
    for tag, lo in (("pinhole", 0), ("free", m)):
        variants[f"occluded_{tag}"] = lambda lo=lo: r.occluded(d_segs[lo:lo + m], p, out=occ[lo:lo + m])
        variants[f"occluded_nofl_{tag}"] = lambda lo=lo: r.occluded(d_segs[lo:lo + m], p_nf, out=occ_nf[lo:lo + m])
        variants[f"hits_{tag}"] = lambda lo=lo: r.trace_rays(d_rays[lo:lo + m], p, want8=False, hits=hits[lo:lo + m])

    def timed(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    for fn in variants.values():  # the first launch of each kernel loads its code
        timed(fn)
    t = hits.cpu().numpy().view(T.QHIT).reshape(-1)["t"]
    got, got_nf, got_w = occ.cpu().numpy(), occ_nf.cpu().numpy(), words.cpu().numpy()
    assert got.tobytes() == (t < T.QSEG_MAX_T).astype(np.uint8).tobytes(), "occluded differs from hits.t < 1e10"
    assert got_nf.tobytes() == got_w.astype(np.uint8).tobytes(), "occluded without the floor differs from shadow_batch"
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
           "occluded_frac": round(float(got.mean()), 4), "occluded_nofl_frac": round(float(got_nf.mean()), 4)}
    for k, v in us.items():
        v = np.asarray(v)
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        res[k] = {"med_us": round(float(med), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2),
                  "iqr_us": round(float(q3 - q1), 2), "ns_per_record": round(float(med) * 1e3 / (m if k.endswith(("_pinhole", "_free")) else n), 4)}
    res["occluded_over_hits"] = round(res["occluded"]["med_us"] / res["hits"]["med_us"], 4)
    res["occluded_nofl_over_shadow_batch"] = round(res["occluded_nofl"]["med_us"] / res["shadow_batch"]["med_us"], 4)
    res["occluded_over_shadow_batch"] = round(res["occluded"]["med_us"] / res["shadow_batch"]["med_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
