#!/usr/bin/env python3
"""Frame-gauge measurements. Needs a GPU: there is no fallback.

(a) pc_frame_gray on 32 frames of 1920 x 1080 and on 8 of 3840 x 2160 already on the device: time per
    call, the 4 bytes a pixel it has to move (3 read, 1 written) per second, and that rate as a fraction
    of the float4 copy rate of §10.3. Two sets of source frames alternate, so that a call reads 400 MB
    other than those the call before it left in the last-level cache.
(b) pc_gray_region_hist on the two 3840 x 280 bars of a letterboxed 4K plane (bars of noise 0 .. 3, and
    of full-range noise, the case the run-merging does not help).
(c) pc_gray_motion on 16 boxes of 400 x 900 of two 4K planes.
(d) per letterboxed 4K host frame: measure + autocrop_borders + faceless_validate_batch of 8 boxes, on
    the device (the frame's upload included) and on this module's NumPy backend on the same host,
    alternated in one process.
A kernel figure is K calls enqueued back to back and one synchronisation, divided by K; medians over
the repetitions after warm-up, with min .. max. Nothing here is a target fixed in advance."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from person_capture_amd import _lib  # noqa: E402
from person_capture_amd.frame_gauges import FrameGauge  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s a float4 copy reaches on this part
HBM_SPEC = 8.0e12


def stats(ts, scale=1e3):
    return {"median_ms": scale * statistics.median(ts), "min_ms": scale * min(ts), "max_ms": scale * max(ts),
            "runs": len(ts)}


def per_call(ctx, enqueue, k, warmup, reps):
    """Seconds per call: k calls back to back, then one synchronisation."""
    for _ in range(warmup):
        enqueue(0)
    ctx.sync()
    ts = []
    for r in range(reps):
        t0 = time.perf_counter()
        for i in range(k):
            enqueue(r * k + i)
        ctx.sync()
        ts.append((time.perf_counter() - t0) / k)
    return ts


def part_gray(ctx, n, h, w, k, warmup, reps):
    rng = np.random.default_rng(1)
    pitch = (w + 15) & ~15
    sets = []
    for s in range(2):
        src = [ctx.upload(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(n)]
        planes = [ctx.alloc(pitch * h) for _ in range(n)]
        sums = ctx.alloc(4 * (h + w) * n)
        d = (_lib.GrayDesc * n)()
        for i in range(n):
            d[i].d_src, d[i].row_stride, d[i].w, d[i].h, d[i].gray_pitch = src[i].ptr, 3 * w, w, h, pitch
            d[i].d_gray = planes[i].ptr
            d[i].d_row_sum = sums.ptr + 4 * (h + w) * i
            d[i].d_col_sum = d[i].d_row_sum + 4 * h
        sets.append((d, src, planes, sums))
    ctx.sync()

    def enqueue(i):
        _lib.check(ctx.lib.pc_frame_gray(ctx.handle, sets[i & 1][0], n), ctx.handle, "frame_gray")
    ts = per_call(ctx, enqueue, k, warmup, reps)
    med = statistics.median(ts)
    nbytes = 4.0 * h * w * n
    return {"frames": n, "h": h, "w": w, "calls_per_sample": k, "call": stats(ts), "bytes": nbytes,
            "bytes_per_s": nbytes / med, "fraction_of_float4_copy": nbytes / med / COPY_RATE,
            "fraction_of_hbm_spec": nbytes / med / HBM_SPEC, "frames_per_s": n / med}


def part_hist(ctx, k, warmup, reps):
    h, w, bar = 2160, 3840, 280
    rng = np.random.default_rng(2)
    out = {}
    for name, hi in (("dark_bars_0_3", 4), ("full_range_noise", 256)):
        plane = rng.integers(0, hi, (h, w), dtype=np.uint8)
        d = ctx.upload(plane)
        regs = (_lib.GrayRegion * 2)()
        for r, y in zip(regs, (0, h - bar)):
            r.d_plane, r.pitch, r.x, r.y, r.w, r.h = d.ptr, w, 0, y, w, bar
        d_out = ctx.alloc(2048)
        ctx.sync()

        def enqueue(i):
            _lib.check(ctx.lib.pc_gray_region_hist(ctx.handle, regs, 2, C.c_void_p(d_out.ptr)), ctx.handle, "hist")
        ts = per_call(ctx, enqueue, k, warmup, reps)
        got = ctx.download(d_out.ptr, (2, 256), np.uint32)
        assert np.array_equal(got[0], np.bincount(plane[:bar].ravel(), minlength=256))
        nbytes = 2.0 * w * bar
        out[name] = {"call": stats(ts), "bytes": nbytes, "bytes_per_s": nbytes / statistics.median(ts)}
    out["strips"] = "2 of 3840 x 280"
    return out


def part_motion(ctx, k, warmup, reps):
    h, w = 2160, 3840
    rng = np.random.default_rng(3)
    cur = rng.integers(0, 256, (h, w), dtype=np.uint8)
    prev = np.clip(cur.astype(np.int16) + rng.integers(-40, 41, (h, w)), 0, 255).astype(np.uint8)
    dc, dp = ctx.upload(cur), ctx.upload(prev)
    n = 16
    mb = (_lib.MotionBox * n)()
    boxes = []
    for i, m in enumerate(mb):
        x1, y1 = 37 + 210 * i, 100 + 60 * (i % 5)
        boxes.append((x1, y1, x1 + 400, y1 + 900))
        m.d_cur, m.d_prev, m.pitch, m.x1, m.y1, m.x2, m.y2 = dc.ptr, dp.ptr, w, x1, y1, x1 + 400, y1 + 900
    d_out = ctx.alloc(4 * n)
    ctx.sync()

    def enqueue(i):
        _lib.check(ctx.lib.pc_gray_motion(ctx.handle, mb, n, 15, C.c_void_p(d_out.ptr)), ctx.handle, "motion")
    ts = per_call(ctx, enqueue, k, warmup, reps)
    got = ctx.download(d_out.ptr, (n,), np.uint32)
    x1, y1, x2, y2 = boxes[3]
    assert int(got[3]) == int(np.count_nonzero(np.abs(cur[y1:y2, x1:x2].astype(np.int16) - prev[y1:y2, x1:x2]) > 15))
    nbytes = 2.0 * 400 * 900 * n
    return {"boxes": "16 of 400 x 900", "call": stats(ts), "bytes": nbytes, "bytes_per_s": nbytes / statistics.median(ts)}


def part_frame(ctx, reps):
    h, w, bar = 2160, 3840, 280
    rng = np.random.default_rng(4)
    frames = []
    for t in range(3):
        f = rng.integers(40, 256, (h, w, 3), dtype=np.uint8)
        f[:bar] = rng.integers(0, 4, (bar, w, 1), dtype=np.uint8)
        f[h - bar:] = rng.integers(0, 4, (bar, w, 1), dtype=np.uint8)
        frames.append(f)
    cfg = types.SimpleNamespace(faceless_min_area_frac=0.03, faceless_max_area_frac=0.55,
                                faceless_center_max_frac=0.12, faceless_min_motion_frac=0.02)
    boxes = [(300.0 + 400 * i, 500.0, 700.0 + 400 * i, 1400.0) for i in range(8)]
    gauges = {"device": FrameGauge(ctx), "numpy": FrameGauge()}
    res = {"device": [], "numpy": []}
    answers = {}

    def step(name, t):
        m = gauges[name].measure(frames[t % 3])
        return m.autocrop_borders(10), m.faceless_validate_batch(boxes, cfg)
    for name in gauges:   # a first frame each: the previous plane, the allocations
        step(name, 0)
    for r in range(reps):
        for name in ("device", "numpy"):
            t0 = time.perf_counter()
            answers[name] = step(name, r + 1)
            res[name].append(time.perf_counter() - t0)
    assert answers["device"] == answers["numpy"] and answers["device"][0][1], answers
    return {"frame": "3840 x 2160 BGR host array, bars of 280 rows", "boxes": 8, "device": stats(res["device"]),
            "numpy_backend": stats(res["numpy"]),
            "numpy_over_device": statistics.median(res["numpy"]) / statistics.median(res["device"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frame-reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "gauge_bench.json"))
    a = ap.parse_args()
    from person_capture_amd.runtime import GpuContext
    ctx = GpuContext(0)
    res = {"args": {k: v for k, v in vars(a).items() if k != "out"}}
    if "a" in a.parts:
        res["a_frame_gray_32x1080p"] = part_gray(ctx, 32, 1080, 1920, a.calls, a.warmup, a.reps)
        res["a_frame_gray_8x4k"] = part_gray(ctx, 8, 2160, 3840, a.calls, a.warmup, a.reps)
        res["a_frame_gray_1x4k"] = part_gray(ctx, 1, 2160, 3840, a.calls, a.warmup, a.reps)
    if "b" in a.parts:
        res["b_region_hist_4k_bars"] = part_hist(ctx, a.calls, a.warmup, a.reps)
    if "c" in a.parts:
        res["c_motion"] = part_motion(ctx, a.calls, a.warmup, a.reps)
    if "d" in a.parts:
        res["d_per_4k_frame"] = part_frame(ctx, a.frame_reps)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
