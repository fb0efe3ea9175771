#!/usr/bin/env python3
"""Curator measurements: (a) crop-metrics throughput on 256 synthetic 768 x 1152
crops already on the device, with the algorithmic bytes and the achieved fraction of HBM,
(b) pc_sim_matrix + pc_mmr_order at n = 2048, dim = 768, k = n, (c) the same two workloads on the
CPU (the NumPy backend on 16 threads; the reference-shaped greedy loop at n <= 512, with its
measured growth). Warm-up, repeated runs, medians and the spread (min .. max). Needs a GPU for
(a) and (b): there is no fallback."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from person_capture_amd import _lib, curate  # noqa: E402

HBM_SPEC = 8.0e12       # bytes/s, MI355X HBM3E


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "runs": len(ts)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def synth(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(xx / (17.0 + seed)) * np.cos(yy / (29.0 + seed))
    img = base[..., None] + rng.normal(0, 20, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def part_a(ctx, n, h, w, warmup, reps):
    src = [synth(h, w, s) for s in range(8)]
    bufs = [ctx.upload(src[i % 8]) for i in range(n)]
    ctx.sync()
    crops = [curate.DeviceCrop(b.ptr, h, w, 3 * w) for b in bufs]
    # the whole Python call: descriptors, one pc_crop_metrics, the download, the host halves
    def whole():
        ms = curate.crop_metrics_batch(crops, ctx=ctx)
        return [(m.phash, m.sharpness, m.exposure, m.black_border) for m in ms]
    t_whole = timed(whole, warmup, reps)
    # the device call alone (four launches), descriptors prebuilt
    descs, tabs, starts = curate.build_descs([(h, w)] * n)
    for d, b in zip(descs, bufs):
        d.d_src, d.row_stride = b.ptr, 3 * w
    off, sb, ob = curate.metrics_layout(descs, n)
    d_s, d_o = ctx.alloc(sb), ctx.alloc(ob)
    dct = curate.dct_table()
    def device():
        _lib.check(ctx.lib.pc_crop_metrics(ctx.handle, descs, n, tabs.ctypes.data_as(C.c_void_p), len(tabs),
                                           starts.ctypes.data_as(C.c_void_p), len(starts),
                                           dct.ctypes.data_as(C.c_void_p), C.c_void_p(d_s.ptr), sb,
                                           C.c_void_p(d_o.ptr), ob), ctx.handle, "crop_metrics")
        ctx.sync()
    t_dev = timed(device, warmup, reps)
    # 3 B/px read, the gray plane written once and read again by the two resizes (1 B/px each way)
    alg = 5.0 * h * w * n
    med = statistics.median(t_dev)
    return {"images": n, "h": h, "w": w, "python_call": stats(t_whole), "device_call": stats(t_dev),
            "images_per_s_python_call": n / statistics.median(t_whole), "images_per_s_device_call": n / med,
            "algorithmic_bytes": alg, "device_call_bytes_per_s": alg / med,
            "device_call_fraction_of_hbm_spec": alg / med / HBM_SPEC}


def part_b(ctx, n, dim, warmup, reps):
    rng = np.random.default_rng(1)
    F = rng.standard_normal((n, dim)).astype(np.float32)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    q = rng.uniform(0, 1, n).astype(np.float32)
    d_F, d_q = ctx.upload(F), ctx.upload(q)
    d_S, d_o = ctx.alloc(4 * n * n), ctx.alloc(4 * n)
    def sim():
        _lib.check(ctx.lib.pc_sim_matrix(ctx.handle, C.c_void_p(d_F.ptr), n, dim, C.c_void_p(d_S.ptr)), ctx.handle, "sim")
        ctx.sync()
    def mmr():
        _lib.check(ctx.lib.pc_mmr_order(ctx.handle, C.c_void_p(d_S.ptr), C.c_void_p(d_q.ptr), n, n, 0.75,
                                        C.c_void_p(d_o.ptr)), ctx.handle, "mmr")
        ctx.sync()
    def both():
        sim()
        mmr()
    t_sim, t_mmr, t_both = timed(sim, warmup, reps), timed(mmr, warmup, reps), timed(both, warmup, reps)
    order = ctx.download(d_o.ptr, (n,), np.int32)
    return {"n": n, "dim": dim, "k": n, "sim": stats(t_sim), "mmr": stats(t_mmr), "sim_plus_mmr": stats(t_both),
            "sim_gflops": 2.0 * n * n * dim / statistics.median(t_sim) / 1e9,
            "order_is_permutation": bool(np.array_equal(np.sort(order), np.arange(n)))}, F, q


def reference_shaped_mmr(q, k, S, alpha):
    """The reference's loop shape: every step walks the remaining items and takes one NumPy max over
    the picked columns per item (O(n^3) element reads, O(n^2) interpreter steps)."""
    n = len(q)
    picked, left = [], list(range(n))
    for _ in range(min(k, n)):
        best, best_s = None, -1e9
        for i in left:
            red = 0.0
            if picked:
                red = max(0.0, float(S[i, picked].max()))
            s = alpha * float(q[i]) - (1.0 - alpha) * red
            if s > best_s:
                best, best_s = i, s
        picked.append(best)
        left.remove(best)
    return picked


def part_c(h, w, F, q, threads, reps):
    imgs = [synth(h, w, s) for s in range(2 * threads)]
    def metrics():
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda im: curate.crop_metrics_batch([im])[0].phash, imgs))
    t_m = timed(metrics, 1, reps)
    out = {"threads": threads, "metrics_images": len(imgs), "metrics": stats(t_m),
           "metrics_images_per_s": len(imgs) / statistics.median(t_m)}
    S = (F @ F.T).astype(np.float32)
    loop = {}
    for n in (128, 256, 512):
        t = timed(lambda: reference_shaped_mmr(q[:n], n, S[:n, :n], 0.75), 0, 3 if n < 512 else 2)
        loop[str(n)] = stats(t)
    out["reference_shaped_loop"] = loop
    out["reference_shaped_loop_growth_exponent_256_to_512"] = float(
        np.log2(loop["512"]["median_ms"] / loop["256"]["median_ms"]))
    n = len(q)
    t_np = timed(lambda: curate.mmr_rank(F, q, alpha=0.75), 1, reps)
    out["numpy_backend_sim_plus_mmr_n%d" % n] = stats(t_np)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--h", type=int, default=1152)
    ap.add_argument("--w", type=int, default=768)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "curate_bench.json"))
    a = ap.parse_args()
    res = {"args": {k: v for k, v in vars(a).items() if k != "out"}}   # (where the file goes is not a parameter)
    rng = np.random.default_rng(1)
    F = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    q = rng.uniform(0, 1, a.n).astype(np.float32)
    if "a" in a.parts or "b" in a.parts:
        from person_capture_amd.runtime import GpuContext
        ctx = GpuContext(0)
        if "a" in a.parts:
            res["a_metrics"] = part_a(ctx, a.images, a.h, a.w, a.warmup, a.reps)
        if "b" in a.parts:
            res["b_ranking"], F, q = part_b(ctx, a.n, a.dim, a.warmup, a.reps)
        ctx.close()
    if "c" in a.parts:
        res["c_cpu"] = part_c(a.h, a.w, F, q, a.threads, max(3, a.reps // 5))
    if "a" in a.parts and "c" in a.parts:
        res["metrics_device_over_cpu"] = res["a_metrics"]["images_per_s_python_call"] / res["c_cpu"]["metrics_images_per_s"]
    if "b" in a.parts and "c" in a.parts:
        res["ranking_device_over_numpy_backend"] = (res["c_cpu"]["numpy_backend_sim_plus_mmr_n%d" % a.n]["median_ms"]
                                                    / res["b_ranking"]["sim_plus_mmr"]["median_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
