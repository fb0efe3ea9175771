#!/usr/bin/env python3
"""NV12 input measurements, written to profiles/nv12_bench.json.

  k  kernels, frames resident in HBM, R launches back to back between two synchronises (run this part
     alone under `rocprofv3 --kernel-trace --stats` for the kernel times proper): pc_nv12_to_bgr at
     32 x 1080p and 8 x 4K with the bytes it needs (4.5 B / pixel) over the time as a share of the
     6.29 TB/s a float4 copy reaches; the fused downscale of 8 x 4K -> 416 wide against
     pc_nv12_to_bgr + pc_resize_area_batch.
  e  end to end from host frames, NV12 against BGR alternated in one process: FaceEmbedder.extract_batch
     of 32 x 1080p, and the pre-scan's upload + downscale of a chunk of 32 x 4K samples (two-step, and
     fused with PERSON_CAPTURE_AMD_NV12_FUSED's path).
  r  frames.reader_nv12_to_bgr per 4K frame (upload, conversion, download) against the NumPy backend on
     the same host.
Warm-up, repeated runs, medians with min and max; the device is synchronised inside the clock.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from person_capture_amd import face_embedder as fe_mod  # noqa: E402
from person_capture_amd import frames  # noqa: E402
from person_capture_amd.prescan import PrescanConfig, PrescanRunner  # noqa: E402

COPY_TBS = 6.29   # float4 copy on this part, DESIGN.md §10.3


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "runs": len(ts)}


def noise_nv12(seed, H, W):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    raw[H * W:] = rng.integers(96, 160, H * W // 2, dtype=np.uint8)
    return frames.Nv12Frame(raw, H, W)


def timed(fn, sync, warmup, reps, inner=1):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / inner)
    return ts


def part_k(ctx, warmup, reps, inner):
    out = {}
    for name, n, H, W in (("32x1080p", 32, 1080, 1920), ("8x4k", 8, 2160, 3840)):
        src = ctx.alloc(n * H * W * 3 // 2)
        ctx.upload(np.random.default_rng(1).integers(0, 256, n * H * W * 3 // 2, dtype=np.uint8), src)
        dst = ctx.alloc(n * H * W * 3)
        fsz = H * W * 3 // 2
        jobs = [(src.ptr + i * fsz, src.ptr + i * fsz + H * W, H, W, W, W, dst.ptr + i * H * W * 3, W * 3)
                for i in range(n)]
        ts = timed(lambda: frames.convert_on_device(ctx, jobs), ctx.sync, warmup, reps, inner)
        need = 4.5 * n * H * W
        med = statistics.median(ts)
        out["nv12_to_bgr_" + name] = {**stats(ts), "launches_per_sample": inner, "bytes_needed": need,
                                      "tb_per_s": need / med / 1e12, "share_of_copy": need / med / 1e12 / COPY_TBS}
        if name == "8x4k":
            OW = 416
            OH = int(round(H * OW / W))
            nv = [frames.Nv12Frame.on_device(j[0], j[1], H, W) for j in jobs]
            full = [fe_mod._DevImage(j[6], H, W, W * 3) for j in jobs]
            kf = [f"bn_f{i}" for i in range(n)]
            kt = [f"bn_t{i}" for i in range(n)]

            def fused():
                return fe_mod.dev_nv12_resize_batch(ctx, nv, kf, (OW, OH))

            def two():
                frames.convert_on_device(ctx, jobs)
                return fe_mod.dev_resize_batch(ctx, full, kt, (OW, OH))

            tf, tt = [], []
            for fn in (fused, two):
                for _ in range(warmup):
                    fn()
            ctx.sync()
            for _ in range(reps):   # alternated
                for fn, acc in ((fused, tf), (two, tt)):
                    t0 = time.perf_counter()
                    for _ in range(inner):
                        fn()
                    ctx.sync()
                    acc.append((time.perf_counter() - t0) / inner)
            a, b = fused(), two()
            same = all(np.array_equal(ctx.download(x.ptr, (OH, OW, 3), np.uint8), ctx.download(y.ptr, (OH, OW, 3), np.uint8))
                       for x, y in zip(a, b))
            out["downscale_8x4k_to_416"] = {"fused": stats(tf), "two_step": stats(tt), "bytes_identical": bool(same),
                                            "two_step_over_fused": statistics.median(tt) / statistics.median(tf)}
    return out


def part_e(warmup, reps):
    os.environ.setdefault("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    out = {}
    nv = [noise_nv12(100 + i, 1080, 1920) for i in range(32)]
    bgr = [frames.nv12_to_bgr(f) for f in nv]
    st0 = fe.policy_state()
    res = {}

    def run(batch):
        fe.set_policy_state(st0)
        return fe.extract_batch(batch)

    for _ in range(warmup):
        res["bgr"], res["nv12"] = run(bgr), run(nv)
    same = all(len(a) == len(b) and all(np.array_equal(x["feat"], y["feat"]) and tuple(x["bbox"]) == tuple(y["bbox"])
                                        for x, y in zip(a, b)) for a, b in zip(res["bgr"], res["nv12"]))
    tb, tn = [], []
    for _ in range(reps):
        for batch, acc in ((bgr, tb), (nv, tn)):
            t0 = time.perf_counter()
            run(batch)
            acc.append(time.perf_counter() - t0)
    out["extract_batch_32x1080p"] = {"bgr": stats(tb), "nv12": stats(tn), "faces": sum(len(r) for r in res["bgr"]),
                                     "results_identical": bool(same),
                                     "h2d_bytes": {"bgr": 32 * 1080 * 1920 * 3, "nv12": 32 * 1080 * 1920 * 3 // 2}}
    del bgr, nv
    # the pre-scan's feed of one chunk: 32 x 4K samples uploaded and downscaled to 416 wide
    H, W, n = 2160, 3840, 32
    nv = [noise_nv12(200 + i % 4, H, W) for i in range(n)]
    bgr = [frames.nv12_to_bgr(f) for f in nv[:4]] * (n // 4)
    r = PrescanRunner(fe, PrescanConfig(), 24.0, n, batch=n)

    def feed(src, fused):
        r.nv12_fused = fused
        ims = r._downscale_many([r._to_device(src[j], f"prescan_src{j}") for j in range(n)], list(range(n)))
        fe._ctx.sync()
        return ims

    cases = (("bgr", bgr, False), ("nv12_two_step", nv, False), ("nv12_fused", nv, True))
    ts = {k: [] for k, _, _ in cases}
    for _ in range(warmup):
        for _, src, fused in cases:
            feed(src, fused)
    for _ in range(reps):
        for k, src, fused in cases:
            t0 = time.perf_counter()
            feed(src, fused)
            ts[k].append(time.perf_counter() - t0)
    out["prescan_feed_32x4k"] = {k: stats(v) for k, v in ts.items()}
    out["prescan_feed_32x4k"]["every_fused_run_beats_every_two_step_run"] = \
        bool(max(ts["nv12_fused"]) < min(ts["nv12_two_step"]))
    return out


def part_r(ctx, warmup, reps):
    H, W = 2160, 3840
    f = noise_nv12(300, H, W)
    raw = f.data.tobytes()

    class Reader:
        _h, _w, _pc_ctx = H, W, ctx
    rd = Reader()
    got = frames.reader_nv12_to_bgr(rd, raw)
    same = bool(np.array_equal(got, frames.nv12_to_bgr(f)))
    td = timed(lambda: frames.reader_nv12_to_bgr(rd, raw), lambda: None, warmup, reps)
    tn = timed(lambda: frames.nv12_to_bgr(f), lambda: None, 1, max(3, reps // 3))
    return {"device_reader_4k": stats(td), "numpy_backend_4k": stats(tn), "bytes_identical": same,
            "numpy_over_device": statistics.median(tn) / statistics.median(td)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ker")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "nv12_bench.json"))
    a = ap.parse_args()
    res = {"args": {k: v for k, v in vars(a).items() if k != "out"}}
    ctx = fe_mod.get_context(0)
    if "k" in a.parts:
        res["kernels"] = part_k(ctx, a.warmup, a.reps, a.inner)
    if "e" in a.parts:
        res["end_to_end"] = part_e(a.warmup, a.reps)
    if "r" in a.parts:
        res["reader"] = part_r(ctx, a.warmup, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
