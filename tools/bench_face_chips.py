#!/usr/bin/env python3
"""OpenCLIP face mode measurements.

(a) Chip stage: 64 face rectangles of a seeded mix of sizes (sides 24 .. 400) on 1080p frames resident
    in HBM, one pc_face_chips call against the per-face FaceEmbedder._resize_chip loop (one launch per
    face, host INTER_AREA tables), alternated in one process; the two outputs are compared byte for byte.
(b) Whole path: FaceEmbedder(use_arcface=False).extract_batch with ViT-L/14 on 64 noise frames
    (1080p, SCRFD-10G at conf 0.5, as bench.py's C3), f32 and f16x3: faces/s, and the stages of one
    embed batch timed one by one - chips / quality / prep (Pillow resample + patch matrix) / tower.
Warm-up, repeated runs, medians with min and max; the device is synchronised inside the clock.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from person_capture_amd import _lib, imageops  # noqa: E402
from person_capture_amd import face_embedder as fe_mod  # noqa: E402

CHIP = _lib.CHIP_BYTES
H, W = 1080, 1920


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "runs": len(ts)}


def rectangles(n, nframes, seed=20260601):
    """(frame, y, x, h, w): sides log-uniform in 24 .. 400 with an aspect jitter, anywhere in the frame."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = float(np.exp(rng.uniform(np.log(24.0), np.log(400.0))))
        h = int(np.clip(round(s * rng.uniform(0.85, 1.25)), 24, 400))
        w = int(np.clip(round(s * rng.uniform(0.8, 1.1)), 24, 400))
        out.append((int(rng.integers(0, nframes)), int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    return out


def part_a(fe, dframes, n, warmup, reps):
    ctx = fe._ectx
    fsz = H * W * 3
    rects = rectangles(n, dframes.nbytes // fsz)
    kinds = {}
    for _, _, _, h, w in rects:
        p = imageops.chip_plan(h, w)
        k = p["kind"] + (str(p["area_mode"]) if p["kind"] == "linear" else "")
        kinds[k] = kinds.get(k, 0) + 1
    ptr = np.array([dframes.ptr + f * fsz + y * W * 3 + x * 3 for f, y, x, _, _ in rects], np.int64)
    hh, ww = np.array([r[3] for r in rects]), np.array([r[4] for r in rects])
    out_b, out_l = ctx.alloc(n * CHIP), ctx.alloc(n * CHIP)

    def batched():   # descriptors built per call, as _embed_launch does
        d = imageops.chip_descs(ptr, hh, ww, W * 3)
        _lib.check(ctx.lib.pc_face_chips(ctx.handle, d.ctypes.data_as(C.POINTER(_lib.ChipDesc)), n, out_b.ptr),
                   ctx.handle, "face_chips")
        ctx.sync()

    def loop():
        for i in range(n):
            fe._resize_chip(fe_mod._DevImage(int(ptr[i]), int(hh[i]), int(ww[i]), W * 3), out_l.ptr + i * CHIP)
        ctx.sync()

    for _ in range(warmup):
        batched()
        loop()
    tb, tl = [], []
    for _ in range(reps):   # alternated, so drift hits both alike
        for fn, ts in ((batched, tb), (loop, tl)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    same = bool(np.array_equal(ctx.download(out_b.ptr, (n * CHIP,), np.uint8), ctx.download(out_l.ptr, (n * CHIP,), np.uint8)))
    src_bytes = int((hh * ww * 3).sum())
    return {"faces": n, "kinds": kinds, "batched_call": stats(tb), "per_face_loop": stats(tl),
            "loop_over_batched": statistics.median(tl) / statistics.median(tb), "bytes_identical": same,
            "source_bytes": src_bytes, "chip_bytes": n * CHIP}


def part_b(prec, tower, frames_n, dframes, steps, warmup, reps):
    os.environ["PERSON_CAPTURE_AMD_FACE_CLIP_PRECISION"] = prec
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_10g_bnkps", conf=0.5, use_arcface=False,
                             clip_model_name=tower)
    fsz = H * W * 3
    devs = [fe_mod._DevImage(dframes.ptr + i * fsz, H, W, W * 3) for i in range(frames_n)]

    def run():
        return fe.extract_batch([None] * frames_n, dev_frames=devs)

    for _ in range(warmup):
        res = run()
    nfaces = sum(len(r) for r in res)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    # one embed batch, stage by stage (each synchronised)
    ctx, eng = fe._ectx, fe._clip
    m = eng.max_batch
    boxes = [(i, f["bbox"]) for i, r in enumerate(res) for f in r][:m]
    m = len(boxes)
    ptr = np.array([devs[i].ptr + int(b[1]) * W * 3 + int(b[0]) * 3 for i, b in boxes], np.int64)
    hh = np.array([int(b[3] - b[1]) for _, b in boxes])
    ww = np.array([int(b[2] - b[0]) for _, b in boxes])
    chips, q, feat = ctx.alloc(m * CHIP), ctx.alloc(m * 8), ctx.alloc(m * eng.dim * 4)
    tok = (eng.side // eng.patch) ** 2 + 1
    prep_out = ctx.alloc(m * tok * 2 * 640 * 4)
    crops = (_lib.CropDesc * m)()
    for j in range(m):
        crops[j].d_src, crops[j].H, crops[j].W, crops[j].row_stride = chips.ptr + j * CHIP, 112, 112, 336
    lib, h = ctx.lib, ctx.handle

    def s_chips():
        d = imageops.chip_descs(ptr, hh, ww, W * 3)
        _lib.check(lib.pc_face_chips(h, d.ctypes.data_as(C.POINTER(_lib.ChipDesc)), m, chips.ptr), h, "face_chips")
        ctx.sync()

    def s_quality():
        _lib.check(lib.pc_face_quality(h, chips.ptr, m, 112, q.ptr), h, "face_quality")
        ctx.sync()

    def s_prep():
        _lib.check(lib.pc_clip_prep_geom(h, eng.precision, eng.side, eng.patch, crops, m, prep_out.ptr), h, "clip_prep")
        ctx.sync()

    def s_embed():
        _lib.check(lib.pc_clip_embed_geom(eng.net.handle, eng.side, eng.patch, crops, m, C.c_void_p(feat.ptr)), h,
                   "clip_embed")
        ctx.sync()

    st = {}
    for name, fn in (("chips", s_chips), ("quality", s_quality), ("prep", s_prep), ("prep_plus_tower", s_embed)):
        st[name] = stats(bench_timed(fn, warmup, reps))
    tower_ms = st["prep_plus_tower"]["median_ms"] - st["prep"]["median_ms"]
    total = st["chips"]["median_ms"] + st["quality"]["median_ms"] + st["prep_plus_tower"]["median_ms"]
    med = statistics.median(ts)
    return {"tower": tower, "precision": prec, "frames": frames_n, "faces_per_step": nfaces, "step": stats(ts),
            "faces_per_s": nfaces / med, "frames_per_s": frames_n / med, "embed_batch_faces": m, "stages": st,
            "tower_ms": tower_ms, "tower_share_of_embed_batch": tower_ms / total}


def bench_timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--faces", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--tower", default="ViT-L-14")
    ap.add_argument("--precisions", default="f32,f16x3")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "face_chips_bench.json"))
    a = ap.parse_args()
    res = {"args": {k: v for k, v in vars(a).items() if k != "out"}}
    os.environ["PERSON_CAPTURE_AMD_ARCFACE"] = "iresnet50"   # (part a's embedder: only its _resize_chip is used)
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    frames = bench.synth_frames(0, a.frames)
    dframes = fe._ctx.alloc(frames.nbytes)
    fe._ctx.upload(frames, dframes)
    fe._ctx.sync()
    if "a" in a.parts:
        res["a_chip_stage"] = part_a(fe, dframes, a.faces, a.warmup, a.reps)
    if "b" in a.parts:
        res["b_whole_path"] = [part_b(p, a.tower, a.frames, dframes, a.steps, 1, max(5, a.reps // 3))
                               for p in a.precisions.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
