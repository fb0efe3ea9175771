#!/usr/bin/env python3
"""Benchmark: frames/sec of detect + embed + match @1080p (BASELINE.json `metric`).

Workload (BASELINE.json configs[2], the single-GPU config the metric is quoted
on): a batch of 64 synthetic 1080p BGR frames resident in HBM; one step =
FaceEmbedder.extract_batch over the batch (SCRFD-10G letterbox + detect + NMS,
5-point align, quality, ArcFace-R100 with flip-TTA, L2) + cosine match of every
face against a 32-entry reference bank on the device. Seeded synthetic
weights (no checkpoints exist offline). Frames shard across ranks with no
collective (weak scaling): each rank runs its own batch; value = all frames /
max-over-ranks time.

Also reported: roofline of the dominant kernel family (the MFMA implicit-GEMM
convs of both networks: algorithmic FLOPs / HIP-event time of their launches
inside the timed region).

A plain run sets up, warms up, times --steps steps, writes the last step's
outputs with --dump-outputs DIR and prints the result line. --full adds what
takes runs of its own after the timed steps: a bounded CPU baseline (the oracle
port of the same pipeline, rank 0, N=1), the parity passes (device f32 mode,
other precisions, CPU oracle), the HBM rates of the bandwidth-bound kernels and
the per-workload breakdowns.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0   # MI355X dense fp16 MFMA (MI355X_MICROARCH.md, chip table)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBPS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md; ~6.3 TB/s achievable)


def _dist_init():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        from person_capture_amd.shard import dist_timeout
        dist.init_process_group("gloo", init_method="env://", world_size=world, rank=rank, timeout=dist_timeout())
    return world, rank, local


def _device(local: int) -> int:
    from person_capture_amd.shard import device_for_rank
    return device_for_rank(local)


def _barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def _max_over_ranks(world, v: float) -> float:
    if world == 1:
        return v
    import torch
    import torch.distributed as dist
    t = torch.tensor([v], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _sum_over_ranks(world, v: float) -> float:
    if world == 1:
        return v
    import torch
    import torch.distributed as dist
    t = torch.tensor([v], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def synth_frames(rank: int, n: int, H: int = 1080, W: int = 1920) -> np.ndarray:
    """np.random.default_rng(seed=20260501 + frame_idx) u8 BGR frames."""
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        out[i] = np.random.default_rng(20260501 + rank * 1_000_000 + i).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return out


def synth_bank(n: int, dim: int = 512) -> np.ndarray:
    b = np.random.default_rng(20260503).standard_normal((n, dim)).astype(np.float32)
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def plant_bank(res, bank_h: np.ndarray) -> int:
    """Plant a quarter of the bank (in place) from the faces of a first pass; returns the count."""
    feats = [f["feat"] for r in res for f in r]
    n_plant = min(len(feats), len(bank_h) // 4)
    if n_plant:
        rng = np.random.default_rng(20260504)
        mean = np.mean(feats, axis=0)
        for k, i in enumerate(rng.choice(len(feats), n_plant, replace=False)):
            v = feats[i] - 0.3 * mean + (0.1 + 0.1 * k) * rng.standard_normal(512).astype(np.float32) / np.sqrt(512.0)
            bank_h[k] = v / np.linalg.norm(v)
    return n_plant


def cpu_baseline(frames: np.ndarray, fe, bank: np.ndarray, n_sample: int, n_sample_1t: int):
    """The oracle port of the same pipeline on the host cores, bounded sample: all-core
    (16 threads, the box's CPU share) and single-thread (the reference CLI pins torch and
    OpenCV to one thread, main.py:3-6,14)."""
    import torch
    from oracle import pipeline as op

    oracle_res = []

    def run(threads, n, keep=False):
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        faces = 0
        for i in range(n):
            r = op.extract_frame(frames[i], fe._scrfd_params, fe.scrfd_variant, fe._arc_params, fe._arc_depth,
                                 conf=fe.conf, D=640, bank=bank)
            faces += 0 if r == op.NEEDS_FALLBACK else len(r)
            if keep:
                oracle_res.append(None if r == op.NEEDS_FALLBACK else r)
        return n / (time.perf_counter() - t0), faces, time.perf_counter() - t0

    threads = min(16, os.cpu_count() or 1)
    v, faces, dt = run(threads, n_sample, keep=True)
    out = {"value": round(v, 4), "unit": "frames/s", "cores": threads, "kind": "port",
           "host_cpu_count": os.cpu_count(),
           "sample": f"{n_sample} of the bench's 1080p frames through oracle/pipeline.extract_frame "
                     f"(fp32 torch-CPU SCRFD-10G + ArcFace-R100 flip-TTA, numpy/C post), {faces} faces, "
                     f"{dt:.1f} s at {threads} threads"}
    if n_sample_1t > 0:
        v1, faces1, dt1 = run(1, n_sample_1t)
        out["value_1_thread"] = round(v1, 4)
        out["sample_1_thread"] = f"first {n_sample_1t} frames, {faces1} faces, {dt1:.1f} s at 1 thread"
    torch.set_num_threads(threads)
    out["_oracle_results"] = oracle_res   # checker results for the parity block (not part of the line)
    return out


def compare_faces(res_a, res_b, band: float = 1e-3) -> dict:
    """Face-by-face comparison of two runs over the same frames (res_b the reference; nearest
    box pairing): face-count / box / accept mismatches at the CLI threshold 0.32 and the GUI's
    0.45, the largest fd difference, and the accept flips whose reference fd lies farther than
    `band` from the threshold (a flip inside the band is the f32-class noise of any
    non-bitwise-identical path: the device f32 mode flips there against the CPU oracle too).
    Frames with res_b None (the oracle's fallback frames) are skipped."""
    n = count_mis = box_mis = acc32 = acc45 = out32 = out45 = box_int = 0
    worst = worst_same = 0.0
    near = []
    margins = []
    for a_f, b_f in zip(res_a, res_b):
        if b_f is None:
            continue
        count_mis += abs(len(a_f) - len(b_f))
        for b in b_f:
            n += 1
            a = min(a_f, key=lambda f: int(np.abs(f["bbox"].astype(np.int64) - b["bbox"]).sum())) if a_f else None
            if a is None:
                box_mis += 1
                continue
            same_box = np.array_equal(a["bbox"], b["bbox"])
            box_mis += int(not same_box)
            if not same_box and "bbox_f" in b:
                # a box that differs by one pixel in coordinates whose reference float value lies
                # next to an integer: the int() of _accumulate (face_embedder.py:2214-2239) on either
                # side of it; margin = the reference coordinate's distance to that integer
                d = np.abs(a["bbox"].astype(np.int64) - b["bbox"].astype(np.int64))
                bf = np.asarray(b["bbox_f"], np.float64)
                if d.max() == 1:
                    box_int += 1
                    margins.append(float(np.abs(bf[d == 1] - np.rint(bf[d == 1])).max()))
            fa, fb = float(a["fd"]), float(b["fd"])
            worst = max(worst, abs(fa - fb))
            if same_box:
                worst_same = max(worst_same, abs(fa - fb))
            for thr, key in ((0.32, 0), (0.45, 1)):
                if (fa <= thr) != (fb <= thr):
                    far = abs(fb - thr) > band
                    if key == 0:
                        acc32 += 1
                        out32 += far
                        near.append(round(abs(fb - thr), 5))
                    else:
                        acc45 += 1
                        out45 += far
    out = {"faces": n, "face_count_mismatch": count_mis, "box_mismatch": box_mis, "accept_mismatch_0.32": acc32,
           "accept_mismatch_0.45": acc45, f"accept_mismatch_outside_{band:g}_band": out32 + out45,
           "max_fd_diff": round(worst, 6), "max_fd_diff_same_box": round(worst_same, 6),
           "flipped_ref_distance_to_0.32": sorted(near)}
    if margins or box_int:
        out["box_mismatch_int_boundary"] = box_int
        out["box_mismatch_int_margin_px"] = round(max(margins), 6)
    return out


def hbm_kernels(fe, devs, H: int, W: int, reps: int = 20, kinds=("letterbox", "warp", "maxpool")) -> dict:
    """Achieved HBM rate of the bandwidth-bound kernels of the path, outside the
    timed region, each on the workload's own data: algorithmic bytes per launch (bytes the op
    must read + write) / average launch time (wall clock over `reps` back-to-back
    launches on the context stream, synchronised; launch overhead included), and the fraction
    of the 8 TB/s HBM3E peak. `pmc_bytes_per_dispatch`: the same kernel's FETCH_SIZE x2 +
    WRITE_SIZE per dispatch in the round's rocprofv3 pass over the bench (bench_traffic.json),
    where it ran on the bench's own launch sizes."""
    import ctypes as C
    from person_capture_amd import imageops
    from person_capture_amd._lib import PC_PREC_F16, LetterboxDesc, WarpDesc, check
    from person_capture_amd.engines import make_letterbox_desc
    from person_capture_amd.face_embedder import dev_resize
    ctx = fe._ctx
    lib, h = ctx.lib, ctx.handle
    traffic = {}
    try:
        traffic = json.load(open(os.path.join(ROOT, "bench_traffic.json"))).get("per_kernel", {})
    except Exception:
        pass

    def pmc(substr):
        for name, c in traffic.items():
            if substr in name and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                return round(2048.0 * c["FETCH_SIZE"]["mean_kib"] + 1024.0 * c["WRITE_SIZE"]["mean_kib"])
        return None

    def timed(fn):
        fn()
        ctx.sync()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        return (time.perf_counter() - t) / reps

    def entry(kernel, per_launch, nbytes, sec, what, pmc_key):
        gbps = nbytes / sec / 1e9
        return {"kernel": kernel, "launch": per_launch, "algorithmic_bytes_per_launch": int(nbytes),
                "bytes": what, "avg_launch_us": round(sec * 1e6, 2), "achieved_gbps": round(gbps, 1),
                "peak_gbps": PEAK_HBM_GBPS, "frac": round(gbps / PEAK_HBM_GBPS, 4),
                "pmc_bytes_per_dispatch": pmc(pmc_key)}

    out = {}
    n, D = min(32, len(devs)), 640
    if "resize_area" in kinds:   # the pre-scan downscale (gui_app.py:1505-1507): 4K -> 416 wide
        from person_capture_amd.face_embedder import dev_resize_batch
        k = devs[0]
        nh = int(round(k.H * (416 / float(k.W))))
        # one speculative pre-scan chunk (the driver's batch, prescan._downscale_many): every sample's
        # frame in one pc_resize_area_batch launch (row-staged kernel)
        nb = min(32, len(devs))
        keys = [f"hbm_area{i}" for i in range(nb)]
        dev_resize_batch(ctx, devs[:nb], keys, (416, nh))   # (the product call; warms the scratch buffers)
        # the launch alone, back to back: dev_resize_batch's Python side (resize plans, area tables,
        # ctypes arrays) took ~0.5 ms per call and the kernel waited on it (round 6 first form: 761 us
        # per launch = 0.13 of HBM was mostly host time)
        p = imageops.resize_plan(k.H, k.W, (416, nh), 0.0, 0.0, True)
        (xt, xs), (yt, ys) = (imageops.area_tables(k.W, p["new_w"], p["scale_x"]),
                              imageops.area_tables(k.H, p["new_h"], p["scale_y"]))
        srcs = (C.c_void_p * nb)(*[d.ptr for d in devs[:nb]])
        dsts = (C.c_void_p * nb)(*[ctx.scratch(kk, p["new_w"] * p["new_h"] * 3).ptr for kk in keys])
        sec = timed(lambda: check(lib.pc_resize_area_batch(h, srcs, dsts, nb, k.stride, xt, xs, len(xt), yt, ys, len(yt),
                                                           p["new_h"], p["new_w"]), h, "resize_area_batch"))
        out["resize_area_u8"] = entry("resize_area_rows_u8 (pc_image.hip)",
                                      f"{nb} frames {k.H}x{k.W} -> {nh}x416 INTER_AREA",
                                      nb * (k.H * k.W * 3 + nh * 416 * 3), sec, "4K frames + 416-wide outputs",
                                      "resize_area_rows")
        out["resize_area_u8"]["with_python_call_us"] = round(timed(lambda: dev_resize_batch(ctx, devs[:nb], keys, (416, nh))) * 1e6, 2)
        sec1 = timed(lambda: dev_resize(ctx, k, "hbm_area", (416, nh), 0.0, 0.0, True))
        out["resize_area_u8"]["one_frame_launch_us"] = round(sec1 * 1e6, 2)
    if "letterbox" not in kinds:
        return out
    # letterbox_blob: a 32-frame detection chunk, 1080p -> 640 f16 NHWC4 blob
    descs = (LetterboxDesc * n)(*[make_letterbox_desc(d.ptr, d.H, d.W, d.stride, D)[0] for d in devs[:n]])
    blob = ctx.scratch("hbm_letterbox", n * D * D * 4 * 2)
    sec = timed(lambda: check(lib.pc_letterbox(h, PC_PREC_F16, descs, n, D, C.c_void_p(blob.ptr)), h, "letterbox"))
    # the INTER_LINEAR resampler reads two source rows per output row: at 1080p -> 640 (scale 3) 720 of the
    # 1080 rows, whole (2 of every 3 pixels: every 64-byte line); the blob is written whole (canvas padding
    # included). r04 counted whole frames (303.9 MB per 32 frames against 237.6 MB of PMC fetch + write).
    d0 = descs[0]
    rows = set()
    for y in range(d0.new_h):
        sy = int(np.floor((y + 0.5) * d0.scale_y - 0.5))
        rows.update((min(max(sy, 0), H - 1), min(max(sy + 1, 0), H - 1)))
    out["letterbox_blob"] = entry("letterbox_blob (pc_image.hip)", f"{n} frames {H}x{W} -> {D}x{D}x4 f16",
                                  n * (len(rows) * W * 3 + D * D * 4 * 2), sec,
                                  f"the {len(rows)} source rows the bilinear taps read + the whole blob", "letterbox")
    # warp_affine_u8: one ArcFace quantum of chips (146 faces) from the 1080p frames, ~100 px faces -> 112x112
    m = 146
    chips = ctx.scratch("hbm_chips", m * 112 * 112 * 3)
    ws = []
    for i in range(m):
        d = devs[i % len(devs)]
        x0, y0 = 40 + (i * 97) % (W - 200), 40 + (i * 61) % (H - 200)
        M = np.array([[1.12, 0.05, -1.12 * x0], [-0.05, 1.12, -1.12 * y0]], np.float64)
        ws.append(imageops.warp_desc(d.ptr, d.stride, W, H, M.reshape(-1), chips.ptr + i * 112 * 112 * 3))
    warr = (WarpDesc * m)(*ws)
    sec = timed(lambda: check(lib.pc_warp_affine(h, warr, m), h, "warp_affine"))
    # source bytes: the 64-byte lines of the rows each chip's taps touch (scale 1/1.12: a ~101 x 101 px region)
    Minv = np.linalg.inv(np.vstack([M, [0, 0, 1]]))
    corners = Minv @ np.array([[0, 111, 0, 111], [0, 0, 111, 111], [1, 1, 1, 1]], np.float64)
    span_x = corners[0].max() - corners[0].min() + 2
    span_y = corners[1].max() - corners[1].min() + 2
    src_bytes = int(np.ceil(span_y)) * int(np.ceil(span_x * 3 / 64.0 + 1)) * 64
    out["warp_affine_u8"] = entry("warp_affine_u8 (pc_image.hip)", f"{m} chips 112x112 from 1080p frames",
                                  m * (112 * 112 * 3 + src_bytes), sec,
                                  "chip written + the 64-byte lines of the source region its taps touch",
                                  "warp_affine")
    # the SCRFD stem max pool (3x3/s2 over the split stem output) inside a 32-frame detection chunk:
    # its HIP-event time from the net profile, bytes from the program's tensors
    eng = fe._engine(640)
    P = eng.program
    mp = [w for w in P.ops if w[0] == 3][0]
    ti, to = P.tensors[mp[2]], P.tensors[mp[1]]
    nbytes = n * 2 * (ti[1] * ti[2] * ti[4] + to[1] * to[2] * to[4])
    eng.net.profile(True)
    for _ in range(3):
        eng.detect_frames([(d.ptr, d.H, d.W, d.stride) for d in devs[:n]], thresh=fe.conf)
    recs = [r for r in eng.net.profile_ops() if int(r[1]) == 3]
    eng.net.profile(False)
    if recs:
        sec = sum(r[2] for r in recs) * 1e-3 / len(recs)
        out["maxpool"] = entry("maxpool_split_f16x8 / maxpool_nhwc_f16x8 (pc_conv.hip)",
                               f"{n} frames {ti[1]}x{ti[2]}x{ti[3]} -> {to[1]}x{to[2]}x{to[3]} f16"
                               + (" (split hi|lo)" if P.tsplit[mp[2]] else ""), nbytes, sec,
                               "input + output activations (HIP events)", "maxpool")
    return out


_F32_REF = {}


def f16_parity(fe16, devs, bank_h, conf: float = 0.5) -> dict:
    """Outside the timed region: the same frames through an f32 FaceEmbedder (the parity mode,
    itself checked against the fp32 CPU oracle in tests/test_gpu_bench_config.py) against the
    f16 throughput mode, face by face (nearest box): how many decisions f16 changes, and where
    the difference enters. f16 is the precision of the reference's TensorRT engines
    (face_embedder.py:1058). Attribution: the f16 pass's own chips are embedded again by the
    f32 ArcFace, which separates the ArcFace error (same chip, f16 vs f32 net) from the
    detection error (SCRFD f16 landmarks -> a different aligned chip)."""
    from person_capture_amd.face_embedder import FaceEmbedder
    from person_capture_amd.match import DeviceBank

    def run(fe, bank):
        fe.debug_chips = True
        try:
            r = fe.extract_batch([None] * len(devs), dev_frames=devs, bank=bank)
        finally:
            fe.debug_chips = False
        fe._ctx.sync()
        fe._ectx.sync()
        return r

    res16 = run(fe16, DeviceBank(fe16._ctx, bank_h))
    old = {k: os.environ.get(k) for k in ("PERSON_CAPTURE_AMD_PRECISION", "PERSON_CAPTURE_AMD_DET_PRECISION",
                                          "PERSON_CAPTURE_AMD_ARC_PRECISION")}
    for k in old:
        os.environ[k] = "f32"
    try:
        # the f32 reference run of these frames / bank / threshold is made once per bench process
        key = (devs[0].ptr, len(devs), conf, float(bank_h.sum()))
        if key not in _F32_REF:
            fe32 = FaceEmbedder(ctx=f"cuda:{_device(int(os.environ.get('LOCAL_RANK', '0')))}",
                                yolo_model="scrfd_10g_bnkps", conf=conf)
            _F32_REF[key] = (fe32, run(fe32, DeviceBank(fe32._ctx, bank_h)))
        fe32, res32 = _F32_REF[key]
        chips16 = [f["chip"] for r in res16 for f in r]
        e32_on16 = fe32._arc.embed(np.stack(chips16), flip=True) if chips16 else np.zeros((0, 512), np.float32)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    fd_arc32 = iter((1.0 - e32_on16 @ bank_h.T).min(1).tolist() if len(chips16) else [])
    for r in res16:
        for f in r:
            f["fd_arc32"] = next(fd_arc32)
    n = count_mis = box_mis = acc_mis = acc_mis_45 = chip_same = arc_flip = box_half = 0
    worst_fd = worst_arc = worst_same = 0.0
    half_margin = []
    kps_d = []
    near = []
    for a16, a32 in zip(res16, res32):
        count_mis += abs(len(a16) - len(a32))
        for b in a32:
            n += 1
            a = min(a16, key=lambda f: int(np.abs(f["bbox"].astype(np.int64) - b["bbox"]).sum())) if a16 else None
            if a is None:
                box_mis += 1
                continue
            same_box = np.array_equal(a["bbox"], b["bbox"])
            if not same_box:
                box_mis += 1
                # a one-pixel box difference whose float coordinate (f32 mode) lies next to an integer:
                # the int() of _accumulate (face_embedder.py:2214-2239) on either side of it
                d = np.abs(a["bbox"].astype(np.int64) - b["bbox"].astype(np.int64))
                if d.max() == 1 and "bbox_f" in b:
                    bf = np.asarray(b["bbox_f"], np.float64)[d == 1]
                    box_half += 1
                    half_margin.append(float(np.abs(bf - np.rint(bf)).max()))
            if a["kps5"] is not None and b["kps5"] is not None:
                kps_d.append(float(np.abs(a["kps5"] - b["kps5"]).max()))
            chip_same += int(np.array_equal(a["chip"], b["chip"]))
            d = abs(float(a["fd"]) - float(b["fd"]))
            worst_fd = max(worst_fd, d)
            if same_box:
                worst_same = max(worst_same, d)
            worst_arc = max(worst_arc, abs(float(a["fd"]) - a["fd_arc32"]))
            arc_flip += (a["fd"] <= 0.32) != (a["fd_arc32"] <= 0.32)
            if (a["fd"] <= 0.32) != (b["fd"] <= 0.32):
                acc_mis += 1
                near.append(round(abs(float(b["fd"]) - 0.32), 5))
            acc_mis_45 += (a["fd"] <= 0.45) != (b["fd"] <= 0.45)
    kps_d = np.array(kps_d) if kps_d else np.zeros(1)
    far = sum(1 for d in near if d > 1e-3)
    return {"reference": "same frames, f32 parity mode on the device", "faces_f32": n, "_res32": res32,
            "_res16": res16, "accept_mismatch_0.32_outside_0.001_band": far,
            "face_count_mismatch": count_mis, "box_mismatch": box_mis, "accept_mismatch_0.32": acc_mis,
            "accept_mismatch_0.45": acc_mis_45, "accept_mismatch_frac_0.32": round(acc_mis / max(1, n), 4),
            "max_fd_diff": round(worst_fd, 6), "max_fd_diff_same_box": round(worst_same, 6),
            "box_mismatch_int_boundary": box_half,
            "box_mismatch_int_margin_px": round(max(half_margin), 6) if half_margin else None,
            "flipped_faces_f32_distance_to_0.32": sorted(near),
            "attribution": {
                "chips_identical": chip_same,
                "kps_abs_diff_px": {"median": round(float(np.median(kps_d)), 5), "max": round(float(kps_d.max()), 5)},
                "arcface_only_max_fd_diff": round(worst_arc, 6),
                "arcface_only_accept_flips_0.32": arc_flip,
                "note": "arcface_only: this mode's fd vs the f32 ArcFace on this mode's own chips; the rest of the "
                        "difference enters through the detector's landmarks (a different aligned chip; the "
                        "bench frames are u8 noise, so a sub-pixel landmark shift resamples the chip)"}}


def _save_outputs(path: str, arrays: dict) -> None:
    """--dump-outputs: one <name>.npy per array, float32 / float64."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(path, name + ".npy"), a if a.dtype == np.float32 else a.astype(np.float64))


def dump_faces(path: str, res, extra: dict = None) -> None:
    """--dump-outputs of an extract_batch result (a list of face dicts per frame): one row per face,
    the faces of a frame ordered by box, so that two builds can be compared row by row."""
    rows = [(i, f) for i, r in enumerate(res) for f in sorted(r, key=lambda f: tuple(int(v) for v in f["bbox"]))]
    out = {"faces_per_frame": np.array([len(r) for r in res], np.float64),
           "frame_index": np.array([i for i, _ in rows], np.float64),
           "bbox": np.array([f["bbox"] for _, f in rows], np.float64).reshape(len(rows), 4),
           "quality": np.array([f["quality"] for _, f in rows], np.float64),
           "feat": np.array([f["feat"] for _, f in rows], np.float32).reshape(len(rows), -1)}
    if rows and all("fd" in f for _, f in rows):
        out["fd"] = np.array([f["fd"] for _, f in rows], np.float64)
    out.update(extra or {})
    _save_outputs(path, out)


def smooth_frames(frames: np.ndarray) -> np.ndarray:
    """The bench frames low-pass filtered (Gaussian, sigma 1.5 px), contrast restored x2.5 about
    the noise mean 127.5 (camera-like images: a sub-pixel landmark shift no longer resamples the
    chip into unrelated pixels)."""
    from scipy.ndimage import gaussian_filter
    sm = np.empty_like(frames)
    for i, f in enumerate(frames):
        g = gaussian_filter(f.astype(np.float32), sigma=(1.5, 1.5, 0))
        sm[i] = np.clip(np.rint(128.0 + 2.5 * (g - 127.5)), 0, 255).astype(np.uint8)
    return sm


def smooth_parity(fe16, frames: np.ndarray, bank_rows: int) -> dict:
    """The timed-mode-vs-f32 comparison on smooth_frames(frames): u8 noise frames resample to
    unrelated chips under a sub-pixel landmark shift, smooth frames (like camera images) do not.
    Same planted-bank construction, own bank."""
    from person_capture_amd.face_embedder import _DevImage
    from person_capture_amd.match import DeviceBank
    sm = smooth_frames(frames)
    ctx = fe16._ctx
    d = ctx.alloc(sm.nbytes)
    ctx.upload(sm, d)
    fsz = sm[0].nbytes
    H, W = sm.shape[1:3]
    devs = [_DevImage(d.ptr + i * fsz, H, W, W * 3) for i in range(len(sm))]
    bank_h = synth_bank(bank_rows)
    conf0 = fe16.conf
    fe16.conf = 0.8   # the synthetic SCRFD fires on ~380 anchors of a smooth 1080p frame at 0.5, ~6 at 0.8
    try:
        first = fe16.extract_batch([None] * len(devs), dev_frames=devs, bank=DeviceBank(ctx, bank_h))
        plant_bank(first, bank_h)
        r = f16_parity(fe16, devs, bank_h, conf=0.8)
    finally:
        fe16.conf = conf0
    r.pop("flipped_faces_f32_distance_to_0.32", None)
    r.pop("_res32", None)
    r.pop("_res16", None)
    r["frames"] = "bench frames, Gaussian sigma 1.5 px, contrast x2.5 about 127.5; SCRFD conf 0.8"
    ctx.sync()
    d.free()
    return r


def _kernel_of(code: float, cfg: float) -> str:
    """Planner code of a profiled conv launch (pc_net_profile_ops) -> kernel instantiation."""
    c = int(code)
    if c == 300:
        return "conv_chain (resident IResNet block chain, pc_conv_chain.hip)"
    if c >= 600:
        return f"conv_fast C8 tile cfg {c - 600} (f16c8, pc_conv_fast.hip kFastCfgs)"
    if c == 500:
        return "conv_hx64 (halo-staged f16x3, pc_conv_hx.hip)"
    if c == 501:
        return "conv_hxg<96,96,5> (halo-staged f16x3 per 32-channel group, pc_conv_hx.hip)"
    if c == 502:
        return "conv_hxi<14,16,14,256,256,8,1> (image-resident, one 14x14 image per workgroup, pc_conv_hxi.hip)"
    if c == 503:
        return "conv_hxi<28,32,7,128,128,4,2> (image-resident, 7 rows of a 28x28 image per workgroup, pc_conv_hxi.hip)"
    if c == 505:
        return "conv_hxi<7,9,7,512,512,8,1> (image-resident, one 7x7 image per workgroup at pitch 9, pc_conv_hxi.hip)"
    if c == 504:
        return "conv_hxg<96,96,1,32,2> (small-batch form: 32 channels of a 16x4 block per workgroup, pc_conv_hx.hip)"
    if c in (506, 507, 508):
        shape = {506: "14,16,7,256,32,2,1", 507: "28,32,7,128,32,2,2", 508: "7,9,7,512,32,2,1"}[c]
        return f"conv_hxi<{shape}> (small-batch form: 32 channels of 7 rows per workgroup, pc_conv_hxi.hip)"
    if c >= 200:
        return f"conv_t2d (2-D block kernel, variant {c - 200})"
    if c >= 100:
        return f"conv_fast tile cfg {c - 100} (pc_conv_fast.hip kFastCfgs)"
    if c >= 0:
        return f"conv_halo tile {c}"
    return f"conv_igemm tile cfg {int(cfg)}"


def _net_roof(name, p_, steps, fe):
    """C3 per-net conv time and algorithmic TF/s; the f16x3 nets also with the MFMA work they
    issue (3 MFMAs per product)."""
    tf = p_["conv_flops"] / (p_["conv_ms"] * 1e-3) / 1e12 if p_["conv_ms"] > 0 else None
    r = {"conv_ms_per_step": round(p_["conv_ms"] / steps, 3), "tflops": round(tf, 1) if tf else None}
    prec = getattr(fe, "arc_precision", None) if name == "arcface" else getattr(fe, "det_precision", None)
    pn = _prec_name(prec)
    if tf:
        r.update(dtype=pn, frac=round(tf / _peak_for(pn), 4))
        if _issue_factor(pn) != 1.0:
            r.update(mfma_tflops=round(_issue_factor(pn) * tf, 1),
                     mfma_frac=round(_issue_factor(pn) * tf / _peak_for(pn), 4))
    return r


def _op_shape(P, op: int) -> str:
    """'14x14x256 <- 14x14x256 3x3/s1' of conv op `op` of program P (logical channels)."""
    w = P.ops[op]
    H, W, C = P.dims(w[1])
    segs = []
    for i in range(w[2]):
        t = w[3 + 5 * i]
        h, ww, c = P.dims(t)
        segs.append(f"{h}x{ww}x{c} {w[4 + 5 * i]}x{w[5 + 5 * i]}/s{w[6 + 5 * i]}")
    return f"{H}x{W}x{C} <- " + " + ".join(segs)


def _op_flops(P, op: int) -> float:
    """Algorithmic FLOPs per image of conv op `op` (the pc_net_create count: true channels)."""
    w = P.ops[op]
    H, W, _ = P.dims(w[1])
    cout = w[27] or w[16]
    return sum(2.0 * H * W * cout * w[4 + 5 * i] * w[5 + 5 * i] * (w[25 + i] or P.dims(w[3 + 5 * i])[2])
               for i in range(w[2]))


def _prec_name(prec) -> str:
    from person_capture_amd._lib import PC_PREC_F16C8, PC_PREC_F16X3, PC_PREC_F32
    return {PC_PREC_F32: "f32", PC_PREC_F16X3: "f16x3", PC_PREC_F16C8: "f16c8"}.get(prec, "f16")


def _peak_for(prec_name: str) -> float:
    """Dense MFMA peak a conv's ALGORITHMIC FLOPs are priced against: the f16 matrix
    rate (2.5 PF/s) for every form that runs on the f16 MFMA - f16, and the f32-class f16x3 / f16c8,
    whose extra correction MFMAs are overhead, not work - and the f32 rate for f32."""
    return PEAK_F32_TFLOPS if prec_name == "f32" else PEAK_F16_TFLOPS


def _issue_factor(prec_name: str) -> float:
    """MFMA work issued per algorithmic FLOP: f16x3 issues 3 f16 MFMAs per product;
    f16c8 2 f16 + 1 block-scaled e4m3 MFMA (of equal issue time) per 64-channel K tile where f16
    takes 2, i.e. 1.5x. `issued_mfma_frac` = frac x this: how busy the matrix pipe is."""
    return {"f16x3": 3.0, "f16c8": 1.5}.get(prec_name, 1.0)


def _dtype_label(fe) -> str:
    """Top-level dtype of a FaceEmbedder run: the arithmetic both nets compute in ("f16x3" when both
    run split), or "det/arcface" when they differ."""
    d, a = _prec_name(fe.det_precision), _prec_name(fe.arc_precision)
    return a if d == a else f"{d} (SCRFD) / {a} (ArcFace)"


def _precision_env(prec: str) -> None:
    """--precision of a FaceEmbedder workload (C3/C4/C5) -> the FaceEmbedder's variables: f16 = the
    timed mode (both nets' defaults), f32 = the parity mode, f16x3 / f16c8 = the timed mode with
    ArcFace in that form (PERSON_CAPTURE_AMD_ARC_PRECISION; the detector stays f16x3)."""
    if prec in ("f16x3", "f16c8"):
        os.environ.setdefault("PERSON_CAPTURE_AMD_PRECISION", "f16")
        os.environ.setdefault("PERSON_CAPTURE_AMD_ARC_PRECISION", prec)
    else:
        os.environ.setdefault("PERSON_CAPTURE_AMD_PRECISION", prec)


def dominant_conv(nets, names, programs=None, precisions=None) -> dict:
    """The conv kernel instantiation with the largest total HIP-event time over the timed
    region (per-launch records of every profiled net), with its algorithmic FLOPs per launch
    and average launch duration: the roofline line is this kernel's. With the nets' programs,
    `layers` names every layer that ran on it - shape, launches and rows (images) per launch,
    FLOPs per launch - so launches x FLOPs per launch reproduce the kernel's FLOPs from the
    program alone."""
    agg = {}
    ops = {}
    total = 0.0
    for j, (n, name) in enumerate(zip(nets, names)):
        for op, kind, ms, fl, code, cfg in n.profile_ops():
            if fl <= 0:
                continue
            k = (name, int(code), int(cfg) if code < 0 else -1)
            a = agg.setdefault(k, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += ms
            a[2] += fl
            total += ms
            o = ops.setdefault(k, {}).setdefault((j, int(op)), [0, 0.0, 0.0])
            o[0] += 1
            o[1] += fl
            o[2] += ms
    if not agg:
        return {"kernel": None, "code": None, "launches": 0, "avg_us": None, "flops_per_launch": None,
                "achieved_tflops": 0.0, "share": None}
    (name, code, cfg), (cnt, ms, fl) = max(agg.items(), key=lambda kv: kv[1][1])
    prec = (precisions or {}).get(name, "f16")
    label = ""
    if code == 113:
        label = (" = conv_fast<f16,256,224,64,8,1,4,1,SPLIT,SX,-,WG> (fused f16x3 split tile, 64-byte K rows, "
                 "weight fragments in registers, 8x1 waves of 32x224; ArcFace 14x14x256 layers)" if prec == "f16x3" else
                 " = conv_fast<f16,256,224,128,4,2,2,1> (ArcFace 14x14x256 layers)" if prec == "f16" else "")
    out = {"kernel": f"{_kernel_of(code, cfg)} in {name}" + label, "precision": prec, "peak_tflops": _peak_for(prec),
           "code": code, "launches": cnt, "avg_us": round(ms * 1e3 / cnt, 2), "flops_per_launch": round(fl / cnt),
           "achieved_tflops": round(fl / (ms * 1e-3) / 1e12, 2), "share": round(ms / total, 4)}
    if programs is not None:
        by_shape = {}
        for (j, op), (c, f, t) in ops[(name, code, cfg)].items():
            P = programs[j]
            if P is None:
                continue
            shp = _op_shape(P, op)
            e = by_shape.setdefault(shp, [0, 0.0, 0.0, set(), _op_flops(P, op)])
            e[0] += c
            e[1] += f
            e[2] += t
            e[3].add(op)
        out["layers"] = [{"shape": shp, "ops": len(e[3]), "launches": e[0],
                          "rows_per_launch": round(e[1] / e[0] / e[4], 2),
                          "flops_per_launch": round(e[1] / e[0]), "ms": round(e[2], 3)}
                         for shp, e in sorted(by_shape.items(), key=lambda kv: -kv[1][2])]
    return out


# conv_fast tile table (pc_conv_fast.hip kFastCfgs): cfg -> (channel tile, pixel tile)
FAST_TILES = {0: (256, 256), 1: (128, 256), 2: (256, 128), 3: (128, 128), 4: (64, 256), 5: (96, 256), 6: (64, 512),
              7: (32, 256), 8: (224, 128), 9: (128, 512), 10: (128, 256), 11: (96, 384), 12: (32, 256),
              13: (256, 224), 14: (128, 224), 15: (64, 64), 16: (64, 128), 17: (128, 64), 18: (32, 64), 19: (96, 64),
              20: (224, 64), 21: (96, 128)}


def _traffic_for(dominant, code, prec="f16"):
    """HBM bytes per launch of the rocprofv3 dominant kernel when it is the bench's dominant conv_fast
    tile: same channel x pixel tile and the same form - the template's last three flags (SPLIT, SX,
    C8) are false for f16, SX for the fused f16x3 tiles, all three for f16c8."""
    if not dominant or code is None:
        return None
    # the halo-staged kernels: one instantiation per code
    hx_names = {500: "conv_hx64", 501: "conv_hxg<96, 96", 502: "conv_hxi<14, 16, 14", 503: "conv_hxi<28, 32, 7, 128, 128",
                505: "conv_hxi<7, 9, 7, 512, 512", 504: "conv_hxg<96, 96, 1, 32", 506: "conv_hxi<14, 16, 7", 507: "conv_hxi<28, 32, 7, 128, 32",
                508: "conv_hxi<7, 9, 7, 512, 32"}
    if code in hx_names:
        return dominant.get("hbm_bytes_per_launch") if hx_names[code] in dominant.get("kernel", "") else None
    if not (100 <= code < 200 or 600 <= code < 700):
        return None
    bc, bp = FAST_TILES.get(code % 100, (0, 0))
    name = dominant.get("kernel", "")
    # template flags after OCC: SPLIT, SX, C8 [, WG]
    tail = name.split(f"Li{bc}ELi{bp}E", 1)[-1] if f"Li{bc}ELi{bp}E" in name else None
    if tail is None:
        return None
    if code >= 600:
        ok = "Lb1ELb1ELb1E" in tail
    elif prec == "f16x3":
        ok = "Lb1ELb1ELb0E" in tail
    else:
        ok = "ELb1ELb1E" not in tail
    if not ok:
        return None
    return dominant.get("hbm_bytes_per_launch")


def load_traffic():
    """HBM bytes per conv launch from the round's rocprofv3 FETCH_SIZE / WRITE_SIZE passes
    (tools/pmc_traffic.py writes bench_traffic.json at the repo root, next to this file, so
    it travels to the GPU box)."""
    tpath = os.path.join(ROOT, "bench_traffic.json")
    if not os.path.isfile(tpath):
        return None, None
    try:
        t = json.load(open(tpath))
    except Exception:
        return None, None
    return t.get("conv_hbm_bytes_per_launch"), t.get("dominant")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bank", type=int, default=32)
    ap.add_argument("--cpu-sample", type=int, default=48)
    ap.add_argument("--cpu-sample-1t", type=int, default=4)
    ap.add_argument("--c5-samples", type=int, default=1024,
                    help="C5: samples of the one clip whose positions are sharded over the ranks (strong scaling; "
                         "1024 = 128 per rank at 8 GPUs, two full speculative chunks of the default batch 64)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything beside the headline figure: the CPU baseline, the "
                         "parity passes against the device f32 mode / other precisions / the CPU oracle, the HBM rates "
                         "of the bandwidth-bound kernels, and the breakdowns that take a step of their own (C2 flip-TTA "
                         "and per-kernel split, C4 stage breakdown, the per-frame mode's profiled step). A plain run "
                         "sets up, warms up, times --steps steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned to its caller as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-parity", action="store_true",
                    help="--full: skip the f16-vs-f32 decision parity passes and the HBM rates")
    ap.add_argument("--precision", default="f16", choices=["f16", "f32", "f16x3", "f16c8"],
                    help="c3/c4/c5: f16 = the timed mode (SCRFD and ArcFace f16x3 by default, DESIGN.md §3.6-3.7), "
                         "f32 = the f32 parity mode; c2: the ArcFace program's precision (f16 = BASELINE C2's fp16, "
                         "f16x3 = the split program C3 embeds with)")
    ap.add_argument("--frames", default="resident", choices=["resident", "host", "per-frame"],
                    help="C3 frame source: resident in HBM (the headline), host arrays through extract_batch "
                         "(H2D inside the timed region), or one extract() per host frame")
    ap.add_argument("--det-size", type=int, default=640, help="C3 --frames per-frame: extract(imgsz=...)")
    ap.add_argument("--face-model", default="scrfd_10g_bnkps",
                    help="C3 FaceEmbedder detector (yolov8l-face.pt: the reference default an unchanged main.py gets)")
    ap.add_argument("--face-conf", type=float, default=0.5,
                    help="C3 SCRFD threshold (the synthetic SCRFD-10G fires on ~1000 anchors of a 1080p noise frame "
                         "at D=1408 and 0.5; 0.75 gives a handful, as at D=640 and 0.5)")
    ap.add_argument("--workload", default="c3", choices=["c2", "c3", "c4", "c5"],
                    help="c3: BASELINE configs[2] (the metric's config, default); c2: ArcFace-R100 embed only at "
                         "batch 256 (the north star's MFMA target); c4: full path with YOLOv8n "
                         "persons + per-crop SCRFD/ArcFace + CLIP ReID; c5: 4K pre-scan (INTER_AREA 416 wide, "
                         "SCRFD @384, 1 ArcFace forward, 1024-entry bank)")
    ap.add_argument("--launch-timeout", type=float, default=1500.0,
                    help="--gpus N self-launch: kill every rank if the job runs longer (seconds)")
    ap.add_argument("--fail-rank", type=int, default=-1, help=argparse.SUPPRESS)   # launcher test hook
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: exercise the rank launcher, dist init and the timing/reduction protocol only")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # --gpus N without torch.distributed.run: start N fresh rank processes (this process has not
        # touched the GPU) and exit with their status
        from person_capture_amd.shard import spawn_local_ranks
        sys.exit(spawn_local_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus,
                                   timeout=args.launch_timeout))
    if args.dry_run:
        return main_dry(args)
    if args.workload == "c2":
        return main_c2(args)
    if args.workload != "c3":
        return main_other(args)

    world, rank, local = _dist_init()
    local = _device(local)
    _precision_env(args.precision)
    os.environ.setdefault("PERSON_CAPTURE_AMD_DET_BATCH", str(args.batch))
    os.environ.setdefault("PERSON_CAPTURE_AMD_ARC_BATCH", "512")
    from person_capture_amd._lib import PC_PREC_F16C8, PC_PREC_F16X3, PC_PREC_F32
    from person_capture_amd.face_embedder import FaceEmbedder, _DevImage
    from person_capture_amd.match import DeviceBank, fd_min

    fe = FaceEmbedder(ctx=f"cuda:{local}", yolo_model=args.face_model, conf=args.face_conf)
    frames = synth_frames(rank, args.batch)
    ctx = fe._ctx
    dframes = ctx.alloc(frames.nbytes)
    ctx.upload(frames, dframes)
    fsz = frames[0].nbytes
    devs = [_DevImage(dframes.ptr + i * fsz, 1080, 1920, 1920 * 3) for i in range(args.batch)]
    bank_h = synth_bank(args.bank)
    bank = DeviceBank(ctx, bank_h)
    ctx.sync()

    host_list = list(frames)

    def step():
        if args.frames == "host":
            # caller frames in pageable host memory: pinned staging + H2D inside the timed region
            return fe.extract_batch(host_list, bank=bank)
        if args.frames == "per-frame":
            # an unchanged caller (main.py:246, gui_app.py:6045): extract() one host frame at a
            # time, fd against the bank on the host as the reference's Processor does
            out = []
            for f in host_list:
                faces = fe.extract(f, imgsz=args.det_size)
                for fc in faces:
                    fc["fd"] = fd_min(fc["feat"], bank_h)
                out.append(faces)
            return out
        return fe.extract_batch([None] * args.batch, dev_frames=devs, bank=bank)

    res = step()
    # plant a quarter of the bank with embeddings of faces the pipeline finds in these frames
    # (a reference bank is built from the target's own faces, gui_app.py:922-986) so the
    # accept path runs too; the rest stay random rows. The synthetic (untrained) embedder's
    # outputs share a large common component, so the planted rows carry 0.3 of the mean
    # removed plus noise of growing strength (as tests/test_gpu_bench_config.planted_bank):
    # the distances then straddle the CLI's 0.32 threshold instead of accepting every face.
    n_plant = plant_bank(res, bank_h)
    if n_plant:
        bank = DeviceBank(ctx, bank_h)
    for _ in range(args.warmup):
        res = step()
    nfaces = sum(len(r) for r in res)
    accept = sum(1 for r in res for f in r if f["fd"] <= 0.45)
    accept_cli = sum(1 for r in res for f in r if f["fd"] <= 0.32)
    if fe.detector_backend == "yolo":
        det_nets = [e.net for e in fe._yf_engines.values()]
        net_names = tuple(f"yolo-face{k}" for k in range(len(det_nets))) + ("arcface",)
    else:
        det_nets = [e.net for e in fe._scrfd_engines.values()] if args.frames == "per-frame" else [fe._engine(640).net]
        net_names = tuple("scrfd" if k == 0 else f"scrfd{k}" for k in range(len(det_nets))) + ("arcface",)
    nets = det_nets + [fe._arc.net]
    # the roofline's HIP events: over the timed region (a profiled run launches its ops eagerly, one event
    # per op boundary). Per-frame mode replays each frame's small runs as HIP graphs (GRAPH_BATCH), which
    # the events would turn into eager launches: its events come from one more, profiled, step after
    # the timed region instead (prof_steps 1)
    prof_timed = not os.getenv("PC_BENCH_NOPROF") and args.frames != "per-frame"
    prof_steps = args.steps if prof_timed else 1
    if prof_timed:
        for n in nets:
            n.profile(True)
    if fe.host_times is not None:
        fe.host_times.clear()
    _barrier(world)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    ctx.sync()
    t1 = time.perf_counter()
    _barrier(world)
    elapsed = _max_over_ranks(world, t1 - t0)
    if args.dump_outputs and rank == 0:
        dump_faces(args.dump_outputs, res)
    prof_after = args.full and not prof_timed and not os.getenv("PC_BENCH_NOPROF")
    if prof_after:
        for n in nets:
            n.profile(True)
        step()
        ctx.sync()
    prof = [n.profile_read() for n in nets]
    if fe.detector_backend == "yolo":
        progs = [getattr(e, "program", None) for e in fe._yf_engines.values()] + [fe._arc.program]
    else:
        progs = ([e.program for e in fe._scrfd_engines.values()] if args.frames == "per-frame"
                 else [fe._engine(640).program]) + [fe._arc.program]
    precs = {name: _prec_name(fe.arc_precision if name == "arcface" else fe.det_precision) for name in net_names}
    dom = dominant_conv(nets, net_names, progs, precs)
    for n in nets:
        n.profile(False)
    if fe.host_times is not None:
        print("host phases ms/step: " + ", ".join(f"{k} {v * 1e3 / args.steps:.2f}" for k, v in fe.host_times.items()),
              file=sys.stderr)
    conv_ms = sum(p["conv_ms"] for p in prof)
    conv_launches = sum(p["conv_launches"] for p in prof)
    conv_flops = sum(p["conv_flops"] for p in prof)
    total_frames = _sum_over_ranks(world, args.batch * args.steps)
    value = total_frames / elapsed
    achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    peak = dom.get("peak_tflops") or (PEAK_F16_TFLOPS if args.precision == "f16" else PEAK_F32_TFLOPS)
    traffic, dominant = load_traffic()
    out = {
        "metric": "frames/sec detect+embed+match @1080p, 1/2/4/8 GPU; MFMA util %",
        "value": round(value, 3),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": _dtype_label(fe),
        "data": "synthetic (seeded u8 1080p frames, seeded synthetic SCRFD-10G/IResNet-100 weights)",
        "config": {"workload": "C3: SCRFD-10G detect + ArcFace-R100 embed (flip-TTA) + cosine match vs "
                               f"{args.bank}-embedding bank, 1080p, batch {args.batch} frames per GPU",
                   "frames_per_step_per_gpu": args.batch, "det_size": args.det_size, "face_model": args.face_model, "face_conf": args.face_conf, "bank": args.bank,
                   "frames": {"resident": "resident in HBM before the timed region",
                              "host": "pageable host arrays, extract_batch: pinned staging + H2D timed",
                              "per-frame": "pageable host arrays, one extract() per frame (unchanged callers), "
                                           "host fd"}[args.frames],
                   "faces_per_frame": round(nfaces / args.batch, 3), "accepted_faces_per_step": accept,
                   "accepted_faces_per_step_cli_0.32": accept_cli, "bank_planted_rows": n_plant,
                   "detector_dtype": {PC_PREC_F32: "f32", PC_PREC_F16X3: "f16x3"}.get(fe.det_precision, "f16"),
                   "arcface_dtype": {PC_PREC_F32: "f32", PC_PREC_F16X3: "f16x3", PC_PREC_F16C8: "f16c8"}.get(
                       fe.arc_precision, "f16"),
                   "parallelism": f"frame-shard x{world} (no collective)"},
        "roofline": {"bound": "mfma", "achieved": dom["achieved_tflops"], "peak": peak, "unit": "TFLOP/s",
                     "frac": round(dom["achieved_tflops"] / peak, 4),
                     "issued_mfma_frac": round(dom["achieved_tflops"] * _issue_factor(dom.get("precision", "f16")) /
                                               peak, 4),
                     "frac_definition": "algorithmic FLOPs of the dominant kernel / its HIP-event launch time / the "
                                        "dense MFMA peak of its arithmetic (f16 MFMA 2500 TF/s for f16 and f16x3); "
                                        "issued_mfma_frac counts the 3 f16 MFMAs f16x3 issues per product",
                     "traffic": _traffic_for(dominant, dom["code"], dom.get("precision", "f16")),
                     "kernel": dom["kernel"], "kernel_launches": dom["launches"],
                     "kernel_avg_launch_us": dom["avg_us"], "kernel_flops_per_launch": dom["flops_per_launch"],
                     "kernel_share_of_conv_time": dom["share"],
                     "kernel_layers": dom.get("layers"),
                     "conv_family": {"achieved": round(achieved, 2), "frac": round(achieved / peak, 4),
                                     "traffic_mean_per_launch": traffic},
                     "launches": conv_launches, "avg_launch_us": round(conv_ms * 1e3 / max(1, conv_launches), 2),
                     "flops_per_launch": round(conv_flops / max(1, conv_launches)),
                     "conv_share_of_step": round(conv_ms / prof_steps * 1e-3 / ((t1 - t0) / args.steps), 4),
                     "streams": 2 if fe._ectx is not fe._ctx else 1,
                     "streams_note": "ArcFace (embed stream) runs beside SCRFD (detection stream): the conv "
                                     "event spans of the two overlap, so conv_share_of_step can exceed 1 and a "
                                     "launch's duration includes the co-running kernels' share of the CUs",
                     "per_net": {name: _net_roof(name, p_, prof_steps, fe) for name, p_ in zip(net_names, prof)},
                     "events": ("HIP events over the timed region" if prof_timed else
                                "HIP events of one profiled step after the timed region (its timed steps replay HIP graphs)"
                                if prof_after else "none (--full adds one profiled step after the timed region)"),
                     "traffic_unit": "HBM bytes per launch of the dominant kernel (rocprofv3 FETCH_SIZE x2 + "
                                     "WRITE_SIZE, bench_traffic.json); conv_family.traffic_mean_per_launch: the mean "
                                     "over all conv launches",
                     "dominant_kernel_rocprof": dominant},
        "cpu_baseline": None,
    }
    res32 = res16 = None
    if rank == 0 and args.full and args.precision == "f16" and not args.no_parity and args.frames == "resident" and \
            fe.detector_backend == "scrfd":
        out["parity"] = f16_parity(fe, devs, bank_h)
        res32, res16 = out["parity"].pop("_res32"), out["parity"].pop("_res16")
        out["parity"]["timed_mode"] = "SCRFD " + out["config"]["detector_dtype"] + " + ArcFace " + \
            out["config"]["arcface_dtype"]

        # the same pipeline with the nets in other precisions: their throughput and decisions
        # (detector f32: the f32 SCRFD kernels, chips identical to the f32 mode's; ArcFace f16: the
        # round-4 timed mode, the reference's TensorRT precision, fd within ~2e-4 only; both f16: the
        # round-3 headline, whose sub-pixel landmark shifts flip decisions on noise frames)
        def alt_mode(env):
            olds = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                fe_d = FaceEmbedder(ctx=f"cuda:{local}", yolo_model="scrfd_10g_bnkps", conf=0.5)
            finally:
                for k, v in olds.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            run_d = lambda: fe_d.extract_batch([None] * args.batch, dev_frames=devs, bank=bank)
            run_d()
            fe_d._ctx.sync()
            t0 = time.perf_counter()
            for _ in range(3):
                run_d()
            fe_d._ctx.sync()
            fe_d._ectx.sync()
            fps_d = 3 * args.batch / (time.perf_counter() - t0)
            pd = f16_parity(fe_d, devs, bank_h)
            return {"frames_per_s": round(fps_d, 2), "steps": 3,
                    **{k: pd[k] for k in ("face_count_mismatch", "box_mismatch", "accept_mismatch_0.32",
                                          "accept_mismatch_0.45", "accept_mismatch_frac_0.32", "max_fd_diff",
                                          "accept_mismatch_0.32_outside_0.001_band")},
                    "chips_identical": pd["attribution"]["chips_identical"]}

        out["parity"]["detector_f32_mode"] = dict(alt_mode({"PERSON_CAPTURE_AMD_DET_PRECISION": "f32"}), note=(
            "SCRFD f32 + the timed mode's ArcFace (PERSON_CAPTURE_AMD_DET_PRECISION=f32): the f32 mode's SCRFD "
            "kernels, identical chips"))
        out["parity"]["arcface_f16_mode"] = dict(alt_mode({"PERSON_CAPTURE_AMD_ARC_PRECISION": "f16"}), note=(
            "the timed mode's SCRFD + plain f16 ArcFace (PERSON_CAPTURE_AMD_ARC_PRECISION=f16, round 4's timed mode: "
            "the reference's TensorRT fp16 precision; its fd moves ~2e-4 on identical chips)"))
        out["parity"]["trt_f16_mode"] = dict(alt_mode({"PERSON_CAPTURE_AMD_DET_PRECISION": "f16",
                                                       "PERSON_CAPTURE_AMD_ARC_PRECISION": "f16"}), note=(
            "plain f16 SCRFD + plain f16 ArcFace (round 3's headline): sub-pixel landmark shifts resample noise chips"))
        out["parity"]["timed_mode_speedup_vs_detector_f32_mode"] = round(
            value / out["parity"]["detector_f32_mode"]["frames_per_s"], 3)
        out["parity"]["smooth_frames"] = smooth_parity(fe, frames, args.bank)
    if rank == 0 and args.full and args.frames == "resident" and not args.no_parity:
        out["hbm"] = hbm_kernels(fe, devs, 1080, 1920)
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(frames, fe, bank_h, args.cpu_sample, args.cpu_sample_1t)
        oracle_res = out["cpu_baseline"].pop("_oracle_results")
        if res16 is not None:
            # the north star's reference: the CPU path itself (oracle port, fp32 torch SCRFD + ArcFace,
            # 0-degree frames) on the sample frames, against the timed mode and the device f32 mode
            out["parity"]["cpu_oracle"] = {
                "frames": len(oracle_res), "frames_needing_fallback_skipped": sum(r is None for r in oracle_res),
                "timed_mode": compare_faces(res16[:len(oracle_res)], oracle_res),
                "device_f32_mode": compare_faces(res32[:len(oracle_res)], oracle_res),
                "note": "the oracle (oracle/pipeline.extract_frame) is the checker here; both device modes are "
                        "compared with it face by face (nearest box)"}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def _timed(world, ctx, steps, step):
    _barrier(world)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    t1 = time.perf_counter()
    _barrier(world)
    return _max_over_ranks(world, t1 - t0), t1 - t0


def main_c2(args):
    """C2 (BASELINE configs[1]): ArcFace-R100 embed only, batch 256 aligned 112x112 faces, f16,
    one GPU per rank. One step = pc_arcface_embed over 256 device-resident u8 chips (preprocess
    -> IResNet-100 -> L2) without flip, i.e. 256 forward rows: the batch the north star's
    '>= 50 % MFMA at batch 256' is quoted on. The flip-TTA form the reference's
    _arcface_encode runs (face_embedder.py:1290-1389: 256 faces = 512 rows) is timed beside it
    (flip_tta). roofline: the whole network's algorithmic FLOPs / step time (all of its MFMA
    work), plus the dominant kernel's own launch rate."""
    world, rank, local = _dist_init()
    local = _device(local)
    from person_capture_amd import models
    from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F16C8, PC_PREC_F16X3, PC_PREC_F32
    from person_capture_amd.engines import ArcFaceEngine
    from person_capture_amd.runtime import GpuContext
    B = 256
    ctx = GpuContext(local)
    prec = {"f16": PC_PREC_F16, "f16x3": PC_PREC_F16X3, "f16c8": PC_PREC_F16C8}.get(args.precision, PC_PREC_F32)
    arc_params = models.synth_iresnet(100, seed=0)
    eng = ArcFaceEngine(ctx, arc_params, 100, precision=prec, max_batch=2 * B)
    chips = np.random.default_rng(20260505 + rank).integers(0, 256, (B, 112, 112, 3), dtype=np.uint8)
    d_chips = ctx.upload(chips)
    d_out = ctx.alloc(B * eng.dim * 4)
    for _ in range(max(1, args.warmup)):
        eng.embed_device(d_chips.ptr, B, False, d_out.ptr)
        if args.full:
            eng.embed_device(d_chips.ptr, B, True, d_out.ptr)
    ctx.sync()
    elapsed, _ = _timed(world, ctx, args.steps, lambda: eng.embed_device(d_chips.ptr, B, False, d_out.ptr))
    if args.dump_outputs and rank == 0:
        _save_outputs(args.dump_outputs, {"embeddings": ctx.download(d_out.ptr, (B, eng.dim), np.float32)})
    dom, recs, t_flip = None, [], None
    if args.full:
        t_flip, _ = _timed(world, ctx, args.steps, lambda: eng.embed_device(d_chips.ptr, B, True, d_out.ptr))
        # per-launch split of one profiled step (HIP events on the net's stream)
        eng.net.profile(True)
        eng.embed_device(d_chips.ptr, B, False, d_out.ptr)
        dom = dominant_conv([eng.net], ("arcface",), [eng.program], {"arcface": args.precision})
        recs = eng.net.profile_ops()
        eng.net.profile(False)
    # algorithmic FLOPs over the dense f16 peak for every f16-MFMA form (f16x3 / f16c8 issue 3x / 1.5x
    # that work: issued_mfma_frac)
    peak = _peak_for(args.precision)
    fl = eng.flops_per_forward * B
    ms = elapsed / args.steps * 1e3
    net_tf = fl / (ms * 1e-3) / 1e12
    split = {}
    for op, kind, t, f, code, cfg in recs:
        k = _kernel_of(code, cfg) if f > 0 else "other"
        a = split.setdefault(k, [0, 0.0, 0.0])
        a[0] += 1; a[1] += t; a[2] += f
    total_faces = _sum_over_ranks(world, B * args.steps)
    out = {
        "metric": "ArcFace-R100 embeddings/sec at batch 256 (C2); MFMA util %",
        "value": round(total_faces / elapsed, 2), "unit": "faces/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.precision,
        "data": "synthetic (seeded u8 112x112 chips, seeded synthetic IResNet-100 weights)",
        "config": {"workload": "C2: ArcFace-R100 embed only, batch 256 aligned 112x112 faces (256 forward rows), "
                               "preprocess + IResNet-100 + L2 on device", "batch": B,
                   "parallelism": f"replica x{world} (no collective)"},
        "roofline": {"bound": "mfma", "achieved": round(net_tf, 2), "peak": peak, "unit": "TFLOP/s",
                     "frac": round(net_tf / peak, 4), "traffic": None,
                     "issued_mfma_frac": round(net_tf * _issue_factor(args.precision) / peak, 4),
                     "scope": "whole IResNet-100 forward: algorithmic conv FLOPs of 256 rows / step time "
                              f"({fl / 1e12:.3f} TFLOP per step)",
                     "dominant_kernel": dom,
                     "per_kernel": {k: {"launches": v[0], "ms": round(v[1], 4),
                                        "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1) if v[1] > 0 and v[2] > 0
                                        else None} for k, v in sorted(split.items(), key=lambda kv: -kv[1][1])}},
        "flip_tta": None,
        "cpu_baseline": None,
    }
    if args.full:
        out["flip_tta"] = {"faces_per_step": B, "rows": 2 * B, "ms_per_step": round(t_flip / args.steps * 1e3, 4),
                           "faces_per_s": round(_sum_over_ranks(world, B * args.steps) / t_flip, 2),
                           "tflops": round(2 * fl / (t_flip / args.steps) / 1e12, 2)}
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline_c2(arc_params, chips, 16)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def main_dry(args):
    """The multi-rank protocol without a GPU (CPU test of the launcher): every rank
    'processes' its contiguous share of a batch with a host stand-in, then the same
    barrier / max-over-ranks time / sum-over-ranks frames reduction as the real run."""
    from person_capture_amd.shard import shard_indices
    if args.fail_rank >= 0 and int(os.environ.get("RANK", "0")) == args.fail_rank:
        sys.exit(1)   # launcher test: this rank dies before the rendezvous
    world, rank, local = _dist_init()
    total = args.batch * max(1, world)
    mine = shard_indices(total, rank, world)
    _barrier(world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sum(i * i for i in mine)
    t1 = time.perf_counter()
    _barrier(world)
    elapsed = max(_max_over_ranks(world, t1 - t0), 1e-9)
    frames = _sum_over_ranks(world, len(mine) * args.steps)
    if rank == 0:
        print(json.dumps({"metric": "dry-run", "value": frames / elapsed, "unit": "frames/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "frames": frames, "local_rank": local}),
              flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def main_other(args):
    """C4 (full path) and C5 (4K pre-scan of one clip, sharded over the ranks): secondary
    workloads, same JSON contract."""
    world, rank, local = _dist_init()
    local = _device(local)
    _precision_env(args.precision)
    os.environ.setdefault("PERSON_CAPTURE_AMD_DET_BATCH", str(args.batch))
    os.environ.setdefault("PERSON_CAPTURE_AMD_ARC_BATCH", "512")
    from person_capture_amd.face_embedder import FaceEmbedder, _DevImage
    from person_capture_amd.match import DeviceBank

    fe = FaceEmbedder(ctx=f"cuda:{local}", yolo_model="scrfd_10g_bnkps", conf=0.5)
    ctx = fe._ctx
    c4 = args.workload == "c4"
    H, W = (1080, 1920) if c4 else (2160, 3840)
    # C5: every rank holds the same clip (one clip sharded over the ranks); C4: per-rank frames
    frames = synth_frames(rank if c4 else 0, args.batch, H, W)
    dframes = ctx.alloc(frames.nbytes)
    ctx.upload(frames, dframes)
    fsz = frames[0].nbytes
    devs = [_DevImage(dframes.ptr + i * fsz, H, W, W * 3) for i in range(args.batch)]
    bank_n = args.bank if c4 else 1024
    bank_h = synth_bank(bank_n)
    bank = DeviceBank(ctx, bank_h)
    stats = {}
    last = {}   # what the last step returned (--dump-outputs)
    nets = [fe._arc.net]
    units_per_step = args.batch
    scaling = "weak"
    if c4:
        from person_capture_amd.detectors import PersonDetector
        from person_capture_amd.reid_embedder import ReIDEmbedder
        det = PersonDetector("yolov8n.pt", device=f"cuda:{local}")
        reid = ReIDEmbedder(device=f"cuda:{local}")
        stats["reid_dtype"] = "f32" if reid._engine.net.precision == 1 else "f16"
        dtuples = [(d.ptr, H, W, W * 3) for d in devs]

        def person_crops():
            crops = []
            for d, dets in zip(devs, det.detect_device(dtuples, conf=0.35)):
                for x1, y1, x2, y2, _ in dets:   # main.py:231-236
                    x1, y1 = max(0, int(x1)), max(0, int(y1))
                    x2, y2 = min(W - 1, int(x2)), min(H - 1, int(y2))
                    if x2 <= x1 + 2 or y2 <= y1 + 2:
                        continue
                    crops.append(_DevImage(d.ptr + y1 * d.stride + x1 * 3, y2 - y1, x2 - x1, d.stride))
            return crops

        # The untrained synthetic SCRFD fires on many anchors of a bilinearly upscaled person crop
        # (its face prior was calibrated on native-scale frames). A trained detector finds the 1-2
        # faces a person crop holds. The threshold is no knob for this: a crop whose 0-degree pass
        # keeps nothing goes to the rotation / upscale fallbacks, which detect at 0.6-0.8 x the
        # threshold at larger sizes (face_embedder.py:2330-2420), so the face count is not
        # monotonic in it (r04: 38-504 faces per crop over thresholds 0.5-0.999). Instead the
        # synthetic SCRFD's face prior - the score heads' bias, which moves every pass's logits
        # alike - is calibrated once, before timing, by bisection on a 48-crop sample through the
        # timed path itself (extract_batch at the reference threshold 0.5) to 1-4 faces per crop,
        # one line per pass. Real weights need no knob.
        crops0 = person_crops()
        sample = crops0[:48]
        fe.conf = 0.5
        keys = [k for k in fe._scrfd_params if k.endswith(".cls.bias")]
        base = {k: np.array(fe._scrfd_params[k], np.float32).copy() for k in keys}

        def faces_per_crop(shift):
            for k in keys:
                fe._scrfd_params[k] = base[k] + np.float32(shift)
            for e in fe._scrfd_engines.values():
                e.net.close()
            fe._scrfd_engines.clear()
            t = time.perf_counter()
            got = fe.extract_batch([None] * len(sample), dev_frames=sample)
            v = sum(len(f) for f in got) / max(1, len(sample))
            print(f"[bench c4] face prior shift {shift:+.3f}: {v:.2f} faces per crop on {len(sample)} crops "
                  f"({time.perf_counter() - t:.1f} s)", file=sys.stderr, flush=True)
            return v
        lo, hi = -12.0, 0.0      # logit shifts: hi too many faces, lo too few
        shift, fpc = hi, faces_per_crop(hi)
        if fpc > 4:
            for _ in range(8):
                mid = (lo + hi) / 2
                v = faces_per_crop(mid)
                shift, fpc = mid, v
                if 1.0 <= v <= 4.0:
                    break
                if v > 4.0:
                    hi = mid
                else:
                    lo = mid
        conf_used = fe.conf
        print(f"[bench c4] {len(crops0)} person crops; face prior shifted by {shift:+.3f} "
              f"({fpc:.2f} faces per crop on the sample, threshold {conf_used})", file=sys.stderr, flush=True)
        stats["face_prior_logit_shift"] = round(shift, 4)
        stats["face_conf_calibrated"] = conf_used

        def step(phases=None):
            # phases (diagnostic pass outside the timed region): wall ms of each stage with the device
            # drained between them, and the FaceEmbedder's host phase times of its extract_batch
            def mark(key):
                if phases is not None:
                    ctx.sync()
                    fe._ectx.sync()
                    reid._ctx.sync()
                    t = time.perf_counter()
                    phases[key] = round((t - phases.pop("_t")) * 1e3, 3)
                    phases["_t"] = t
            if phases is not None:
                ctx.sync()
                phases["_t"] = time.perf_counter()
            crops = person_crops()
            mark("persons_yolo_ms")
            faces = fe.extract_batch([None] * len(crops), dev_frames=crops, bank=bank) if crops else []
            mark("faces_extract_batch_ms")
            feats = reid.extract_device([(c.ptr, c.H, c.W, c.stride) for c in crops])
            mark("reid_ms")
            stats["persons"] = len(crops)
            stats["faces"] = sum(len(f) for f in faces)
            stats["faces_per_crop"] = round(stats["faces"] / max(1, len(crops)), 3)
            last["faces"] = faces
            return feats
        nets += [fe._engine(640).net, reid._engine.net]
        wl = (f"C4: YOLOv8n persons + SCRFD-10G@640 per person crop + ArcFace-R100 flip-TTA + CLIP ViT-L/14 ReID "
              f"per crop + match vs {bank_n}-embedding bank, 1080p, batch {args.batch} frames per GPU")
    else:
        # the pre-scan driver (Processor._prescan's sampling loop) over ONE clip of c5_samples samples at
        # stride 24 (gui_app.py:555), the clip's sample positions sharded over the ranks
        # (prescan_shard.run_sharded: speculation per rank, rank-0 replay with re-extraction of
        # misses, the single-stream spans and bank): strong scaling. The resident 4K frames are the
        # clip's sampled frames (cycled), downscaled to 416 wide on the device.
        from person_capture_amd.prescan import PrescanConfig, PrescanRunner
        from person_capture_amd.prescan_shard import run_sharded
        pcfg = PrescanConfig()
        stride = pcfg.prescan_stride
        S = args.c5_samples
        units_per_step = S
        scaling = "strong"
        total = S * stride
        at = lambda idx: devs[(idx // stride) % len(devs)]
        # plant a quarter of the bank from faces of the first samples (downscaled as the driver
        # does) so spans open and the escalated two-forward path is timed too
        r0 = PrescanRunner(fe, pcfg, 30.0, total, ref_feat=None, batch=args.batch)
        ims = [r0._downscale(devs[i], i) for i in range(min(16, len(devs)))]
        fe.set_prescan_fast(True, mode="rr")
        seed_res = fe.extract_batch([None] * len(ims), dev_frames=ims)
        fe.set_prescan_fast(False)
        stats["bank_planted_rows"] = plant_bank(seed_res, bank_h)

        def step():
            r = run_sharded(fe, pcfg, 30.0, total, at, ref_feat=bank_h, batch=args.batch, rank=rank, world=world)
            if r is not None:
                spans, _, recs, ms = r
                stats["faces"] = sum(x.n_faces for x in recs)
                stats["extracted_samples"] = sum(1 for x in recs if x.extracted)
                stats["spans"] = len(spans)
                # the serial part of a sharded clip: rank 0's replay (host logic over every sample) and
                # its batched chunks for speculation misses
                stats["merge"] = {"reused": ms.reused, "misses": ms.misses, "rank0_chunks": ms.rechunks,
                                  "reextracted_on_rank0": ms.reextracted, "served_by_rank0_chunks": ms.from_rechunks,
                                  "skipped": ms.skipped, "speculated_per_rank": ms.per_rank_spec,
                                  "merge_serial_ms": round(ms.merge_s * 1e3, 2)}
            return r
        wl = (f"C5: pre-scan of one clip of {S} samples at stride {stride} (4K frames -> INTER_AREA 416 wide, "
              f"fast pre-scan SCRFD-10G, ArcFace-R100 1 forward / 2 while a span is active, fd vs a {bank_n}-embedding "
              f"bank, bank growth and span hysteresis), sample positions sharded over {world} rank(s) with the "
              f"single-stream result (rank-0 replay)")
    for k in range(args.warmup):
        t = time.perf_counter()
        step()
        ctx.sync()
        print(f"[bench {args.workload}] warmup {k}: {time.perf_counter() - t:.3f} s {stats}", file=sys.stderr,
              flush=True)
    if not c4:
        nets += [e.net for e in fe._scrfd_engines.values()]
    for n in nets:
        n.profile(True)
    def timed_step():
        last["out"] = step()
    elapsed, local_dt = _timed(world, ctx, args.steps, timed_step)
    if args.dump_outputs and rank == 0:
        if c4:
            dump_faces(args.dump_outputs, last["faces"], {"reid_feat": np.asarray(last["out"], np.float32)})
        else:
            spans, grown, recs, _ = last["out"]
            _save_outputs(args.dump_outputs, {
                "spans": np.asarray(spans, np.float64).reshape(-1, 2),
                "bank": np.asarray(grown, np.float32),
                "records": np.array([[x.idx, x.extracted, x.best, x.n_faces, x.active] for x in recs], np.float64)})
    prof = [n.profile_read() for n in nets]
    for n in nets:
        n.profile(False)
    if c4 and args.full:
        # where a C4 step goes: one more step, stage by stage with the device drained
        # between stages (so the stages do not overlap here as they may in the timed steps), with the
        # FaceEmbedder's host phase timers on
        phases = {}
        fe.host_times = {}
        fe.fb_stats[:] = [0, 0]
        fe.fb_kind_stats.clear()
        fe.spec_stats[:] = [0, 0]
        n_eng = len(fe._scrfd_engines)
        step(phases)
        stats["face_pass_counts_one_step"] = {
            "zero_degree_speculative_hit_rerun": list(fe.spec_stats),
            "fallback_prefetched_inline": list(fe.fb_stats),
            "fallback_by_kind_prefetched_inline": {k: list(v) for k, v in fe.fb_kind_stats.items()},
            "scrfd_det_sizes": sorted(fe._scrfd_engines), "scrfd_engines_created_in_step": len(fe._scrfd_engines) - n_eng}
        phases.pop("_t", None)
        stats["phase_ms_one_step"] = phases
        stats["face_host_phase_ms_one_step"] = {k: round(v * 1e3, 3) for k, v in fe.host_times.items()}
        fe.host_times = None
    conv_ms = sum(p["conv_ms"] for p in prof)
    conv_flops = sum(p["conv_flops"] for p in prof)
    conv_launches = sum(p["conv_launches"] for p in prof)
    achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    # per-net roofline at its own dtype's peak (the ReID tower runs f32 like the reference: 157 TF/s)
    names = ["arcface"] + (["scrfd", "reid"] if c4 else [f"scrfd{i}" for i in range(len(nets) - 1)])
    per_net = {}
    for nm, n, p_ in zip(names, nets, prof):
        if p_["conv_ms"] <= 0:
            continue
        f32 = n.precision == 1
        tf = p_["conv_flops"] / (p_["conv_ms"] * 1e-3) / 1e12
        pn = "f32" if f32 else _prec_name(fe.arc_precision if nm == "arcface" else
                                           getattr(fe, "det_precision", None) if nm.startswith("scrfd") else None)
        pk = _peak_for(pn)
        per_net[nm] = {"dtype": pn, "conv_ms_per_step": round(p_["conv_ms"] / args.steps, 3),
                       "achieved_tflops": round(tf, 1), "peak": round(pk, 1), "frac": round(tf / pk, 4)}
        if _issue_factor(pn) != 1.0:   # algorithmic FLOPs above; MFMA work issued
            per_net[nm].update(mfma_tflops=round(_issue_factor(pn) * tf, 1),
                               mfma_frac=round(_issue_factor(pn) * tf / pk, 4))
    peak = _peak_for(args.precision)
    total_units = units_per_step * args.steps if scaling == "strong" else _sum_over_ranks(world, units_per_step *
                                                                                           args.steps)
    out = {
        "metric": "frames/sec detect+embed+match @1080p, 1/2/4/8 GPU; MFMA util %" if c4
        else "frames/sec pre-scan detect+embed+match @4K, 1/2/4/8 GPU; MFMA util %",
        "value": round(total_units / elapsed, 3), "unit": "frames/s" if c4 else "samples/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": _dtype_label(fe),
        "data": "synthetic (seeded u8 frames, seeded synthetic weights of every net)",
        "config": {"workload": wl, ("frames_per_step_per_gpu" if c4 else "samples_per_clip"): units_per_step,
                   "bank": bank_n, **{k: v for k, v in stats.items()},
                   "parallelism": f"frame-shard x{world} (no collective)" if c4 else
                   f"sample-position shard x{world}, host gather + rank-0 replay (no device collective)"},
        "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                     "frac": round(achieved / peak, 4), "traffic": None,
                     "kernel": "implicit-GEMM MFMA convs (all nets, ViT linears as 1x1)", "launches": conv_launches,
                     "avg_launch_us": round(conv_ms * 1e3 / max(1, conv_launches), 2),
                     "conv_share_of_step": round(conv_ms * 1e-3 / local_dt, 4), "per_net": per_net},
        "cpu_baseline": None,
    }
    if rank == 0 and not c4 and args.full and not args.no_parity:
        out["hbm"] = hbm_kernels(fe, devs, H, W, kinds=("resize_area",))
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        print(f"[bench {args.workload}] CPU baseline (oracle port) ...", file=sys.stderr, flush=True)
        out["cpu_baseline"] = cpu_baseline_c4(frames, fe, det, bank_h) if c4 else \
            cpu_baseline_c5(frames, fe, bank_h, stride)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def cpu_baseline_c2(params, chips: np.ndarray, n: int) -> dict:
    """The oracle's fp32 torch-CPU IResNet-100 (+ L2) on a bounded sample of the C2 chips."""
    import torch
    from oracle import nets_torch as nt
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    x = nt.arcface_input_from_chips(chips[:n])
    t0 = time.perf_counter()
    with torch.no_grad():
        nt.iresnet_forward(params, 100, x)
    dt = time.perf_counter() - t0
    return {"value": round(n / dt, 3), "unit": "faces/s", "cores": threads, "kind": "port",
            "host_cpu_count": os.cpu_count(),
            "sample": f"{n} of the C2 chips through oracle/nets_torch.iresnet_forward (fp32 torch CPU, one batch), "
                      f"{dt:.1f} s at {threads} threads"}


def cpu_baseline_c4(frames: np.ndarray, fe, det, bank: np.ndarray, max_crops: int = 4) -> dict:
    """The oracle chain of C4 on the host cores for one frame: YOLOv8n person heads + postprocess,
    the person crops' SCRFD + ArcFace branch (OracleFaceEmbedder, same calibrated threshold),
    ViT-L/14 ReID of each crop, fd against the bank. Bounded sample: the frame's first crops."""
    import torch
    from oracle import nets_torch as nt
    from oracle import pipeline as op
    from oracle import ref_algos as ra
    from person_capture_amd.reid_embedder import clip_weights
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    frame = frames[0]
    H, W = frame.shape[:2]
    o = op.OracleFaceEmbedder(fe._scrfd_params, fe.scrfd_variant, fe._arc_params, fe._arc_depth, conf=fe.conf)
    cw = clip_weights("ViT-L-14", 0)
    t0 = time.perf_counter()
    with torch.no_grad():
        canvas, (_, _, _, _, Hp, Wp) = ra.yolo_letterbox(frame)
        x = torch.from_numpy(np.ascontiguousarray(canvas[None].transpose(0, 3, 1, 2)))
        heads = [t[0].numpy() for t in nt.yolov8_forward(det._params, "n", x)]
        persons = ra.yolo_postprocess(heads, 0.35, 0.45, 40, Hp, Wp, H, W)
        crops = []
        for p in persons:
            x1, y1 = max(0, int(p[0])), max(0, int(p[1]))
            x2, y2 = min(W - 1, int(p[2])), min(H - 1, int(p[3]))
            if x2 > x1 + 2 and y2 > y1 + 2:
                crops.append(frame[y1:y2, x1:x2])
        crops = crops[:max_crops]
        faces = 0
        for c in crops:
            for f in o.extract(c):
                ra.fd_min(f["feat"], bank)
                faces += 1
        if crops:
            nt.clip_vit_forward(cw, "ViT-L-14", torch.stack([nt.clip_preprocess_pil(c) for c in crops]))
    dt = time.perf_counter() - t0
    per_frame = dt / max(1, len(crops)) * max(1, len(persons))   # scaled to all of the frame's persons
    return {"value": round(1.0 / per_frame, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "host_cpu_count": os.cpu_count(),
            "sample": f"frame 0: YOLOv8n oracle + {len(crops)} of its {len(persons)} person crops (SCRFD-10G + "
                      f"ArcFace-R100 oracle branch, {faces} faces; ViT-L/14 fp32) in {dt:.1f} s at {threads} threads, "
                      f"scaled to the frame's {len(persons)} crops"}


def cpu_baseline_c5(frames: np.ndarray, fe, bank: np.ndarray, stride: int, n: int = 6) -> dict:
    """The oracle pre-scan loop (oracle/prescan.prescan over OracleFaceEmbedder: INTER_AREA to 416,
    fast pre-scan SCRFD + ArcFace, bank, hysteresis) on the host cores, a bounded clip of n samples."""
    import torch
    from oracle import pipeline as op
    from oracle import prescan as oprescan
    from person_capture_amd.prescan import PrescanConfig
    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    o = op.OracleFaceEmbedder(fe._scrfd_params, fe.scrfd_variant, fe._arc_params, fe._arc_depth, conf=0.5)
    t0 = time.perf_counter()
    _, _, recs = oprescan.prescan(o, PrescanConfig(), 30.0, n * stride, lambda idx: frames[(idx // stride) % len(frames)],
                                  ref_feat=bank)
    dt = time.perf_counter() - t0
    return {"value": round(n / dt, 4), "unit": "samples/s", "cores": threads, "kind": "port",
            "host_cpu_count": os.cpu_count(),
            "sample": f"a {n}-sample clip of the bench's 4K frames through oracle/prescan.prescan "
                      f"({sum(1 for r in recs if r[1])} extracted, {sum(r[3] for r in recs)} faces), {dt:.1f} s at "
                      f"{threads} threads"}


if __name__ == "__main__":
    main()
