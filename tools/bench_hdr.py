#!/usr/bin/env python3
"""HDR input measurements, written to profiles/hdr_bench.json. For 1920 x 1080 and
3840 x 2160, PQ and HLG:

  kernel   pc_hdr_to_bgr of one frame resident in HBM (planar, aligned), timed by HIP events around R
           launches back to back on the context's stream;
  stage    frames_hdr.stage_hdr of the same host frame (pinned ring in row blocks + H2D), wall clock with the
           stream synchronised inside;
  cpu      the reference's own _eotf_pq / _eotf_hlg + _python_tonemap_to_bgr8 on that frame on this host,
           lifted from <reference root>/person_capture/video_io.py by AST as tools/gen_golden_hdr.py lifts
           them (skipped without --reference), and this package's NumPy backend.
Warm-up, repeated runs, medians with min and max. The comparison that matters is kernel against stage: the
conversion should hide behind the frame's own upload. Needs a GPU (there is no fallback), except with
--cpu-only, which records the cpu columns alone on the host that holds the reference."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from person_capture_amd import frames_hdr  # noqa: E402
from person_capture_amd.runtime import GpuContext  # noqa: E402


def stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "runs": len(ts)}


def signal(seed, H, W, transfer):
    rng = np.random.default_rng(seed)
    lo, hi = (0.0, 0.75) if transfer == "hlg" else (0.1, 0.85)   # HLG: both branches of the EOTF
    return np.float32(lo) + np.float32(hi - lo) * rng.random(3 * H * W, dtype=np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference snapshot (for the CPU column)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--cpu-only", action="store_true", help="only the CPU columns (a host without a GPU)")
    ap.add_argument("--out", default=os.path.join("profiles", "hdr_bench.json"))
    a = ap.parse_args()
    if not a.cpu_only:
        import torch
        ctx = GpuContext(0)
        stream = torch.cuda.ExternalStream(ctx.stream)
    R = None
    if a.reference:
        import gen_golden_hdr
        R = gen_golden_hdr.reference_functions(a.reference)
    out = {"device": None if a.cpu_only else torch.cuda.get_device_name(0), "numpy": np.__version__,
           "host_cpus": os.cpu_count()}
    for res, H, W in (("1080p", 1080, 1920), ("4k", 2160, 3840)):
        for tr in ("pq", "hlg"):
            raw = signal(H + len(tr), H, W, tr)
            f = frames_hdr.HdrFrame(raw, H, W, tr, 200.0, 1000.0)
            rec, got = {}, None
            if not a.cpu_only:
                src = ctx.alloc(f.packed_bytes)
                dst = ctx.alloc(H * W * 3)
                dev = frames_hdr.stage_hdr(ctx, f, src.ptr)
                job = [dev.job(dst.ptr)]
                for _ in range(a.warmup):
                    frames_hdr.convert_on_device(ctx, job)
                ctx.sync()
                tk = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.inner):
                        frames_hdr.convert_on_device(ctx, job)
                    e1.record(stream)
                    e1.synchronize()
                    tk.append(e0.elapsed_time(e1) / 1e3 / a.inner)
                ts = []
                for i in range(a.warmup + a.reps):
                    ctx.sync()
                    t0 = time.perf_counter()
                    frames_hdr.stage_hdr(ctx, f, src.ptr)
                    ctx.sync()
                    if i >= a.warmup:
                        ts.append(time.perf_counter() - t0)
                rec = {"kernel": stats(tk), "stage": stats(ts), "source_bytes": f.packed_bytes,
                       "stage_gb_per_s": f.packed_bytes / statistics.median(ts) / 1e9,
                       "kernel_over_stage": statistics.median(tk) / statistics.median(ts),
                       "mpix_per_s_kernel": H * W / statistics.median(tk) / 1e6}
                got = ctx.download(dst.ptr, (H, W, 3), np.uint8)
            tn = []
            for _ in range(a.cpu_reps):
                t0 = time.perf_counter()
                twin = frames_hdr.hdr_to_bgr(f)
                tn.append(time.perf_counter() - t0)
            rec["numpy_backend"] = stats(tn)
            if got is None:
                got = twin
            else:
                rec["device_equals_numpy_backend"] = bool(np.array_equal(got, twin))
            if R is not None:
                planar = raw.reshape(3, H, W)
                tc = []
                for _ in range(a.cpu_reps):
                    t0 = time.perf_counter()
                    rgb = np.stack((planar[2], planar[0], planar[1]), axis=-1)
                    with np.errstate(all="ignore"):
                        lin = (R["_eotf_hlg"] if tr == "hlg" else R["_eotf_pq"])(rgb)
                        ref = R["_python_tonemap_to_bgr8"](lin, peak_nits=1000.0, target_nits=200.0)
                    tc.append(time.perf_counter() - t0)
                d = np.abs(ref.astype(np.int16) - got.astype(np.int16))
                rec["reference_cpu"] = stats(tc)
                rec["against_reference"] = {"max_diff": int(d.max()), "differing": int(np.count_nonzero(d)),
                                            "bytes": int(d.size)}
                if not a.cpu_only:
                    rec["reference_cpu_over_kernel"] = statistics.median(tc) / statistics.median(tk)
            out[f"{res}_{tr}"] = rec
            print(res, tr, json.dumps(rec), flush=True)
            if not a.cpu_only:
                src.free()
                dst.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("->", a.out)


if __name__ == "__main__":
    main()
