#!/usr/bin/env python3
"""Timings of the OpenCLIP ViT family on the MI355X. Standalone; bench.py is not involved.

1. Towers: per-image time of ClipEngine.embed_device (preprocessing + tower + normalise) at batch 32 for
   ViT-B-32, ViT-B-16, ViT-L-14, ViT-L-14-336 and ViT-H-14 in f16, f16x3 and f32. B/32, B/16 and L/14
   (head dim 64, at most 272 tokens) run mha_tokens by default and are timed both ways: default dispatch and
   PERSON_CAPTURE_AMD_ATTN=stream; L/14-336 and H/14 always stream. Host clock around a window of calls that
   ends in a device synchronise, the call count sized per configuration to at least `--window` seconds;
   warm-up first; the configurations of a tower are interleaved (one timed window of each per round) and
   the median over the rounds is reported.
2. The attention kernel alone at ViT-L/14 geometry (N = 32, T = 257, 16 heads, d = 64): a one-op program
   per kernel, timed by the net's own per-op HIP events (pc_net_profile), interleaved in one process:
   mha_tokens<f16> (the default dispatch) against the matrix-core form, and mha_tokens<float> against the
   streaming f32-class form (PERSON_CAPTURE_AMD_ATTN=stream, read when a net is created).

Weights are random with one array per parameter shape shared by all layers (timing does not depend on
their values, and ViT-H/14 has 0.6 G parameters). Prints one JSON document; --out also writes it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from person_capture_amd import models_clip as mc   # noqa: E402
from person_capture_amd import program as pg       # noqa: E402
from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F16X3, PC_PREC_F32   # noqa: E402
from person_capture_amd.reid_embedder import ClipEngine   # noqa: E402
from person_capture_amd.runtime import GpuContext, Net   # noqa: E402

TOWERS = ["ViT-B-32", "ViT-B-16", "ViT-L-14", "ViT-L-14-336", "ViT-H-14"]
PRECS = [("f16", PC_PREC_F16), ("f16x3", PC_PREC_F16X3), ("f32", PC_PREC_F32)]
OP_ATTENTION = 6


def shared_weights(name: str) -> dict:
    """synth_clip_vit's shapes and scales, one random array per (shape, scale) for all layers."""
    c = mc.clip_cfg(name)
    w, L, ps = c["width"], c["layers"], c["patch"]
    rng = np.random.default_rng(7)
    cache = {}

    def f(shape, std):
        if (shape, std) not in cache:
            cache[(shape, std)] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(std))
        return cache[(shape, std)]

    p = {"visual.conv1.weight": f((w, 3, ps, ps), (3 * ps * ps) ** -0.5), "visual.class_embedding": f((w,), w ** -0.5),
         "visual.positional_embedding": f(((c["image"] // ps) ** 2 + 1, w), w ** -0.5), "visual.proj": f((w, c["out"]), w ** -0.5)}
    gamma = rng.uniform(0.8, 1.2, w).astype(np.float32)
    proj_std = (w ** -0.5) * ((2 * L) ** -0.5)
    lns = ["visual.ln_pre", "visual.ln_post"]
    for i in range(L):
        pre = f"visual.transformer.resblocks.{i}"
        lns += [pre + ".ln_1", pre + ".ln_2"]
        p[pre + ".attn.in_proj_weight"] = f((3 * w, w), w ** -0.5)
        p[pre + ".attn.in_proj_bias"] = f((3 * w,), 0.02)
        p[pre + ".attn.out_proj.weight"] = f((w, w), proj_std)
        p[pre + ".attn.out_proj.bias"] = f((w,), 0.02)
        p[pre + ".mlp.c_fc.weight"] = f((c["mlp"], w), (2 * w) ** -0.5)
        p[pre + ".mlp.c_fc.bias"] = f((c["mlp"],), 0.02)
        p[pre + ".mlp.c_proj.weight"] = f((w, c["mlp"]), proj_std)
        p[pre + ".mlp.c_proj.bias"] = f((w,), 0.02)
    for n in lns:
        p[n + ".weight"], p[n + ".bias"] = gamma, f((w,), 0.05)
    return p


def bench_towers(ctx, towers, batch, warmup, rounds, calls, window):
    rng = np.random.default_rng(3)
    crops = [rng.integers(0, 256, (256, 128, 3), dtype=np.uint8) for _ in range(batch)]
    bufs = [ctx.upload(c) for c in crops]
    descs = [(b.ptr, c.shape[0], c.shape[1], c.strides[0]) for b, c in zip(bufs, crops)]
    rows = []
    for name in towers:   # one tower at a time (ViT-H/14 in f16x3 alone is a 7.5 GB program)
        p = shared_weights(name)
        c = mc.clip_cfg(name)
        # head dim 64 with at most 272 tokens (B/32, B/16, L/14) is mha_tokens' by default: time it both ways
        switched = c["width"] // c["heads"] == 64 and (c["image"] // c["patch"]) ** 2 + 1 <= 272
        cfgs = []
        for attn in (["mha_tokens", "stream"] if switched else ["stream"]):
            for pname, prec in PRECS:
                if attn == "stream" and switched:
                    os.environ["PERSON_CAPTURE_AMD_ATTN"] = "stream"
                eng = ClipEngine(ctx, p, name, precision=prec, max_batch=batch)
                os.environ.pop("PERSON_CAPTURE_AMD_ATTN", None)
                eng.program = None
                cfgs.append(((pname, attn), eng, ctx.alloc(batch * eng.dim * 4)))
                print(f"built {name} {pname} {attn}", file=sys.stderr, flush=True)
        ncall = {}
        for key, eng, out in cfgs:
            for _ in range(warmup):
                eng.embed_device(descs, out.ptr)
            ctx.sync()
            t0 = time.perf_counter()
            eng.embed_device(descs, out.ptr)
            ctx.sync()
            # a timed window of at least `window` seconds of device work
            ncall[key] = max(calls, int(np.ceil(window / max(time.perf_counter() - t0, 1e-6))))
        times = {key: [] for key, _, _ in cfgs}
        for _ in range(rounds):   # this tower's configurations interleaved
            for key, eng, out in cfgs:
                t0 = time.perf_counter()
                for _ in range(ncall[key]):
                    eng.embed_device(descs, out.ptr)
                ctx.sync()
                times[key].append((time.perf_counter() - t0) / (ncall[key] * batch) * 1e3)
        for key, eng, out in cfgs:
            t = times[key]
            med = statistics.median(t)
            rows.append({"tower": name, "precision": key[0], "attention": key[1], "calls_per_window": ncall[key],
                         "ms_per_image": round(med, 4), "min": round(min(t), 4),
                         "max": round(max(t), 4), "images_per_s": round(1e3 / med, 1),
                         "tflops": round(eng.flops_per_image / med / 1e9, 1)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            eng.net.close()
            out.free()
    return rows


def _lin(P, out, x, W):
    cout, cin = W.shape
    wp = np.zeros((pg.cpad(cout), P.dims(x)[2]), np.float32)
    wp[:cout, :cin] = W
    P.conv(out, [(x, 1, 1, 1, 0, cin)], wp, cout, bias=np.zeros(pg.cpad(cout), np.float64))


def attention_net(ctx, f32, stream, N, T, heads, d, cin=64):
    """qkv projection -> attention -> a 32-channel f32 projection; only the attention op is timed."""
    rng = np.random.default_rng(11)
    P = pg.Program()
    E = heads * d
    x = P.input_tensor(1, T, cin)
    qkv = P.act(1, T, 3 * E)
    _lin(P, qkv, x, rng.standard_normal((3 * E, cin)).astype(np.float32) * cin ** -0.5)
    a = P.act(1, T, E)
    P.attention(a, qkv, heads, d)
    o = P.act(1, T, 32, is_f32=1)
    _lin(P, o, a, rng.standard_normal((32, E)).astype(np.float32) * E ** -0.5)
    P.outputs = [o]
    if stream:
        os.environ["PERSON_CAPTURE_AMD_ATTN"] = "stream"
    else:
        os.environ.pop("PERSON_CAPTURE_AMD_ATTN", None)
    net = Net(ctx, P.serialize(), precision=PC_PREC_F32 if f32 else PC_PREC_F16, max_batch=N)
    os.environ.pop("PERSON_CAPTURE_AMD_ATTN", None)
    return net


def bench_attention(ctx, warmup, rounds, calls, N=32, T=257, heads=16, d=64):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 1, T, 64)).astype(np.float16).astype(np.float32)
    d16, d32 = ctx.upload(x.astype(np.float16)), ctx.upload(x)
    kernels = [("mha_tokens<f16> (default)", False, False), ("mha_mfma (f16 matrix cores)", False, True),
               ("mha_tokens<float> (default)", True, False), ("mha_stream (f32 class)", True, True)]
    nets = [(k, attention_net(ctx, f32, stream, N, T, heads, d), d32 if f32 else d16) for k, f32, stream in kernels]
    outs = {}
    for k, net, din in nets:
        for _ in range(warmup):
            net.run(din.ptr, N)
        outs[k] = net.read_output(0, N).astype(np.float32)
    times = {k: [] for k, _, _ in nets}
    for _ in range(rounds):
        for k, net, din in nets:
            net.profile(True)
            for _ in range(calls):
                net.run(din.ptr, N)
            ctx.sync()
            ops = net.profile_ops()
            net.profile(False)
            ms = [r[2] for r in ops if int(r[1]) == OP_ATTENTION]
            assert len(ms) == calls
            times[k].append(statistics.median(ms))
    flops = 4.0 * T * T * heads * d * N
    rows = []
    for k, _, _ in nets:
        med = statistics.median(times[k])
        rows.append({"kernel": k, "ms": round(med, 4), "min": round(min(times[k]), 4), "max": round(max(times[k]), 4),
                     "tflops": round(flops / med / 1e9, 1)})
    diffs = {"mfma_vs_tokens_f16_max_abs": float(np.abs(outs[kernels[1][0]] - outs[kernels[0][0]]).max()),
             "stream_vs_tokens_f32_max_abs": float(np.abs(outs[kernels[3][0]] - outs[kernels[2][0]]).max())}
    return {"shape": {"N": N, "T": T, "heads": heads, "head_dim": d}, "rows": rows, "outputs": diffs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--towers", default=",".join(TOWERS))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="least embed calls per timed window")
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of device work per timed window")
    ap.add_argument("--attn-calls", type=int, default=20)
    ap.add_argument("--skip-towers", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = GpuContext(0)
    res = {"method": "towers: host clock around a window of embed_device calls (at least --window s) ending in a device "
                     "synchronise, median of interleaved rounds; attention: per-op HIP events (pc_net_profile), median of interleaved rounds",
           "batch": a.batch, "warmup": a.warmup, "rounds": a.rounds, "calls": a.calls, "window_s": a.window}
    res["attention"] = bench_attention(ctx, a.warmup, a.rounds, a.attn_calls)
    if not a.skip_towers:
        res["towers"] = bench_towers(ctx, [t for t in a.towers.split(",") if t], a.batch, a.warmup, a.rounds, a.calls, a.window)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
