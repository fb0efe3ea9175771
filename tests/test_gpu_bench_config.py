"""Parity of exactly the configuration bench.py measures (BASELINE configs[2], C3) and of
C2, plus the device bank match on the reference's own fd_min golden vectors.

* C3 as benched: bench.synth_frames(0, 64) resident in HBM, DET_BATCH 64, ARC_BATCH 512,
  PIPE_CHUNK 32, PIPE_AHEAD 2 (two pipelined detection chunks, shared chips/feats/fd
  scratch across ArcFace launches, pinned readbacks behind fences), a 32-row bank with
  planted rows (oracle embeddings of some faces plus noise) so accept decisions go both
  ways. f32 (the parity mode) against oracle/pipeline.extract_frame, every frame:
  identical int boxes; a face whose chip is byte-identical to the oracle's has its
  embedding and bank distance within 1e-4 (north_star) and its quality within 1e-9 rel;
  a face whose landmarks differ in the last f32 bits (so a few warped pixels differ) is
  checked through the chain — the oracle's align of the device landmarks gives the
  device chip byte for byte, the oracle embedding / fd of that chip match within 1e-4.
  Accept/reject at 0.32 and 0.45 identical (outside a 1e-4 band); at 0.32 they go both ways.
* C3 in the timed mode (f16x3 SCRFD + f16 ArcFace) and with the detector in f32 or plain f16:
  face-count, box and accept mismatches against the same oracle, counted like bench.py's parity
  block (nearest box), printed, persisted and bounded.
* C2: ArcFace-R100 at batch 256 (512 rows with flip) through ArcFaceEngine(max_batch=512)
  against the oracle on a 32-chip subset (f32 1e-4, f16 1e-2).
* pc_bank_match on tests/golden/fd_min.npz (B = 1/32/64/1024, empty bank -> 9.0, 1-D bank).
"""
import json
import os

import numpy as np
import pytest

import bench
from golden_parts import load_golden
from oracle import cv_ops
from oracle import nets_torch as nt
from oracle import pipeline as op
from oracle import ref_algos as ra
from person_capture_amd import face_embedder as fe_mod
from person_capture_amd import models
from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F16C8, PC_PREC_F16X3, PC_PREC_F32
from person_capture_amd.engines import ArcFaceEngine
from person_capture_amd.match import DeviceBank

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BENCH_ENV = {"PERSON_CAPTURE_AMD_DET_BATCH": "64", "PERSON_CAPTURE_AMD_ARC_BATCH": "512",
             "PERSON_CAPTURE_AMD_PIPE_CHUNK": "32", "PERSON_CAPTURE_AMD_PIPE_AHEAD": "2"}
NFRAMES = 64
TOL = 1e-4


def planted_bank(oracle_results, n_rows: int = 32, seed: int = 5) -> np.ndarray:
    """n_rows unit rows: 12 are oracle embeddings of chosen faces plus Gaussian noise of
    growing strength, the rest random. The synthetic (untrained) embedder's outputs share a
    large common component (their mean has norm ~0.86), so the planted rows have 0.3 of the
    mean removed: the bank distances of the 64 benched frames then straddle the CLI
    threshold 0.32 (~100 of ~380 faces accepted; all at the GUI's 0.45)."""
    feats = [f["feat"] for r in oracle_results if r != op.NEEDS_FALLBACK for f in r]
    mean = np.mean(feats, axis=0)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(feats), 12, replace=False)
    rows = []
    for k, i in enumerate(pick):
        v = feats[i] - 0.3 * mean + (0.1 + 0.1 * k) * rng.standard_normal(512).astype(np.float32) / np.sqrt(512.0)
        rows.append(v / np.linalg.norm(v))
    rest = rng.standard_normal((n_rows - len(rows), 512)).astype(np.float32)
    rows.extend(rest / np.linalg.norm(rest, axis=1, keepdims=True))
    return np.stack(rows).astype(np.float32)


@pytest.fixture(scope="module")
def c3_frames():
    return bench.synth_frames(0, NFRAMES)


@pytest.fixture(scope="module")
def c3_oracle(c3_frames):
    """oracle/pipeline.extract_frame of every benched frame (fp32 torch-CPU nets), then the
    planted bank and the oracle fd of every face against it."""
    p_s = fe_mod.synthetic_weights("scrfd_10g", 0)
    p_a = fe_mod.synthetic_weights("iresnet100", 0)
    res = [op.extract_frame(f, p_s, "10g", p_a, 100, conf=0.5, D=640) for f in c3_frames]
    bank = planted_bank(res)
    for r in res:
        if r != op.NEEDS_FALLBACK:
            for f in r:
                f["fd"] = ra.fd_min(f["feat"], bank)
    return res, bank


def _run_bench_config(monkeypatch, frames, bank, prec, conf=0.5):
    for k, v in BENCH_ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", prec)
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_10g_bnkps", conf=conf)
    assert fe._pipe_chunk == 32 and fe._pipe_ahead == 2 and fe._arc.max_batch == 512 and fe._det_batch == 64
    ctx = fe._ctx
    d = ctx.alloc(frames.nbytes)
    ctx.upload(frames, d)
    fsz = frames[0].nbytes
    H, W = frames.shape[1:3]
    devs = [fe_mod._DevImage(d.ptr + i * fsz, H, W, W * 3) for i in range(len(frames))]
    dbank = DeviceBank(ctx, bank)
    plain = fe.extract_batch([None] * len(frames), dev_frames=devs, bank=dbank)
    # the same run again with the chips read back (debug readback only adds a D2H copy)
    fe2 = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_10g_bnkps", conf=conf)
    fe2.debug_chips = True
    dbg = fe2.extract_batch([None] * len(frames), dev_frames=devs, bank=dbank)
    for a, b in zip(plain, dbg):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x["bbox"], y["bbox"]) and np.array_equal(x["feat"], y["feat"])
            assert x["fd"] == y["fd"] and x["quality"] == y["quality"]
    return fe2, dbg


def _persist(name, obj):
    """Keep a test's measured counts (pytest -q drops prints): gpurun_out/parity/<name>.json,
    which gpurun copies back from the GPU box."""
    root = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    d = os.path.join(root, "gpurun_out", "parity")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name + ".json"), "w") as f:
        json.dump(obj, f, indent=1)


def _oracle_embed_chip(fe, chip):
    e = nt.iresnet_forward(fe._arc_params, 100, nt.arcface_input_from_chips(chip[None])).numpy()
    ef = nt.iresnet_forward(fe._arc_params, 100, nt.arcface_input_from_chips(chip[None, :, ::-1])).numpy()
    return ra.arcface_postprocess(e, ef)[0]


def test_c3_bench_config_parity_f32(gpu_ctx, monkeypatch, c3_frames, c3_oracle):
    ores, bank = c3_oracle
    fe, got = _run_bench_config(monkeypatch, c3_frames, bank, "f32")
    n_exact = n_chained = n_acc = n_rej = n_fallback = 0
    e2e_fd, e2e_feat, e2e_flip = [], [], 0
    for fi, (frame, g, r) in enumerate(zip(c3_frames, got, ores)):
        if r == op.NEEDS_FALLBACK:   # the oracle stops at the fallback branches
            n_fallback += 1
            continue
        assert len(g) == len(r), f"frame {fi}: {len(g)} faces vs oracle {len(r)}"
        gs = sorted(g, key=lambda f: tuple(f["bbox"]))
        rs = sorted(r, key=lambda f: tuple(f["bbox"]))
        for a, b in zip(gs, rs):
            assert np.array_equal(a["bbox"], b["bbox"]), (fi, a["bbox"], b["bbox"])
            if np.array_equal(a["chip"], b["chip"]):
                assert np.abs(a["feat"] - b["feat"]).max() < TOL
                assert abs(a["fd"] - b["fd"]) < TOL
                assert abs(a["quality"] - b["quality"]) <= 1e-9 * max(1.0, b["quality"])
                ref_fd = b["fd"]
                n_exact += 1
            else:
                assert np.abs(a["kps5"] - b["kps5"]).max() < 1e-3
                x1, y1, x2, y2 = a["bbox"]
                chip = op.align_chip(frame[y1:y2, x1:x2], ra.canon_5pts(a["kps5"]))
                assert np.array_equal(chip, a["chip"])
                assert abs(cv_ops.face_quality(chip) - a["quality"]) <= 1e-9 * max(1.0, a["quality"])
                feat = _oracle_embed_chip(fe, chip)
                assert np.abs(feat - a["feat"]).max() < TOL
                ref_fd = ra.fd_min(feat, bank)
                assert abs(a["fd"] - ref_fd) < TOL
                n_chained += 1
                # end to end (the oracle's own landmarks): a few chip pixels differ
                e2e_fd.append(abs(a["fd"] - b["fd"]))
                e2e_feat.append(float(np.abs(a["feat"] - b["feat"]).max()))
                e2e_flip += sum((a["fd"] <= t) != (b["fd"] <= t) for t in (0.32, 0.45) if abs(b["fd"] - t) > 1e-3)
            for thr in (0.32, 0.45):
                if abs(ref_fd - thr) > TOL:
                    assert (a["fd"] <= thr) == (ref_fd <= thr)
            n_acc += a["fd"] <= 0.32
            n_rej += a["fd"] > 0.32
    print(f"C3 f32 bench config: {n_exact} faces exact, {n_chained} chained, {n_fallback} fallback frames, "
          f"{n_acc} accepted / {n_rej} rejected at 0.32; chained faces end to end: max |dfd| "
          f"{max(e2e_fd, default=0):.2e}, max |dfeat| {max(e2e_feat, default=0):.2e}, "
          f"decision flips outside 1e-3 {e2e_flip}")
    _persist("c3_f32", {"faces_exact": n_exact, "faces_chained": n_chained, "fallback_frames": n_fallback,
                        "accepted_0.32": int(n_acc), "rejected_0.32": int(n_rej),
                        "chained_e2e_max_dfd": max(e2e_fd, default=0.0), "chained_e2e_max_dfeat": max(e2e_feat, default=0.0),
                        "decision_flips_outside_1e-3": int(e2e_flip)})
    assert n_fallback <= 2
    assert n_exact + n_chained >= 4 * NFRAMES
    # measured r03 (profiles/r03_parity_c3_f32.json): 332 chained faces, max |dfd| 6.6e-4
    assert e2e_flip == 0 and max(e2e_fd, default=0) < 1e-3
    assert n_acc > 0 and n_rej > 0


def _vs_oracle(got, ores):
    """bench.compare_faces against the oracle (nearest-box pairing, the count the bench's parity
    block reports); the oracle's fallback frames are skipped."""
    return bench.compare_faces(got, [None if r == op.NEEDS_FALLBACK else r for r in ores], band=1e-3)


def test_c3_detector_f32_mode_decisions(gpu_ctx, monkeypatch, c3_frames, c3_oracle):
    """PERSON_CAPTURE_AMD_DET_PRECISION=f32 (SCRFD f32, ArcFace f16) vs the fp32 oracle: the
    detector's landmarks are the f32 path's, so counts and boxes are identical and only the f16
    ArcFace's ~2e-4 fd differences remain, plus the f32 path's own end-to-end chip differences
    against the oracle (a landmark a few f32 bits apart moves a few chip pixels: up to 7e-4 in
    fd, test_c3_bench_config_parity_f32); no accept flip outside a 1e-3 band of the thresholds."""
    ores, bank = c3_oracle
    monkeypatch.setenv("PERSON_CAPTURE_AMD_DET_PRECISION", "f32")
    _, got = _run_bench_config(monkeypatch, c3_frames, bank, "f16")
    report = _vs_oracle(got, ores)
    print("C3 detector-f32 mode vs fp32 oracle: " + json.dumps(report))
    _persist("c3_det_f32", report)
    assert report["face_count_mismatch"] == 0 and report["box_mismatch"] == 0
    assert report["accept_mismatch_outside_0.001_band"] == 0
    assert report["max_fd_diff"] < 2e-3


def test_c3_timed_mode_decisions(gpu_ctx, monkeypatch, c3_frames, c3_oracle):
    """The timed mode (bench.py C3: f16x3 SCRFD + f16x3 ArcFace) vs the fp32 oracle, counted as the
    bench's parity block counts (nearest box): identical face counts and boxes, no accept flip at
    0.32 or 0.45 outside a 1e-3 band of the threshold (a face within the band flips under any
    path that is not bitwise the oracle's: the f32 device mode's own chips differ from the
    oracle's by up to 7e-4 in fd), at most 1 % of the faces flipping inside it."""
    ores, bank = c3_oracle
    monkeypatch.delenv("PERSON_CAPTURE_AMD_DET_PRECISION", raising=False)
    monkeypatch.delenv("PERSON_CAPTURE_AMD_ARC_PRECISION", raising=False)
    fe, got = _run_bench_config(monkeypatch, c3_frames, bank, "f16")
    assert fe.det_precision == 2 and fe.arc_precision == 2   # PC_PREC_F16X3, the defaults
    report = _vs_oracle(got, ores)
    print("C3 timed mode (f16x3 SCRFD) vs fp32 oracle: " + json.dumps(report))
    _persist("c3_timed", report)
    assert report["face_count_mismatch"] == 0 and report["box_mismatch"] == 0
    # r05 (f16x3 ArcFace, gpurun_out/parity/c3_timed.json): no accept flip at either threshold; max |dfd|
    # 1.02e-3, all of it the noise chips' few differing pixels (the device f32 mode: 6.6e-4)
    assert report["accept_mismatch_0.32"] == 0 and report["accept_mismatch_0.45"] == 0
    assert report["max_fd_diff"] < 1.5e-3


SMOOTH_N = 32   # r05: 8 frames / 42 faces; widened so the 3e-4 same-box bound sees ~170 faces


@pytest.fixture(scope="module")
def smooth_c3(c3_frames):
    """bench.smooth_frames of the first SMOOTH_N benched frames (the bench's parity.smooth_frames
    input) through the oracle at SCRFD conf 0.8 (as bench.smooth_parity), with a planted bank."""
    sm = bench.smooth_frames(c3_frames[:SMOOTH_N])
    p_s = fe_mod.synthetic_weights("scrfd_10g", 0)
    p_a = fe_mod.synthetic_weights("iresnet100", 0)
    res = [op.extract_frame(f, p_s, "10g", p_a, 100, conf=0.8, D=640) for f in sm]
    bank = planted_bank(res)
    for r in res:
        if r != op.NEEDS_FALLBACK:
            for f in r:
                f["fd"] = ra.fd_min(f["feat"], bank)
    return sm, res, bank


def test_c3_smooth_frames_timed_mode(gpu_ctx, monkeypatch, smooth_c3):
    """The timed mode on smooth (camera-like) frames against the CPU oracle, counted like the bench
    (nearest box). Face counts equal; a box may differ only by one pixel in coordinates whose oracle
    float value lies within 2e-3 px of an integer - the int() of _accumulate
    (face_embedder.py:2214-2239) on the other side of it, which any path not bitwise the oracle's can
    meet (the f16x3 boxes are within 1e-3 px of the f32 path's, test_gpu_scrfd_split.py) - and such a
    face's keypoints then sit one pixel over in crop coordinates, so its chip's border reflection
    differs; faces with equal boxes keep fd within 3e-4 and no accept decision flips (r04's smooth-frame
    report had one such box against the device f32 mode, and no test)."""
    sm, ores, bank = smooth_c3
    monkeypatch.delenv("PERSON_CAPTURE_AMD_DET_PRECISION", raising=False)
    monkeypatch.delenv("PERSON_CAPTURE_AMD_ARC_PRECISION", raising=False)
    fe, got = _run_bench_config(monkeypatch, sm, bank, "f16", conf=0.8)
    report = _vs_oracle(got, ores)
    print("C3 timed mode on smooth frames vs fp32 oracle: " + json.dumps(report))
    _persist("c3_smooth_timed", report)
    assert report["faces"] >= 3 * SMOOTH_N
    assert report["face_count_mismatch"] == 0
    assert report["box_mismatch"] == report.get("box_mismatch_int_boundary", 0)
    assert report.get("box_mismatch_int_margin_px", 0.0) < 2e-3
    assert report["accept_mismatch_0.32"] == 0 and report["accept_mismatch_0.45"] == 0
    # r05: 42 faces, max |dfd| 1.08e-4 (smooth chips barely change under last-bit landmark shifts)
    assert report["max_fd_diff_same_box"] < 3e-4


def test_c3_plain_f16_detector_mismatches(gpu_ctx, monkeypatch, c3_frames, c3_oracle):
    """The plain f16 detector (PERSON_CAPTURE_AMD_DET_PRECISION=f16, round 3's headline) vs the
    fp32 oracle, counted like the bench (nearest box): its sub-pixel landmark shifts resample the
    noise-frame chips, so decisions flip; bounded at what was measured (r03 bench: 15 count / 35
    box / 25 accept mismatches of 383 faces)."""
    ores, bank = c3_oracle
    monkeypatch.setenv("PERSON_CAPTURE_AMD_DET_PRECISION", "f16")
    _, got = _run_bench_config(monkeypatch, c3_frames, bank, "f16")
    report = _vs_oracle(got, ores)
    print("C3 plain f16 detector vs fp32 oracle: " + json.dumps(report))
    _persist("c3_f16_detector", report)
    n = report["faces"]
    assert report["face_count_mismatch"] <= NFRAMES // 4
    assert report["box_mismatch"] <= n // 5
    assert report["accept_mismatch_0.32"] <= max(2, n // 10)
    # (max_fd_diff is not bounded here: a shifted box pairs the nearest other face, measured 0.26)


# measured r05 (gpurun_out/parity/c2_prec*.json): f32 6.7e-7, f16x3 2.7e-6, f16c8 1.5e-5, f16 5.4e-4
@pytest.mark.parametrize("prec,tol", [(PC_PREC_F32, 1e-5), (PC_PREC_F16X3, 1e-5), (PC_PREC_F16C8, 5e-5),
                                      (PC_PREC_F16, 1e-3)])
def test_c2_arcface_batch256(gpu_ctx, prec, tol):
    """BASELINE C2: 256 chips -> 512 rows with flip in one ArcFaceEngine(max_batch=512) launch,
    max |embedding - oracle| on 32 chips, bounded ~2-3x above the measured error of each mode."""
    p = models.synth_iresnet(100, seed=0)
    chips = np.random.default_rng(256).integers(0, 256, (256, 112, 112, 3), dtype=np.uint8)
    eng = ArcFaceEngine(gpu_ctx, p, 100, precision=prec, max_batch=512)
    got = eng.embed(chips, flip=True)
    assert got.shape == (256, 512)
    sub = np.arange(0, 256, 8)   # 32 chips spread over the batch
    e = nt.iresnet_forward(p, 100, nt.arcface_input_from_chips(chips[sub])).numpy()
    ef = nt.iresnet_forward(p, 100, nt.arcface_input_from_chips(chips[sub][:, :, ::-1])).numpy()
    ref = ra.arcface_postprocess(e, ef)
    err = float(np.abs(got[sub] - ref).max())
    _persist(f"c2_prec{prec}", {"max_abs_embedding_err": err, "chips_checked": len(sub)})
    assert err < tol, err
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)


def test_bank_match_on_fd_min_goldens(gpu_ctx):
    """pc_bank_match vs the reference's own _fd_min outputs (tools/gen_golden.py): the dot
    products are summed in a different order than numpy's sgemv, so 1e-6."""
    d = load_golden(os.path.join(G, "fd_min.npz"))
    feats = np.ascontiguousarray(d["feats"], np.float32)
    dq = gpu_ctx.upload(feats)
    fd = gpu_ctx.alloc(4 * len(feats))
    idx = gpu_ctx.alloc(4 * len(feats))
    off = 0
    for i, B in enumerate(d["bank_sizes"]):
        bank = d["banks"][off:off + B]
        off += B
        db = DeviceBank(gpu_ctx, bank)
        db.match_device(dq.ptr + i * 2048, 1, fd.ptr, idx.ptr)
        got = float(gpu_ctx.download(fd.ptr, (1,), np.float32)[0])
        assert abs(got - d["fd"][i]) < 1e-6, (int(B), got, d["fd"][i])
    e = d["fd_edge"]
    db = DeviceBank(gpu_ctx, np.zeros((0, 512), np.float32))            # empty bank -> 9.0
    db.match_device(dq.ptr, 1, fd.ptr, idx.ptr)
    assert float(gpu_ctx.download(fd.ptr, (1,), np.float32)[0]) == e[2] == 9.0
    db = DeviceBank(gpu_ctx, d["banks"][0])                               # 1-D bank: 1 - dot
    db.match_device(dq.ptr, 1, fd.ptr, idx.ptr)
    assert abs(float(gpu_ctx.download(fd.ptr, (1,), np.float32)[0]) - e[3]) < 1e-6
    with pytest.raises(ValueError):                                       # np.dot((512,), (0,)) raises
        DeviceBank(gpu_ctx, np.zeros((0,), np.float32))
    # the whole feature batch against the largest bank in one launch (C5's 1024 rows)
    big = int(np.argmax(d["bank_sizes"]))
    o = int(np.sum(d["bank_sizes"][:big]))
    bank = d["banks"][o:o + d["bank_sizes"][big]]
    assert len(bank) == 1024
    db = DeviceBank(gpu_ctx, bank)
    db.match_device(dq.ptr, len(feats), fd.ptr, idx.ptr)
    got = gpu_ctx.download(fd.ptr, (len(feats),), np.float32)
    ref = np.array([ra.fd_min(f, bank) for f in feats])
    assert np.abs(got - ref).max() < 1e-6
