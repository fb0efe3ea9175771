"""FaceEmbedder(use_arcface=False): OpenCLIP face embeddings on the SCRFD backend
(face_embedder.py:955-965, 1649-1661, 2454-2465), against the CPU oracles.

No alignment in this mode: every kept face box becomes resize_for_arc(frame[y1:y2, x1:x2]) (one
pc_face_chips call per embed batch), its quality is the Laplacian variance of that chip, and its
feature is open_clip's preprocess + image tower + F.normalize of the chip
(oracle/nets_torch.clip_preprocess_pil + clip_vit_forward) within 1e-4, the project's f32 bound
(north_star, as tests/test_gpu_c4_composed.py). The detector policy is the ArcFace mode's: boxes,
output order and policy state are compared with oracle/pipeline.OracleFaceEmbedder (whose boxes do
not depend on the embedder) over the fallback sequence of tests/test_gpu_fallbacks.py.

Towers: ViT-tiny-16 (out 64) and ViT-L-14-d2 (out 768); detector scrfd_2.5g on 240x320 frames with the
score-bias shift of tests/test_gpu_fallbacks.py.
"""
import numpy as np
import pytest
import torch

from oracle import cv_ops
from oracle import nets_torch as nt
from oracle import pipeline as op
from oracle import ref_algos as ra
from person_capture_amd import face_embedder as fe_mod
from person_capture_amd import models_clip
from person_capture_amd.match import DeviceBank
from person_capture_amd.reid_embedder import clip_weights
from test_gpu_fallbacks import _noise, fallback_sequence, shifted_params

pytestmark = pytest.mark.gpu

TOL = 1e-4
TOWER = "ViT-tiny-16"


def _embedder(monkeypatch, tower=TOWER, prec=None, shift=True, **kw):
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PIPE_CHUNK", "4")   # several pipelined detection chunks
    if prec is None:
        monkeypatch.delenv("PERSON_CAPTURE_AMD_FACE_CLIP_PRECISION", raising=False)
    else:
        monkeypatch.setenv("PERSON_CAPTURE_AMD_FACE_CLIP_PRECISION", prec)
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5, use_arcface=False,
                             clip_model_name=tower, **kw)
    if shift:
        fe._scrfd_params = shifted_params(fe._scrfd_params)
        fe._scrfd_engines.clear()
        fe.scrfd = fe._engine(640)
    fe.debug_chips = True
    return fe


def _tower(chips_bgr, tower=TOWER):
    """Oracle unit embeddings of BGR images (any sizes)."""
    side = models_clip.clip_cfg(tower)["image"]
    x = torch.stack([nt.clip_preprocess_pil(np.ascontiguousarray(c), side) for c in chips_bgr])
    return torch.nn.functional.normalize(nt.clip_vit_forward(clip_weights(tower, 0), tower, x), dim=1).numpy()


def _noise_frames(n, seed=40):
    return [_noise(seed + i) for i in range(n)]


def test_clip_encode(gpu_ctx, monkeypatch):
    fe = _embedder(monkeypatch, shift=False)
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 30), (112, 112), (300, 500))]
    got = fe._clip_encode(imgs)
    assert got.shape == (3, 64) and got.dtype == np.float32
    d = np.abs(got - _tower(imgs)).max()
    print(f"_clip_encode max |d| {d:.2e}")
    assert d < TOL
    assert fe._clip_encode([]) == []


def test_extract_batch_fallback_sequence(gpu_ctx, monkeypatch):
    fe = _embedder(monkeypatch)
    fe.rot_every_n = 3
    fe.rot_after_hit_frames = 6
    o = op.OracleFaceEmbedder(fe._scrfd_params, "2.5g", fe_mod.synthetic_weights("iresnet50", 0), 50, conf=0.5,
                              rot_phase=id(fe) & 7)
    o.rot_every_n, o.rot_after_hit_frames = 3, 6
    frames = fallback_sequence()
    got = fe.extract_batch(frames)
    traces = set()
    chips, feats = [], []
    for fi, (frame, g) in enumerate(zip(frames, got)):
        r = o.extract(frame, keep_chips=False)
        traces.update(o.trace)
        assert len(g) == len(r), f"frame {fi}: {len(g)} faces vs oracle {len(r)}"
        gs = sorted(g, key=lambda f: tuple(f["bbox"]))
        rs = sorted(r, key=lambda f: tuple(f["bbox"]))
        for a, b in zip(gs, rs):
            assert np.array_equal(a["bbox"], b["bbox"]), (fi, a["bbox"], b["bbox"])
            x1, y1, x2, y2 = a["bbox"]
            chip = op.resize_for_arc(np.ascontiguousarray(frame[y1:y2, x1:x2]))
            assert np.array_equal(a["chip"], chip), (fi, a["bbox"])   # landmarks or not: no alignment
            q = cv_ops.face_quality(chip)
            assert abs(a["quality"] - q) <= 1e-9 * max(1.0, q)
            assert a["feat"].shape == (64,)
            chips.append(chip)
            feats.append(a["feat"])
        keys = [(f["quality"], int((f["bbox"][2] - f["bbox"][0]) * (f["bbox"][3] - f["bbox"][1]))) for f in g]
        assert keys == sorted(keys, reverse=True)
    print("branches:", sorted(traces), "faces:", len(chips))
    assert len(chips) >= 10
    d = np.abs(np.stack(feats) - _tower(chips)).max()
    print(f"max |dfeat| {d:.2e}")
    assert d < TOL
    assert any(t.startswith("tta") for t in traces) and any(t.startswith("rot") for t in traces)
    assert fe.policy_state() == o.state()


def test_extract_equals_extract_batch(gpu_ctx, monkeypatch):
    """extract(f) frame by frame == extract_batch([f ...]): identical bytes (the tower's rows do not
    depend on the batch they run in)."""
    frames = _noise_frames(3)
    fa = _embedder(monkeypatch, shift=False)
    one = [fa.extract(f) for f in frames]
    fb = _embedder(monkeypatch, shift=False)
    bat = fb.extract_batch(frames)
    n = 0
    for a, b in zip(one, bat):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x["bbox"], y["bbox"])
            assert np.array_equal(x["chip"], y["chip"])
            assert x["quality"] == y["quality"]
            assert x["feat"].tobytes() == y["feat"].tobytes()
            n += 1
    assert n >= 3


def test_bank_match(gpu_ctx, monkeypatch):
    fe = _embedder(monkeypatch, shift=False)
    frames = _noise_frames(2)
    first = fe.extract_batch(frames)
    planted = [f["feat"] for lst in first for f in lst][:4]
    assert planted
    rng = np.random.default_rng(9)
    bank = rng.standard_normal((16, 64)).astype(np.float32)
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    for k, v in enumerate(planted):   # planted rows: a face's own feature, rotated a little
        w = v + 0.3 * bank[k]
        bank[k] = w / np.linalg.norm(w)
    got = fe.extract_batch(frames, bank=DeviceBank(fe._ctx, bank))
    n = 0
    for lst in got:
        for f in lst:
            assert abs(f["fd"] - ra.fd_min(f["feat"], bank)) < 1e-6
            n += 1
    assert n >= len(planted)
    wide = rng.standard_normal((4, 512)).astype(np.float32)
    with pytest.raises(ValueError):
        fe.extract_batch(frames, bank=DeviceBank(fe._ctx, wide))


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_precisions(gpu_ctx, monkeypatch, prec):
    tower = "ViT-L-14-d2"
    fe = _embedder(monkeypatch, tower=tower, prec=prec, shift=False)
    faces = [f for lst in fe.extract_batch(_noise_frames(1)) for f in lst][:6]
    assert faces
    got = np.stack([f["feat"] for f in faces])
    assert got.shape[1] == 768
    ref = _tower([f["chip"] for f in faces], tower)
    if prec == "f16x3":
        assert np.abs(got - ref).max() < TOL
    else:
        assert (got * ref).sum(1).min() >= 0.99


def test_unknown_precision_word_raises(gpu_ctx, monkeypatch):
    with pytest.raises(ValueError):
        _embedder(monkeypatch, prec="bf16", shift=False)


def test_constructor(gpu_ctx, monkeypatch):
    lines = []
    fe = _embedder(monkeypatch, shift=False, progress=lines.append)
    assert fe.use_arcface is False and fe.backend == "clip"
    assert fe._arc is None and not hasattr(fe, "_arc_params")
    assert "arcface" not in fe.weights_source and fe.weights_source["clip_face"].startswith("synthetic:")
    assert any("OpenCLIP" in s and "synthetic" in s for s in lines)
    assert fe._arc_feat_dim == 64 and fe._embed_per() == 32
    monkeypatch.setenv("PERSON_CAPTURE_AMD_FACE_CLIP_BATCH", "8")
    assert _embedder(monkeypatch, shift=False)._embed_per() == 8
    with pytest.raises(RuntimeError, match="YOLOv8-face"):
        fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="yolov8l-face.pt", use_arcface=False)
    with pytest.raises(RuntimeError):
        fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", use_arcface=False, clip_model_name="RN50x64")


@pytest.mark.slow
@pytest.mark.timeout(600)
def test_curator_keywords_default_tower(gpu_ctx, monkeypatch):
    """The curator's constructor call without a reference image (dataset_curator.py:329-336) and the
    default ViT-L/14: constructs and extracts."""
    monkeypatch.delenv("PERSON_CAPTURE_AMD_FACE_CLIP_PRECISION", raising=False)
    fe = fe_mod.FaceEmbedder(ctx="cuda", yolo_model="scrfd_10g_bnkps", conf=0.5, use_arcface=False, progress=print,
                             trt_lib_dir=None)
    faces = fe.extract(_noise(50))
    assert fe._arc_feat_dim == 768
    for f in faces:
        assert f["feat"].shape == (768,) and abs(float(np.linalg.norm(f["feat"])) - 1.0) < 1e-5
