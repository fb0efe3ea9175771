"""CPU checks of the YOLOv8 person-detector build: the compiled program (in-place
concat slices, padded channel maps, fused Detect stems, BN eps 1e-3 folding) run
through the device-semantics emulator must match the literal oracle forward; the
ultralytics letterbox / scale_boxes geometry; the oracle post-processing contract."""
import numpy as np
import pytest
import torch

from oracle import nets_torch as nt
from oracle import ref_algos as ra
from person_capture_amd import models_yolo as my
from program_emulator import run_program


@pytest.fixture(scope="module")
def y8n():
    return my.synth_yolov8("n", seed=3)


def test_layer_table_yolov8n():
    L = my.yolo_layers("n")
    assert [l["cout"] for l in L[:10]] == [16, 32, 32, 64, 64, 128, 128, 256, 256, 256]
    assert [l.get("n") for l in L if l["type"] == "C2f"] == [1, 2, 2, 1, 1, 1, 1, 1]
    d = L[22]
    assert d["ch"] == [64, 128, 256] and d["c2b"] == 64 and d["c3"] == 80
    assert [l["cout"] for l in my.yolo_layers("s")[:2]] == [32, 64]


@pytest.mark.parametrize("Hp,Wp", [(128, 192), (96, 160)])
def test_yolo_program_matches_oracle(y8n, Hp, Wp):
    rng = np.random.default_rng(5)
    x = np.zeros((2, Hp, Wp, 4), np.float32)
    x[..., :3] = rng.integers(0, 256, (2, Hp, Wp, 3)).astype(np.float32) / 255.0
    ref = nt.yolov8_forward(y8n, "n", torch.from_numpy(np.ascontiguousarray(x[..., :3].transpose(0, 3, 1, 2))))
    P = my.compile_yolov8(y8n, "n", Hp, Wp)
    outs = run_program(P, x)
    assert len(outs) == 3
    for o, r in zip(outs, ref):
        got = o.permute(0, 2, 3, 1).numpy()
        r = r.numpy()
        assert got.shape == r.shape
        assert np.abs(got - r).max() / max(1.0, np.abs(r).max()) < 1e-4


def test_letterbox_geometry():
    # ultralytics LetterBox(auto=True, stride=32): 1080p -> 640x360 centred in 640x384
    assert my.letterbox_geometry(1080, 1920) == (640, 360, 12, 0, 384, 640)
    assert my.letterbox_geometry(2160, 3840) == (640, 360, 12, 0, 384, 640)
    assert my.letterbox_geometry(480, 640) == (640, 480, 0, 0, 480, 640)
    nw, nh, top, left, Hp, Wp = my.letterbox_geometry(1000, 333)
    assert (nh, Hp % 32, Wp % 32) == (640, 0, 0) and left + nw <= Wp
    # odd remainder splits round(d - 0.1) / round(d + 0.1)
    nw, nh, top, left, Hp, Wp = my.letterbox_geometry(500, 640)
    assert (Hp - nh - top) - top in (0, 1)
    g, px, py = my.scale_geometry(384, 640, 1080, 1920)
    assert abs(g - 1 / 3) < 1e-12 and (px, py) == (0, 12)


def test_yolo_letterbox_canvas():
    fr = np.random.default_rng(1).integers(0, 256, (90, 160, 3), dtype=np.uint8)
    img, (nw, nh, top, left, Hp, Wp) = ra.yolo_letterbox(fr)
    assert img.shape == (Hp, Wp, 3) and img.dtype == np.float32
    assert np.all(img[:top] == np.float32(114) / np.float32(255))
    # identity path when the frame already has the letterbox size
    fr2 = np.random.default_rng(2).integers(0, 256, (360, 640, 3), dtype=np.uint8)
    img2, g2 = ra.yolo_letterbox(fr2)
    assert g2[:2] == (640, 360)
    assert np.array_equal(img2[g2[2]:g2[2] + 360], fr2[..., ::-1].astype(np.float32) / np.float32(255))


def test_yolo_postprocess_contract():
    """Planted head maps: a strong class-0 anchor, a weaker overlapping one (suppressed
    at IoU 0.45), a class-3 anchor (filtered by classes=[0]) and a separate class-0 box."""
    heads = [np.full((h, w, 144), -20.0, np.float32) for h, w in ((48, 80), (24, 40), (12, 20))]
    for hd in heads:
        hd[..., :64] = 0.0
    def plant(lvl, y, x, cls, logit, bins=(3, 5, 3, 5)):
        hd = heads[lvl]
        hd[y, x, :64] = -8.0
        for k, b in enumerate(bins):
            hd[y, x, 16 * k + b] = 8.0
        hd[y, x, 64 + cls] = logit
    plant(0, 20, 30, 0, 3.0)
    plant(0, 20, 31, 0, 2.0)     # overlaps the first
    plant(0, 30, 60, 3, 5.0)     # not a person
    plant(1, 5, 5, 0, 1.0)
    d = ra.yolo_postprocess(heads, 0.35, 0.45, 40, 384, 640, 1080, 1920)
    assert d.shape == (2, 5)
    assert d[0, 4] > d[1, 4] > 0.35
    assert np.all(d[:, 0] >= 0) and np.all(d[:, 2] <= 1920) and np.all(d[:, 3] <= 1080)
    # box of the first: anchor (30.5, 20.5)*8 +- (3,5,3,5)*8 (DFL peak), scaled by 3, minus pad 12
    cx, cy = 30.5 * 8, 20.5 * 8
    np.testing.assert_allclose(d[0, :4], [(cx - 24) * 3, (cy - 40 - 12) * 3, (cx + 24) * 3, (cy + 40 - 12) * 3],
                               atol=0.05)
    assert len(ra.yolo_postprocess(heads, 0.99, 0.45, 40, 384, 640, 1080, 1920)) == 0


@pytest.fixture(scope="module")
def y8face():
    return my.synth_yolov8_face("n", seed=4)


def test_face_pose_layer_table():
    """yolov8-pose head (the YOLOv8-face models, kpt_shape [5, 3]): cv4 width max(ch0 // 4, 15)."""
    L = my.yolo_layers("l", 1, (5, 3))[22]
    assert L["type"] == "Pose" and L["nk"] == 15 and L["c4"] == max(L["ch"][0] // 4, 15) and L["nc"] == 1


@pytest.mark.parametrize("Hp,Wp", [(128, 192)])
def test_yolo_face_program_matches_oracle(y8face, Hp, Wp):
    """The Pose program's [DFL | cls | kpt] head maps against the literal oracle forward."""
    rng = np.random.default_rng(6)
    x = np.zeros((2, Hp, Wp, 4), np.float32)
    x[..., :3] = rng.integers(0, 256, (2, Hp, Wp, 3)).astype(np.float32) / 255.0
    ref = nt.yolov8_forward(y8face, "n", torch.from_numpy(np.ascontiguousarray(x[..., :3].transpose(0, 3, 1, 2))),
                            nc=1, kpt=(5, 3))
    outs = run_program(my.compile_yolov8(y8face, "n", Hp, Wp, nc=1, kpt=(5, 3)), x)
    for o, r in zip(outs, ref):
        got = o.permute(0, 2, 3, 1).numpy()
        r = r.numpy()
        assert got.shape == r.shape and r.shape[-1] == 64 + 1 + 15
        assert np.abs(got - r).max() / max(1.0, np.abs(r).max()) < 1e-4


def test_yolo_pose_postprocess_contract():
    """A planted face anchor: keypoints decode as (raw * 2 + anchor - 0.5) * stride, scale_coords
    with the unrounded pad, invisible points (sigmoid < 0.5) zeroed as Results.keypoints does."""
    heads = [np.full((h, w, 80), -20.0, np.float32) for h, w in ((48, 80), (24, 40), (12, 20))]
    hd = heads[0]
    hd[..., :64] = 0.0
    hd[20, 30, :64] = -8.0
    for k, b in enumerate((3, 5, 3, 5)):
        hd[20, 30, 16 * k + b] = 8.0
    hd[20, 30, 64] = 3.0
    raw = np.array([[0.1, 0.2, 4.0], [0.9, 0.2, 4.0], [0.5, 0.6, 4.0], [0.2, 0.9, -4.0], [0.8, 0.9, 4.0]],
                   np.float32)
    hd[20, 30, 65:] = raw.reshape(-1)
    d, k = ra.yolo_postprocess(heads, 0.3, 0.3, 60, 384, 640, 1080, 1920, nk=15)
    assert d.shape == (1, 5) and k.shape == (1, 5, 3)
    gain = 1 / 3
    for q in range(5):
        if raw[q, 2] < 0:
            assert k[0, q, 0] == 0 and k[0, q, 1] == 0
            continue
        x = (raw[q, 0] * 2 + 30) * 8
        y = (raw[q, 1] * 2 + 20) * 8
        assert abs(k[0, q, 0] - x / gain) < 1e-2 and abs(k[0, q, 1] - (y - 12) / gain) < 1e-2


# ---------------------------------------------------------------------------
# yolo_postprocess_vec (the reference of tests/test_gpu_yolo_nms.py) == the scalar oracle, bit for bit
# ---------------------------------------------------------------------------
VEC_HP, VEC_WP = 192, 256


def _random_heads(seed, nc, nk, box=2.0, quant=None, cls_bias=0.0):
    """Random head maps of a 192x256 canvas (1008 anchors): DFL logits peaked near bin `box`, class
    logits normal (quant: rounded to that step, so most scores tie), raw keypoints with both signs
    of the visibility logit."""
    rng = np.random.default_rng(seed)
    heads = []
    for s in (8, 16, 32):
        h, w = VEC_HP // s, VEC_WP // s
        hd = rng.normal(0.0, 1.0, (h, w, 64 + nc + nk)).astype(np.float32)
        hd[..., :64] -= (0.8 * np.abs(np.arange(16) - box * 8 / s)).astype(np.float32)[np.tile(np.arange(16), 4)]
        hd[..., 64] += np.float32(cls_bias)       # class 0 (person) against the other classes
        if quant:
            hd[..., 64:64 + nc] = np.round(hd[..., 64:64 + nc] / quant) * np.float32(quant)
        heads.append(hd)
    return heads


def _both(heads, conf, iou, max_det, H0, W0, nk=0, **kw):
    a = ra.yolo_postprocess(heads, conf, iou, max_det, VEC_HP, VEC_WP, H0, W0, nk=nk, **kw)
    b = ra.yolo_postprocess_vec(heads, conf, iou, max_det, VEC_HP, VEC_WP, H0, W0, nk=nk, **kw)
    if nk:
        assert a[0].dtype == b[0].dtype == np.float32 and a[1].dtype == b[1].dtype == np.float32
        assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        return a
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(a, b)
    return a, None


# frame 300x420 on the 192x256 canvas: gain 0.6095, pad (0, 5), clipping at the frame edges
VEC_FRAME = (300, 420)


@pytest.mark.parametrize("nc,nk,conf", [(1, 0, 0.6), (80, 0, 0.5), (1, 15, 0.6), (80, 15, 0.5)])
def test_yolo_postprocess_vec_equals_scalar(nc, nk, conf):
    heads = _random_heads(11 + nc + nk, nc, nk, cls_bias=0.0 if nc == 1 else 2.5)
    g, px, py = my.scale_geometry(VEC_HP, VEC_WP, *VEC_FRAME)
    assert g not in (0.0, 1.0) and (px, py) != (0, 0)
    d, k = _both(heads, conf, 0.45, 1000, *VEC_FRAME, nk=nk)
    n = len(ra.yolo_candidate_scores(heads, conf, nk))
    print("candidates", n, "kept", len(d))
    assert n >= 100 and 0 < len(d) < n          # some suppressed
    assert (d[:, :4] == 0).any() or (d[:, 2] == VEC_FRAME[1]).any() or (d[:, 3] == VEC_FRAME[0]).any()   # clipped
    if nk:
        assert (k[..., 2] < 0.5).any() and (k[..., 2] >= 0.5).any()


def test_yolo_postprocess_vec_ties():
    """Class logits on a 0.5 grid: most candidates share their score with another, so the order is
    decided by the anchor index."""
    heads = _random_heads(21, 1, 0, quant=0.5)
    s = ra.yolo_candidate_scores(heads, 0.6)
    _, counts = np.unique(s, return_counts=True)
    tied = int(counts[counts > 1].sum())
    assert len(s) >= 300 and tied >= 0.9 * len(s), (len(s), tied)
    d, _ = _both(heads, 0.6, 0.45, 1000, *VEC_FRAME)
    assert np.all(np.diff(d[:, 4]) <= 0) and len(np.unique(d[:, 4])) < len(d)


def test_yolo_postprocess_vec_max_det_and_max_nms():
    heads = _random_heads(31, 1, 15, box=1.0)
    full, kf = _both(heads, 0.5, 0.45, 1000, *VEC_FRAME, nk=15)
    assert len(full) > 60
    for md in (40, 1):
        d, k = _both(heads, 0.5, 0.45, md, *VEC_FRAME, nk=15)
        assert len(d) == md and np.array_equal(d, full[:md]) and np.array_equal(k, kf[:md])
    # max_nms: only the 50 best candidates enter the NMS; None: all of them
    cut, _ = _both(heads, 0.5, 0.45, 1000, *VEC_FRAME, nk=15, max_nms=50)
    assert 0 < len(cut) < len(full) and np.array_equal(cut, full[:len(cut)])
    unc, _ = _both(heads, 0.5, 0.45, 1000, *VEC_FRAME, nk=15, max_nms=None)
    assert np.array_equal(unc, full)       # below the default 30000 the cut is void
    assert len(ra.yolo_candidate_scores(heads, 0.5, 15)) > 50


def test_yolo_postprocess_vec_empty():
    heads = _random_heads(41, 1, 15)
    d, k = _both(heads, 0.9999, 0.45, 40, *VEC_FRAME, nk=15)
    assert d.shape == (0, 5) and k.shape == (0, 5, 3)
    assert len(ra.yolo_candidate_scores(heads, 0.9999, 15)) == 0


@pytest.mark.parametrize("nkpt", [0, 5])
def test_head_program_interface_and_knobs(nkpt):
    """tests/yolo_head_program.py (the net of tests/test_gpu_yolo_nms.py) through the emulator: three
    heads of 64 + 1 (+ 15) channels at strides 8 / 16 / 32; brightness steers the score, `box` the
    box size, and the interior anchors of constant 64-px tiles tie exactly."""
    import yolo_head_program as yh
    Hp = Wp = 256

    def heads(fr, box):
        x = np.zeros((1, Hp, Wp, 4), np.float32)
        x[0, ..., :3] = fr[..., ::-1].astype(np.float32) / np.float32(255)
        outs = run_program(yh.head_program(Hp, Wp, nkpt, box), x)
        return [o.permute(0, 2, 3, 1).numpy()[0] for o in outs]

    hn = heads(yh.noise_frame(Hp, Wp, 1), 2.0)
    assert [h.shape for h in hn] == [(Hp // s, Wp // s, 65 + 3 * nkpt) for s in (8, 16, 32)]
    nk = 3 * nkpt
    total = Hp * Wp * 21 // 1024
    assert len(ra.yolo_candidate_scores(hn, 0.1, nk)) > 0.95 * total
    assert len(ra.yolo_candidate_scores(heads(yh.dark_frame(Hp, Wp), 2.0), 0.1, nk)) == 0
    small = ra.yolo_postprocess_vec(hn, 0.1, 0.45, total, Hp, Wp, Hp, Wp, nk=nk)
    large = ra.yolo_postprocess_vec(heads(yh.noise_frame(Hp, Wp, 1), 8.0), 0.1, 0.45, total, Hp, Wp, Hp, Wp, nk=nk)
    if nkpt:
        small, large = small[0], large[0]
    assert len(small) > 4 * len(large) > 0
    s = ra.yolo_candidate_scores(heads(yh.tiled_frame(Hp, Wp, 2, lo=32, hi=224), 2.0), 0.0, nk)
    _, counts = np.unique(s, return_counts=True)
    assert counts[counts > 1].sum() >= 16 * 25      # 16 tiles, at least 5x5 interior stride-8 anchors each
