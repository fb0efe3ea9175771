"""YOLOv8 post-processing on the device (yolo_decode, yolo_nms, yolo_nms_big, yolo_kpts) at
scale: long kept lists, ties, the 16384-candidate path edge, ultralytics' max_nms = 30000 cut
and max_det, through the head-only program of tests/yolo_head_program.py (nc = 1: every anchor
is a class-0 candidate).

Every case runs the device pipeline (pc_yolo_detect / pc_yolo_pose_detect), reads back the
device's own f32 heads and feeds them to oracle/ref_algos.yolo_postprocess_vec (pinned bit for
bit to the scalar oracle in tests/test_yolo_cpu.py) with the same conf, iou, max_det and
geometry: identical floats in identical order, the same count, and ncand equal to the
reference's uncapped candidate count. No tolerance. Each case also asserts, from the reference
on the device heads, that it is in the regime it claims (candidate count, kept count, ties).
"""
import numpy as np
import pytest

import yolo_head_program as yh
from oracle import ref_algos as ra
from person_capture_amd.runtime import GpuContext

pytestmark = pytest.mark.gpu

LDS_CAP = 16384      # pc_yolo.hip YNMS_CAP: above it yolo_nms_big takes the image
MAX_NMS = 30000      # pc_yolo.hip YMAX_NMS


def _anchors(Hp, Wp):
    return Hp * Wp * 21 // 1024


@pytest.fixture(scope="module")
def engine(gpu_ctx):
    cache = {}

    def get(Hp, Wp, nkpt=0, box=2.0, max_batch=1):
        key = (Hp, Wp, nkpt, box, max_batch)
        if key not in cache:
            cache[key] = yh.HeadEngine(gpu_ctx, Hp, Wp, nkpt=nkpt, box=box, max_batch=max_batch)
        return cache[key]

    yield get
    for e in cache.values():
        e.net.close()


def _ref(r, fr, eng, conf, iou, max_det, **kw):
    out = ra.yolo_postprocess_vec(r["heads"], conf, iou, max_det, eng.Hp, eng.Wp, fr.shape[0], fr.shape[1],
                                  nk=3 * eng.nkpt, **kw)
    return out if eng.nkpt else (out, None)


def _ncand(r, eng, conf):
    return len(ra.yolo_candidate_scores(r["heads"], conf, 3 * eng.nkpt))


def _tied(r, eng, conf):
    _, counts = np.unique(ra.yolo_candidate_scores(r["heads"], conf, 3 * eng.nkpt), return_counts=True)
    return int(counts[counts > 1].sum())


def _check(name, r, fr, eng, conf, iou, max_det):
    """Device result r of frame fr == the reference on the device's heads. Returns (dets, kpts, ncand)."""
    wd, wk = _ref(r, fr, eng, conf, iou, max_det)
    n = _ncand(r, eng, conf)
    print(f"{name}: ncand {n} (device {r['ncand']}), kept {len(wd)} (device {r['count']}), max_det {max_det}")
    assert r["ncand"] == n
    assert r["count"] == len(wd)
    assert r["dets"].shape == wd.shape and np.array_equal(r["dets"], wd)
    if eng.nkpt:
        assert r["kpts"].shape == wk.shape and np.array_equal(r["kpts"], wk)
    return wd, wk, n


def _same(a, b):
    return (a["count"] == b["count"] and a["ncand"] == b["ncand"] and a["dets"].tobytes() == b["dets"].tobytes()
            and (a["kpts"] is None or a["kpts"].tobytes() == b["kpts"].tobytes()))


# ---- yolo_nms (LDS), 640x640: 8400 anchors ---------------------------------------
def test_lds_long_kept_list_and_max_det(engine):
    eng = engine(640, 640)
    fr = yh.noise_frame(640, 640, 1)
    total = _anchors(640, 640)
    r = eng.detect([fr], 640, 0.1, 0.45, total)[0]
    wd, _, n = _check("lds long", r, fr, eng, 0.1, 0.45, total)
    assert 2000 <= n <= LDS_CAP and 500 <= len(wd) < n       # thousands sorted, a long kept list, some suppressed
    for md in (40, 1):       # the product's max_det, and the smallest
        rc = eng.detect([fr], 640, 0.1, 0.45, md)[0]
        wc, _, _ = _check(f"lds max_det {md}", rc, fr, eng, 0.1, 0.45, md)
        assert len(wc) == md < len(wd) and np.array_equal(wc, wd[:md])


def test_lds_ties(engine):
    eng = engine(640, 640)
    fr = yh.tiled_frame(640, 640, 2, lo=32, hi=224)
    total = _anchors(640, 640)
    r = eng.detect([fr], 640, 0.1, 0.45, total)[0]
    wd, _, n = _check("lds ties", r, fr, eng, 0.1, 0.45, total)
    tied = _tied(r, eng, 0.1)
    print("tied", tied)
    assert n <= LDS_CAP and tied >= 1000
    assert len(np.unique(wd[:, 4])) < len(wd)        # ties among the kept too


def test_empty(engine):
    eng = engine(640, 640)
    for name, fr, conf in (("dark", yh.dark_frame(640, 640), 0.1), ("conf above all", yh.noise_frame(640, 640, 1), 0.999)):
        r = eng.detect([fr], 640, conf, 0.45, 40)[0]
        wd, _, n = _check("empty " + name, r, fr, eng, conf, 0.45, 40)
        assert len(wd) == 0 and n == 0 and r["count"] == 0 and r["ncand"] == 0


# ---- the path edge and yolo_nms_big, 1024x1024: 21504 anchors ---------------------
def test_path_edge_16384_16385(engine):
    eng = engine(1024, 1024, box=4.0)
    fr = yh.noise_frame(1024, 1024, 3)
    first = eng.detect([fr], 1024, 0.1, 0.45, 4096)[0]
    s = ra.yolo_candidate_scores(first["heads"], 0.0)
    assert len(s) == _anchors(1024, 1024)
    assert s[LDS_CAP - 1] > s[LDS_CAP] > s[LDS_CAP + 1]      # distinct scores at the ranks used as thresholds
    for want_n, conf in ((LDS_CAP, float(s[LDS_CAP])), (LDS_CAP + 1, float(s[LDS_CAP + 1]))):
        r = eng.detect([fr], 1024, conf, 0.45, 4096)[0]
        wd, _, n = _check(f"path edge {want_n}", r, fr, eng, conf, 0.45, 4096)
        assert n == want_n and r["ncand"] == want_n
        assert 500 <= len(wd) < 4096


def test_big_path_and_order_independence(engine):
    """P = 32768: one global bitonic stage over four sorted tiles. Run twice: the decode's slot order
    (an atomic counter) varies between runs, the result may not."""
    eng = engine(1024, 1024, box=4.0)
    fr = yh.noise_frame(1024, 1024, 3)
    r = eng.detect([fr], 1024, 0.1, 0.45, 4096)[0]
    wd, _, n = _check("big", r, fr, eng, 0.1, 0.45, 4096)
    assert LDS_CAP < n <= MAX_NMS and 1024 < len(wd) < 4096      # kept list longer than a block, not cut
    again = eng.detect([fr], 1024, 0.1, 0.45, 4096)[0]
    assert _same(r, again)


def test_big_path_max_det_inside_a_block(engine):
    eng = engine(1024, 1024, box=4.0)
    fr = yh.noise_frame(1024, 1024, 3)
    full = None
    for md in (4096, 300, 1):
        r = eng.detect([fr], 1024, 0.1, 0.45, md)[0]
        wd, _, n = _check(f"big max_det {md}", r, fr, eng, 0.1, 0.45, md)
        assert n > LDS_CAP
        if full is None:
            full = wd
            assert len(full) > 300
        else:
            assert len(wd) == md and np.array_equal(wd, full[:md])


def test_big_path_padded_canvas(engine):
    """720x1280 at imgsz 1280: a 736x1280 canvas (19320 anchors), pad_y = 8, boxes clipped to the frame."""
    eng = engine(736, 1280, box=4.0)
    fr = yh.noise_frame(720, 1280, 5)
    r = eng.detect([fr], 1280, 0.1, 0.45, 4096)[0]
    wd, _, n = _check("big padded", r, fr, eng, 0.1, 0.45, 4096)
    assert n > LDS_CAP
    assert (wd[:, 1] == 0).any() and (wd[:, 3] == 720).any() and (wd[:, 0] == 0).any() and (wd[:, 2] == 1280).any()
    assert (wd[:, 3] > 712).any()        # the pad is subtracted: boxes reach the last rows of the frame


def test_big_path_ties(engine):
    eng = engine(1024, 1024, box=4.0)
    fr = yh.tiled_frame(1024, 1024, 4, lo=32, hi=224)
    r = eng.detect([fr], 1024, 0.02, 0.45, 4096)[0]
    wd, _, n = _check("big ties", r, fr, eng, 0.02, 0.45, 4096)
    tied = _tied(r, eng, 0.02)
    print("tied", tied)
    assert n > LDS_CAP and tied >= 1000
    assert len(np.unique(wd[:, 4])) < len(wd)


def test_big_path_max_nms_cut(engine):
    """1280x1280 (33600 anchors, P = 65536), a bright part and a black strip: the strip's anchors
    rank last, and those past rank 30000 never enter the NMS."""
    eng = engine(1280, 1280, box=8.0)
    fr = yh.split_frame(1280, 1280, 6, 256)
    r = eng.detect([fr], 1280, 0.01, 0.45, 1024)[0]
    wd, _, n = _check("big max_nms", r, fr, eng, 0.01, 0.45, 1024)
    assert n > MAX_NMS
    unc, _ = _ref(r, fr, eng, 0.01, 0.45, 1024, max_nms=None)
    print("kept with the cut", len(wd), "without", len(unc))
    assert len(wd) < 1024 and len(unc) > len(wd) and np.array_equal(unc[:len(wd)], wd)


def test_mixed_batch(engine):
    """One launch with an empty image, one of the LDS path and one of the global-memory path."""
    eng = engine(1024, 1024, box=4.0, max_batch=3)
    half = yh.noise_frame(1024, 1024, 8)
    half[:, 512:] = 0
    frames = [yh.dark_frame(1024, 1024), yh.noise_frame(1024, 1024, 3), half]
    got = eng.detect(frames, 1024, 0.1, 0.45, 2048)
    ns = [_check(f"mixed {i}", r, fr, eng, 0.1, 0.45, 2048)[2] for i, (r, fr) in enumerate(zip(got, frames))]
    assert ns[0] == 0 and ns[1] > LDS_CAP and 1000 < ns[2] <= LDS_CAP
    for r, fr in zip(got, frames):
        assert _same(r, eng.detect([fr], 1024, 0.1, 0.45, 2048)[0])


def test_pose_on_the_big_path(engine):
    """keep_anchor handed from yolo_nms_big to yolo_kpts."""
    eng = engine(1024, 1024, nkpt=5, box=7.0)
    fr = yh.noise_frame(1024, 1024, 7)
    r = eng.detect([fr], 1024, 0.1, 0.45, 1024)[0]
    wd, wk, n = _check("pose big", r, fr, eng, 0.1, 0.45, 1024)
    assert n > LDS_CAP and 100 <= len(wd) < 1024         # every block walked, not cut by max_det
    assert (wk[..., 2] < 0.5).any() and (wk[..., 2] >= 0.5).any()
    assert np.all(wk[wk[..., 2] < 0.5][:, :2] == 0) and (wk[wk[..., 2] >= 0.5][:, :2] > 0).any()


# ---- candidate / key scratch shared by every engine of a context ------------------
def test_scratch_reuse_across_canvases_and_batches():
    """ycand / ycount / ybig are regrown by image count and by candidate rows: 640 -> 1280 -> 640,
    batch 1 -> 3 -> 1 on one context gives what single calls on a fresh context give."""
    ctx = GpuContext(0)
    fresh = GpuContext(0)
    try:
        e640 = yh.HeadEngine(ctx, 640, 640, box=2.0, max_batch=3)
        e1280 = yh.HeadEngine(ctx, 1280, 1280, box=8.0)
        f640 = [yh.noise_frame(640, 640, 20 + i) for i in range(3)]
        f1280 = yh.split_frame(1280, 1280, 6, 256)

        def small(frames):
            got = e640.detect(frames, 640, 0.1, 0.45, 300)
            for r, fr in zip(got, frames):
                _check("scratch 640", r, fr, e640, 0.1, 0.45, 300)
            return got

        def big():
            r = e1280.detect([f1280], 1280, 0.01, 0.45, 1024)[0]
            assert _check("scratch 1280", r, f1280, e1280, 0.01, 0.45, 1024)[2] > MAX_NMS
            return r

        a = small(f640[:1])[0]
        b = big()                        # more candidate rows, keys for P = 65536
        assert _same(a, small(f640[:1])[0])      # fewer rows than the scratch holds
        three = small(f640)              # more images, fewer rows each
        assert _same(a, three[0])
        assert _same(b, big())           # one image of more rows than three small ones
        g640 = yh.HeadEngine(fresh, 640, 640, box=2.0)
        for r, fr in zip(three, f640):
            assert _same(r, g640.detect([fr], 640, 0.1, 0.45, 300)[0])
        assert _same(b, yh.HeadEngine(fresh, 1280, 1280, box=8.0).detect([f1280], 1280, 0.01, 0.45, 1024)[0])
    finally:
        ctx.close()
        fresh.close()
