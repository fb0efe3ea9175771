"""SCRFD post-processing on the device (scrfd_decode, scrfd_nms, scrfd_nms_big) at its own
edges: score ties, the 8160-candidate path edge and the first global sort stage, max_det cuts,
nms_thresh 0 and 1, empty images and a batch that mixes all three kinds, through the head-only
program of tests/scrfd_head_program.py at D = 640 (16800 anchors).

Every case runs pc_scrfd_detect, reads back the device's own f32 heads and feeds them to
oracle/ref_algos.scrfd_detect_post with the call's det_thresh, det_scale and nms_thresh: identical
floats in identical order, count equal to the reference's full kept number (also above max_det),
ncand equal to the reference's candidate count, and every row at or past min(count, max_det) (and
GUARD rows past the buffers' end) still holding the byte pattern they were prefilled with. No
tolerance. Each case asserts from the device heads that it is in the regime it claims.

Where a case needs exactly K candidates, det_thresh is the K-th largest score of the device's
heads (f64 sigmoid rounded to f32, as the oracle and the kernel compute it), which must exceed the
(K+1)-th: score >= det_thresh then holds for exactly K anchors.
"""
import numpy as np
import pytest

import scrfd_head_program as sh
from oracle import ref_algos as ra

pytestmark = pytest.mark.gpu

D = 640
ANCHORS = 16800
NMS_CAP = 8160       # pc_detect.hip: above it scrfd_nms_big takes the image
BIG_TILE = 8192      # pc_detect.hip: scrfd_nms_big sorts tiles of this many keys in the LDS


@pytest.fixture(scope="module")
def engine(gpu_ctx):
    cache = {}

    def get(shared=False):
        if shared not in cache:
            cache[shared] = sh.HeadEngine(gpu_ctx, D, box=2.0, shared=shared, max_batch=3)
        return cache[shared]

    yield get
    for e in cache.values():
        e.net.close()


@pytest.fixture(scope="module")
def heads_of(engine):
    """The device's head tensors of one frame (they do not depend on the thresholds), once per frame."""
    cache = {}

    def get(name, frame, shared=False):
        key = (name, shared)
        if key not in cache:
            r = engine(shared).detect([frame], 2.0, 0.4, 1)[0]
            assert r["count"] == 0 and r["ncand"] == 0
            cache[key] = r["heads"]
        return cache[key]

    return get


def _scores(heads):
    """Every anchor's score in anchor order, as ref_algos.scrfd_decode computes it."""
    return np.concatenate([(1.0 / (1.0 + np.exp(-h[..., 0:2].astype(np.float64)))).astype(np.float32).reshape(-1)
                           for h in heads])


def _thresh_for(heads, K):
    s = np.sort(_scores(heads))[::-1]
    assert len(s) == ANCHORS
    if K == ANCHORS:
        return 0.0
    assert s[K - 1] > s[K], "the scores at the ranks used as the threshold must differ"
    return float(s[K - 1])


def _untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == sh.FILL))


def _check(name, r, det_thresh, nms_thresh, max_det, want_k=None):
    """Device result r == the reference on the device's heads. Returns the reference's full (dets, kps) and K."""
    wd, wk = ra.scrfd_detect_post(r["heads"], det_thresh, r["det_scale"], nms_thresh)
    wk = wk.reshape(-1, 10)
    K = int((_scores(r["heads"]) >= np.float32(det_thresh)).sum())
    print(f"{name}: ncand {K} (device {r['ncand']}), kept {len(wd)} (device {r['count']}), max_det {max_det}")
    if want_k is not None:
        assert K == want_k
    assert r["ncand"] == K
    assert r["count"] == len(wd)
    m = min(len(wd), max_det)
    assert np.array_equal(r["dets"][:m], wd[:m])
    assert np.array_equal(r["kps"][:m], wk[:m])
    assert _untouched(r["dets"][m:]) and _untouched(r["kps"][m:])
    if "guard" in r:
        assert _untouched(r["guard"][0]) and _untouched(r["guard"][1])
    return wd, wk, K


def _order_and_keep(heads, det_thresh, det_scale, nms_thresh):
    """(candidates in the NMS walk order [K][5], walk positions of the kept ones), by the oracle's own steps."""
    pre, _ = ra.scrfd_decode(heads, det_thresh, det_scale)
    pre = pre[np.argsort(pre[:, 4], kind="stable")[::-1]]
    walk = np.argsort(pre[:, 4], kind="stable")[::-1]         # scrfd_nms_keep's order: score desc, anchor asc
    pos = np.empty(len(walk), np.int64)
    pos[walk] = np.arange(len(walk))
    return pre[walk], pos[np.asarray(ra.scrfd_nms_keep(pre, nms_thresh), np.int64)]


def _iou(a, b):
    """SCRFD.nms overlap of box rows a and b ('+1' areas, f32)."""
    one = np.float32(1)
    w = np.maximum(np.float32(0), np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]) + one)
    h = np.maximum(np.float32(0), np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]) + one)
    inter = w * h
    area = lambda q: (q[:, 2] - q[:, 0] + one) * (q[:, 3] - q[:, 1] + one)
    return inter / (area(a) + area(b) - inter)


def _tie_stats(heads, det_thresh, det_scale, nms_thresh):
    """(candidates whose score another candidate shares, neighbours in the walk order with one score
    and an overlap above nms_thresh: pairs whose order decides which of the two is kept)."""
    walk, _ = _order_and_keep(heads, det_thresh, det_scale, nms_thresh)
    _, counts = np.unique(walk[:, 4], return_counts=True)
    same = walk[1:, 4] == walk[:-1, 4]
    over = _iou(walk[:-1], walk[1:]) > np.float32(nms_thresh)
    return int(counts[counts > 1].sum()), int((same & over).sum())


# ---- ties -------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["neighbours", "same_centre"])
def test_lds_ties(engine, heads_of, shared):
    """Tiled frame: neighbouring anchors of a tile (and, shared, the two anchors of a location) have
    bit-equal scores and overlapping boxes, so the anchor-index tie order decides the kept set."""
    eng = engine(shared)
    fr = sh.tiled_frame(D, D, 2)
    heads = heads_of("tiled", fr, shared)
    s = np.sort(_scores(heads))[::-1]
    thr = float(s[6000])                 # ties may straddle this rank: K >= 6001, asserted <= NMS_CAP
    r = eng.detect([fr], thr, 0.4, ANCHORS)[0]
    wd, _, K = _check("lds ties", r, thr, 0.4, ANCHORS)
    tied, deciding = _tie_stats(r["heads"], thr, r["det_scale"], 0.4)
    print("tied", tied, "tied overlapping neighbours", deciding)
    assert 6000 < K <= NMS_CAP and tied >= 1000 and deciding >= 100
    assert len(np.unique(wd[:, 4])) < len(wd)        # ties among the kept too
    if shared:
        sc = _scores(r["heads"]).reshape(-1, 2)
        assert np.array_equal(sc[:, 0], sc[:, 1])        # every location: a same-centre tie, IoU 1
        assert tied == K


def test_big_ties(engine, heads_of):
    """The same frame at det_thresh 0: K = 16800, P = 32768."""
    eng = engine()
    fr = sh.tiled_frame(D, D, 2)
    r = eng.detect([fr], 0.0, 0.4, ANCHORS)[0]
    wd, _, K = _check("big ties", r, 0.0, 0.4, ANCHORS, want_k=ANCHORS)
    tied, deciding = _tie_stats(r["heads"], 0.0, r["det_scale"], 0.4)
    print("tied", tied, "tied overlapping neighbours", deciding)
    assert tied >= 1000 and deciding >= 100
    assert len(np.unique(wd[:, 4])) < len(wd)


# ---- the path edge ------------------------------------------------------------------
@pytest.mark.parametrize("K", [NMS_CAP - 1, NMS_CAP, NMS_CAP + 1, BIG_TILE, BIG_TILE + 1, 2 * BIG_TILE])
def test_path_edge(engine, heads_of, K):
    """8159 / 8160: the last LDS counts; 8161: the first of scrfd_nms_big; 8192: P == BIG_TILE, no
    global stage; 8193: the first global stage; 16384: the most candidates one global stage sorts."""
    eng = engine()
    fr = sh.noise_frame(D, D, 1)
    thr = _thresh_for(heads_of("noise1", fr), K)
    r = eng.detect([fr], thr, 0.4, ANCHORS)[0]
    wd, _, _ = _check(f"path edge {K}", r, thr, 0.4, ANCHORS, want_k=K)
    assert 64 < len(wd) < K          # more than one block of kept boxes, some suppressed


def test_big_path_slot_order_independence(engine, heads_of):
    """The decode's slot order (an atomic counter) may differ between two runs; the result may not."""
    eng = engine()
    fr = sh.noise_frame(D, D, 1)
    a = eng.detect([fr], 0.0, 0.4, ANCHORS)[0]
    _check("big, first run", a, 0.0, 0.4, ANCHORS, want_k=ANCHORS)
    b = eng.detect([fr], 0.0, 0.4, ANCHORS)[0]
    assert a["count"] == b["count"] and a["ncand"] == b["ncand"]
    assert a["dets"].tobytes() == b["dets"].tobytes() and a["kps"].tobytes() == b["kps"].tobytes()


# ---- max_det ----------------------------------------------------------------------
@pytest.mark.parametrize("K,block,max_det", [(8000, 64, 100), (2 * BIG_TILE, 1024, 300)], ids=["lds", "big"])
def test_max_det_cut_inside_a_block(engine, heads_of, K, block, max_det):
    """count is the full kept number, rows [0, max_det) are the first max_det of the full list and
    nothing is written past them, with the cut between two kept boxes of one block of the walk."""
    eng = engine()
    fr = sh.noise_frame(D, D, 1)
    heads = heads_of("noise1", fr)
    thr = _thresh_for(heads, K)
    _, kept_pos = _order_and_keep(heads, thr, 1.0, 0.4)
    assert len(kept_pos) > max_det
    assert kept_pos[max_det - 1] // block == kept_pos[max_det] // block       # the cut falls inside a block
    assert kept_pos[max_det - 1] >= block                                     # and not in the first one
    r = eng.detect([fr], thr, 0.4, max_det)[0]
    assert r["det_scale"] == 1.0
    wd, _, _ = _check(f"max_det {max_det} at K {K}", r, thr, 0.4, max_det, want_k=K)
    assert r["count"] == len(wd) == len(kept_pos) > max_det
    r1 = eng.detect([fr], thr, 0.4, 1)[0]
    _check(f"max_det 1 at K {K}", r1, thr, 0.4, 1, want_k=K)


# ---- nms_thresh 0 and 1 -------------------------------------------------------------
@pytest.mark.parametrize("K", [NMS_CAP, NMS_CAP + 140], ids=["lds", "big"])
def test_nms_thresh_one_keeps_all(engine, heads_of, K):
    """Nothing is suppressed: the longest kept list of the LDS kernel, one barrier round per box in
    the big one."""
    eng = engine()
    fr = sh.noise_frame(D, D, 1)
    thr = _thresh_for(heads_of("noise1", fr), K)
    r = eng.detect([fr], thr, 1.0, ANCHORS)[0]
    wd, _, _ = _check(f"nms 1.0 at K {K}", r, thr, 1.0, ANCHORS, want_k=K)
    assert len(wd) == K and r["count"] == K


@pytest.mark.parametrize("K", [NMS_CAP, NMS_CAP + 140], ids=["lds", "big"])
def test_nms_thresh_zero_keeps_disjoint(engine, heads_of, K):
    eng = engine()
    fr = sh.noise_frame(D, D, 1)
    thr = _thresh_for(heads_of("noise1", fr), K)
    r = eng.detect([fr], thr, 0.0, ANCHORS)[0]
    wd, _, _ = _check(f"nms 0.0 at K {K}", r, thr, 0.0, ANCHORS, want_k=K)
    assert 1 < len(wd) < K // 8
    i, j = np.triu_indices(len(wd), 1)
    assert np.all(_iou(wd[i], wd[j]) == 0)           # only disjoint boxes survive


# ---- empty and mixed ------------------------------------------------------------------
def test_empty(engine):
    eng = engine()
    fr = sh.dark_frame(D, D)
    r = eng.detect([fr], 0.5, 0.4, 64)[0]
    assert _scores(r["heads"]).max() < 0.5
    wd, _, K = _check("empty", r, 0.5, 0.4, 64, want_k=0)
    assert len(wd) == 0 and r["count"] == 0 and r["ncand"] == 0
    assert _untouched(r["dets"]) and _untouched(r["kps"])


def test_mixed_batch(engine):
    """One launch: an empty image, one of the LDS kernel and one of the global-memory kernel (each
    kernel is launched over all three and leaves the others' images alone), at three frame sizes:
    det_scale 2, 1 and 0.5."""
    eng = engine()
    frames = [sh.dark_frame(320, 320), sh.split_frame(D, D, 3, 288), sh.noise_frame(1280, 1280, 4)]
    max_det = 4096
    got = eng.detect(frames, 0.3, 0.4, max_det)
    thr = float(np.float32(0.3))
    assert [r["det_scale"] for r in got] == [2.0, 1.0, 0.5]
    res = [_check(f"mixed {i}", r, thr, 0.4, max_det) for i, r in enumerate(got)]
    ks = [k for _, _, k in res]
    assert ks[0] == 0 and 1000 < ks[1] <= NMS_CAP < ks[2]
    assert len(res[0][0]) == 0 and 64 < len(res[1][0]) < max_det and 64 < len(res[2][0]) < max_det
