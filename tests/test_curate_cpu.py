"""The curator's NumPy backend and host halves (person_capture_amd/curate.py) against the oracle's
OpenCV restatements, an f64 DCT and a plain restatement of the reference's greedy MMR. No GPU."""
import functools

import numpy as np
import pytest
import scipy.fft

from oracle import cv_ops
from person_capture_amd import curate, utils

from curate_cases import MMR_CASES, PHASH_IMAGES, SHAPES, greedy_mmr, image, mmr_inputs

COEF_TOL = 2.0 ** -22     # one f32 rounding of a coefficient; the f64 sum of 1024 terms is far below it


@functools.lru_cache(maxsize=None)
def backend(h, w, seed=0):
    return curate.crop_metrics_batch([image(h, w, seed)], keep_planes=True)[0]


def rep3(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def dct_ref(p32):
    return scipy.fft.dctn(p32.astype(np.float64), norm="ortho")[:8, :8]


# ---- gray, histogram and sums ----
@pytest.mark.parametrize("h,w", SHAPES)
def test_gray_hist_sums(h, w):
    m = backend(h, w)
    g = cv_ops.gray_u8(image(h, w))
    assert np.array_equal(m.planes["gray"], g)
    assert np.array_equal(m.hist, np.bincount(g.ravel(), minlength=256))
    assert np.array_equal(m.row_sum, g.sum(axis=1)) and np.array_equal(m.col_sum, g.sum(axis=0))
    assert m.hist.dtype == np.uint32 and m.row_sum.dtype == np.uint32 and m.col_sum.dtype == np.uint32


# ---- resize ----
@pytest.mark.parametrize("h,w", SHAPES)
def test_planes_match_cv_resize(h, w):
    m = backend(h, w)
    g3 = rep3(cv_ops.gray_u8(image(h, w)))
    mx = max(h, w)
    if mx <= 256:
        assert (m.w2, m.h2) == (w, h) and np.array_equal(m.planes["g2"], g3[..., 0])
    else:
        s = 256.0 / float(mx)
        assert (m.w2, m.h2) == (int(round(w * s)), int(round(h * s)))
        ref = cv_ops.resize(g3, (m.w2, m.h2), interpolation=cv_ops.INTER_AREA)
        assert np.array_equal(ref[..., 0], ref[..., 1])
        assert np.array_equal(m.planes["g2"], ref[..., 0])
    ref32 = cv_ops.resize(g3, (32, 32), interpolation=cv_ops.INTER_AREA)
    assert m.planes["p32"].shape == (32, 32) and np.array_equal(m.planes["p32"], ref32[..., 0])


def test_thin_planes():
    assert (backend(8200, 32).w2, backend(8200, 32).h2) == (1, 256)
    assert (backend(32, 8200).w2, backend(32, 8200).h2) == (256, 1)


def test_size_limits():
    for shape in [(31, 40, 3), (40, 31, 3), (40, 40, 4), (40, 40)]:
        with pytest.raises(ValueError):
            curate.crop_metrics_batch([np.zeros(shape, np.uint8)])
    with pytest.raises(ValueError):
        curate.plane_plans(32, 16385)
    with pytest.raises(ValueError):
        curate.plane_plans(16384, 32)    # int(round(32 * 256 / 16384)) == 0: cv2.resize raises there too
    assert curate.phash64(None) == 0 and curate.sharpness_norm(None) == 0.0 and curate.exposure_score(None) == 0.0
    assert curate.phash64(np.zeros((0, 0, 3), np.uint8)) == 0
    assert utils.detect_black_borders(None) == (0, 0, 0, 0)


def test_layout_query_is_host_only():
    """pc_crop_metrics_layout needs no device: sizes, offsets and the descriptor checks."""
    import ctypes as C
    from person_capture_amd import _lib
    sizes = [(640, 427), (256, 256), (32, 32), (512, 384)]
    descs, tabs, starts = curate.build_descs(sizes)
    for d, (h, w) in zip(descs, sizes):
        d.row_stride = 3 * w
    off, sb, ob = curate.metrics_layout(descs, len(sizes))
    assert [int(k) for k in descs[0].kind] == [_lib.PC_CURATE_AREA, _lib.PC_CURATE_AREA]
    assert [int(k) for k in descs[1].kind] == [_lib.PC_CURATE_COPY, _lib.PC_CURATE_FAST]
    assert [int(k) for k in descs[2].kind] == [_lib.PC_CURATE_COPY, _lib.PC_CURATE_COPY]
    assert [int(k) for k in descs[3].kind] == [_lib.PC_CURATE_FAST, _lib.PC_CURATE_FAST]
    assert (off[:, :3] % 16 == 0).all() and (off[:, 4] % 16 == 0).all()
    assert off[1, 1] == off[1, 0] and off[2, 1] == off[2, 0] == off[2, 2]      # copies are the gray plane
    assert off[0, 1] == off[0, 0] + 432 * 640 and off[0, 2] == off[0, 1] + 176 * 256
    assert sb == int(off[3, 2]) + 1024
    assert [int(v) for v in off[:, 3]] == [i * _lib.CURATE_RECORD_BYTES for i in range(4)]
    assert ob == int(off[3, 4]) + 4 * (512 + 384)
    for field, value in [("w2", 170), ("h2", 255), ("w", 31), ("h", 16385), ("row_stride", 3 * 427 - 1)]:
        bad = (_lib.CurateDesc * 1)()
        C.memmove(bad, descs, C.sizeof(bad))
        setattr(bad[0], field, value)
        with pytest.raises(ValueError):
            curate.metrics_layout(bad, 1)
    bad = (_lib.CurateDesc * 1)()
    C.memmove(bad, descs, C.sizeof(bad))
    bad[0].kind[0] = _lib.PC_CURATE_FAST       # integer ratios that run past the source
    bad[0].isx[0], bad[0].isy[0] = 3, 3
    with pytest.raises(ValueError):
        curate.metrics_layout(bad, 1)
    assert curate.metrics_layout(descs, 0)[1:] == (0, 0)


# ---- sharpness ----
def _flat(h, w):
    return np.full((h, w, 3), 93, np.uint8)


def _step(h, w):
    img = np.full((h, w, 3), 20, np.uint8)
    img[:, w // 2:] = 220
    return img


@pytest.mark.parametrize("name,img", [("flat", _flat(300, 200)), ("flat_small", _flat(64, 48)),
                                      ("step", _step(300, 200)), ("step_small", _step(40, 70)),
                                      ("noise", image(257, 129)), ("noise_small", image(97, 61)),
                                      ("noise_big", image(640, 427))])
def test_sharpness_sums(name, img):
    m = curate.crop_metrics_batch([img], keep_planes=True)[0]
    g2 = m.planes["g2"]
    ref = cv_ops.face_quality(rep3(g2))
    if name.startswith("flat"):
        assert m.sum_lap == 0 and m.sum_lap2 == 0 and m.lap_var == 0.0 and m.sharpness == 0.0
    else:
        assert ref > 0 and abs(m.lap_var - ref) <= 1e-12 * ref
    assert m.sum_g2 == int(g2.astype(np.int64).sum())
    mean = float(g2.astype(np.float64).mean())
    want = float(np.tanh(np.log1p(ref / (mean * mean + 1e-6))))
    assert abs(m.sharpness - want) <= 1e-12
    assert curate.sharpness_norm(img) == m.sharpness


def test_laplacian_one_pixel_axis():
    """On an axis of length 1 the neighbour is the pixel itself (cv::borderInterpolate)."""
    for h, w in [(8200, 32), (32, 8200)]:
        m = backend(h, w)
        g = m.planes["g2"].astype(np.int64).ravel()
        p = np.pad(g, 1, mode="reflect")
        lap = p[:-2] + p[2:] - 2 * g          # the two neighbours across the thin axis cancel 2 of the -4
        assert (m.sum_lap, m.sum_lap2) == (int(lap.sum()), int((lap * lap).sum()))


# ---- pHash ----
@pytest.mark.parametrize("h,w,seed", PHASH_IMAGES)
def test_dct_coefficients(h, w, seed):
    m = backend(h, w, seed)
    ref = dct_ref(m.planes["p32"])
    assert np.all(np.abs(m.coef.astype(np.float64) - ref) <= COEF_TOL * np.maximum(1.0, np.abs(ref)))


def test_phash_bits():
    assert len(PHASH_IMAGES) >= 8
    for h, w, seed in PHASH_IMAGES:
        m = backend(h, w, seed)
        ref = dct_ref(m.planes["p32"])
        assert curate.phash_margin(ref) > 1e-3, (h, w, seed)      # no coefficient within 1e-3 of the median
        assert m.phash == curate.phash_from_coef(ref.astype(np.float32)), (h, w, seed)
        assert 0 <= m.phash < (1 << 64)
    assert curate.phash64(image(97, 61, 1)) == backend(97, 61, 1).phash


def test_phash_packing():
    coef = np.zeros((8, 8), np.float32)
    coef[0, 0] = 1e6            # DC is zeroed before the median
    coef[0, 1] = 5.0            # bit 1
    coef[7, 7] = 2.0            # bit 63
    assert curate.phash_from_coef(coef) == (1 << 1) | (1 << 63)


# ---- scalar helpers, hand-computed ----
def test_scalar_helpers():
    assert curate.hamming64(0, 0) == 0 and curate.hamming64(0b1011, 0b0001) == 2
    assert curate.hamming64((1 << 64) | 1, 0) == 1           # bits above 64 are masked
    assert curate.hamming64((1 << 64) - 1, 0) == 64
    assert curate.face_fraction(None, 100, 200) == 0.0
    assert curate.face_fraction((10, 20, 50, 70), 100, 200) == 0.25
    assert curate.face_fraction((10, 20, 50, 20), 100, 0) == 1.0
    assert curate.yaw_roll_from_5pts(None) == (0.0, 0.0)
    assert curate.yaw_roll_from_5pts(np.zeros((4, 2))) == (0.0, 0.0)
    pts = np.array([[0, 0], [10, 0], [5, 5], [2, 9], [8, 9]], np.float32)
    yaw, roll = curate.yaw_roll_from_5pts(pts)
    assert yaw == 0.0 and roll == 0.0
    pts[1] = [10, 10]                                        # eye line at 45 degrees
    pts[2] = [5 + 14.142135, 5]
    yaw, roll = curate.yaw_roll_from_5pts(pts)
    assert abs(roll - 45.0) < 1e-4 and abs(yaw - 45.0) < 1e-4
    # (x1, y1, x2, y2) keeps 50 x 50 of 100 x 100; as (x, y, w, h) the same tuple keeps more (75 x 75)
    assert curate._bb_frac_from_tuple((25, 25, 75, 75), 100, 100) == 1.0 - 0.5625
    # only the (x, y, w, h) reading is valid: a <= x
    assert curate._bb_frac_from_tuple((50, 50, 40, 40), 100, 100) == 1.0 - 0.16
    assert curate._bb_frac_from_tuple((0, 0, 100, 100), 100, 100) == 0.0
    assert curate._bb_frac_from_tuple(None, 100, 100) == 0.0 and curate._bb_frac_from_tuple((1, 2, 3), 9, 9) == 0.0
    assert curate._bb_frac_from_tuple((0, 0, -5, -5), 100, 100) == 1.0


def test_quality_score():
    q = curate.quality_score(face_fd=0.25, sharpness=0.5, exposure=1.0, face_quality=600.0)
    assert abs(q - (0.45 * 0.5 + 0.30 * 0.5 + 0.20 + 0.05 * 0.5)) < 1e-15
    assert curate.quality_score(0.9, 0.0, 0.0, 0.0) == 0.0                 # fd beyond 0.5 clips to 0
    assert abs(curate.quality_score(-1.0, 1.0, 1.0, 5000.0) - 1.0) < 1e-15   # every term saturates
    base = curate.quality_score(0.0, 1.0, 1.0, 1200.0)
    assert abs(curate.quality_score(0.0, 1.0, 1.0, 1200.0, wmark=0.5) - base * 0.7) < 1e-15
    # the border fraction is clamped at 0.4
    assert curate.quality_score(0.0, 1.0, 1.0, 1200.0, black_border_frac=0.9) == \
        curate.quality_score(0.0, 1.0, 1.0, 1200.0, black_border_frac=0.4)
    assert abs(curate.quality_score(0.0, 1.0, 1.0, 1200.0, black_border_frac=0.4) - base * 0.76) < 1e-15
    it = curate.Item(face_fd=0.25, sharpness=0.5, exposure=1.0, face_quality=600.0, meta={"black_border_frac": 0.2})
    assert abs(it.quality_score - q * 0.88) < 1e-15


# ---- exposure and borders ----
def test_exposure():
    black = np.zeros((64, 48, 3), np.uint8)
    white = np.full((64, 48, 3), 255, np.uint8)
    mid = np.full((64, 48, 3), 128, np.uint8)
    half = mid.copy()
    half[:32] = 0
    assert curate.exposure_score(black) == 0.0 and curate.exposure_score(white) == 0.0
    assert curate.exposure_score(mid) == 1.0 and curate.exposure_score(half) == 0.25
    # the reference's float32 expressions on a real histogram
    img = image(97, 61)
    hist = np.bincount(cv_ops.gray_u8(img).ravel(), minlength=256).astype(np.float32)
    hist = hist / max(1.0, hist.sum())
    want = float(max(0.0, min(1.0, hist[16:240].sum() - 0.5 * (hist[:8].sum() + hist[-8:].sum()))))
    assert curate.exposure_score(img) == want


def borders_restated(gray, thr=10, max_scan=None):
    """The reference's scan on row and column means, restated."""
    H, W = gray.shape
    if max_scan is None:
        max_scan = max(64, min(H, W) // 8)
    rows = [float(gray[r, :].mean()) for r in range(H)]
    cols = [float(gray[:, c].mean()) for c in range(W)]

    def run(vals, n):
        lo = 0
        while lo < min(n, max_scan) and not vals[lo] > thr:
            lo += 1
        hi = n
        while hi > max(n - max_scan, 0) and not vals[hi - 1] > thr:
            hi -= 1
        return lo, hi

    top, bottom = run(rows, H)
    left, right = run(cols, W)
    cl = lambda v, a, b: max(a, min(b, v))
    left = cl(left, 0, right - 1)
    top = cl(top, 0, bottom - 1)
    right = cl(right, left + 1, W)
    bottom = cl(bottom, top + 1, H)
    return left, top, right, bottom


def test_black_borders():
    box = np.full((200, 160, 3), 200, np.uint8)
    letter = box.copy()
    letter[:20] = 0
    letter[180:] = 3
    pillar = box.copy()
    pillar[:, :30] = 0
    pillar[:, 130:] = 9
    edge = letter.copy()
    edge[20] = 10                       # a row whose mean is exactly thr is still border
    allblack = np.zeros((100, 100, 3), np.uint8)
    assert utils.detect_black_borders(letter) == (0, 20, 160, 180)
    assert utils.detect_black_borders(pillar) == (30, 0, 130, 200)
    assert utils.detect_black_borders(edge) == (0, 21, 160, 180)
    assert utils.detect_black_borders(edge, thr=9) == (0, 20, 160, 180)
    assert utils.detect_black_borders(allblack) == (35, 35, 36, 36)     # the clamps
    assert utils.detect_black_borders(letter, max_scan=10) == (0, 10, 160, 190)
    for img in (letter, pillar, edge, allblack, np.zeros((200, 160, 3), np.uint8), image(97, 61)):
        assert utils.detect_black_borders(img) == borders_restated(cv_ops.gray_u8(img))
        assert curate.crop_metrics_batch([img])[0].black_border == utils.detect_black_borders(img)


# ---- MMR ----
@pytest.mark.parametrize("n,k,alpha,flavour", MMR_CASES)
def test_mmr_matches_restated_loop(n, k, alpha, flavour):
    S, q = mmr_inputs(n, flavour)
    want = greedy_mmr(q, k, S, alpha)
    got = curate.mmr_select_with_q(q, k, S, alpha)
    assert got == want and len(got) == min(k, n) and len(set(got)) == len(got)
    if n == 300:
        assert greedy_mmr(q, k, S, alpha, literal=False) == want


def test_mmr_properties():
    S, q = mmr_inputs(65, "dup")
    order = curate.mmr_select_with_q(q, 65, S, 1.0)
    # alpha = 1 ranks by quality alone; equal qualities come out in ascending index order
    assert order == sorted(range(65), key=lambda i: (-float(q[i]), i))
    assert curate.mmr_select_with_q(q, 65, None, 0.75) == order            # sim_mat=None: quality alone
    assert curate.mmr_select_with_q(q, 7, None, 0.75) == greedy_mmr(q, 7, None, 0.75)
    assert curate.mmr_select_with_q(q, 1000, S, 0.75) == curate.mmr_select_with_q(q, 65, S, 0.75)   # k > n
    assert curate.mmr_select_with_q(np.zeros(0, np.float32), 3, None) == []
    # duplicates: after the first of a pair is picked the second is fully redundant
    S2 = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], np.float32)
    # (0.75 * 0.9 - 0.25 * 1 = 0.425 against 0.75 * 0.7 = 0.525)
    assert curate.mmr_select_with_q(np.array([0.9, 0.9, 0.7], np.float32), 3, S2, 0.75) == [0, 2, 1]
    # negative similarities clamp to 0: the order is by quality
    assert curate.mmr_select_with_q(np.array([0.1, 0.9, 0.5], np.float32), 3, -np.ones((3, 3), np.float32), 0.5) == [1, 2, 0]


def test_mmr_rank_cpu():
    from curate_cases import unit_rows
    F = unit_rows(65, 77, 5, zero_rows=(3, 40))
    q = np.random.default_rng(6).uniform(0, 1, 65).astype(np.float32)
    order, S = curate.mmr_rank(F, q, alpha=0.75, return_sim=True)
    assert S.shape == (65, 65) and not S[3].any() and not S[:, 40].any()
    assert order == greedy_mmr(q, 65, S, 0.75) == curate.mmr_select_with_q(q, 65, S, 0.75)
    assert curate.mmr_rank(F, q, k=5) == order[:5]
