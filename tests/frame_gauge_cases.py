"""Inputs of the frame-gauge tests (test_frame_gauges_cpu.py, test_gpu_frame_gauges.py) and of the golden
generator (tools/gen_golden_gauges.py), rebuilt from seeds: only the reference's outputs are stored in
tests/golden/frame_gauges.npz.

Frames are 120 x 160 BGR with B = G = R, so the gray value of a pixel is the byte written (the
14-bit coefficients sum to 2^14). THR = 10 gives max_luma = 18, the p99 cap 22 and max_std 3.5."""
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_gauges.npz")
H, W = 120, 160
THR = 10
SCAN_FRAC = 0.25

# name: (top, bottom, left, right, bar kind)
#   black     all 0                              noisy     uniform 0 .. 5 (std about 1.7)
#   p99       2 % of the bar at 24, rest 0: p95 = 0, std about 3.4, p99 = 24 > 22 (only p99 rejects)
#   subtitle  four 200-valued pixels in each of ten rows of a bar (a row's mean stays at 5)
#   textured  uniform 0 .. 14: p95, p99 <= 14, std about 4.3 > 3.5 (only std rejects)
BORDER_CASES = {
    "sym_bars": (14, 14, 0, 0, "black"),
    "sym_noisy": (14, 14, 0, 0, "noisy"),
    "one_sided_top": (14, 0, 0, 0, "black"),
    "one_sided_left": (0, 0, 20, 0, "black"),
    "unequal_beyond_tol": (10, 30, 0, 0, "black"),
    "unequal_within_tol": (14, 16, 0, 0, "black"),
    "subtitle_p99": (14, 14, 0, 0, "p99"),
    "subtitle_bright": (14, 14, 0, 0, "subtitle"),
    "textured_std": (14, 14, 0, 0, "textured"),
    "pillarbox": (0, 0, 21, 19, "noisy"),
    "both": (12, 12, 17, 17, "noisy"),
    "no_border": (0, 0, 0, 0, "black"),
}
BORDER_NAMES = tuple(BORDER_CASES)


def _bar(rng, shape, kind):
    n = shape[0] * shape[1]
    if kind == "black":
        return np.zeros(shape, np.uint8)
    if kind == "noisy":
        return rng.integers(0, 6, shape, dtype=np.uint8)
    if kind == "textured":
        return rng.integers(0, 15, shape, dtype=np.uint8)
    if kind == "p99":
        v = np.zeros(n, np.uint8)
        v[rng.permutation(n)[:int(round(0.02 * n))]] = 24
        return v.reshape(shape)
    if kind == "subtitle":
        v = np.zeros(shape, np.uint8)
        for r in range(2, 12):
            v[r, rng.permutation(shape[1])[:4]] = 200
        return v
    raise KeyError(kind)


def border_frame(name: str) -> np.ndarray:
    top, bottom, left, right, kind = BORDER_CASES[name]
    rng = np.random.default_rng(1000 + BORDER_NAMES.index(name))
    g = rng.integers(60, 256, (H, W), dtype=np.uint8)
    if top:
        g[:top] = _bar(rng, (top, W), kind)
    if bottom:
        g[H - bottom:] = _bar(rng, (bottom, W), kind)
    if left:
        g[:, :left] = _bar(rng, (H, left), kind)
    if right:
        g[:, W - right:] = _bar(rng, (H, right), kind)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


# ---- motion ----
CFG_DEFAULT = types.SimpleNamespace(faceless_min_area_frac=0.03, faceless_max_area_frac=0.55,
                                    faceless_center_max_frac=0.12, faceless_min_motion_frac=0.02)
CFG_OPEN = types.SimpleNamespace(faceless_min_area_frac=0.0, faceless_max_area_frac=1.0,
                                 faceless_center_max_frac=0.12, faceless_min_motion_frac=0.02)
CFGS = {"default": CFG_DEFAULT, "open": CFG_OPEN}


def motion_pair():
    """(prev, cur) BGR frames. Columns 0 .. 39 differ by exactly 15 (not motion), 40 .. 79 by exactly 16
    (motion), both signs by row parity; 80 .. 119 are equal; 120 .. 159 differ at random."""
    rng = np.random.default_rng(77)
    p = rng.integers(40, 200, (H, W), dtype=np.int32)
    c = p.copy()
    sign = np.where(np.arange(H)[:, None] % 2 == 0, 1, -1)
    c[:, 0:40] += 15 * sign
    c[:, 40:80] += 16 * sign
    c[:, 120:] = rng.integers(0, 256, (H, 40))
    to3 = lambda g: np.ascontiguousarray(np.repeat(g.astype(np.uint8)[:, :, None], 3, axis=2))
    return to3(p), to3(c)


# (box x1, y1, x2, y2 as the detector hands them out: floats; cfg name; lock_last_bbox or None)
MOTION_CASES = (
    ((2.0, 3.0, 38.0, 100.0), "open", None),             # differences of exactly 15: count 0 -> "motion"
    ((41.0, 3.0, 79.0, 100.0), "open", None),            # exactly 16: every pixel moved
    ((33.4, 10.6, 47.5, 90.2), "open", None),            # straddles 15 | 16, unaligned x1
    ((81.0, 0.0, 119.0, 120.0), "open", None),           # equal planes
    ((50.2, 60.4, 50.9, 60.6), "open", None),            # rounds to an empty box: 1 x 1 at (50, 60), moved
    ((10.0, 10.0, 10.0, 10.0), "open", None),            # 1 x 1 at (10, 10), difference 15
    ((150.4, 100.2, 171.0, 130.0), "open", None),        # clamped at the frame's right and bottom edge
    ((-20.0, -5.0, 30.0, 40.0), "open", None),           # clamped at the left and top edge
    ((0.0, 0.0, 160.0, 120.0), "open", None),            # the whole frame: "ok" by motion, area_max by default
    ((0.0, 0.0, 160.0, 120.0), "default", None),
    ((3.0, 3.0, 9.0, 9.0), "default", None),             # area_min
    ((100.0, 20.0, 158.0, 110.0), "default", (0, 0, 40, 40)),     # center_drift
    ((100.0, 20.0, 158.0, 110.0), "default", (95, 25, 60, 80)),   # near the lock: decided by motion
    ((60.0, 20.0, 118.0, 110.0), "default", (55, 25, 60, 80)),    # 16-columns + equal columns
)

REASONS = (None, "area_min", "area_max", "center_drift", "motion")


# ---- the clip of the sequence test ----
CLIP_LEN = 6
CLIP_BOXES = ((30.0, 20.0, 90.0, 100.0), (80.0, 30.0, 130.0, 100.0), (5.0, 16.0, 20.0, 30.0))


def clip_frame(t: int) -> np.ndarray:
    """Frame t of a letterboxed clip (bars of 14 rows, values 0 .. 3): a textured background that stays,
    and a bright 40 x 50 block that moves 7 columns per frame."""
    g = np.random.default_rng(5).integers(60, 200, (H, W), dtype=np.uint8)
    x = 20 + 7 * t
    g[30:80, x:x + 40] = np.random.default_rng(50 + t).integers(200, 256, (50, 40), dtype=np.uint8)
    bars = np.random.default_rng(90 + t)
    g[:14] = bars.integers(0, 4, (14, W), dtype=np.uint8)
    g[H - 14:] = bars.integers(0, 4, (14, W), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


def clip_run(gauge, batch: bool):
    """The clip through gauge.measure frame by frame, or through one measure_batch: per frame
    (autocrop_borders, has_previous, motion_counts, faceless decisions, row_sum, col_sum, gray plane)."""
    frames = [clip_frame(t) for t in range(CLIP_LEN)]
    ms = gauge.measure_batch(frames) if batch else None
    out = []
    for t in range(CLIP_LEN):
        m = ms[t] if batch else gauge.measure(frames[t])
        out.append((m.autocrop_borders(THR, SCAN_FRAC), m.has_previous, m.motion_counts(CLIP_BOXES),
                    m.faceless_validate_batch(CLIP_BOXES, CFG_OPEN), m.row_sum, m.col_sum, m.gray()))
    return out


def check_clip(golden, run) -> None:
    """A clip_run against the reference's decisions."""
    for t, ((roi, acc), has_prev, counts, decisions, _, _, _) in enumerate(run):
        assert roi == tuple(int(v) for v in golden["clip_roi"][t]) and acc == bool(golden["clip_accepted"][t])
        assert has_prev == (t > 0)
        assert counts == (None if t == 0 else [int(c) for c in golden["clip_count"][t]])
        assert decisions == [(bool(o), REASONS[int(r)]) for o, r in zip(golden["clip_ok"][t], golden["clip_reason"][t])]


def same_runs(a, b) -> None:
    for ra, rb in zip(a, b):
        assert ra[:4] == rb[:4]
        for x, y in zip(ra[4:], rb[4:]):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def load_golden():
    return np.load(GOLDEN)
