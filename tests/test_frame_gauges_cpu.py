"""frame_gauges on the NumPy backend: the host halves against NumPy itself (percentile_from_hist ==
np.percentile bit for bit, std_from_hist against np.std within the recorded bound) and every golden
case of the reference's own _autocrop_borders / _is_real_letterbox_crop / _faceless_validate
(tools/gen_golden_gauges.py) reproduced exactly, integers and decisions."""
import numpy as np
import pytest

from person_capture_amd import frame_gauges as fg
from person_capture_amd.frame_gauges import FrameGauge

import frame_gauge_cases as fc

# np.std of a float32 vector rounds the mean, every deviation and square, their pairwise sum, the
# quotient and the root in f32: a handful of roundings of 2^-24 each on the way to the result. Eight of
# them is the bound; the largest difference seen is 6.1e-8 on the golden strips, 1.8e-7 on the vectors below.
STD_REL_BOUND = 8 * 2.0 ** -24


def _hist(v):
    return np.bincount(np.asarray(v, np.uint8), minlength=256)


def _vectors():
    rng = np.random.default_rng(3)
    for n in (1, 2, 19, 20, 21, 100, 101, 2000):
        yield f"random{n}", rng.integers(0, 256, n)
        yield f"dark{n}", rng.integers(0, 24, n)
        yield f"const{n}", np.full(n, 7)
        two = np.full(n, 3)
        two[:n // 3] = 200
        yield f"two{n}", two
        # the lower order statistic of p95 sits on the 18 of max_luma: floor(0.95 (n - 1)) values up to 18
        k = int(np.floor(np.float32(n - 1) * (np.float32(95) / np.float32(100))))
        edge = np.full(n, 40)
        edge[:k + 1] = 18
        edge[:k] = rng.integers(0, 19, k)
        yield f"edge{n}", edge


@pytest.mark.parametrize("q", [95.0, 99.0])
def test_percentile_from_hist_equals_numpy(q):
    for name, v in _vectors():
        want = float(np.percentile(v.astype(np.uint8).reshape(-1).astype(np.float32), q))
        got = fg.percentile_from_hist(_hist(v), q)
        assert got == want, (name, q, got, want)


def test_percentile_lower_statistic_on_threshold():
    """n = 21: the virtual index of p95 is 19: the answer is the 20th value itself, 18 = max_luma, and the
    strip passes p95 (<=) whatever the largest value is."""
    v = np.array([18] * 20 + [255])
    assert fg.percentile_from_hist(_hist(v), 95.0) == float(np.percentile(v.astype(np.float32), 95.0)) == 18.0


def test_std_from_hist_against_numpy():
    worst = 0.0
    for name, v in _vectors():
        want = float(np.std(v.astype(np.uint8).astype(np.float32)))
        got = fg.std_from_hist(_hist(v))
        exact = float(np.std(v.astype(np.float64)))
        assert abs(got - exact) <= 1e-12 * max(1.0, exact), name   # the f64 two-pass value is close to exact
        if got == 0.0:
            assert want == 0.0, name
            continue
        worst = max(worst, abs(want - got) / got)
        assert abs(want - got) <= STD_REL_BOUND * got, (name, want, got)
    print(f"largest relative |np.std f32 - std_from_hist| {worst:.3e}")
    assert float(fc.load_golden()["std_rel_diff_max"]) <= STD_REL_BOUND


def test_std_from_hist_is_exactly_rounded():
    from fractions import Fraction
    v = np.random.default_rng(9).integers(0, 256, 777)
    h = _hist(v)
    n, s1, s2 = len(v), int(v.sum()), int((v.astype(np.int64) ** 2).sum())
    var = Fraction(n * s2 - s1 * s1, n * n)
    got = fg.std_from_hist(h)
    lo, hi = np.nextafter(got, 0.0), np.nextafter(got, np.inf)
    # got is the nearest double to sqrt(var): var lies between the squares of the neighbouring midpoints
    assert ((Fraction(lo) + Fraction(got)) / 2) ** 2 <= var <= ((Fraction(got) + Fraction(hi)) / 2) ** 2


@pytest.fixture(scope="module")
def golden():
    return fc.load_golden()


@pytest.mark.parametrize("name", fc.BORDER_NAMES)
def test_border_cases_reproduce_the_reference(golden, name):
    i = fc.BORDER_NAMES.index(name)
    m = FrameGauge().measure(fc.border_frame(name))
    roi, accepted = m.autocrop_borders(fc.THR, fc.SCAN_FRAC)
    assert roi == tuple(int(v) for v in golden["border_roi"][i]) and accepted == bool(golden["border_accepted"][i])
    h, w = m.shape
    x1, y1, x2, y2 = m.black_borders(fc.THR, int(round(min(h, w) * fc.SCAN_FRAC)))
    assert m.is_real_letterbox_crop((x1, y1, x2, y2), fc.THR) == bool(golden["border_real"][i])


def test_border_cases_cover_every_rule(golden):
    acc = dict(zip(fc.BORDER_NAMES, golden["border_accepted"]))
    assert acc["sym_bars"] and acc["pillarbox"] and acc["both"] and acc["unequal_within_tol"]
    for name in ("one_sided_top", "one_sided_left", "unequal_beyond_tol", "subtitle_p99", "subtitle_bright",
                 "textured_std"):
        assert not acc[name], name
    # which rule rejects: the geometric ones ask for no histogram, p99 and std each alone
    g = FrameGauge()
    for name in ("one_sided_top", "unequal_beyond_tol", "no_border"):
        m = g.measure(fc.border_frame(name))
        m.autocrop_borders(fc.THR, fc.SCAN_FRAC)
        assert m.strip_calls == 0, name
    max_luma = 18.0
    m = g.measure(fc.border_frame("subtitle_p99"))
    hst = m.strip_hists([(0, 0, fc.W, 14)])[0]
    assert fg.percentile_from_hist(hst, 95.0) <= max_luma and fg.std_from_hist(hst) <= fg.MAX_STD
    assert fg.percentile_from_hist(hst, 99.0) > max_luma + 4.0
    m = g.measure(fc.border_frame("textured_std"))
    hst = m.strip_hists([(0, 0, fc.W, 14)])[0]
    assert fg.percentile_from_hist(hst, 95.0) <= max_luma and fg.percentile_from_hist(hst, 99.0) <= max_luma + 4.0
    assert fg.std_from_hist(hst) > fg.MAX_STD
    m = g.measure(fc.border_frame("both"))
    assert m.autocrop_borders(fc.THR, fc.SCAN_FRAC)[1] and m.strip_calls == 1   # four strips, one call


def test_motion_cases_reproduce_the_reference(golden):
    prev, cur = fc.motion_pair()
    g = FrameGauge()
    g.measure(prev)
    m = g.measure(cur)
    assert m.has_previous
    for i, (box, cfg, lock) in enumerate(fc.MOTION_CASES):
        ok, reason = m.faceless_validate(box, fc.CFGS[cfg], lock)
        assert (ok, reason) == (bool(golden["motion_ok"][i]), fc.REASONS[int(golden["motion_reason"][i])]), (i, box)
        want = int(golden["motion_count"][i])
        if want >= 0:
            assert m.motion_counts([box]) == [want], (i, box)
    # the batch form: one call, the same answers
    for cfg in fc.CFGS:
        boxes = [b for b, c, l in fc.MOTION_CASES if c == cfg and l is None]
        idx = [i for i, (b, c, l) in enumerate(fc.MOTION_CASES) if c == cfg and l is None]
        got = m.faceless_validate_batch(boxes, fc.CFGS[cfg])
        assert got == [(bool(golden["motion_ok"][i]), fc.REASONS[int(golden["motion_reason"][i])]) for i in idx]
    counts = dict(zip([c[0] for c in fc.MOTION_CASES], golden["motion_count"]))
    assert counts[(2.0, 3.0, 38.0, 100.0)] == 0                      # exactly 15 is no motion
    assert counts[(41.0, 3.0, 79.0, 100.0)] == (79 - 41) * (100 - 3)  # exactly 16 is
    assert counts[(50.2, 60.4, 50.9, 60.6)] == 1 and counts[(10.0, 10.0, 10.0, 10.0)] == 0   # 1 x 1 boxes


def test_clip_frame_by_frame_and_batched(golden):
    one = fc.clip_run(FrameGauge(), batch=False)
    fc.check_clip(golden, one)
    many = fc.clip_run(FrameGauge(), batch=True)
    fc.check_clip(golden, many)
    fc.same_runs(one, many)


class _Processor:
    """What the drop-ins touch of the reference's Processor."""
    _autocrop_borders = fg.processor_autocrop_borders
    _is_real_letterbox_crop = fg.processor_is_real_letterbox_crop
    _faceless_validate = fg.processor_faceless_validate

    def __init__(self, auto_crop):
        import types
        self.cfg = types.SimpleNamespace(border_scan_frac=fc.SCAN_FRAC, auto_crop_borders=auto_crop, **vars(fc.CFG_OPEN))
        self._prev_gray, self._lock_last_bbox, self.messages = None, None, []

    def _status(self, msg, **kw):
        self.messages.append(msg)


@pytest.mark.parametrize("auto_crop", [True, False])
def test_processor_drop_ins_on_the_clip(golden, auto_crop):
    """The three methods as Processor.run calls them (gui_app.py:5754-5761, 7695, 8000), with the border
    crop on (every frame measured once, the motion count from that measurement) and off (the planes the
    Processor holds)."""
    p = _Processor(auto_crop)
    for t in range(fc.CLIP_LEN):
        frame = fc.clip_frame(t)
        gray = FrameGauge().measure(frame).gray()
        if auto_crop:
            out, (ox, oy) = p._autocrop_borders(frame, fc.THR)
            assert (ox, oy, ox + out.shape[1], oy + out.shape[0]) == tuple(int(v) for v in golden["clip_roi"][t])
        got = [p._faceless_validate(b, frame.shape, gray) for b in fc.CLIP_BOXES]
        assert got == [(bool(o), fc.REASONS[int(r)]) for o, r in zip(golden["clip_ok"][t], golden["clip_reason"][t])], t
        p._prev_gray = gray.copy()
    assert p.messages == []
    q = _Processor(True)
    for i, name in enumerate(fc.BORDER_NAMES):
        frame = fc.border_frame(name)
        out, (ox, oy) = q._autocrop_borders(frame, fc.THR)
        assert (ox, oy, ox + out.shape[1], oy + out.shape[0]) == tuple(int(v) for v in golden["border_roi"][i]), name
    assert len(q.messages) == int(golden["border_status"].sum())


def test_measure_gray_takes_the_plane_as_it_is():
    a, b = fc.clip_frame(2), fc.clip_frame(3)
    ref = FrameGauge()
    ref.measure(a)
    want = ref.measure(b)
    g = FrameGauge()
    g.measure_gray(FrameGauge().measure(a).gray())
    m = g.measure_gray(want.gray())
    assert np.array_equal(m.row_sum, want.row_sum) and np.array_equal(m.col_sum, want.col_sum)
    assert m.motion_counts(fc.CLIP_BOXES) == want.motion_counts(fc.CLIP_BOXES)
    with pytest.raises(ValueError):
        g.measure_gray(a)


def test_previous_plane_rules():
    g = FrameGauge()
    a, b = fc.clip_frame(0), fc.clip_frame(1)
    assert g.measure(a).motion_counts([(0, 0, 10, 10)]) is None
    assert g.measure(b).motion_counts([(0, 0, 10, 10)]) is not None
    g.reset()
    assert not g.measure(a).has_previous
    small = np.ascontiguousarray(b[:64, :96])
    m = g.measure(small)                       # another size: no previous plane (gui_app.py:4276)
    assert not m.has_previous and m.faceless_validate((0, 0, 90, 60), fc.CFG_OPEN) == (True, None)
    assert g.measure(small).has_previous


def test_saliency_plane_and_patch_mean():
    rng = np.random.default_rng(4)
    frame = rng.integers(0, 256, (100, 200, 3), dtype=np.uint8)
    m = FrameGauge().measure(frame)
    sal, sx, sy = m.saliency()
    assert sal.shape == (100, 200) and sal.dtype == np.float32 and (sx, sy) == (1.0, 1.0)   # W <= 384: identity
    g = m.gray().astype(np.int64)
    p = np.pad(g, 1, mode="reflect")
    gx = sum(k * (p[1 + dy:101 + dy, 2:] - p[1 + dy:101 + dy, :-2]) for dy, k in ((-1, 1), (0, 2), (1, 1)))
    gy = sum(k * (p[2:, 1 + dx:201 + dx] - p[:-2, 1 + dx:201 + dx]) for dx, k in ((-1, 1), (0, 2), (1, 1)))
    mag = np.sqrt((gx * gx + gy * gy).astype(np.float32))
    want = np.clip(mag / float(np.percentile(mag, 95)), 0.0, 1.0)
    assert np.array_equal(sal, want)
    assert m.saliency_of((10, 20, 50, 60)) == float(np.mean(want[20:60, 10:50]))
    assert m.saliency_of((190, 95, 500, 500)) == float(np.mean(want[95:100, 190:200]))
    big = FrameGauge().measure(rng.integers(0, 256, (350, 500, 3), dtype=np.uint8))
    sal, sx, sy = big.saliency()
    assert sal.shape == (269, 384) and sx == 384 / 500.0 and sy == 269 / 350.0


def test_refusals():
    g = FrameGauge()
    with pytest.raises(ValueError):
        g.measure(np.zeros((31, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        g.measure(np.zeros((64, 64, 3), np.float32))
    with pytest.raises(ValueError):
        fg.small_plane_size(100, 15)
    from person_capture_amd.curate import DeviceCrop
    with pytest.raises(ValueError):
        g.measure(DeviceCrop(4096, 64, 64, 192))
