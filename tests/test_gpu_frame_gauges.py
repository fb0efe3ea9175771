"""The frame-gauge kernels (pc_gauge.hip) through the C ABI and through frame_gauges.FrameGauge: every
integer from the device equals the NumPy backend's (the gray plane also oracle.cv_ops.gray_u8), nothing is
written outside what a call owns (guard bytes), refused arguments launch nothing, and a clip gives the
reference's decisions frame by frame and batched."""
import ctypes as C

import numpy as np
import pytest

from person_capture_amd import _lib, curate, frame_gauges as fg, frames, frames_hdr
from person_capture_amd.frame_gauges import FrameGauge

import frame_gauge_cases as fc

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def image(h, w, seed=0):
    return np.random.default_rng(seed * 100003 + h * 131 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def guarded(ctx, nbytes):
    """A device buffer of nbytes between two guards, all filled with FILL: (buffer, pointer of the payload)."""
    host = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
    return ctx.upload(host), host


def read_guarded(ctx, buf, nbytes):
    raw = ctx.download(buf.ptr, (nbytes + 2 * GUARD,), np.uint8)
    assert np.all(raw[:GUARD] == FILL) and np.all(raw[GUARD + nbytes:] == FILL), "guard bytes overwritten"
    return raw[GUARD:GUARD + nbytes]


def run_frame_gray(ctx, items):
    """pc_frame_gray on (image, row_stride, byte shift of the base pointer): every plane and every pair of
    sum arrays in a buffer of its own between guards. Returns [(gray, row_sum, col_sum)]."""
    n = len(items)
    descs = (_lib.GrayDesc * n)()
    keep = []
    for d, (img, stride, shift) in zip(descs, items):
        h, w = img.shape[:2]
        host = np.zeros(h * stride + 64, np.uint8)
        np.lib.stride_tricks.as_strided(host[shift:], (h, w * 3), (stride, 1))[:] = img.reshape(h, w * 3)
        src = ctx.upload(host)
        pitch = (w + 15) & ~15
        plane, _ = guarded(ctx, pitch * h)
        sums, _ = guarded(ctx, 4 * (h + w))
        d.d_src, d.row_stride, d.w, d.h, d.gray_pitch = src.ptr + shift, stride, w, h, pitch
        d.d_gray, d.d_row_sum, d.d_col_sum = plane.ptr + GUARD, sums.ptr + GUARD, sums.ptr + GUARD + 4 * h
        keep.append((src, plane, sums, h, w, pitch))
    _lib.check(ctx.lib.pc_frame_gray(ctx.handle, descs, n), ctx.handle, "frame_gray")
    out = []
    for src, plane, sums, h, w, pitch in keep:
        g = read_guarded(ctx, plane, pitch * h).reshape(h, pitch)
        assert not g[:, w:].any(), "padding bytes of a gray row are written as 0"
        s = read_guarded(ctx, sums, 4 * (h + w)).view(np.uint32)
        out.append((g[:, :w].copy(), s[:h].copy(), s[h:].copy()))
    return out


def check_gray(got, img):
    from oracle.cv_ops import gray_u8
    ref = FrameGauge().measure(img)
    g, rs, cs = got
    assert np.array_equal(g, ref.gray()) and np.array_equal(g, gray_u8(img))
    assert rs.dtype == ref.row_sum.dtype and np.array_equal(rs, ref.row_sum) and np.array_equal(cs, ref.col_sum)


def test_frame_gray_paths(gpu_ctx):
    """34 x 50: rows of 150 bytes, the byte path; 64 x 96: aligned 16-byte loads; a source whose rows are
    further apart than 3 w and whose base is 3 bytes past a 16-byte boundary."""
    items = [(image(34, 50), 150, 0), (image(64, 96), 288, 0), (image(40, 96), 288 + 29, 3), (image(64, 96), 288 + 32, 16)]
    for it, got in zip(items, run_frame_gray(gpu_ctx, items)):
        check_gray(got, it[0])


def test_frame_gray_batches_of_1_and_5(gpu_ctx):
    one = [(image(33, 47, 1), 141, 0)]
    check_gray(run_frame_gray(gpu_ctx, one)[0], one[0][0])
    # widths on both sides of the 2048-pixel row split, heights that are no multiple of the band
    five = [(image(34, 50, 2), 150, 0), (image(97, 1030, 2), 3090, 0), (image(33, 2100, 2), 6300, 0),
            (image(64, 96, 2), 288, 0), (image(130, 513, 2), 1539 + 5, 1)]
    for it, got in zip(five, run_frame_gray(gpu_ctx, five)):
        check_gray(got, it[0])


def test_frame_gray_every_band_height(gpu_ctx):
    """A launch takes bands of 32 rows when that gives 1024 workgroups, else 16, else 8 (the batches above):
    16384 rows make 1024 bands of 16, twice that 1024 of 32. 131 and 193 chunks a row: one row a workgroup
    pass with an idle wave, and two passes over the row."""
    tall = [(image(16384, 40, 6), 120, 0)]
    check_gray(run_frame_gray(gpu_ctx, tall)[0], tall[0][0])
    two = [(image(16384, 33, 7), 99, 0), (image(16384, 35, 7), 105 + 7, 1)]
    for it, got in zip(two, run_frame_gray(gpu_ctx, two)):
        check_gray(got, it[0])
    wide = [(image(40, 2090, 8), 6270, 0), (image(33, 3085, 8), 9255 + 9, 0), (image(35, 4100, 8), 12300, 0)]
    for it, got in zip(wide, run_frame_gray(gpu_ctx, wide)):
        check_gray(got, it[0])


def test_frame_gray_strided_view_and_device_crop(gpu_ctx):
    big = image(80, 140, 3)
    view = big[5:71, 7:119]           # 66 x 112, rows 420 bytes apart, 21 bytes into a row
    ref = FrameGauge().measure(np.ascontiguousarray(view))
    g = FrameGauge(gpu_ctx)
    m = g.measure(view)
    assert np.array_equal(m.gray(), ref.gray()) and np.array_equal(m.row_sum, ref.row_sum)
    assert np.array_equal(m.col_sum, ref.col_sum)
    d = gpu_ctx.upload(big)
    m = g.measure(curate.DeviceCrop(d.ptr + 5 * 420 + 21, 66, 112, 420))
    assert np.array_equal(m.gray(), ref.gray()) and np.array_equal(m.col_sum, ref.col_sum)
    assert m.has_previous and m.motion_counts([(0, 0, 112, 66)]) == [0]


# ---- pc_gray_region_hist ----
def run_hist(ctx, plane, regions, pitch=None):
    h, w = plane.shape
    pitch = w if pitch is None else pitch
    host = np.zeros(h * pitch, np.uint8)[: (h - 1) * pitch + w]   # the plane ends on its last byte
    np.lib.stride_tricks.as_strided(host, (h, w), (pitch, 1))[:] = plane
    d = ctx.upload(host)
    n = len(regions)
    regs = (_lib.GrayRegion * max(n, 1))()
    for r, (x, y, rw, rh) in zip(regs, regions):
        r.d_plane, r.pitch, r.x, r.y, r.w, r.h = d.ptr, pitch, x, y, rw, rh
    out, _ = guarded(ctx, 1024 * n)
    _lib.check(ctx.lib.pc_gray_region_hist(ctx.handle, regs, n, C.c_void_p(out.ptr + GUARD)), ctx.handle, "hist")
    return read_guarded(ctx, out, 1024 * n).view(np.uint32).reshape(n, 256)


def test_region_hist(gpu_ctx):
    rng = np.random.default_rng(11)
    H, W = 70, 93
    plane = rng.integers(0, 256, (H, W), dtype=np.uint8)
    plane[:9] = rng.integers(0, 3, (9, W))      # a nearly constant bar: the run-merging path
    regions = [(40, 0, 1, H), (3, 5, 17, 40), (0, 0, W, H), (0, 0, 12, H), (W - 12, 0, 12, H), (0, 0, W, 9),
               (0, H - 9, W, 9), (W - 20, H - 3, 20, 3), (W - 1, H - 1, 1, 1), (0, 0, 1, 1), (13, 1, 16, 2),
               (16, 0, 32, 1)]
    got = run_hist(gpu_ctx, plane, regions)
    for (x, y, w, h), hst in zip(regions, got):
        assert np.array_equal(hst, fg._hist_np(plane, (x, y, w, h))), (x, y, w, h)
    many = []
    for _ in range(33):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        many.append((x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
    for pitch in (W, 96, 101):   # rows whose alignment differs from row to row, and rows that share it
        got = run_hist(gpu_ctx, plane, many, pitch)
        for r, hst in zip(many, got):
            assert np.array_equal(hst, fg._hist_np(plane, r)), (pitch, r)
            assert int(hst.sum()) == r[2] * r[3]


# ---- pc_gray_motion ----
def run_motion(ctx, cur, prev, boxes, thresh, pitch=None, prev_shift=0):
    h, w = cur.shape
    pitch = w if pitch is None else pitch

    def up(p, shift):
        host = np.zeros(h * pitch + 32, np.uint8)
        np.lib.stride_tricks.as_strided(host[shift:], (h, w), (pitch, 1))[:] = p
        return ctx.upload(host)
    dc, dp = up(cur, 0), up(prev, prev_shift)
    n = len(boxes)
    mb = (_lib.MotionBox * max(n, 1))()
    for m, (x1, y1, x2, y2) in zip(mb, boxes):
        m.d_cur, m.d_prev, m.pitch, m.x1, m.y1, m.x2, m.y2 = dc.ptr, dp.ptr + prev_shift, pitch, x1, y1, x2, y2
    out, _ = guarded(ctx, 4 * max(n, 1))
    _lib.check(ctx.lib.pc_gray_motion(ctx.handle, mb, n, thresh, C.c_void_p(out.ptr + GUARD)), ctx.handle, "motion")
    raw = read_guarded(ctx, out, 4 * max(n, 1)).view(np.uint32)
    return raw[:n].tolist(), raw


def test_motion(gpu_ctx):
    """128 x 512 planes holding every (cur, prev) pair once: the difference takes every value 0 .. 255 with
    both signs."""
    i = np.arange(128 * 512)
    cur = (i // 256).astype(np.uint8).reshape(128, 512)
    prev = (i % 256).astype(np.uint8).reshape(128, 512)
    rng = np.random.default_rng(12)
    boxes = [(0, 0, 512, 128), (3, 1, 200, 77), (17, 0, 18, 1), (511, 127, 512, 128), (0, 5, 1, 6), (250, 3, 262, 128),
             (5, 0, 21, 128), (16, 2, 48, 3)]
    for thresh in (15, 0, 16, 254, 255):
        got, _ = run_motion(gpu_ctx, cur, prev, boxes, thresh)
        assert got == [fg._motion_np(cur, prev, b, thresh) for b in boxes], thresh
    full = run_motion(gpu_ctx, cur, prev, [(0, 0, 512, 128)], 15)[0][0]
    assert full == sum(256 - min(256, c + 16) + max(0, c - 15) for c in range(256))   # strictly more than 15
    many = []
    for _ in range(65):
        x1, y1 = int(rng.integers(0, 512)), int(rng.integers(0, 128))
        many.append((x1, y1, int(rng.integers(x1 + 1, 513)), int(rng.integers(y1 + 1, 129))))
    want = [fg._motion_np(cur, prev, b, 15) for b in many]
    assert run_motion(gpu_ctx, cur, prev, many, 15)[0] == want
    # a pitch that is no multiple of 16, and a previous plane 5 bytes out of step with the current one
    assert run_motion(gpu_ctx, cur, prev, many, 15, pitch=517)[0] == want
    assert run_motion(gpu_ctx, cur, prev, many, 15, pitch=528, prev_shift=5)[0] == want
    got, raw = run_motion(gpu_ctx, cur, prev, [], 15)   # 0 boxes: PC_OK, nothing written
    assert got == [] and np.all(raw.view(np.uint8) == FILL)


# ---- the small plane ----
@pytest.mark.parametrize("h,w,kind,small", [(120, 200, "copy", (120, 200)), (1080, 1920, "area_fast", (216, 384)),
                                            (700, 1000, "area", (269, 384))])
def test_small_plane(gpu_ctx, h, w, kind, small):
    assert fg.small_plane_plan(h, w)["kind"] == kind
    img = image(h, w, 4)
    ref = FrameGauge().measure(img).small_plane()
    m = FrameGauge(gpu_ctx).measure(img)
    got = m.small_plane()
    assert got.shape == small == ref.shape and np.array_equal(got, ref)
    sal, sx, sy = m.saliency()
    assert sal.shape == small and sx == small[1] / w and sy == small[0] / h


# ---- argument checks ----
def test_argument_checks_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    img = image(64, 96)
    src = ctx.upload(img)
    plane, _ = guarded(ctx, 96 * 64)
    sums, _ = guarded(ctx, 4 * 160)
    hist, _ = guarded(ctx, 2048)
    cnt, _ = guarded(ctx, 8)

    def gray_desc(**kw):
        d = (_lib.GrayDesc * 2)()
        for k in range(2):
            d[k].d_src, d[k].row_stride, d[k].w, d[k].h, d[k].gray_pitch = src.ptr, 288, 96, 64, 96
            d[k].d_gray, d[k].d_row_sum, d[k].d_col_sum = plane.ptr + GUARD, sums.ptr + GUARD, sums.ptr + GUARD + 256
        for k, v in kw.items():
            setattr(d[1], k, v)   # the second frame of the batch is the bad one
        return d
    bad_gray = [dict(w=31), dict(h=16385), dict(row_stride=287), dict(gray_pitch=100), dict(gray_pitch=80),
                dict(d_src=None), dict(d_gray=plane.ptr + GUARD + 4), dict(d_row_sum=sums.ptr + GUARD + 2),
                dict(d_col_sum=None)]
    for kw in bad_gray:
        assert ctx.lib.pc_frame_gray(ctx.handle, gray_desc(**kw), 2) == 1, kw
    assert ctx.lib.pc_frame_gray(ctx.handle, gray_desc(), -1) == 1
    assert ctx.lib.pc_frame_gray(ctx.handle, None, 1) == 1
    assert ctx.lib.pc_frame_gray(ctx.handle, None, 0) == 0

    def region(**kw):
        r = (_lib.GrayRegion * 2)()
        for k in range(2):
            r[k].d_plane, r[k].pitch, r[k].x, r[k].y, r[k].w, r[k].h = plane.ptr + GUARD, 96, 0, 0, 96, 64
        for k, v in kw.items():
            setattr(r[1], k, v)
        return r
    out = C.c_void_p(hist.ptr + GUARD)
    for kw in (dict(w=0), dict(h=0), dict(x=-1), dict(y=-1), dict(x=1), dict(w=97), dict(d_plane=None), dict(h=16385),
               dict(y=16384), dict(pitch=(1 << 20) + 16)):
        assert ctx.lib.pc_gray_region_hist(ctx.handle, region(**kw), 2, out) == 1, kw
    assert ctx.lib.pc_gray_region_hist(ctx.handle, region(), 2, None) == 1
    assert ctx.lib.pc_gray_region_hist(ctx.handle, region(), 2, C.c_void_p(hist.ptr + GUARD + 2)) == 1
    assert ctx.lib.pc_gray_region_hist(ctx.handle, region(), -1, out) == 1
    assert ctx.lib.pc_gray_region_hist(ctx.handle, region(), 65536, out) == 1

    def box(**kw):
        b = (_lib.MotionBox * 2)()
        for k in range(2):
            b[k].d_cur, b[k].d_prev, b[k].pitch = plane.ptr + GUARD, plane.ptr + GUARD, 96
            b[k].x1, b[k].y1, b[k].x2, b[k].y2 = 0, 0, 96, 64
        for k, v in kw.items():
            setattr(b[1], k, v)
        return b
    outc = C.c_void_p(cnt.ptr + GUARD)
    for kw in (dict(x1=-1), dict(y1=-1), dict(x2=0), dict(y2=0), dict(x1=96), dict(x2=97), dict(d_cur=None),
               dict(d_prev=None), dict(y2=16385)):
        assert ctx.lib.pc_gray_motion(ctx.handle, box(**kw), 2, 15, outc) == 1, kw
    assert ctx.lib.pc_gray_motion(ctx.handle, box(), 2, -1, outc) == 1
    assert ctx.lib.pc_gray_motion(ctx.handle, box(), 2, 256, outc) == 1
    assert ctx.lib.pc_gray_motion(ctx.handle, box(), 2, 15, None) == 1
    assert ctx.lib.pc_gray_motion(ctx.handle, box(), -1, 15, outc) == 1

    xt, xs = fg.imageops.area_tables(96, 40)
    yt, ys = fg.imageops.area_tables(64, 30)
    small, _ = guarded(ctx, 48 * 32)

    def resize(kind=_lib.PC_CURATE_AREA, w=96, h=64, ow=40, oh=30, isx=0, isy=0, dpitch=48, xtab=xt, nx=None):
        return ctx.lib.pc_gray_resize_area(ctx.handle, C.c_void_p(plane.ptr + GUARD), 96, w, h, kind, isx, isy, xtab, xs,
                                           len(xt) if nx is None else nx, yt, ys, len(yt),
                                           C.c_void_p(small.ptr + GUARD), dpitch, ow, oh)
    assert resize(kind=_lib.PC_CURATE_COPY) == 1
    assert resize(kind=_lib.PC_CURATE_FAST, isx=3, isy=2) == 1       # 40 * 3 > 96
    assert resize(kind=_lib.PC_CURATE_FAST, isx=2, isy=0) == 1
    assert resize(ow=97) == 1 and resize(oh=65) == 1 and resize(dpitch=39) == 1 and resize(w=97) == 1
    assert resize(w=95) == 1                                         # the x table reads column 95
    assert resize(xtab=None) == 1 and resize(nx=len(xt) - 1) == 1
    ctx.sync()
    # nothing was launched: every output still holds its fill
    for buf, nbytes in ((plane, 96 * 64), (sums, 640), (hist, 2048), (cnt, 8), (small, 48 * 32)):
        assert np.all(ctx.download(buf.ptr, (nbytes + 2 * GUARD,), np.uint8) == FILL)
    assert resize() == 0                                             # and the good call works
    got = read_guarded(ctx, small, 48 * 32).reshape(32, 48)[:30, :40]
    src_plane = np.full((64, 96), FILL, np.uint8)
    assert np.array_equal(got, curate._resize_area_np(src_plane, fg.imageops.resize_plan(64, 96, dsize=(40, 30), area=True)))


# ---- sequences ----
def test_clip_frame_by_frame_and_batched(gpu_ctx):
    golden = fc.load_golden()
    host = fc.clip_run(FrameGauge(), batch=False)
    one = fc.clip_run(FrameGauge(gpu_ctx), batch=False)
    fc.check_clip(golden, one)
    many = fc.clip_run(FrameGauge(gpu_ctx), batch=True)
    fc.check_clip(golden, many)
    fc.same_runs(one, many)
    fc.same_runs(one, host)


def test_previous_plane_reset_resize_and_recycling(gpu_ctx):
    g = FrameGauge(gpu_ctx)
    a, b = fc.clip_frame(0), fc.clip_frame(1)
    ref = FrameGauge()
    ref.measure(a)
    want = ref.measure(b).motion_counts(fc.CLIP_BOXES)
    m0 = g.measure(a)
    assert m0.motion_counts(fc.CLIP_BOXES) is None
    m1 = g.measure(b)
    assert m1.motion_counts(fc.CLIP_BOXES) == want
    g.reset()
    assert not g.measure(a).has_previous
    small = np.ascontiguousarray(b[:64, :96])
    m = g.measure(small)                    # another size: no previous plane (gui_app.py:4276)
    assert not m.has_previous and m.motion_counts([(0, 0, 5, 5)]) is None
    m2 = g.measure(small)
    assert m2.motion_counts([(0, 0, 96, 64)]) == [0]
    n_planes = len(g._pool)
    for _ in range(4):
        g.measure(small)
    assert len(g._pool) == n_planes          # the planes go round, none is added
    with pytest.raises(RuntimeError):
        m2.motion_counts([(0, 0, 96, 64)])   # its planes have been handed out again


def test_measure_gray_on_device(gpu_ctx):
    """A gray plane the caller holds is uploaded as it is (98 columns: a pitch of 112) and chains with
    measured frames."""
    a, b = image(66, 98, 30), image(66, 98, 31)
    ref = FrameGauge()
    ga = ref.measure(a).gray()
    want = ref.measure(b)
    boxes = [(0, 0, 98, 66), (7, 3, 50, 40)]
    g = FrameGauge(gpu_ctx)
    g.measure_gray(ga)
    m = g.measure(b)
    assert m.motion_counts(boxes) == want.motion_counts(boxes)
    m2 = g.measure_gray(ga)
    assert np.array_equal(m2.gray(), ga) and m2.motion_counts(boxes) == want.motion_counts(boxes)
    assert np.array_equal(m2.strip_hists([(90, 0, 8, 66)]), fg._hist_np(ga, (90, 0, 8, 66))[None])


def test_border_and_motion_cases_on_device(gpu_ctx):
    golden = fc.load_golden()
    g = FrameGauge(gpu_ctx)
    ms = g.measure_batch([fc.border_frame(n) for n in fc.BORDER_NAMES])
    for i, (name, m) in enumerate(zip(fc.BORDER_NAMES, ms)):
        roi, acc = m.autocrop_borders(fc.THR, fc.SCAN_FRAC)
        assert roi == tuple(int(v) for v in golden["border_roi"][i]) and acc == bool(golden["border_accepted"][i]), name
    assert ms[fc.BORDER_NAMES.index("both")].strip_calls == 1 and ms[fc.BORDER_NAMES.index("one_sided_top")].strip_calls == 0
    g.reset()
    prev, cur = fc.motion_pair()
    m = g.measure_batch([prev, cur])[1]
    for cfg in fc.CFGS:
        idx = [i for i, (b, c, l) in enumerate(fc.MOTION_CASES) if c == cfg and l is None]
        got = m.faceless_validate_batch([fc.MOTION_CASES[i][0] for i in idx], fc.CFGS[cfg])
        assert got == [(bool(golden["motion_ok"][i]), fc.REASONS[int(golden["motion_reason"][i])]) for i in idx]
    open_idx = [i for i, c in enumerate(fc.MOTION_CASES) if golden["motion_count"][i] >= 0]
    assert m.motion_counts([fc.MOTION_CASES[i][0] for i in open_idx]) == [int(golden["motion_count"][i]) for i in open_idx]


def test_nv12_and_hdr_frames(gpu_ctx):
    rng = np.random.default_rng(21)
    H, W = 66, 98
    nv = frames.Nv12Frame(rng.integers(0, 256, H * W * 3 // 2, dtype=np.uint8), H, W)
    hdr = frames_hdr.HdrFrame(rng.random(3 * H * W, dtype=np.float32), H, W, "pq", 200.0, 1000.0)
    bgr = image(H, W, 5)
    want = [frames.nv12_to_bgr(nv, gpu_ctx), frames_hdr.hdr_to_bgr(hdr, gpu_ctx), bgr]
    ref = FrameGauge().measure_batch(want)
    got = FrameGauge(gpu_ctx).measure_batch([nv, hdr, bgr])
    boxes = [(3, 2, 90, 60), (0, 0, W, H)]
    for r, m in zip(ref, got):
        assert np.array_equal(m.gray(), r.gray()) and np.array_equal(m.row_sum, r.row_sum)
        assert np.array_equal(m.col_sum, r.col_sum) and m.motion_counts(boxes) == r.motion_counts(boxes)
        assert np.array_equal(m.strip_hists([(0, 0, W, 7), (5, 0, 9, H)]), r.strip_hists([(0, 0, W, 7), (5, 0, 9, H)]))
