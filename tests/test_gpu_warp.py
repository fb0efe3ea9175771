"""pc_warp_affine (pc_image.hip warp_affine_u8) at its edges, bit for bit against
oracle/cv_ops.c cv_warp_affine_u8: BORDER_CONSTANT, output sizes mixed in one call, degenerate
crops, reflection many periods out, the +-32768 saturation of the source coordinate, exact .5
rounding ties, mirrored maps and workgroup counts that are no multiple of 8.

Layout of every call: the sources are crops inside one larger uploaded frame (row_stride > 3 w, a
crop pointer that is not 16-byte aligned, some crops on the frame's last row and column); the
destinations are packed into one buffer, each followed by a gap of GAP pattern bytes that must be
intact afterwards (the grid is sized by the largest job: the spare workgroups of a smaller job
must write nothing). The oracle gets the same dst -> src matrix iM as the descriptor carries.
Every case computes the source coordinates on the CPU as the kernel does and asserts that it
reaches the regime it is about.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cv_ops
from person_capture_amd import imageops
from person_capture_amd._lib import WarpDesc, check

pytestmark = pytest.mark.gpu

FH, FW = 150, 181            # the frame: row stride 543 bytes, odd
GAP = 37                     # pattern bytes after every destination (keeps the next one unaligned)
PATTERN = 0xC3
REFLECT, REFLECT_101 = imageops.BORDER_REFLECT, imageops.BORDER_REFLECT_101
BORDERS = [imageops.border_constant(114), REFLECT, REFLECT_101]


@pytest.fixture(scope="module")
def frame(gpu_ctx):
    f = np.random.default_rng(77).integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    return f, gpu_ctx.upload(f)


def _job(x0, y0, w, h, iM, ow, oh, border):
    assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= FW and y0 + h <= FH
    return (x0, y0, w, h, np.ascontiguousarray(iM, np.float64).reshape(6), ow, oh, border)


def _inv(M_fwd):
    return cv_ops.invert_affine(np.asarray(M_fwd, np.float64).reshape(6))


def _coords(iM, ow, oh):
    """The kernel's fixed-point source coordinates (cv::warpAffine: AB_BITS 10, INTER_BITS 5) of an
    ow x oh output: sx, sy [oh][ow] before the +-32768 clamp."""
    x = np.arange(ow, dtype=np.float64)
    y = np.arange(oh, dtype=np.float64)
    ad = np.rint(iM[0] * x * 1024).astype(np.int64)
    bd = np.rint(iM[3] * x * 1024).astype(np.int64)
    X0 = np.rint((iM[1] * y + iM[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((iM[4] * y + iM[5]) * 1024).astype(np.int64) + 16
    assert max(np.abs(ad).max(), np.abs(bd).max(), np.abs(X0).max(), np.abs(Y0).max()) < 2 ** 30
    return (X0[:, None] + ad[None, :]) >> 10, (Y0[:, None] + bd[None, :]) >> 10


def _run(ctx, frame, jobs):
    """One pc_warp_affine call over `jobs`; every job against the oracle, every gap intact."""
    f, d_f = frame
    rs = f.strides[0]
    offs, total = [], 0
    for (_, _, _, _, _, ow, oh, _) in jobs:
        offs.append(total)
        total += ow * oh * 3 + GAP
    d_out = ctx.alloc(total)
    ctx.memset(d_out.ptr, PATTERN, total)
    arr = (WarpDesc * len(jobs))()
    unaligned = 0
    for d, off, (x0, y0, w, h, iM, ow, oh, border) in zip(arr, offs, jobs):
        d.d_src = d_f.ptr + y0 * rs + x0 * 3
        unaligned += d.d_src % 16 != 0
        d.row_stride, d.w, d.h = rs, w, h
        for i in range(6):
            d.M[i] = float(iM[i])
        d.d_dst = d_out.ptr + off
        d.out_w, d.out_h, d.border = ow, oh, border
    assert unaligned > 0 and all(rs > 3 * j[2] for j in jobs)
    check(ctx.lib.pc_warp_affine(ctx.handle, arr, len(jobs)), ctx.handle, "warp_affine")
    got = ctx.download(d_out.ptr, (total,), np.uint8)
    d_out.free()
    lib = cv_ops.lib()
    for k, (off, (x0, y0, w, h, iM, ow, oh, border)) in enumerate(zip(offs, jobs)):
        crop = f[y0:y0 + h, x0:x0 + w]
        ref = np.empty((oh, ow, 3), np.uint8)
        lib.cv_warp_affine_u8(C.c_void_p(crop.ctypes.data), rs, w, h, C.c_void_p(iM.ctypes.data),
                              C.c_void_p(ref.ctypes.data), ow, oh, border)
        n = ow * oh * 3
        g = got[off:off + n].reshape(oh, ow, 3)
        assert np.array_equal(g, ref), f"job {k}: crop {(x0, y0, w, h)} -> {ow}x{oh}, border {border:#x}, " \
                                       f"{int((g != ref).any(axis=2).sum())} pixels differ"
        assert np.all(got[off + n:off + n + GAP] == PATTERN), f"job {k}: bytes after the destination overwritten"


def _workgroups(jobs):
    gx = (max(j[5] * j[6] for j in jobs) + 255) // 256
    return gx * len(jobs)


# ---- BORDER_CONSTANT -----------------------------------------------------------------
def _tap_flag_sets(jobs):
    seen = set()
    for (_, _, w, h, iM, ow, oh, _) in jobs:
        sx, sy = _coords(iM, ow, oh)
        x0, x1 = (sx >= 0) & (sx < w), (sx + 1 >= 0) & (sx + 1 < w)
        y0, y1 = (sy >= 0) & (sy < h), (sy + 1 >= 0) & (sy + 1 < h)
        flags = np.stack([x0 & y0, x1 & y0, x0 & y1, x1 & y1], axis=-1).reshape(-1, 4)
        seen |= {tuple(int(v) for v in r) for r in np.unique(flags, axis=0)}
    return seen


# the four taps (x, y), (x+1, y), (x, y+1), (x+1, y+1) of a pixel lie in a 2x2 square, so these are
# all the in/out combinations there are: inside, outside, the four edges and the four corners
_ALL_TAP_FLAGS = {(1, 1, 1, 1), (0, 0, 0, 0),
                  (1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 0, 0), (0, 0, 1, 1),
                  (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)}


@pytest.mark.parametrize("value", [0, 114, 255])
def test_border_constant_every_tap_combination(gpu_ctx, frame, value):
    b = imageops.border_constant(value)
    ang = 0.5
    rot = _inv([1.7 * np.cos(ang), -1.7 * np.sin(ang), 9.0, 1.7 * np.sin(ang), 1.7 * np.cos(ang), 4.0])
    jobs = [_job(7, 5, 10, 8, [1, 0, -4.3, 0, 1, -5.6], 20, 20, b),          # the crop with a margin all round
            _job(FW - 21, FH - 17, 21, 17, rot, 61, 47, b),                # rotated, on the last row and column
            _job(33, 20, 1, 1, [0.25, 0, -1.1, 0, 0.25, -1.2], 12, 12, b),   # one pixel: never two taps of a row inside
            _job(90, 40, 40, 30, [0.5, 0, 3.3, 0, 0.5, 2.2], 50, 40, b)]     # fully inside
    for j in jobs:
        assert _tap_flag_sets([j]) <= _ALL_TAP_FLAGS
    assert _tap_flag_sets(jobs[:2]) == _ALL_TAP_FLAGS
    assert _tap_flag_sets(jobs[3:]) == {(1, 1, 1, 1)}
    _run(gpu_ctx, frame, jobs)


# ---- output sizes mixed in one call -----------------------------------------------------
@pytest.mark.parametrize("border", BORDERS, ids=["constant", "reflect", "reflect101"])
def test_mixed_output_sizes(gpu_ctx, frame, border):
    """1x1, 7x5, 112x112, 160x96 and a whole crop rolled by 90 degrees (w x h -> h x w), one call: the
    grid has 60 workgroups per job, of which the small jobs use one."""
    w, h = 90, 61
    jobs = []
    for k, (ow, oh) in enumerate([(1, 1), (7, 5), (112, 112), (160, 96)]):
        ang, sc = 0.3 * k - 0.4, 0.6 + 0.5 * k
        M = [sc * np.cos(ang), -sc * np.sin(ang), 3.0 + 2 * k, sc * np.sin(ang), sc * np.cos(ang), -2.0 + k]
        jobs.append(_job(11 + 6 * k, 3 + 4 * k, 50 + 7 * k, 40 + 5 * k, _inv(M), ow, oh, border))
    jobs.append(_job(FW - w, FH - h, w, h, _inv([0, -1, h - 1, 1, 0, 0]), h, w, border))     # (x, y) -> (h-1-y, x)
    sx, sy = _coords(jobs[-1][4], h, w)
    assert sx.min() == 0 and sx.max() == w - 1 and sy.min() == 0 and sy.max() == h - 1       # the whole crop, exactly
    assert _workgroups(jobs) == 60 * 5
    _run(gpu_ctx, frame, jobs[::-1])
    _run(gpu_ctx, frame, jobs)


# ---- degenerate crops -------------------------------------------------------------------
@pytest.mark.parametrize("border", [REFLECT, REFLECT_101], ids=["reflect", "reflect101"])
def test_degenerate_crops(gpu_ctx, frame, border):
    """1x1, 1xN, Nx1 and 2x2 crops read far outside themselves (len == 1 always gives 0)."""
    ang = 0.7
    rot = [1.9 * np.cos(ang), -1.9 * np.sin(ang), -20.0, 1.9 * np.sin(ang), 1.9 * np.cos(ang), -30.0]
    jobs = []
    for k, (w, h) in enumerate([(1, 1), (1, 9), (9, 1), (2, 2), (1, 2), (2, 1)]):
        x0, y0 = (FW - w, FH - h) if k % 2 else (13 + 10 * k, 7 + 3 * k)
        jobs.append(_job(x0, y0, w, h, [0.37, 0, -6.2, 0, 0.41, -7.9], 40, 36, border))
        jobs.append(_job(x0, y0, w, h, rot, 33, 29, border))
        sx, sy = _coords(jobs[-1][4], 33, 29)
        assert sx.min() < -w and sx.max() > 2 * w and sy.min() < -h and sy.max() > 2 * h
    _run(gpu_ctx, frame, jobs)


# ---- reflection many periods out -------------------------------------------------------
@pytest.mark.parametrize("border", [REFLECT, REFLECT_101], ids=["reflect", "reflect101"])
@pytest.mark.parametrize("length", [2, 3, 13])
def test_reflection_far_out(gpu_ctx, frame, border, length):
    """The kernel's closed-form reflection against the oracle's loop, tens of periods away on both
    sides of the crop, in both axes."""
    jobs = []
    for (w, h) in [(length, length), (length, 17), (23, length)]:
        s = 1.25 * max(w, h)
        iM = [s, 0.31, -40.0 * w - 0.3, -0.23, s * h / max(w, h) + 0.5, -40.0 * h - 0.6]
        j = _job(FW - w - 5, FH - h, w, h, iM, 64, 64, border)
        sx, sy = _coords(j[4], 64, 64)
        assert sx.min() < -10 * w and sx.max() > 10 * w and sy.min() < -10 * h and sy.max() > 10 * h
        assert max(np.abs(sx).max(), np.abs(sy).max()) < 32768
        jobs.append(j)
    _run(gpu_ctx, frame, jobs)


# ---- saturation of the source coordinate ---------------------------------------------------
@pytest.mark.parametrize("border", BORDERS, ids=["constant", "reflect", "reflect101"])
def test_coordinate_saturation(gpu_ctx, frame, border):
    """X >> 5 is clamped to [-32768, 32767] (OpenCV keeps it in a short) before the border rule."""
    jobs = []
    for (w, h), iM in [((13, 11), [1100.0, 0, -34000.3, 0, 1100.0, -34000.7]),
                       ((13, 11), [-1100.0, 3.0, 35000.2, 5.0, -1100.0, 35000.4]),
                       ((6, 7), [1100.0, 0, -34000.3, 0, 0.5, 1.0]),           # x alone
                       ((6, 7), [0.5, 0, 1.0, 0, 1100.0, -34000.7])]:          # y alone
        j = _job(19, 23, w, h, iM, 64, 64, border)
        sx, sy = _coords(j[4], 64, 64)
        if abs(iM[0]) > 1:
            assert sx.min() < -32768 and sx.max() > 32767
        if abs(iM[4]) > 1:
            assert sy.min() < -32768 and sy.max() > 32767
        jobs.append(j)
    _run(gpu_ctx, frame, jobs)


# ---- exact .5 rounding ties ----------------------------------------------------------------
def _halves(v):
    """(ties with an even integer part, ties with an odd one) among the values v."""
    fl = np.floor(v)
    tie = (v - fl) == 0.5
    return int((tie & (fl % 2 == 0)).sum()), int((tie & (fl % 2 == 1)).sum())


@pytest.mark.parametrize("border", [imageops.border_constant(114), REFLECT], ids=["constant", "reflect"])
def test_rounding_ties(gpu_ctx, frame, border):
    """__double2int_rn against lrint at exact halves (round half to even) in all four products of
    the coordinate: M[0] x 1024, M[3] x 1024, (M[1] y + M[2]) 1024 and (M[4] y + M[5]) 1024,
    with positive and negative values. Every term is exact in f64 (a few bits each)."""
    u = 1.0 / 1024
    mats = [[1 + 0.5 * u, 1.5 * u, 3.0, 0.5 * u, 1 + 1.5 * u, 2.0 + 0.5 * u],
            [-(1 + 0.5 * u), -1.5 * u, 70.0, -0.5 * u, -(1 + 1.5 * u), 60.0 - 0.5 * u]]
    ow, oh = 64, 48
    x, y = np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64)
    jobs = []
    for iM in mats:
        for v in (iM[0] * x * 1024, iM[3] * x * 1024, (iM[1] * y + iM[2]) * 1024, (iM[4] * y + iM[5]) * 1024):
            even, odd = _halves(v)
            assert even >= 4 and odd >= 4, (even, odd)
        jobs.append(_job(21, 9, 80, 70, iM, ow, oh, border))
    _run(gpu_ctx, frame, jobs)


# ---- mirrored maps -------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS, ids=["constant", "reflect", "reflect101"])
def test_mirror(gpu_ctx, frame, border):
    mats = [[-1.3, 0.2, 100.0, 0.1, 1.1, 5.0], [0.9, 0.3, -4.0, 0.4, -0.8, 70.0], [0.2, 1.4, 3.0, 1.2, 0.1, -6.0]]
    jobs = []
    for k, M in enumerate(mats):
        assert M[0] * M[4] - M[1] * M[3] < 0
        jobs.append(_job(31 + k, 17 + k, 70, 55, _inv(M), 112, 112, border))
    _run(gpu_ctx, frame, jobs)


# ---- workgroup counts ------------------------------------------------------------------------
def _varied_jobs(n, sizes, seed):
    rng = np.random.default_rng(seed)
    jobs = []
    for k in range(n):
        ow, oh = sizes[k % len(sizes)]
        w, h = int(rng.integers(1, 60)), int(rng.integers(1, 50))
        x0, y0 = int(rng.integers(0, FW - w + 1)), int(rng.integers(0, FH - h + 1))
        ang, sc = rng.uniform(-3.1, 3.1), rng.uniform(0.4, 2.5)
        M = [sc * np.cos(ang), -sc * np.sin(ang), rng.uniform(-20, 60), sc * np.sin(ang), sc * np.cos(ang),
             rng.uniform(-20, 60)]
        jobs.append(_job(x0, y0, w, h, _inv(M), ow, oh, BORDERS[k % 3]))
    return jobs


@pytest.mark.parametrize("n,sizes", [(1, [(7, 5)]), (3, [(16, 16), (1, 1)]), (5, [(112, 112), (9, 9)]),
                                     (13, [(40, 33), (3, 50)]), (147, [(112, 112), (37, 23), (1, 1), (64, 64), (5, 90)])])
def test_workgroup_counts(gpu_ctx, frame, n, sizes):
    """Grids of 1, 3, 245, 78 and 7203 workgroups: none a multiple of 8, so the XCD remap deals
    unequal shares; every job of every call is checked (147: the chips of one busy batch)."""
    jobs = _varied_jobs(n, sizes, 100 + n)
    assert _workgroups(jobs) % 8 != 0
    _run(gpu_ctx, frame, jobs)
