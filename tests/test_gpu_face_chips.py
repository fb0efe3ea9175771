"""pc_face_chips: the unaligned face chips of the OpenCLIP face mode (face_embedder.py:2454-2460), all
rectangles of a batch in one call, against oracle/pipeline.resize_for_arc (the CPU restatement of
cv2.resize(face, (112,112), INTER_AREA if max(h,w) > 112 else INTER_LINEAR)) and against the bytes the
per-face kernels write for the same rectangle (cv_resize_into: pc_copy_2d / pc_resize_area_fast /
pc_resize_area / pc_resize_linear). Everything is compared with ==.

The 16 rectangles cover every path of cv::resize's dispatch (imageops.resize_plan): area_fast x4
(ratio 1 on one axis included), area x3, linear in area mode x4, plain linear x4, copy x1. They sit at
odd x offsets of the frame (misaligned 3-byte pixels) and two of them end on the frame's last pixel,
so a load past a source row's end would leave the allocation.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import pipeline as op
from person_capture_amd import _lib, imageops
from person_capture_amd import face_embedder as fe_mod

pytestmark = pytest.mark.gpu

CHIP = _lib.CHIP_BYTES
FH, FW = 1100, 720
SHAPES = [(224, 224), (336, 224), (224, 112), (448, 560), (150, 130), (112, 300), (1080, 700), (200, 90), (90, 200),
          (113, 40), (7, 113), (60, 50), (111, 112), (112, 112), (1, 1), (2, 3)]
KINDS = {"area_fast": 4, "area": 3, "linear1": 4, "linear0": 4, "copy": 1}


def _boxes():
    """(y, x, H, W) per shape, at odd x offsets; (1080, 700) (the one even offset: it only fits at
    x = 20) and (7, 113) (x = 607) end on the frame's last pixel."""
    out = []
    for i, (h, w) in enumerate(SHAPES):
        if (h, w) in ((1080, 700), (7, 113)):
            y, x = FH - h, FW - w
        else:
            y, x = 3 * i, 2 * i + 1
        assert y + h <= FH and x + w <= FW and (x % 2 == 1 or (h, w) == (1080, 700))
        out.append((y, x, h, w))
    return out


@pytest.fixture(scope="module")
def frame():
    return np.random.default_rng(11).integers(0, 256, (FH, FW, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def want(frame):
    """The oracle chips of the 16 rectangles (computed once, read-only)."""
    w = np.stack([op.resize_for_arc(np.ascontiguousarray(frame[y:y + h, x:x + ww])) for y, x, h, ww in _boxes()])
    w.setflags(write=False)
    return w


def _call(ctx, rects, d_chips):
    """rects: (device pointer, H, W, row_stride) -> status of pc_face_chips."""
    g = np.array(rects, dtype=np.int64).reshape(-1, 4)
    descs = imageops.chip_descs(g[:, 0], g[:, 1], g[:, 2], g[:, 3])
    return ctx.lib.pc_face_chips(ctx.handle, descs.ctypes.data_as(C.POINTER(_lib.ChipDesc)), len(g), d_chips)


def test_kinds_cover_every_path():
    got = {}
    for h, w in SHAPES:
        p = imageops.resize_plan(h, w, (112, 112), area=max(h, w) > 112)
        k = p["kind"] + (str(p["area_mode"]) if p["kind"] == "linear" else "")
        got[k] = got.get(k, 0) + 1
    assert got == KINDS


def test_mixed_rectangles_one_call(gpu_ctx, frame, want):
    ctx = gpu_ctx
    d = ctx.alloc(frame.nbytes)
    ctx.upload(frame, d)
    boxes = _boxes()
    n = len(boxes)
    out = ctx.alloc(n * CHIP)
    rects = [(d.ptr + y * FW * 3 + x * 3, h, w, FW * 3) for y, x, h, w in boxes]
    assert _call(ctx, rects, out.ptr) == 0
    got = ctx.download(out.ptr, (n, 112, 112, 3), np.uint8)
    one = ctx.alloc(CHIP)
    for i, (y, x, h, w) in enumerate(boxes):
        assert np.array_equal(got[i], want[i]), (i, h, w)
        # the per-face kernels on the same rectangle
        crop = fe_mod._DevImage(rects[i][0], h, w, FW * 3)
        fe_mod.cv_resize_into(ctx, crop, imageops.resize_plan(h, w, (112, 112), area=max(h, w) > 112), one.ptr)
        assert np.array_equal(ctx.download(one.ptr, (112, 112, 3), np.uint8), got[i]), (i, h, w)


@pytest.mark.parametrize("n", [1, 33])
def test_batch_sizes_two_frames_guard(gpu_ctx, frame, want, n):
    """Descriptors into two frames (the second a padded-row copy of the first: row_stride > 3 W), the
    chip buffer followed by a guard chip that stays untouched."""
    ctx = gpu_ctx
    pitch = FW * 3 + 37
    padded = np.zeros((FH, pitch), np.uint8)
    padded[:, :FW * 3] = frame.reshape(FH, FW * 3)
    d0, d1 = ctx.alloc(frame.nbytes), ctx.alloc(padded.nbytes)
    ctx.upload(frame, d0)
    ctx.upload(padded, d1)
    boxes = _boxes()
    out = ctx.alloc((n + 1) * CHIP)
    ctx.memset(out.ptr, 0xA5, (n + 1) * CHIP)
    rects, idx = [], []
    for k in range(n):
        i = (5 * k + 3) % len(boxes)
        y, x, h, w = boxes[i]
        base, rs = (d1.ptr, pitch) if k % 2 else (d0.ptr, FW * 3)
        rects.append((base + y * rs + x * 3, h, w, rs))
        idx.append(i)
    assert _call(ctx, rects, out.ptr) == 0
    got = ctx.download(out.ptr, (n + 1, 112, 112, 3), np.uint8)
    for k, i in enumerate(idx):
        assert np.array_equal(got[k], want[i]), (k, SHAPES[i])
    assert (got[n] == 0xA5).all()


def test_argument_errors_launch_nothing(gpu_ctx, frame):
    ctx = gpu_ctx
    d = ctx.alloc(frame.nbytes)
    ctx.upload(frame, d)
    out = ctx.alloc(2 * CHIP)
    ctx.memset(out.ptr, 0x5A, 2 * CHIP)
    good = (d.ptr + 3, 100, 100, FW * 3)
    bad = [(d.ptr, 0, 100, FW * 3), (d.ptr, 100, 16385, 16385 * 3), (0, 100, 100, FW * 3),
           (d.ptr, 100, 100, 299)]
    for b in bad:
        assert _call(ctx, [good, b], out.ptr) == 1, b   # PC_ERR_ARG
    descs = imageops.chip_descs([good[0]], [100], [100], [FW * 3])
    p = descs.ctypes.data_as(C.POINTER(_lib.ChipDesc))
    assert ctx.lib.pc_face_chips(ctx.handle, p, -1, out.ptr) == 1
    assert ctx.lib.pc_face_chips(ctx.handle, None, 1, out.ptr) == 1
    assert ctx.lib.pc_face_chips(ctx.handle, p, 1, None) == 1
    assert ctx.lib.pc_face_chips(ctx.handle, p, 0, out.ptr) == 0     # n == 0: PC_OK, nothing enqueued
    assert ctx.lib.pc_face_chips(ctx.handle, None, 0, None) == 0
    assert (ctx.download(out.ptr, (2 * CHIP,), np.uint8) == 0x5A).all()
