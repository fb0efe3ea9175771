"""The gray-plane measurements of the reference's main pass (Processor.run, person_capture/gui_app.py:
5740-8002) behind one object per video: the per-frame BGR2GRAY (:5754) with the previous plane
(:8000), _autocrop_borders with _is_real_letterbox_crop (:3360-3448), _faceless_validate's motion test
(:4242-4286) and _smart_crop_box's gradient saliency (:8291-8309, :8371-8380).

The split follows DESIGN.md §10.1 (here §14): the device returns exact integers (the gray plane, its
row and column sums, 256-bin histograms of the border strips, moved-pixel counts, the small
INTER_AREA plane) and every decision is taken here with the reference's own expressions. With a
GpuContext the integers come from pc_frame_gray / pc_gray_region_hist / pc_gray_motion /
pc_gray_resize_area; with ctx=None a NumPy backend in this module produces the same integers by the
same rules.

Limits: frames with 32 <= h, w <= 16384 (ValueError otherwise). A frame narrower than 16 pixels would
make the reference upscale the saliency plane with INTER_LINEAR, which is not restated (ValueError).
A FrameGauges refers to device planes the gauge recycles: its strip statistics, motion counts and
saliency are available until the next measure / measure_batch / reset of its gauge (RuntimeError
afterwards); what it has computed by then stays."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, curate, imageops
from .curate import DeviceCrop
from .frames import Nv12Frame
from .frames_hdr import HdrFrame
from .utils import black_border_roi

MOTION_THRESH = 15          # cv2.threshold(diff, 15, 255, THRESH_BINARY), gui_app.py:4281
MAX_STD = 3.5               # gui_app.py:3427
SALIENCY_MAX_W = 384        # gui_app.py:8295


# ---------------------------------------------------------------------------
# host halves: the reference's expressions on the device's integers
# ---------------------------------------------------------------------------
def _order_stat(cum: np.ndarray, k: int) -> int:
    """The k-th smallest value (k from 0) of the samples a histogram counts: the first bin whose
    cumulative count exceeds k."""
    return int(np.searchsorted(cum, k, side="right"))


def percentile_from_hist(hist, q: float) -> float:
    """np.percentile(values.astype(np.float32), q) (gui_app.py:3435-3436) from the values' 256-bin
    histogram, bit for bit: NumPy's linear method takes the virtual index (n - 1) * (q / 100) in the
    array's dtype, float32, and interpolates the two neighbouring order statistics with its _lerp
    (a + d g below g = 0.5, b - d (1 - g) from there), also in float32."""
    cum = np.cumsum(np.asarray(hist, dtype=np.int64))
    n = int(cum[-1])
    if n <= 0:
        raise ValueError("percentile_from_hist: empty histogram")
    vi = np.float32(n - 1) * (np.float32(q) / np.float32(100))
    prev = int(np.floor(vi))
    nxt = min(prev + 1, n - 1)
    g = np.float32(vi - np.float32(prev))
    a = np.float32(_order_stat(cum, prev))
    b = np.float32(_order_stat(cum, nxt))
    d = np.float32(b - a)
    r = a + d * g if g < np.float32(0.5) else b - d * (np.float32(1) - g)
    return float(np.float32(r))


def std_from_hist(hist) -> float:
    """sqrt((n sum v^2 - (sum v)^2) / n^2) of the samples a histogram counts, the exactly rounded f64
    value (integer arithmetic, one rounding). The reference's np.std of a float32 vector
    (gui_app.py:3437) differs from it by its own f32 summation error."""
    h = [int(c) for c in np.asarray(hist).reshape(-1)]
    n = sum(h)
    if n <= 0:
        raise ValueError("std_from_hist: empty histogram")
    s1 = sum(v * c for v, c in enumerate(h))
    s2 = sum(v * v * c for v, c in enumerate(h))
    num = n * s2 - s1 * s1
    if num == 0:
        return 0.0
    # sqrt(num) / n: floor(sqrt(num) 2^128) with a sticky bit sits on the same side of every f64
    # rounding boundary as the true value (a boundary times n 2^128 is an integer at these sizes),
    # and int / int is correctly rounded
    k = 128
    s = math.isqrt(num << (2 * k))
    sticky = 0 if s * s == (num << (2 * k)) else 1
    return (2 * s + sticky) / ((2 * n) << k)


def strip_ok(hist, thr: int) -> bool:
    """_strip_ok of _is_real_letterbox_crop (gui_app.py:3429-3438) on a strip's histogram."""
    max_luma = max(float(thr) + 8.0, 18.0)
    p95 = percentile_from_hist(hist, 95.0)
    p99 = percentile_from_hist(hist, 99.0)
    std = std_from_hist(hist)
    return p95 <= max_luma and p99 <= (max_luma + 4.0) and std <= MAX_STD


def border_strips(shape: Tuple[int, int], crop_xyxy) -> Tuple[Optional[bool], List[Tuple[int, int, int, int]]]:
    """The geometric half of _is_real_letterbox_crop (gui_app.py:3403-3423, 3440-3447): (decision, strips).
    decision True / False when the symmetry rules decide alone, None when the strips (x, y, w, h), in the
    reference's order left, right, top, bottom, have to be looked at."""
    h, w = int(shape[0]), int(shape[1])
    x1, y1, x2, y2 = [int(v) for v in crop_xyxy]
    left = max(0, x1)
    top = max(0, y1)
    right = max(0, w - x2)
    bottom = max(0, h - y2)
    if left <= 0 and top <= 0 and right <= 0 and bottom <= 0:
        return True, []
    tol = max(3, int(round(min(w, h) * 0.006)))
    if (left > 0) != (right > 0):
        return False, []
    if (top > 0) != (bottom > 0):
        return False, []
    if left and right and abs(left - right) > max(tol, int(0.35 * max(left, right))):
        return False, []
    if top and bottom and abs(top - bottom) > max(tol, int(0.35 * max(top, bottom))):
        return False, []
    strips = []
    # (gray[:, :left] with left > w is the whole plane: the slices clamp)
    if left:
        strips.append((0, 0, min(left, w), h))
    if right:
        strips.append((max(0, w - right), 0, min(right, w), h))
    if top:
        strips.append((0, 0, w, min(top, h)))
    if bottom:
        strips.append((0, max(0, h - bottom), w, min(bottom, h)))
    return None, strips


def clamp_box(box_xyxy, shape: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """_faceless_validate's box (gui_app.py:4248-4254): rounded, clamped into the frame, at least 1 x 1."""
    H, W = int(shape[0]), int(shape[1])
    x1, y1, x2, y2 = [int(round(v)) for v in box_xyxy]
    x1 = max(0, min(W - 1, x1))
    y1 = max(0, min(H - 1, y1))
    x2 = max(x1 + 1, min(W, x2))
    y2 = max(y1 + 1, min(H, y2))
    return x1, y1, x2, y2


def small_plane_size(h: int, w: int) -> Tuple[int, int]:
    """(small_w, small_h) of the saliency plane (gui_app.py:8295-8297)."""
    if w < 16:
        raise ValueError("frame_gauges: a frame narrower than 16 pixels (the reference upscales it with INTER_LINEAR)")
    small_w = max(16, min(SALIENCY_MAX_W, int(w)))
    scale_x = small_w / float(w)
    small_h = max(16, int(round(float(h) * scale_x)))
    return small_w, small_h


def small_plane_plan(h: int, w: int) -> dict:
    """cv2.resize dispatch (imageops.resize_plan) of the saliency plane: identity, integer ratios or
    generic INTER_AREA tables."""
    sw, sh = small_plane_size(h, w)
    if (sw, sh) == (w, h):
        return {"kind": "copy", "new_w": w, "new_h": h}
    p = imageops.resize_plan(h, w, dsize=(sw, sh), area=True)
    if p["kind"] not in ("area_fast", "area"):   # (32 <= h: both axes downscale)
        raise ValueError(f"frame_gauges: the saliency plane of a {w}x{h} frame is no INTER_AREA downscale")
    return p


def sobel_magnitude(small: np.ndarray) -> np.ndarray:
    """cv2.magnitude(Sobel(small, CV_32F, 1, 0, ksize=3), Sobel(small, CV_32F, 0, 1, ksize=3))
    (gui_app.py:8302-8304) with BORDER_REFLECT_101: both gradients in integers, then np.sqrt of the exact
    sum of squares (at most 2 080 800: exact in float32) as float32."""
    p = np.pad(small.astype(np.int32), 1, mode="reflect")
    s = p[:-2] + 2 * p[1:-1] + p[2:]          # vertical smoothing, per column
    gx = s[:, 2:] - s[:, :-2]
    t = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]  # horizontal smoothing, per row
    gy = t[2:] - t[:-2]
    return np.sqrt((gx * gx + gy * gy).astype(np.float32))


def _hist_np(gray: np.ndarray, strip) -> np.ndarray:
    x, y, w, h = strip
    return np.bincount(gray[y:y + h, x:x + w].ravel(), minlength=256).astype(np.uint32)


def _motion_np(cur: np.ndarray, prev: np.ndarray, box, thresh: int) -> int:
    x1, y1, x2, y2 = box
    d = np.abs(cur[y1:y2, x1:x2].astype(np.int16) - prev[y1:y2, x1:x2].astype(np.int16))
    return int(np.count_nonzero(d > thresh))


# ---------------------------------------------------------------------------
# planes
# ---------------------------------------------------------------------------
class _DevPlane:
    """One gray plane on the device (rows `pitch` bytes apart). gen counts how often the buffer has been
    handed out: a FrameGauges remembers the value it saw."""
    __slots__ = ("buf", "h", "w", "pitch", "gen")

    def __init__(self, buf):
        self.buf, self.h, self.w, self.pitch, self.gen = buf, 0, 0, 0, 0


class FrameGauges:
    """The measurements of one frame. row_sum [h] and col_sum [w] (u32) are the gray plane's; shape is
    (h, w)."""

    def __init__(self, gauge: "FrameGauge", shape, row_sum, col_sum, cur, prev):
        self._gauge = gauge
        self.shape = (int(shape[0]), int(shape[1]))
        self.row_sum, self.col_sum = row_sum, col_sum
        self._cur, self._prev = cur, prev
        self._gens = tuple(p.gen if isinstance(p, _DevPlane) else 0 for p in (cur, prev))
        self._sal = None
        self.strip_calls = 0   # pc_gray_region_hist calls (or NumPy histogram rounds) made for this frame

    # ---- plane access ----
    def _live(self, which: int):
        p = (self._cur, self._prev)[which]
        if isinstance(p, _DevPlane) and p.gen != self._gens[which]:
            raise RuntimeError("FrameGauges: its gray plane has been recycled by a later measure() of the gauge")
        return p

    @property
    def has_previous(self) -> bool:
        return self._prev is not None

    def gray(self) -> np.ndarray:
        """The h x w gray plane (a download with a context)."""
        return self._gauge._plane_host(self._live(0))

    # ---- borders ----
    def black_borders(self, thr: int = 10, max_scan: Optional[int] = None) -> Tuple[int, int, int, int]:
        """detect_black_borders (utils.py:152-196) on this frame."""
        return black_border_roi(self.row_sum, self.col_sum, thr, max_scan)

    def strip_hists(self, strips: Sequence[Tuple[int, int, int, int]]) -> np.ndarray:
        """[n][256] u32 histograms of rectangles (x, y, w, h) of the gray plane, one call."""
        self.strip_calls += 1
        return self._gauge._hists(self._live(0), list(strips))

    def is_real_letterbox_crop(self, crop_xyxy, thr: int) -> bool:
        """_is_real_letterbox_crop (gui_app.py:3386-3448)."""
        decided, strips = border_strips(self.shape, crop_xyxy)
        if decided is not None:
            return decided
        hists = self.strip_hists(strips)
        for hst in hists:   # (the reference returns at the first strip that fails: the same answer)
            if not strip_ok(hst, int(thr)):
                return False
        return True

    def autocrop_borders(self, thr: int, scan_frac: float = 0.25) -> Tuple[Tuple[int, int, int, int], bool]:
        """_autocrop_borders (gui_app.py:3360-3384): ((x1, y1, x2, y2), accepted). The box is what the
        reference crops the frame to: the border ROI when it is accepted as a real letterbox, else
        the whole frame (no border found, or a false one ignored: accepted False in both cases)."""
        h, w = self.shape
        scan_frac = float(scan_frac)
        max_scan = int(round(min(h, w) * max(0.0, scan_frac))) if scan_frac > 0 else None
        x1, y1, x2, y2 = self.black_borders(thr=int(thr), max_scan=max_scan)
        x1 = max(0, min(w - 1, int(x1)))
        y1 = max(0, min(h - 1, int(y1)))
        x2 = max(x1 + 1, min(w, int(x2)))
        y2 = max(y1 + 1, min(h, int(y2)))
        if (x1, y1, x2, y2) == (0, 0, w, h):
            return (0, 0, w, h), False
        if not self.is_real_letterbox_crop((x1, y1, x2, y2), int(thr)):
            return (0, 0, w, h), False
        return (x1, y1, x2, y2), True

    # ---- motion ----
    def motion_counts(self, boxes: Sequence[Sequence[float]]) -> Optional[List[int]]:
        """Pixels with |cur - prev| > 15 inside each box (rounded and clamped as _faceless_validate does,
        gui_app.py:4250-4254, 4277-4282), one call for all boxes. None without a previous plane of this
        frame's shape (gui_app.py:4275-4276)."""
        if self._prev is None:
            return None
        clamped = [clamp_box(b, self.shape) for b in boxes]
        return self._gauge._motion(self._live(0), self._live(1), clamped, MOTION_THRESH)

    def faceless_validate_batch(self, boxes: Sequence[Sequence[float]], cfg, lock_last_bbox=None):
        """_faceless_validate (gui_app.py:4242-4286) for all boxes of the frame: [(ok, reason)], with one
        motion call for the boxes the area and drift rules let through. cfg carries faceless_min_area_frac,
        faceless_max_area_frac, faceless_center_max_frac and faceless_min_motion_frac."""
        H, W = self.shape
        out: List[Optional[Tuple[bool, Optional[str]]]] = []
        pending = []
        for k, box in enumerate(boxes):
            x1, y1, x2, y2 = clamp_box(box, self.shape)
            w = max(1, x2 - x1)
            h = max(1, y2 - y1)
            area = float(w * h)
            frame_area = float(max(1, W * H))
            frac = area / frame_area
            if frac < float(cfg.faceless_min_area_frac):
                out.append((False, "area_min"))
                continue
            if frac > float(cfg.faceless_max_area_frac):
                out.append((False, "area_max"))
                continue
            if lock_last_bbox is not None:
                lx, ly, lw, lh = lock_last_bbox
                lock_cx = float(lx) + float(lw) / 2.0
                lock_cy = float(ly) + float(lh) / 2.0
                cx = x1 + w / 2.0
                cy = y1 + h / 2.0
                diag = math.hypot(W, H)
                if diag > 0:
                    drift = math.hypot(cx - lock_cx, cy - lock_cy) / diag
                    if drift > float(cfg.faceless_center_max_frac):
                        out.append((False, "center_drift"))
                        continue
            out.append(None)
            pending.append((k, (x1, y1, x2, y2), area))
        if pending and self._prev is not None:
            counts = self._gauge._motion(self._live(0), self._live(1), [b for _, b, _ in pending], MOTION_THRESH)
            for (k, _, area), motion in zip(pending, counts):
                motion_frac = motion / area if area > 0 else 0.0
                if motion_frac < float(cfg.faceless_min_motion_frac):
                    out[k] = (False, "motion")
        return [(True, None) if r is None else r for r in out]

    def faceless_validate(self, box, cfg, lock_last_bbox=None) -> Tuple[bool, Optional[str]]:
        return self.faceless_validate_batch([box], cfg, lock_last_bbox)[0]

    # ---- saliency ----
    def small_plane(self) -> np.ndarray:
        """cv2.resize(gray, (small_w, small_h), INTER_AREA) (gui_app.py:8295-8301), exact u8."""
        return self._gauge._small(self._live(0))

    def saliency(self) -> Tuple[np.ndarray, float, float]:
        """(sal, scale_x, scale_y) of _smart_crop_box (gui_app.py:8291-8307)."""
        if self._sal is None:
            H, W = self.shape
            small = self.small_plane()
            small_h, small_w = small.shape
            scale_x = small_w / float(W)
            scale_y = small_h / float(H)
            sal = sobel_magnitude(small)
            denom = float(np.percentile(sal, 95)) if sal.size else 1.0
            if denom > 1e-6:
                sal = np.clip(sal / denom, 0.0, 1.0)
            self._sal = (sal, scale_x, scale_y)
        return self._sal

    def saliency_of(self, crop) -> float:
        """_smart_crop_box's _saliency(crop) (gui_app.py:8371-8380): the mean of the patch of sal."""
        sal, scale_x, scale_y = self.saliency()
        x1, y1, x2, y2 = crop
        sx1 = max(0, min(sal.shape[1] - 1, int(round(x1 * scale_x))))
        sx2 = max(sx1 + 1, min(sal.shape[1], int(round(x2 * scale_x))))
        sy1 = max(0, min(sal.shape[0] - 1, int(round(y1 * scale_y))))
        sy2 = max(sy1 + 1, min(sal.shape[0], int(round(y2 * scale_y))))
        patch = sal[sy1:sy2, sx1:sx2]
        return float(np.mean(patch)) if patch.size else 0.0


# ---------------------------------------------------------------------------
# the gauge
# ---------------------------------------------------------------------------
def _frame_hw(f) -> Tuple[int, int]:
    if isinstance(f, DeviceCrop):
        h, w = int(f.h), int(f.w)
        if f.row_stride < 3 * w:
            raise ValueError("frame_gauges: row_stride smaller than 3 * w")
    elif isinstance(f, (Nv12Frame, HdrFrame)):
        h, w = f.H, f.W
    else:
        if not isinstance(f, np.ndarray) or f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
            raise ValueError("frame_gauges: expected a (h, w, 3) uint8 BGR array, an Nv12Frame, an HdrFrame or a DeviceCrop")
        h, w = int(f.shape[0]), int(f.shape[1])
    if not (32 <= h <= _lib.PC_GAUGE_MAX_SIDE and 32 <= w <= _lib.PC_GAUGE_MAX_SIDE):
        raise ValueError(f"frame_gauges: frame {w}x{h} outside 32 <= h, w <= {_lib.PC_GAUGE_MAX_SIDE}")
    return h, w


def _up16(v: int) -> int:
    return (int(v) + 15) & ~15


class FrameGauge:
    """Holds the previous gray plane (Processor._prev_gray) and, with a context, the device planes."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self._prev = None            # np.ndarray (NumPy backend) or _DevPlane
        self._pool: List[_DevPlane] = []

    def reset(self) -> None:
        """self._prev_gray = None (gui_app.py:4437, 5626)."""
        self._prev = None

    def measure(self, frame) -> FrameGauges:
        return self.measure_batch([frame])[0]

    def measure_batch(self, frames: Sequence[Any]) -> List[FrameGauges]:
        """One FrameGauges per frame; frame i's previous plane is frame i - 1's (the gauge's own for
        frame 0), and the last frame's plane becomes the gauge's (gui_app.py:8000)."""
        frames = list(frames)
        if not frames:
            return []
        sizes = [_frame_hw(f) for f in frames]
        planes, sums = (self._gray_np if self.ctx is None else self._gray_dev)(frames, sizes)
        return self._chain(sizes, planes, sums)

    def measure_gray(self, gray: np.ndarray) -> FrameGauges:
        """A frame whose h x w u8 gray plane the caller already holds on the host (Processor.run's own
        BGR2GRAY, gui_app.py:5754): the plane is taken as it is (uploaded with a context) and its sums are
        taken here."""
        if not isinstance(gray, np.ndarray) or gray.ndim != 2 or gray.dtype != np.uint8:
            raise ValueError("frame_gauges: expected an (h, w) uint8 gray plane")
        h, w = _frame_hw(np.empty((gray.shape[0], gray.shape[1], 3), np.uint8))
        sums = (gray.sum(axis=1, dtype=np.uint64).astype(np.uint32), gray.sum(axis=0, dtype=np.uint64).astype(np.uint32))
        if self.ctx is None:
            plane = np.ascontiguousarray(gray)
        else:
            plane = self._take_planes([(h, w)])[0]
            padded = np.zeros((h, plane.pitch), np.uint8)
            padded[:, :w] = gray
            self.ctx.upload(padded, plane.buf)
        return self._chain([(h, w)], [plane], [sums])[0]

    def _chain(self, sizes, planes, sums) -> List[FrameGauges]:
        out = []
        prev = self._prev
        for (h, w), pl, (rs, cs) in zip(sizes, planes, sums):
            # (a previous plane of another shape is none: gui_app.py:4276)
            same = prev is not None and (h, w) == (prev.shape if isinstance(prev, np.ndarray) else (prev.h, prev.w))
            out.append(FrameGauges(self, (h, w), rs, cs, pl, prev if same else None))
            prev = pl
        self._prev = prev
        return out

    # ---- NumPy backend ----
    @staticmethod
    def _bgr_np(f) -> np.ndarray:
        if isinstance(f, DeviceCrop):
            raise ValueError("frame_gauges: a DeviceCrop needs a context")
        if isinstance(f, Nv12Frame):
            from .frames import nv12_to_bgr_numpy
            return nv12_to_bgr_numpy(f)
        if isinstance(f, HdrFrame):
            from .frames_hdr import hdr_to_bgr_numpy
            return hdr_to_bgr_numpy(f)
        return f

    def _gray_np(self, frames, sizes):
        planes = [curate._gray_np(self._bgr_np(f)) for f in frames]
        sums = [(g.sum(axis=1, dtype=np.uint64).astype(np.uint32), g.sum(axis=0, dtype=np.uint64).astype(np.uint32))
                for g in planes]
        return planes, sums

    # ---- device backend ----
    def _take_planes(self, sizes) -> List[_DevPlane]:
        """A plane per frame from the pool: every plane but the gauge's previous one is free."""
        free = [p for p in self._pool if p is not self._prev]
        got = []
        for h, w in sizes:
            need = _up16(w) * h
            fit = [p for p in free if p.buf.nbytes >= need]
            if fit:
                p = min(fit, key=lambda q: q.buf.nbytes)
                free.remove(p)
            else:
                p = _DevPlane(self.ctx.alloc(need))
                self._pool.append(p)
            p.h, p.w, p.pitch = h, w, _up16(w)
            p.gen += 1
            got.append(p)
        # planes that fitted nothing this time are dropped once the pool outgrows the call
        if len(self._pool) > len(sizes) + 2:
            for p in free:
                self._pool.remove(p)
        return got

    def _gray_dev(self, frames, sizes):
        ctx = self.ctx
        n = len(frames)
        # BGR sources: host arrays and converted NV12 / HDR frames go into one scratch, each from a 16-byte boundary
        bgr_off, bgr_bytes, nv_bytes, hdr_bytes = [], 0, 0, 0
        for f, (h, w) in zip(frames, sizes):
            if isinstance(f, DeviceCrop):
                bgr_off.append(-1)
                continue
            bgr_off.append(bgr_bytes)
            bgr_bytes += _up16(h * w * 3)
            if isinstance(f, Nv12Frame) and not f.is_device:
                nv_bytes += _up16(f.packed_bytes)
            if isinstance(f, HdrFrame) and not f.is_device:
                hdr_bytes += _up16(f.packed_bytes)
        d_in = ctx.scratch("gauge_in", bgr_bytes) if bgr_bytes else None
        d_nv = ctx.scratch("gauge_nv12", nv_bytes) if nv_bytes else None
        d_hdr = ctx.scratch("gauge_hdr", hdr_bytes) if hdr_bytes else None
        nv_jobs, hdr_jobs, nv_at, hdr_at = [], [], 0, 0
        descs = (_lib.GrayDesc * n)()
        for i, (f, (h, w)) in enumerate(zip(frames, sizes)):
            d = descs[i]
            if isinstance(f, DeviceCrop):
                d.d_src, d.row_stride = int(f.ptr), int(f.row_stride)
                continue
            dst = d_in.ptr + bgr_off[i]
            d.d_src, d.row_stride = dst, 3 * w
            if isinstance(f, Nv12Frame):
                from . import frames as _frames
                dev = f
                if not f.is_device:
                    dev = _frames.stage_nv12(ctx, f, d_nv.ptr + nv_at)
                    nv_at += _up16(f.packed_bytes)
                nv_jobs.append(dev.job(dst))
            elif isinstance(f, HdrFrame):
                from . import frames_hdr as _hdr
                dev = f
                if not f.is_device:
                    dev = _hdr.stage_hdr(ctx, f, d_hdr.ptr + hdr_at)
                    hdr_at += _up16(f.packed_bytes)
                hdr_jobs.append(dev.job(dst))
            else:
                ctx.stage_frame(f, dst)
        if nv_jobs:
            from . import frames as _frames
            _frames.convert_on_device(ctx, nv_jobs)
        if hdr_jobs:
            from . import frames_hdr as _hdr
            _hdr.convert_on_device(ctx, hdr_jobs)
        planes = self._take_planes(sizes)
        sum_off, total = [], 0
        for h, w in sizes:
            sum_off.append(total)
            total += 4 * (h + w)
        d_sums = ctx.scratch("gauge_sums", total)
        for i, ((h, w), p) in enumerate(zip(sizes, planes)):
            d = descs[i]
            d.w, d.h, d.gray_pitch, d.d_gray = w, h, p.pitch, p.buf.ptr
            d.d_row_sum = d_sums.ptr + sum_off[i]
            d.d_col_sum = d_sums.ptr + sum_off[i] + 4 * h
        _lib.check(ctx.lib.pc_frame_gray(ctx.handle, descs, n), ctx.handle, "frame_gray")
        raw = ctx.download(d_sums.ptr, (total // 4,), np.uint32)
        sums = []
        for (h, w), o in zip(sizes, sum_off):
            sums.append((raw[o // 4:o // 4 + h].copy(), raw[o // 4 + h:o // 4 + h + w].copy()))
        return planes, sums

    # ---- what a FrameGauges asks of its gauge ----
    def _plane_host(self, p) -> np.ndarray:
        if isinstance(p, np.ndarray):
            return p
        return self.ctx.download(p.buf.ptr, (p.h, p.pitch), np.uint8)[:, :p.w].copy()

    def _hists(self, p, strips) -> np.ndarray:
        n = len(strips)
        if n == 0:
            return np.zeros((0, 256), np.uint32)
        if isinstance(p, np.ndarray):
            return np.stack([_hist_np(p, s) for s in strips])
        ctx = self.ctx
        regs = (_lib.GrayRegion * n)()
        for r, (x, y, w, h) in zip(regs, strips):
            if x < 0 or y < 0 or w < 1 or h < 1 or x + w > p.w or y + h > p.h:
                raise ValueError(f"frame_gauges: strip {(x, y, w, h)} outside the {p.w}x{p.h} plane")
            r.d_plane, r.pitch, r.x, r.y, r.w, r.h = p.buf.ptr, p.pitch, x, y, w, h
        d_out = ctx.scratch("gauge_hist", 1024 * n)
        _lib.check(ctx.lib.pc_gray_region_hist(ctx.handle, regs, n, C.c_void_p(d_out.ptr)), ctx.handle, "gray_region_hist")
        return ctx.download(d_out.ptr, (n, 256), np.uint32)

    def _motion(self, cur, prev, boxes, thresh: int) -> List[int]:
        n = len(boxes)
        if n == 0:
            return []
        if isinstance(cur, np.ndarray):
            return [_motion_np(cur, prev, b, thresh) for b in boxes]
        ctx = self.ctx
        mb = (_lib.MotionBox * n)()
        for m, (x1, y1, x2, y2) in zip(mb, boxes):
            if x1 < 0 or y1 < 0 or x2 <= x1 or y2 <= y1 or x2 > cur.w or y2 > cur.h:
                raise ValueError(f"frame_gauges: box {(x1, y1, x2, y2)} outside the {cur.w}x{cur.h} plane")
            m.d_cur, m.d_prev, m.pitch, m.x1, m.y1, m.x2, m.y2 = cur.buf.ptr, prev.buf.ptr, cur.pitch, x1, y1, x2, y2
        d_out = ctx.scratch("gauge_motion", 4 * n)
        _lib.check(ctx.lib.pc_gray_motion(ctx.handle, mb, n, int(thresh), C.c_void_p(d_out.ptr)), ctx.handle, "gray_motion")
        return [int(v) for v in ctx.download(d_out.ptr, (n,), np.uint32)]

    def _small(self, p) -> np.ndarray:
        h, w = (p.shape if isinstance(p, np.ndarray) else (p.h, p.w))
        plan = small_plane_plan(h, w)
        if isinstance(p, np.ndarray):
            return curate._resize_area_np(p, plan)
        if plan["kind"] == "copy":
            return self._plane_host(p)
        ctx = self.ctx
        ow, oh = plan["new_w"], plan["new_h"]
        pitch = _up16(ow)
        d_out = ctx.scratch("gauge_small", pitch * oh)
        if plan["kind"] == "area_fast":
            rc = ctx.lib.pc_gray_resize_area(ctx.handle, C.c_void_p(p.buf.ptr), p.pitch, w, h, _lib.PC_CURATE_FAST,
                                             plan["isx"], plan["isy"], None, None, 0, None, None, 0,
                                             C.c_void_p(d_out.ptr), pitch, ow, oh)
        else:
            xt, xs = imageops.area_tables(w, ow)
            yt, ys = imageops.area_tables(h, oh)
            rc = ctx.lib.pc_gray_resize_area(ctx.handle, C.c_void_p(p.buf.ptr), p.pitch, w, h, _lib.PC_CURATE_AREA, 0, 0,
                                             xt, xs, len(xt), yt, ys, len(yt), C.c_void_p(d_out.ptr), pitch, ow, oh)
        _lib.check(rc, ctx.handle, "gray_resize_area")
        return ctx.download(d_out.ptr, (oh, pitch), np.uint8)[:, :ow].copy()


# ---------------------------------------------------------------------------
# drop-ins for the reference's Processor: three methods replaced by assignment
# ---------------------------------------------------------------------------
_PROCESSOR_CTX = None


def set_processor_context(ctx) -> None:
    """The GpuContext the Processor drop-ins measure on (None: the NumPy backend, same integers)."""
    global _PROCESSOR_CTX
    _PROCESSOR_CTX = ctx


def _processor_measure(self, frame) -> FrameGauges:
    """The frame's measurement, taken once however many of the drop-ins ask for it. The gauge follows
    the Processor's own previous-plane state: no previous plane while self._prev_gray is None
    (gui_app.py:4437, 5626)."""
    last = self.__dict__.get("_amd_last")
    if last is not None and last[0] is frame:
        return last[1]
    gauge = self.__dict__.get("_amd_gauge")
    if gauge is None:
        gauge = self.__dict__["_amd_gauge"] = FrameGauge(_PROCESSOR_CTX)
    prev = getattr(self, "_prev_gray", None)
    if prev is None:
        gauge.reset()
    m = gauge.measure(frame)
    self.__dict__["_amd_last"] = (frame, m, prev)
    return m


def processor_is_real_letterbox_crop(self, frame, crop_xyxy, thr: int) -> bool:
    """Processor._is_real_letterbox_crop (gui_app.py:3386-3448)."""
    if frame is None or getattr(frame, "size", 0) == 0:
        return False
    return _processor_measure(self, frame).is_real_letterbox_crop(crop_xyxy, int(thr))


def processor_autocrop_borders(self, frame, thr):
    """Processor._autocrop_borders (gui_app.py:3360-3384): (frame or its crop, (x offset, y offset)), with
    the reference's status message when a border candidate is ignored."""
    m = _processor_measure(self, frame)
    h, w = m.shape
    scan_frac = float(getattr(self.cfg, "border_scan_frac", 0.25))
    max_scan = int(round(min(h, w) * max(0.0, scan_frac))) if scan_frac > 0 else None
    x1, y1, x2, y2 = m.black_borders(thr=int(thr), max_scan=max_scan)
    x1 = max(0, min(w - 1, int(x1)))
    y1 = max(0, min(h - 1, int(y1)))
    x2 = max(x1 + 1, min(w, int(x2)))
    y2 = max(y1 + 1, min(h, int(y2)))
    if (x1, y1, x2, y2) == (0, 0, w, h):
        return frame, (0, 0)
    if not self._is_real_letterbox_crop(frame, (x1, y1, x2, y2), int(thr)):
        self._status(f"Ignoring false border crop x={x1} y={y1} w={x2 - x1} h={y2 - y1}", key="border_guard",
                     interval=2.0)
        return frame, (0, 0)
    return frame[y1:y2, x1:x2], (x1, y1)


def processor_faceless_validate(self, box_xyxy, frame_shape, gray_frame):
    """Processor._faceless_validate (gui_app.py:4242-4286). The motion count comes from the measurement
    _autocrop_borders took of this frame (cfg.auto_crop_borders on: every processed frame is measured
    once, so the gauge's previous plane is the previous frame's). A frame that was not measured never
    reached the device: its planes are the two the Processor holds on the host (gray_frame,
    self._prev_gray), and the count is taken from them with the same rules."""
    if gray_frame is None or frame_shape is None:
        return True, None
    if len(frame_shape) < 2:
        return True, None
    shape = (int(frame_shape[0]), int(frame_shape[1]))
    prev = getattr(self, "_prev_gray", None)
    last = self.__dict__.get("_amd_last")
    if last is not None and last[2] is prev and last[1].shape == shape and tuple(gray_frame.shape) == shape \
            and bool(getattr(self.cfg, "auto_crop_borders", False)):
        m = last[1]
    else:
        host = FrameGauge()
        if prev is not None:
            host.measure_gray(prev)
        m = host.measure_gray(gray_frame)
    return m.faceless_validate(box_xyxy, self.cfg, self._lock_last_bbox)
