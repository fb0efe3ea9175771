"""Hot-path helpers with the reference's semantics (person_capture/utils.py):
vector normalisation / cosine distance used by the match step, and the crop
geometry the callers apply to accepted boxes."""
from __future__ import annotations

import os
from typing import Iterable

import numpy as np


def parse_ratio(s: str):
    """utils.py:101-103 — 'W:H' -> (float W, float H)."""
    w, h = s.split(":")
    return float(w), float(h)


def ensure_dir(p) -> None:
    os.makedirs(p, exist_ok=True)


def l2_normalize(x, eps: float = 1e-10):
    """utils.py:108-110: x / (||x|| + eps)."""
    return x / (np.linalg.norm(x) + eps)


def cosine_distance(a: Iterable[float], b: Iterable[float]) -> float:
    """utils.py:260-268: 1 - dot(a/(|a|+1e-9), b/(|b|+1e-9)) in float32."""
    va = np.asarray(list(a), dtype=np.float32).reshape(-1)
    vb = np.asarray(list(b), dtype=np.float32).reshape(-1)
    na = float(np.linalg.norm(va)) + 1e-9
    nb = float(np.linalg.norm(vb)) + 1e-9
    return 1.0 - float(np.dot(va / na, vb / nb))


def crop_img(frame, box):
    x1, y1, x2, y2 = [int(v) for v in box]
    return frame[y1:y2, x1:x2]


def _clamp(v, lo, hi):
    return max(lo, min(hi, v))


def black_border_roi(row_sum, col_sum, thr=10, max_scan=None):
    """The scan of detect_black_borders (utils.py:162-196) on the gray plane's row and column sums:
    a row of W pixels has `mean > thr` exactly when `sum > thr * W` (integer sums; the f64 quotient
    cannot round across an integer threshold at W <= 16384)."""
    H, W = len(row_sum), len(col_sum)
    if max_scan is None:
        max_scan = max(64, min(H, W) // 8)
    top = 0
    for r in range(min(H, max_scan)):
        if int(row_sum[r]) > thr * W:
            break
        top = r + 1
    bottom = H
    for r in range(H - 1, max(H - max_scan - 1, -1), -1):
        if int(row_sum[r]) > thr * W:
            break
        bottom = r
    left = 0
    for c in range(min(W, max_scan)):
        if int(col_sum[c]) > thr * H:
            break
        left = c + 1
    right = W
    for c in range(W - 1, max(W - max_scan - 1, -1), -1):
        if int(col_sum[c]) > thr * H:
            break
        right = c
    left = _clamp(left, 0, right - 1)
    top = _clamp(top, 0, bottom - 1)
    right = _clamp(right, left + 1, W)
    bottom = _clamp(bottom, top + 1, H)
    return int(left), int(top), int(right), int(bottom)


def detect_black_borders(bgr, thr=10, max_scan=None):
    """utils.py:152-196: ROI (x1, y1, x2, y2) inside constant black borders. The gray plane's row and
    column sums come from curate.crop_metrics_batch (the device with a default context, else NumPy)."""
    if bgr is None or bgr.size == 0:
        return (0, 0, 0, 0)
    from . import curate
    m = curate.crop_metrics_batch([bgr])[0]
    return black_border_roi(m.row_sum, m.col_sum, thr, max_scan)


def expand_box_to_ratio(x1, y1, x2, y2, ratio_w, ratio_h, frame_w, frame_h, anchor=None, head_bias=0.0):
    """utils.py:198-257: the smallest box of exactly ratio_w:ratio_h around the input box
    (optionally re-centred on `anchor` and shifted by head_bias * box height), clamped into
    the frame and shrunk symmetrically if clamping broke the ratio."""
    x1, y1, x2, y2 = (float(v) for v in (x1, y1, x2, y2))
    bw = max(1.0, x2 - x1)
    bh = max(1.0, y2 - y1)
    target = float(ratio_w) / float(ratio_h)
    cx, cy = (float(anchor[0]), float(anchor[1])) if anchor is not None else (x1 + bw * 0.5, y1 + bh * 0.5)
    cy -= head_bias * bh
    new_w, new_h = (target * bh, bh) if bw / bh < target else (bw, bw / target)
    l, t = _clamp(cx - new_w * 0.5, 0, frame_w - 1), _clamp(cy - new_h * 0.5, 0, frame_h - 1)
    r, b = _clamp(cx + new_w * 0.5, 0, frame_w - 1), _clamp(cy + new_h * 0.5, 0, frame_h - 1)
    cw, ch = r - l, b - t
    if cw <= 1 or ch <= 1:
        return int(l), int(t), int(r), int(b)
    cur = cw / ch
    if abs(cur - target) > 1e-4:
        if cur < target:
            dy = (ch - cw / target) * 0.5
            t += dy
            b -= dy
        else:
            dx = (cw - ch * target) * 0.5
            l += dx
            r -= dx
        l, t = _clamp(l, 0, frame_w - 1), _clamp(t, 0, frame_h - 1)
        r, b = _clamp(r, 0, frame_w - 1), _clamp(b, 0, frame_h - 1)
    return int(round(l)), int(round(t)), int(round(r)), int(round(b))
