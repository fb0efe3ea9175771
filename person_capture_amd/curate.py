"""The dataset curator's per-crop metrics and MMR ranking (person_capture/dataset_curator.py:55-238,
961-977) behind the reference's function names.

The work is split so that the device returns exact integers (gray histogram, row / column sums,
the INTER_AREA planes, Laplacian sums) or values with a derived bound (the 8x8 DCT block, F F^T),
and everything that decides something runs here with the reference's own NumPy expressions
(DESIGN.md §10). With a GpuContext (argument or set_default_context) the integers come from
pc_crop_metrics / pc_sim_matrix / pc_mmr_order; without one, a NumPy backend produces the same
integers by the same rules.

Limits: BGR u8 crops with 32 <= h, w <= 16384 (ValueError otherwise; the reference would upscale
smaller ones through cv2's linear kernel, which this module does not restate); exposure_score is
bit-identical to the reference's float32 arithmetic while h * w < 2**24 (above that calcHist's f32
counts stop being exact in the reference itself); ranking takes n <= 8192 on the device.
textlike_corners_score (MSER) is not provided: its value is the caller's (Item.wmark)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, imageops
from .utils import black_border_roi

MMR_MAX_N = 8192
_TAB_DTYPE = np.dtype([("si", np.int32), ("di", np.int32), ("alpha", np.float32)])
_DEFAULT_CTX = None


def set_default_context(ctx) -> None:
    """The GpuContext the reference-named functions use when none is passed (None: NumPy backend)."""
    global _DEFAULT_CTX
    _DEFAULT_CTX = ctx


@dataclass
class DeviceCrop:
    """A BGR u8 crop already on the device (ptr: top-left byte, row_stride: bytes per row)."""
    ptr: int
    h: int
    w: int
    row_stride: int


@dataclass
class CropMetrics:
    """What the device (or the NumPy backend) returns for one crop, and the reference's values derived
    from it on the host."""
    w: int
    h: int
    w2: int
    h2: int
    hist: np.ndarray        # [256] u32, full-size gray plane
    row_sum: np.ndarray     # [h] u32
    col_sum: np.ndarray     # [w] u32
    sum_g2: int             # over the <= 256 plane
    sum_lap: int
    sum_lap2: int
    coef: np.ndarray        # [8][8] f32 DCT block of the 32x32 plane
    planes: Optional[Dict[str, np.ndarray]] = None   # 'gray', 'g2', 'p32' on request

    @property
    def lap_var(self) -> float:
        """var(Laplacian) = (sum L^2 - (sum L)^2 / n) / n from the exact integers, rounded once."""
        n = self.w2 * self.h2
        return (self.sum_lap2 * n - self.sum_lap * self.sum_lap) / (n * n)

    @property
    def sharpness(self) -> float:
        return sharpness_from_sums(self.sum_g2, self.sum_lap, self.sum_lap2, self.w2 * self.h2)

    @property
    def exposure(self) -> float:
        return exposure_from_hist(self.hist)

    @property
    def phash(self) -> int:
        return phash_from_coef(self.coef)

    @property
    def black_border(self) -> Tuple[int, int, int, int]:
        return black_border_roi(self.row_sum, self.col_sum)


# ---------------------------------------------------------------------------
# host halves: the reference's expressions on the device's integers
# ---------------------------------------------------------------------------
def sharpness_from_sums(sum_g2: int, sum_lap: int, sum_lap2: int, n: int) -> float:
    """sharpness_norm's tail (dataset_curator.py:93-98). var and mean are the exactly rounded f64
    values of what the reference sums in f32 (np.var / np.mean of a float32 Laplacian and a u8 plane):
    the difference is the reference's own summation error, about 1e-6 relative."""
    var = (int(sum_lap2) * n - int(sum_lap) * int(sum_lap)) / (n * n)
    mean = int(sum_g2) / n
    v = var / (mean * mean + 1e-6)
    return float(np.tanh(np.log1p(v)))


def exposure_from_hist(hist_u32: np.ndarray) -> float:
    """exposure_score's tail (dataset_curator.py:106-113) on the integer histogram: calcHist's float32
    counts are these integers while h * w < 2**24, and every line below is the reference's."""
    hist = np.asarray(hist_u32).astype(np.float32)
    hist = hist / max(1.0, hist.sum())
    low = hist[:8].sum()
    high = hist[-8:].sum()
    mid = hist[16:240].sum()
    s = mid - 0.5 * (low + high)
    return float(max(0.0, min(1.0, s)))


def phash_from_coef(coef: np.ndarray) -> int:
    """phash64's tail (dataset_curator.py:64-71) on the 8x8 low-frequency block."""
    block = np.asarray(coef, np.float32).reshape(8, 8).copy()
    block[0, 0] = 0.0
    med = np.median(block)
    bits = (block > med).astype(np.uint8).flatten()
    out = 0
    for i, b in enumerate(bits):
        out |= int(b) << i
    return out


def phash_margin(coef: np.ndarray) -> float:
    """Smallest |coefficient - median| of the hashed block: bits of coefficients within rounding of
    the median are unpinned against cv2.dct."""
    block = np.asarray(coef, np.float64).reshape(8, 8).copy()
    block[0, 0] = 0.0
    return float(np.abs(block - np.median(block)).min())


def dct_table() -> np.ndarray:
    """Rows 0..7 of the orthonormal 32-point DCT-II matrix (cv2.dct's normalisation), f64."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(32, dtype=np.float64)[None, :]
    c = np.cos(np.pi * (2.0 * x + 1.0) * u / 64.0) * math.sqrt(2.0 / 32.0)
    c[0, :] = math.sqrt(1.0 / 32.0)
    return np.ascontiguousarray(c)


# ---------------------------------------------------------------------------
# geometry shared by both backends
# ---------------------------------------------------------------------------
def _check_image(img) -> Tuple[int, int]:
    if isinstance(img, DeviceCrop):
        h, w = int(img.h), int(img.w)
        if img.row_stride < 3 * w:
            raise ValueError("curate: row_stride smaller than 3 * w")
    else:
        if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError("curate: expected a (h, w, 3) uint8 BGR array")
        h, w = int(img.shape[0]), int(img.shape[1])
    if not (32 <= h <= 16384 and 32 <= w <= 16384):
        raise ValueError(f"curate: crop {w}x{h} outside 32 <= h, w <= 16384")
    return h, w


def plane_plans(h: int, w: int) -> Tuple[dict, dict]:
    """cv2.resize dispatch (imageops.resize_plan) of the two INTER_AREA targets of a gray h x w plane:
    sharpness_norm's (int(round(w s)), int(round(h s))), s = 256 / max(h, w), when max(h, w) > 256
    (dataset_curator.py:86-92), and phash64's 32 x 32 (dataset_curator.py:60)."""
    m = max(h, w)
    if m > 256:
        s = 256.0 / float(m)
        w2, h2 = int(round(w * s)), int(round(h * s))
        if w2 < 1 or h2 < 1:
            raise ValueError(f"curate: crop {w}x{h} resizes to an empty plane (cv2.resize raises there too)")
        p2 = imageops.resize_plan(h, w, dsize=(w2, h2), area=True)
    else:
        p2 = {"kind": "copy", "new_w": w, "new_h": h}
    p32 = imageops.resize_plan(h, w, dsize=(32, 32), area=True)
    for p in (p2, p32):
        if p["kind"] not in ("copy", "area_fast", "area"):   # both axes downscale: never the linear kernel
            raise AssertionError(p)
    return p2, p32


def _tables_np(ssize: int, dsize: int) -> Tuple[np.ndarray, np.ndarray]:
    tab, starts = imageops.area_tables(ssize, dsize)
    return (np.frombuffer(tab, dtype=_TAB_DTYPE) if len(tab) else np.zeros(0, _TAB_DTYPE),
            np.frombuffer(starts, dtype=np.int32))


# ---------------------------------------------------------------------------
# NumPy backend: the same integers by the same rules
# ---------------------------------------------------------------------------
def _gray_np(bgr: np.ndarray) -> np.ndarray:
    b = bgr[..., 0].astype(np.int32)
    g = bgr[..., 1].astype(np.int32)
    r = bgr[..., 2].astype(np.int32)
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def _padded_taps(tab: np.ndarray, starts: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """[d][maxt] source indices and weights of every destination, in table order; padding repeats
    index 0 with weight 0 (adds +0 to a non-negative sum)."""
    d = len(starts) - 1
    cnt = np.diff(starts)
    maxt = int(cnt.max())
    si = np.zeros((d, maxt), np.int64)
    al = np.zeros((d, maxt), np.float32)
    for t in range(maxt):
        sel = cnt > t
        k = starts[:-1][sel] + t
        si[sel, t] = tab["si"][k]
        al[sel, t] = tab["alpha"][k]
    return si, al


def _resize_area_np(g: np.ndarray, plan: dict) -> np.ndarray:
    """One-channel cv2.resize INTER_AREA with the arithmetic of pc_area.h: integer ratios sum the
    block ((sum + 2) >> 2 at 2x2, else rint(f32(sum) * f32(1 / area))); otherwise float32 weights
    summed per destination pixel in source order (x window of every source row, then the rows),
    rounded half to even and saturated."""
    if plan["kind"] == "copy":
        return g
    ow, oh = plan["new_w"], plan["new_h"]
    if plan["kind"] == "area_fast":
        isx, isy = plan["isx"], plan["isy"]
        s = g[:oh * isy, :ow * isx].astype(np.int32).reshape(oh, isy, ow, isx).sum(axis=(1, 3))
        if isx == 2 and isy == 2:
            v = (s + 2) >> 2
        else:
            scale = np.float32(1.0) / np.float32(isx * isy)
            v = np.rint(s.astype(np.float32) * scale).astype(np.int32)
        return np.clip(v, 0, 255).astype(np.uint8)
    H, W = g.shape
    xsi, xal = _padded_taps(*_tables_np(W, ow))
    ysi, yal = _padded_taps(*_tables_np(H, oh))
    gf = g.astype(np.float32)
    rs = np.zeros((H, ow), np.float32)
    for t in range(xsi.shape[1]):
        rs = rs + gf[:, xsi[:, t]] * xal[None, :, t]
    acc = np.zeros((oh, ow), np.float32)
    for t in range(ysi.shape[1]):
        acc = acc + rs[ysi[:, t], :] * yal[:, t, None]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def _laplace_sums_np(g2: np.ndarray) -> Tuple[int, int, int]:
    g = g2.astype(np.int64)
    # BORDER_REFLECT_101; an axis of length 1 reflects onto itself (cv::borderInterpolate)
    p = np.pad(g, ((1, 1) if g.shape[0] > 1 else (0, 0), (1, 1) if g.shape[1] > 1 else (0, 0)), mode="reflect")
    if g.shape[0] == 1:
        p = np.concatenate([p, p, p], axis=0)
    if g.shape[1] == 1:
        p = np.concatenate([p, p, p], axis=1)
    lap = p[1:-1, :-2] + p[1:-1, 2:] + p[:-2, 1:-1] + p[2:, 1:-1] - 4 * g
    return int(g.sum()), int(lap.sum()), int((lap * lap).sum())


def _metrics_np(bgr: np.ndarray, keep_planes: bool) -> CropMetrics:
    h, w = _check_image(bgr)
    p2, p32 = plane_plans(h, w)
    gray = _gray_np(bgr)
    g2 = _resize_area_np(gray, p2)
    x32 = _resize_area_np(gray, p32)
    sg, sl, sl2 = _laplace_sums_np(g2)
    c8 = dct_table()
    coef = (c8 @ x32.astype(np.float64) @ c8.T).astype(np.float32)
    return CropMetrics(w=w, h=h, w2=int(g2.shape[1]), h2=int(g2.shape[0]),
                       hist=np.bincount(gray.ravel(), minlength=256).astype(np.uint32),
                       row_sum=gray.sum(axis=1, dtype=np.uint64).astype(np.uint32),
                       col_sum=gray.sum(axis=0, dtype=np.uint64).astype(np.uint32),
                       sum_g2=sg, sum_lap=sl, sum_lap2=sl2, coef=coef,
                       planes={"gray": gray, "g2": g2, "p32": x32} if keep_planes else None)


# ---------------------------------------------------------------------------
# device backend
# ---------------------------------------------------------------------------
_KIND = {"copy": _lib.PC_CURATE_COPY, "area_fast": _lib.PC_CURATE_FAST, "area": _lib.PC_CURATE_AREA}


class _TableSet:
    """The batch's INTER_AREA tables, one copy per (source, destination) length."""

    def __init__(self):
        self.tabs: List[np.ndarray] = []
        self.starts: List[np.ndarray] = []
        self.n_tabs = 0
        self.n_starts = 0
        self.where: Dict[Tuple[int, int], int] = {}

    def add(self, ssize: int, dsize: int) -> int:
        key = (ssize, dsize)
        at = self.where.get(key)
        if at is None:
            tab, st = _tables_np(ssize, dsize)
            at = self.where[key] = self.n_starts
            self.tabs.append(tab)
            self.starts.append(st + np.int32(self.n_tabs))
            self.n_tabs += len(tab)
            self.n_starts += len(st)
        return at


def build_descs(sizes: Sequence[Tuple[int, int]]):
    """pc_curate_desc array (d_src / row_stride left to the caller) and the shared tables for crops
    of the given (h, w)."""
    n = len(sizes)
    descs = (_lib.CurateDesc * n)()
    ts = _TableSet()
    for i, (h, w) in enumerate(sizes):
        d = descs[i]
        p2, p32 = plane_plans(h, w)
        d.w, d.h, d.w2, d.h2 = w, h, p2["new_w"], p2["new_h"]
        for t, p in enumerate((p2, p32)):
            d.kind[t] = _KIND[p["kind"]]
            if p["kind"] == "area_fast":
                d.isx[t], d.isy[t] = p["isx"], p["isy"]
            elif p["kind"] == "area":
                d.xs[t] = ts.add(w, p["new_w"])
                d.ys[t] = ts.add(h, p["new_h"])
    tabs = np.concatenate(ts.tabs) if ts.tabs else np.zeros(0, _TAB_DTYPE)
    starts = np.concatenate(ts.starts).astype(np.int32) if ts.starts else np.zeros(0, np.int32)
    return descs, np.ascontiguousarray(tabs), np.ascontiguousarray(starts)


def metrics_layout(descs, n: int) -> Tuple[np.ndarray, int, int]:
    """pc_crop_metrics_layout: ([n][5] byte offsets, scratch bytes, output bytes)."""
    lib = _lib.load()
    off = np.zeros((max(n, 1), 5), np.uint64)
    sb, ob = C.c_size_t(), C.c_size_t()
    rc = lib.pc_crop_metrics_layout(descs, n, off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(sb), C.byref(ob))
    if rc != 0:
        raise ValueError(f"curate: bad crop descriptor (status {rc})")
    return off[:n], int(sb.value), int(ob.value)


_REC_DTYPE = np.dtype([("sum_g2", np.uint64), ("sum_lap", np.int64), ("sum_lap2", np.uint64), ("w2", np.int32),
                       ("h2", np.int32), ("hist", np.uint32, 256), ("coef", np.float32, 64)])
assert _REC_DTYPE.itemsize == _lib.CURATE_RECORD_BYTES


def _metrics_dev(images: Sequence[Any], ctx, keep_planes: bool) -> List[CropMetrics]:
    n = len(images)
    sizes = [_check_image(im) for im in images]
    descs, tabs, starts = build_descs(sizes)
    # host crops go up packed, each from a 16-byte boundary
    up_off, up_bytes = [], 0
    for im, (h, w) in zip(images, sizes):
        if not isinstance(im, DeviceCrop):
            up_off.append(up_bytes)
            up_bytes += (h * w * 3 + 15) & ~15
        else:
            up_off.append(-1)
    d_in = ctx.scratch("curate_in", up_bytes) if up_bytes else None
    for i, (im, (h, w)) in enumerate(zip(images, sizes)):
        if isinstance(im, DeviceCrop):
            descs[i].d_src, descs[i].row_stride = int(im.ptr), int(im.row_stride)
        else:
            ctx.upload(np.ascontiguousarray(im), d_in, up_off[i])
            descs[i].d_src, descs[i].row_stride = d_in.ptr + up_off[i], 3 * w
    off, sbytes, obytes = metrics_layout(descs, n)
    d_scr = ctx.scratch("curate_scratch", sbytes)
    d_out = ctx.scratch("curate_out", obytes)
    dct = dct_table()
    _lib.check(ctx.lib.pc_crop_metrics(ctx.handle, descs, n, tabs.ctypes.data_as(C.c_void_p), len(tabs),
                                       starts.ctypes.data_as(C.c_void_p), len(starts),
                                       dct.ctypes.data_as(C.c_void_p), C.c_void_p(d_scr.ptr), sbytes,
                                       C.c_void_p(d_out.ptr), obytes), ctx.handle, "crop_metrics")
    raw = ctx.download(d_out.ptr, (obytes,), np.uint8)
    recs = raw[:n * _REC_DTYPE.itemsize].view(_REC_DTYPE)
    out = []
    for i, (h, w) in enumerate(sizes):
        r = recs[i]
        rc = raw[int(off[i, 4]):int(off[i, 4]) + 4 * (h + w)].view(np.uint32)
        m = CropMetrics(w=w, h=h, w2=int(r["w2"]), h2=int(r["h2"]), hist=r["hist"].copy(), row_sum=rc[:h].copy(),
                        col_sum=rc[h:].copy(), sum_g2=int(r["sum_g2"]), sum_lap=int(r["sum_lap"]),
                        sum_lap2=int(r["sum_lap2"]), coef=r["coef"].reshape(8, 8).copy())
        if keep_planes:
            def plane(at, pw, ph):
                pitch = (pw + 15) & ~15
                return ctx.download(d_scr.ptr + int(at), (ph, pitch), np.uint8)[:, :pw].copy()
            # (a PC_CURATE_COPY target is the gray plane: same size, same pitch)
            m.planes = {"gray": plane(off[i, 0], w, h), "g2": plane(off[i, 1], m.w2, m.h2),
                        "p32": plane(off[i, 2], 32, 32)}
        out.append(m)
    return out


def crop_metrics_batch(images: Sequence[Any], ctx=None, keep_planes: bool = False) -> List[CropMetrics]:
    """The metrics of a batch of BGR u8 crops ((h, w, 3) arrays, or DeviceCrop with a context) of any
    mix of sizes: one CropMetrics per crop, with the raw integers and the derived phash, sharpness,
    exposure and black_border. With a context (or a default one) the integers come from the device in
    one pc_crop_metrics call; otherwise from the NumPy backend."""
    ctx = ctx if ctx is not None else _DEFAULT_CTX
    images = list(images)
    if not images:
        return []
    if ctx is None:
        return [_metrics_np(im, keep_planes) for im in images]
    return _metrics_dev(images, ctx, keep_planes)


# ---------------------------------------------------------------------------
# the reference's names
# ---------------------------------------------------------------------------
def phash64(bgr: np.ndarray) -> int:
    """dataset_curator.py:55-71. The DCT is the f64 orthonormal DCT-II rounded once to f32, not
    cv2.dct's f32 butterflies: bits of coefficients within rounding of the median are unpinned."""
    if bgr is None or bgr.size == 0:
        return 0
    return crop_metrics_batch([bgr])[0].phash


def hamming64(a: int, b: int) -> int:
    """dataset_curator.py:74-78."""
    x = (a ^ b) & ((1 << 64) - 1)
    return bin(x).count("1")


def sharpness_norm(bgr: np.ndarray) -> float:
    """dataset_curator.py:81-98."""
    if bgr is None or bgr.size == 0:
        return 0.0
    return crop_metrics_batch([bgr])[0].sharpness


def exposure_score(bgr: np.ndarray) -> float:
    """dataset_curator.py:101-113."""
    if bgr is None or bgr.size == 0:
        return 0.0
    return crop_metrics_batch([bgr])[0].exposure


def face_fraction(face_xyxy: Optional[Tuple[int, int, int, int]], crop_w: int, crop_h: int) -> float:
    """dataset_curator.py:116-125."""
    if face_xyxy is None:
        return 0.0
    x1, y1, x2, y2 = face_xyxy
    fh = max(1, y2 - y1)
    return float(fh) / float(max(1, crop_h))


def yaw_roll_from_5pts(pts5: np.ndarray) -> Tuple[float, float]:
    """dataset_curator.py:128-141: (yaw, roll) in degrees from (le, re, nose, lm, rm)."""
    if pts5 is None or pts5.shape != (5, 2):
        return 0.0, 0.0
    le, re, nose, lm, rm = pts5
    roll = float(np.degrees(np.arctan2(re[1] - le[1], re[0] - le[0])))
    eye_mid = (le + re) * 0.5
    dx = nose[0] - eye_mid[0]
    iod = np.linalg.norm(re - le) + 1e-6
    yaw = float(np.degrees(np.arctan2(dx, iod)))
    return float(yaw), float(roll)


def _bb_frac_from_tuple(bb: Any, W: int, H: int) -> float:
    """dataset_curator.py:173-208: black-border fraction from (x, y, w, h) or (x1, y1, x2, y2),
    whichever keeps the larger area."""
    if bb is None:
        return 0.0
    if not isinstance(bb, (tuple, list)) or len(bb) != 4:
        return 0.0
    x, y, a, b = [float(t) for t in bb]

    def area(x2: float, y2: float) -> float:
        cx1, cy1 = max(0.0, min(float(W), x)), max(0.0, min(float(H), y))
        cx2, cy2 = max(0.0, min(float(W), x2)), max(0.0, min(float(H), y2))
        ww, hh = max(0.0, cx2 - cx1), max(0.0, cy2 - cy1)
        return ww * hh if ww > 0.0 and hh > 0.0 else 0.0

    area_xyxy = area(a, b) if a > x and b > y else 0.0
    area_xywh = area(x + a, y + b) if a > 0.0 and b > 0.0 else 0.0
    keep = max(area_xyxy, area_xywh)
    total = max(1.0, float(W) * float(H))
    frac = 1.0 - (keep / total)
    return float(max(0.0, min(1.0, frac)))


def quality_score(face_fd: float, sharpness: float, exposure: float, face_quality: float, wmark: float = 0.0,
                  black_border_frac: float = 0.0) -> float:
    """Item.quality_score (dataset_curator.py:265-284)."""
    fd = max(0.0, float(face_fd))
    idq = float(np.clip(1.0 - (fd / 0.5), 0.0, 1.0))
    q = 0.45 * idq + 0.30 * sharpness + 0.20 * exposure + 0.05 * min(1.0, face_quality / 1200.0)
    q *= float(max(0.0, 1.0 - 0.6 * wmark))
    bb = float(min(max(float(black_border_frac), 0.0), 0.4))
    q *= float(max(0.0, 1.0 - 0.6 * bb))
    return float(max(0.0, min(1.0, q)))


@dataclass
class Item:
    """dataset_curator.py:244-284: the scored candidate (the fields quality_score reads, and the rest
    with defaults)."""
    path: str = ""
    face_fd: float = 0.0
    face_quality: float = 0.0
    sharpness: float = 0.0
    exposure: float = 0.0
    face_frac: float = 0.0
    yaw: float = 0.0
    roll: float = 0.0
    ratio: str = ""
    phash: int = 0
    face_feat: Optional[np.ndarray] = None
    bg_clip: Optional[np.ndarray] = None
    kps5: Optional[np.ndarray] = None
    wmark: float = 0.0
    bbox: Optional[Tuple[int, int, int, int]] = None
    meta: Dict[str, float] = field(default_factory=dict)
    ts: float = 0.0
    scene: int = -1

    @property
    def quality_score(self) -> float:
        return quality_score(self.face_fd, self.sharpness, self.exposure, self.face_quality, self.wmark,
                             float(self.meta.get("black_border_frac", 0.0)))


# ---------------------------------------------------------------------------
# ranking
# ---------------------------------------------------------------------------
def _mmr_np(S: Optional[np.ndarray], q: np.ndarray, k: int, alpha: float) -> List[int]:
    """The greedy loop on the host: red_i = max(0, max over picked j of S[i][j]) as a running f32
    maximum, score_i = alpha q_i - (1 - alpha) red_i in f64, greatest first, lowest index on ties."""
    n = len(q)
    alpha = float(alpha)
    qa = alpha * q.astype(np.float64)
    red = np.zeros(n, np.float32)
    open_ = np.ones(n, bool)
    order: List[int] = []
    for _ in range(k):
        s = np.where(open_, qa - (1.0 - alpha) * red.astype(np.float64), -np.inf)
        i = int(np.argmax(s))
        order.append(i)
        open_[i] = False
        if S is not None:
            red = np.maximum(red, S[:, i])
    return order


def _mmr_dev(ctx, d_S: int, q: np.ndarray, n: int, k: int, alpha: float) -> List[int]:
    d_q = ctx.upload(np.ascontiguousarray(q, np.float32), ctx.scratch("curate_q", 4 * n))
    d_o = ctx.scratch("curate_order", 4 * k)
    _lib.check(ctx.lib.pc_mmr_order(ctx.handle, C.c_void_p(int(d_S)), C.c_void_p(d_q.ptr), n, k, float(alpha),
                                    C.c_void_p(d_o.ptr)), ctx.handle, "mmr_order")
    return ctx.download(d_o.ptr, (k,), np.int32).tolist()


def sim_matrix(F: np.ndarray, ctx=None) -> np.ndarray:
    """S = F F^T in f32 (dataset_curator.py:971-973); rows of F are unit vectors or all zero (an item the
    reference gives None). On the device every element is one fmaf chain over the dimension ascending;
    the NumPy backend is the BLAS product the reference itself takes."""
    ctx = ctx if ctx is not None else _DEFAULT_CTX
    F = np.ascontiguousarray(F, np.float32)
    n, dim = F.shape
    if ctx is None or n == 0:
        return F @ F.T
    if n > MMR_MAX_N:
        raise ValueError(f"curate: n = {n} > {MMR_MAX_N} (S would exceed 256 MB)")
    d_F = ctx.upload(F, ctx.scratch("curate_F", F.nbytes))
    d_S = ctx.scratch("curate_S", 4 * n * n)
    _lib.check(ctx.lib.pc_sim_matrix(ctx.handle, C.c_void_p(d_F.ptr), n, dim, C.c_void_p(d_S.ptr)), ctx.handle,
               "sim_matrix")
    return ctx.download(d_S.ptr, (n, n), np.float32)


def mmr_rank(F: np.ndarray, q: np.ndarray, alpha: float = 0.75, k: Optional[int] = None, ctx=None,
             return_sim: bool = False):
    """Similarity and greedy MMR in one go (Curator.select's per-scene step, dataset_curator.py:961-977):
    the order of the k best (default all), and S on request. With a context S stays on the device
    between the two kernels."""
    ctx = ctx if ctx is not None else _DEFAULT_CTX
    F = np.ascontiguousarray(F, np.float32)
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    n = F.shape[0]
    if len(q) != n:
        raise ValueError("curate: len(q) != len(F)")
    k = n if k is None else max(0, min(int(k), n))
    if n == 0 or k == 0:
        return ([], np.zeros((n, n), np.float32)) if return_sim else []
    if ctx is None:
        S = F @ F.T
        order = _mmr_np(S, q, k, alpha)
        return (order, S) if return_sim else order
    if n > MMR_MAX_N:
        raise ValueError(f"curate: n = {n} > {MMR_MAX_N} (S would exceed 256 MB)")
    d_F = ctx.upload(F, ctx.scratch("curate_F", F.nbytes))
    d_S = ctx.scratch("curate_S", 4 * n * n)
    _lib.check(ctx.lib.pc_sim_matrix(ctx.handle, C.c_void_p(d_F.ptr), n, F.shape[1], C.c_void_p(d_S.ptr)), ctx.handle,
               "sim_matrix")
    order = _mmr_dev(ctx, d_S.ptr, q, n, k, alpha)
    if return_sim:
        return order, ctx.download(d_S.ptr, (n, n), np.float32)
    return order


def mmr_select_with_q(q_vals: np.ndarray, k: int, sim_mat: Optional[np.ndarray], alpha: float = 0.75,
                      ctx=None) -> List[int]:
    """dataset_curator.py:211-238. sim_mat (n x n, taken as float32, the dtype Curator.select builds)
    or None (rank by quality alone). With a context the matrix is uploaded and pc_mmr_order runs the
    loop; it reads row `picked` of what it is given, so the transpose goes up and a matrix that is not
    symmetric still gives the reference's sim_mat[i, picked]. (The reference's `s > -1e9` guard, which
    ends the loop early when every score is below -1e9, is not restated.)"""
    ctx = ctx if ctx is not None else _DEFAULT_CTX
    n = int(len(q_vals))
    if n <= 0:
        return []
    k = max(0, min(int(k), n))
    if k == 0:
        return []
    q = np.asarray(q_vals, np.float32).reshape(-1)
    S = None
    if sim_mat is not None:
        S = np.asarray(sim_mat, np.float32)
        if S.shape != (n, n):
            raise ValueError("curate: sim_mat must be n x n")
    if ctx is None:
        return _mmr_np(S, q, k, alpha)
    if n > MMR_MAX_N:
        raise ValueError(f"curate: n = {n} > {MMR_MAX_N} (S would exceed 256 MB)")
    d_S = ctx.scratch("curate_S", 4 * n * n)
    if S is None:
        ctx.memset(d_S.ptr, 0, 4 * n * n)
    else:
        ctx.upload(np.ascontiguousarray(S.T), d_S)
    return _mmr_dev(ctx, d_S.ptr, q, n, k, alpha)
