"""HDR linear-light frames: the third wire format of the reference's frame source.

An HDR source on an ffmpeg that has neither libplacebo nor zscale + tonemap makes the reference's
FfmpegPipeReader ask the pipe for gbrpf32le (video_io.py:2513-2520): planar float32 G, B, R of the PQ or
HLG signal, 12 bytes per pixel. Per frame the reference then restacks to RGB (video_io.py:3005-3014),
applies _eotf_pq or _eotf_hlg (:3015-3018, :3239-3258) and _python_tonemap_to_bgr8 (:3183-3192,
:3276-3291: BT.2020 luminance, Hable filmic curve, rescale, BT.709 OETF, u8), all in float32 NumPy on the
CPU. This module states that operation once and offers it on the device (pc_hdr_to_bgr, csrc/pc_hdr.hip).

The operation, exactly. Every arithmetic operation is float32, rounded once, in the order written; no
fused multiply-add; divisions correctly rounded; f32 subnormals kept. A Python-float constant meeting an
f32 array is that constant rounded to f32; a product or quotient of Python floats is taken in f64 first
and rounded once (C*B, D*E, D*F, E/F, white = h(11.2), max(peak_nits, 1e-3)). The two transcendentals
cannot be reproduced bit for bit from NumPy's f32 power / exp; they are defined as the exactly rounded
value of what the reference approximates (the stance DESIGN.md §10.1 takes for sharpness):
    P(x, e) = f32(pow((double)x, (double)(float)e))     the exponent rounded to f32 first, as NumPy applies it
    X(x)    = f32(exp((double)x))
Per pixel, signal (r, g, b), t32 = f32(target_nits), peak = f32(max(peak_nits, 1e-3)):
  * PQ (transfer='pq'), per channel:
        v = clip(x, 0, 1); p = P(v, 32/2523)
        vp = max(p - c1, 0); den = c2 - c3 * p; den = 1e-6 if |den| < 1e-6 else den
        lin = clip(P(vp / den, 16384/2610), 0, 1)
    c1, c2, c3 = 3424/4096, 2413/128, 2392/128 (the reference computes p twice, to the same value).
  * HLG (transfer='hlg'; the reader picks it when _transfer == "arib-std-b67"), per channel:
        v = clip(x, 0, 1)
        lin = (v * v) / 3 if v <= 0.5 else (X((v - c) / a) + b) / 12
    a, b, c = 0.17883277, 0.28466892, 0.55991073.
  * linear (transfer='linear'): lin = x, for callers that already hold linear light.
  * tone map:
        lin = clip(lin, 0, 1); L = lin * 10000
        Y = (0.2627 L_r + 0.6780 L_g) + 0.0593 L_b
        x = Y / peak
        h(y) = ((y * (A y + CB) + DE) / (y * (A y + B) + DF)) - EF,  A, B, C, D, E, F = .15, .50, .10, .20, .02, .30
        Yt = clip(h(x) / white, 0, 1) * t32
        s = Yt / max(Y, 1e-6)
        per channel T = clip(L * s, 0, t32); N = clip(T / 100, 0, 1)
  * OETF and store:
        o = 4.5 N if N < 0.018 else 1.099 P(N, 0.45) - 0.099
        o = clip(o, 0, 1); byte = trunc(o * 255 + 0.5); stored B, G, R.
  * +-inf clips as the reference clips it. A NaN input is outside the contract (the reference's
    astype(uint8) of NaN is undefined): some byte is written there and nothing else is touched.
  * H and W 1 .. 16384, no parity requirement.

`HdrFrame` entries are accepted wherever this package takes a BGR frame (FaceEmbedder.extract /
extract_batch, PersonDetector.detect / detect_batch, PrescanRunner's frame_at), alone or mixed with BGR
and NV12 entries. The float source is 4 x the BGR frame, so host frames go through TWO source scratch
buffers (HdrStager), whatever the batch, and are converted into the per-frame BGR buffers.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import PC_HDR_MAX_SIDE, PC_HDR_TRANSFERS, HdrDesc, check

LAYOUTS = ("planar_gbr", "rgb")
STAGE_BLOCK_BYTES = 8 << 20   # stage_hdr's row blocks: what one pinned slot of the staging ring holds

_f = np.float32
# _hable_filmic's constants (video_io.py:3268-3273): products and quotients in f64, rounded once
_A, _B, _C, _D, _E, _F, _W = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30, 11.2
_CB, _DE, _DF, _EF = _f(_C * _B), _f(_D * _E), _f(_D * _F), _f(_E / _F)


def _h64(y: float) -> float:
    return ((y * (_A * y + _C * _B) + _D * _E) / (y * (_A * y + _B) + _D * _F)) - _E / _F


WHITE = _f(_h64(_W))
PQ_E1 = 1.0 / (2523.0 / 32.0)      # as _eotf_pq writes them: 1 / m2, 1 / m1
PQ_E2 = 1.0 / (2610.0 / 16384.0)


def _check_size(H: int, W: int) -> None:
    if H < 1 or W < 1 or H > PC_HDR_MAX_SIDE or W > PC_HDR_MAX_SIDE:
        raise ValueError(f"HDR frame {H} x {W}: H and W must be 1 .. {PC_HDR_MAX_SIDE}")


def _check_params(transfer: str, layout: str, sdr_nits: float, peak_nits: float) -> None:
    if transfer not in PC_HDR_TRANSFERS:
        raise ValueError(f"HDR transfer {transfer!r}: one of {tuple(PC_HDR_TRANSFERS)}")
    if layout not in LAYOUTS:
        raise ValueError(f"HDR layout {layout!r}: one of {LAYOUTS}")
    for v in (sdr_nits, peak_nits):
        if not np.isfinite(v) or v <= 0:
            raise ValueError("HDR sdr_nits and peak_nits must be finite and > 0")


class HdrFrame:
    """One HDR frame of float32 samples.

    Host form, HdrFrame(data, H, W, transfer, sdr_nits, peak_nits, layout): `data` is bytes, a memoryview
    or a float32 array. layout 'planar_gbr': what the reference's pipe delivers, planes G, B, R of H rows,
    row_stride floats apart (default W), planes plane_stride floats apart (default H * row_stride).
    layout 'rgb': the H x W x 3 array FfmpegPipeReader.grab builds, rows row_stride floats apart (default
    3 W). sdr_nits is the tone map's target_nits (the reader's _sdr_nits).
    Device form, HdrFrame.on_device(r_ptr, g_ptr, b_ptr, H, W, pix_stride, row_stride, ...): samples
    already in HBM, pix_stride 1 (planes) or 3 (interleaved)."""

    __slots__ = ("H", "W", "transfer", "sdr_nits", "peak_nits", "layout", "pix_stride", "row_stride",
                 "plane_stride", "data", "ptrs", "_buf")

    def __init__(self, data, H: int, W: int, transfer: str = "pq", sdr_nits: float = 200.0,
                 peak_nits: float = 1000.0, layout: str = "planar_gbr", row_stride: Optional[int] = None,
                 plane_stride: Optional[int] = None):
        self.H, self.W = int(H), int(W)
        _check_size(self.H, self.W)
        self.transfer, self.layout = str(transfer), str(layout)
        self.sdr_nits, self.peak_nits = float(sdr_nits), float(peak_nits)
        _check_params(self.transfer, self.layout, self.sdr_nits, self.peak_nits)
        self.pix_stride = 1 if self.layout == "planar_gbr" else 3
        if isinstance(data, np.ndarray):
            if data.dtype != np.float32:
                raise ValueError("HDR data must be bytes or a float32 array")
            a = data
        else:
            mv = memoryview(data)
            if mv.nbytes % 4:
                raise ValueError("HDR data: a whole number of float32 samples is needed")
            a = np.frombuffer(mv, dtype=np.float32)
        a = np.ascontiguousarray(a).reshape(-1)
        self.row_stride = self.W * self.pix_stride if row_stride is None else int(row_stride)
        if self.row_stride < self.W * self.pix_stride:
            raise ValueError(f"HDR row stride {self.row_stride} shorter than the row ({self.W * self.pix_stride} floats)")
        row_span = (self.H - 1) * self.row_stride + self.W * self.pix_stride
        if self.layout == "planar_gbr":
            self.plane_stride = self.H * self.row_stride if plane_stride is None else int(plane_stride)
            if self.plane_stride < row_span:
                raise ValueError("HDR planes overlap")
            need = 2 * self.plane_stride + row_span
        else:
            if plane_stride is not None:
                raise ValueError("layout 'rgb' has no plane stride")
            self.plane_stride = 0
            need = row_span
        if a.size < need:
            raise ValueError(f"HDR frame {self.H} x {self.W} ({self.layout}): {a.size} floats, {need} needed")
        self.data, self.ptrs, self._buf = a, (0, 0, 0), None

    @classmethod
    def on_device(cls, r_ptr: int, g_ptr: int, b_ptr: int, H: int, W: int, pix_stride: int = 1,
                  row_stride: Optional[int] = None, transfer: str = "pq", sdr_nits: float = 200.0,
                  peak_nits: float = 1000.0, buf=None) -> "HdrFrame":
        f = cls.__new__(cls)
        f.H, f.W = int(H), int(W)
        _check_size(f.H, f.W)
        f.pix_stride = int(pix_stride)
        if f.pix_stride not in (1, 3):
            raise ValueError("HDR device frame: pix_stride is 1 (planes) or 3 (interleaved)")
        f.layout = "planar_gbr" if f.pix_stride == 1 else "rgb"
        f.transfer, f.sdr_nits, f.peak_nits = str(transfer), float(sdr_nits), float(peak_nits)
        _check_params(f.transfer, f.layout, f.sdr_nits, f.peak_nits)
        f.row_stride = f.W * f.pix_stride if row_stride is None else int(row_stride)
        f.ptrs = (int(r_ptr), int(g_ptr), int(b_ptr))
        if f.row_stride < f.W * f.pix_stride or not all(f.ptrs) or any(p & 3 for p in f.ptrs):
            raise ValueError("HDR device frame: null or misaligned samples, or a stride shorter than the row")
        f.plane_stride, f.data, f._buf = 0, None, buf
        return f

    @property
    def is_device(self) -> bool:
        return self.data is None

    # what the entry points ask of a frame before they look at its pixels
    @property
    def shape(self) -> Tuple[int, int, int]:
        return (self.H, self.W, 3)

    @property
    def ndim(self) -> int:
        return 3

    @property
    def size(self) -> int:
        return self.H * self.W * 3

    @property
    def packed_bytes(self) -> int:
        return self.H * self.W * 12

    def job(self, d_dst: int, dst_stride: Optional[int] = None) -> tuple:
        """The pc_hdr_to_bgr job (hdr_descs) of this device frame into d_dst (rows 3 W bytes apart by
        default)."""
        if not self.is_device:
            raise ValueError("a host HDR frame is staged first (stage_hdr)")
        return self.ptrs + (self.H, self.W, self.pix_stride, self.row_stride, int(d_dst),
                            3 * self.W if dst_stride is None else int(dst_stride), self.transfer, self.sdr_nits,
                            self.peak_nits)

    def channels(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(R, G, B), each an H x W f32 view of the host data."""
        if self.is_device:
            raise ValueError("a device HDR frame has no host samples")
        H, W, a, rs = self.H, self.W, self.data, self.row_stride

        def view(off: int) -> np.ndarray:
            return np.lib.stride_tricks.as_strided(a[off:], (H, W), (4 * rs, 4 * self.pix_stride), writeable=False)
        if self.layout == "planar_gbr":   # pipe order G, B, R (video_io.py:3013-3014)
            return view(2 * self.plane_stride), view(0), view(self.plane_stride)
        return view(0), view(1), view(2)


# ---- the NumPy backend ----
def _P(x: np.ndarray, e: float) -> np.ndarray:
    return np.power(x.astype(np.float64), np.float64(_f(e))).astype(np.float32)


def _X(x: np.ndarray) -> np.ndarray:
    return np.exp(x.astype(np.float64)).astype(np.float32)


def _clip01(x: np.ndarray) -> np.ndarray:
    return np.minimum(np.maximum(x, _f(0.0)), _f(1.0))


def eotf_numpy(x: np.ndarray, transfer: str) -> np.ndarray:
    """One channel (or any f32 array) of signal -> linear light, 1.0 = 10 000 nits."""
    x = np.asarray(x, np.float32)
    if transfer == "linear":
        return x
    v = _clip01(x)
    if transfer == "pq":
        p = _P(v, PQ_E1)
        vp = np.maximum(p - _f(3424.0 / 4096.0), _f(0.0))
        den = _f(2413.0 / 128.0) - _f(2392.0 / 128.0) * p
        den = np.where(np.abs(den) < _f(1e-6), _f(1e-6), den)
        return _clip01(_P(vp / den, PQ_E2))
    if transfer == "hlg":
        a, b, c = _f(0.17883277), _f(0.28466892), _f(0.55991073)
        lo = v <= _f(0.5)
        out = (v * v) / _f(3.0)
        hi = ~lo
        out[hi] = (_X((v[hi] - c) / a) + b) / _f(12.0)
        return out
    raise ValueError(f"HDR transfer {transfer!r}")


def tonemap_numpy(lin: Sequence[np.ndarray], target_nits: float, peak_nits: float) -> np.ndarray:
    """(R, G, B) linear light -> H x W x 3 BGR u8: the tone map, OETF and store of the module docstring."""
    t32 = _f(target_nits)
    peak = _f(max(float(peak_nits), 1e-3))
    L = [_clip01(np.asarray(c, np.float32)) * _f(10000.0) for c in lin]
    Y = (_f(0.2627) * L[0] + _f(0.6780) * L[1]) + _f(0.0593) * L[2]
    x = Y / peak
    A, B = _f(_A), _f(_B)
    hx = ((x * (A * x + _CB) + _DE) / (x * (A * x + B) + _DF)) - _EF
    Yt = _clip01(hx / WHITE) * t32
    s = Yt / np.maximum(Y, _f(1e-6))
    out = np.empty(Y.shape + (3,), np.uint8)
    for ch in range(3):
        T = np.minimum(np.maximum(L[ch] * s, _f(0.0)), t32)
        N = _clip01(T / _f(100.0))
        o = _f(4.5) * N
        hi = ~(N < _f(0.018))
        o[hi] = _f(1.099) * _P(N[hi], 0.45) - _f(0.099)
        out[..., 2 - ch] = (_clip01(o) * _f(255.0) + _f(0.5)).astype(np.uint8)
    return out


def hdr_to_bgr_numpy(frame: HdrFrame) -> np.ndarray:
    """The operation of the module docstring in NumPy: float32, every operation rounded once, the
    transcendentals in f64 rounded to f32."""
    with np.errstate(all="ignore"):
        lin = [eotf_numpy(c, frame.transfer) for c in frame.channels()]
        return tonemap_numpy(lin, frame.sdr_nits, frame.peak_nits)


# ---- device ----
def hdr_descs(jobs: Sequence[tuple]):
    """pc_hdr_desc array of (r_ptr, g_ptr, b_ptr, H, W, pix_stride, row_stride, dst_ptr, dst_stride, transfer,
    target_nits, peak_nits) tuples; transfer a name of PC_HDR_TRANSFERS or its code."""
    descs = (HdrDesc * max(1, len(jobs)))()
    for d, (rp, gp, bp, H, W, ps, rs, dp, ds, tr, tn, pn) in zip(descs, jobs):
        d.d_r, d.d_g, d.d_b, d.H, d.W, d.pix_stride, d.row_stride, d.d_dst, d.dst_stride = rp, gp, bp, H, W, ps, rs, dp, ds
        d.transfer = PC_HDR_TRANSFERS[tr] if isinstance(tr, str) else int(tr)
        d.target_nits, d.peak_nits = tn, pn
    return descs


def convert_on_device(ctx, jobs) -> None:
    """One pc_hdr_to_bgr over `jobs` (see hdr_descs) on the context's stream."""
    if jobs:
        check(ctx.lib.pc_hdr_to_bgr(ctx.handle, hdr_descs(jobs), len(jobs)), ctx.handle, "hdr_to_bgr")


def stage_hdr(h2d, frame: HdrFrame, d_dst: int, threads: int = 4) -> HdrFrame:
    """A host HDR frame -> d_dst packed in its own layout (three H x W planes G, B, R, or H x W x 3)
    through the context's pinned staging ring (pc_frame_stage), the float rows staged as bytes. A slot of
    the ring grows to what it is given and stays that size, and the ring has four: a 4K frame (99.5 MB) in
    one piece would pin 400 MB. The rows therefore go in blocks of at most STAGE_BLOCK_BYTES, which
    also lets the copy of one block run behind the packing of the next. Returns the device form."""
    H, W, ps = frame.H, frame.W, frame.pix_stride
    row = W * ps * 4
    bytes_ = frame.data.view(np.uint8)
    per = max(1, STAGE_BLOCK_BYTES // row)

    def rows(src_off: int, dst_off: int, n: int, stride: int) -> None:
        for r0 in range(0, n, per):
            r1 = min(n, r0 + per)
            a = np.lib.stride_tricks.as_strided(bytes_[4 * (src_off + r0 * stride):], (r1 - r0, row, 1),
                                                (4 * stride, 1, 1), writeable=False)
            h2d.stage_frame(a, d_dst + dst_off + r0 * row, threads)
    if ps == 3:
        rows(0, 0, H, frame.row_stride)
        return HdrFrame.on_device(d_dst, d_dst + 4, d_dst + 8, H, W, 3, 3 * W, frame.transfer, frame.sdr_nits,
                                  frame.peak_nits)
    if frame.plane_stride == H * frame.row_stride:
        rows(0, 0, 3 * H, frame.row_stride)
    else:
        for p in range(3):
            rows(p * frame.plane_stride, p * H * row, H, frame.row_stride)
    plane = H * W * 4
    return HdrFrame.on_device(d_dst + 2 * plane, d_dst, d_dst + plane, H, W, 1, W, frame.transfer, frame.sdr_nits,
                              frame.peak_nits)


class HdrStager:
    """Host HDR frames -> BGR at their destinations through at most TWO source scratch buffers.

    Frame k of a run is staged into scratch k % 2 on the copy context `h2d` and converted on `ctx` into
    its own BGR buffer. Two orderings hold: the conversion waits for its frame's copy
    (a fence of h2d), and a copy into a scratch waits for the conversion that last read that scratch (a
    fence of ctx). With h2d is ctx the one stream orders both. `reuses` counts the copies that went into
    a scratch an earlier frame had used."""

    def __init__(self, ctx, h2d=None, threads: int = 4, key: str = "hdr_src"):
        self.ctx, self.h2d = ctx, (ctx if h2d is None else h2d)
        self.threads, self.key = int(threads), key
        self._next = 0
        self._read = [None, None]   # per scratch: the fence behind the conversion that last read it
        self.reuses = 0

    @classmethod
    def shared(cls, ctx, h2d=None, threads: int = 4, key: str = "hdr_src") -> "HdrStager":
        """The one stager of (ctx, h2d, key): the scratch buffers are named buffers of ctx, so every
        consumer of that context must see the same last-reader state."""
        table = ctx.__dict__.setdefault("_hdr_stagers", {})
        k = (id(ctx if h2d is None else h2d), key)
        if k not in table:
            table[k] = cls(ctx, h2d, threads, key)
        return table[k]

    def convert(self, entries: Sequence[tuple]) -> None:
        """entries of (frame, destination pointer[, destination stride]). Device frames are converted in
        one launch; each host frame is staged and converted on its own, so that the copy of the next
        one runs behind it."""
        dev_jobs = []
        for e in entries:
            f, d_dst, ds = e[0], e[1], (e[2] if len(e) > 2 else None)
            if f.is_device:
                dev_jobs.append(f.job(d_dst, ds))
                continue
            k = self._next
            self._next = 1 - k
            two = self.h2d is not self.ctx
            if self._read[k] is not None:
                self.reuses += 1
                if two:
                    self.h2d.wait_fence(self._read[k])
            buf = self.ctx.scratch(f"{self.key}{k}", f.packed_bytes)
            dev = stage_hdr(self.h2d, f, buf.ptr, self.threads)
            if two:
                self.ctx.wait_fence(self.h2d.fence(f"{self.key}{k}_copied"))
            convert_on_device(self.ctx, [dev.job(d_dst, ds)])
            self._read[k] = self.ctx.fence(f"{self.key}{k}_read") if two else True
        convert_on_device(self.ctx, dev_jobs)


def hdr_to_bgr(frame: HdrFrame, ctx=None) -> np.ndarray:
    """H x W x 3 BGR u8 of an HDR frame. ctx=None: the NumPy backend; a runtime.GpuContext: upload,
    pc_hdr_to_bgr, download (the same bytes)."""
    if ctx is None:
        return hdr_to_bgr_numpy(frame)
    H, W = frame.H, frame.W
    dev = frame if frame.is_device else stage_hdr(ctx, frame, ctx.scratch("hdr_src", frame.packed_bytes).ptr)
    out = ctx.scratch("hdr_bgr", H * W * 3)
    convert_on_device(ctx, [dev.job(out.ptr)])
    return ctx.download(out.ptr, (H, W, 3), np.uint8)


# ---- reader drop-ins ----
_reader_ctx = None
_reader_numpy = False
_READER_NITS = (200.0, 1000.0)   # placeholders of a token: the tone map is called with its own values


def set_reader_backend(backend) -> None:
    """What reader_python_tonemap_to_bgr8 converts on: a runtime.GpuContext, None (a module-wide context on
    device 0, created at the first frame) or "numpy" (the NumPy backend, for a box without a GPU: it must
    be asked for, nothing falls back to it)."""
    global _reader_ctx, _reader_numpy
    if backend is not None and backend != "numpy" and not hasattr(backend, "handle"):
        raise ValueError("reader backend: a GpuContext, None or 'numpy'")
    _reader_numpy = isinstance(backend, str)
    _reader_ctx = None if _reader_numpy else backend


def _token(rgb, transfer: str) -> HdrFrame:
    a = np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected the reader's H x W x 3 float32 RGB array")
    if a.dtype != np.float32 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=np.float32)
    return HdrFrame(a, a.shape[0], a.shape[1], transfer, *_READER_NITS, layout="rgb")


def reader_eotf_pq(v) -> HdrFrame:
    """Drop-in for video_io._eotf_pq (video_io.py:3239-3251) in FfmpegPipeReader.grab: an HdrFrame over
    the reader's H x W x 3 array with transfer 'pq' recorded. Nothing is computed. Install with
        video_io._eotf_pq = frames_hdr.reader_eotf_pq"""
    return _token(v, "pq")


def reader_eotf_hlg(v) -> HdrFrame:
    """Drop-in for video_io._eotf_hlg (video_io.py:3254-3258): as reader_eotf_pq, transfer 'hlg'.
        video_io._eotf_hlg = frames_hdr.reader_eotf_hlg"""
    return _token(v, "hlg")


def reader_python_tonemap_to_bgr8(rgb_linear, peak_nits: float = 1000.0, target_nits: float = 200.0) -> np.ndarray:
    """Drop-in for video_io._python_tonemap_to_bgr8 (video_io.py:3276-3291), converting on the device: the
    H x W x 3 BGR u8 array of a token of reader_eotf_pq / reader_eotf_hlg, or of a plain linear ndarray
    (transfer 'linear'), with the peak_nits / target_nits it is called with. Install with
        video_io._python_tonemap_to_bgr8 = frames_hdr.reader_python_tonemap_to_bgr8
    The context is the one of set_reader_backend, else a module-wide context on device 0."""
    global _reader_ctx
    f = rgb_linear if isinstance(rgb_linear, HdrFrame) else _token(rgb_linear, "linear")
    if f.is_device:
        g = HdrFrame.on_device(*f.ptrs, f.H, f.W, f.pix_stride, f.row_stride, f.transfer, float(target_nits),
                               float(peak_nits), f._buf)
    else:
        g = HdrFrame(f.data, f.H, f.W, f.transfer, float(target_nits), float(peak_nits), f.layout, f.row_stride,
                     f.plane_stride if f.layout == "planar_gbr" else None)
    if _reader_numpy:
        return hdr_to_bgr_numpy(g)
    if _reader_ctx is None or not _reader_ctx.handle:
        from .runtime import GpuContext
        _reader_ctx = GpuContext(0)
    return hdr_to_bgr(g, _reader_ctx)
