"""NV12 frames: the second wire format of the reference's frame source.

With PC_PIPE_PIXFMT=nv12 (or after a pipe ENOMEM, video_io.py:1225-1228, 1901-1904) the reference's
FfmpegPipeReader receives NV12 from the decoder and converts every frame to BGR on the CPU with
float32 NumPy (FfmpegPipeReader._nv12_to_bgr, video_io.py:2888-2912). This module states that
operation once and offers it on the device (pc_nv12_to_bgr, csrc/pc_nv12.hip).

The operation, exactly:
  * Y plane H x W u8; UV plane (H/2) x W u8, interleaved U, V; each chroma sample is replicated
    2 x 2, no interpolation.
  * in float32, each operation rounded once, in this order (C = y - 16, D = u - 128, E = v - 128,
    constants rounded to f32):
        r = k0 C + k1 E
        g = (k0 C - k2 D) - k3 E
        b = k0 C + k4 D
    k = (1.16438356, 1.79274107, 0.21324861, 0.53290933, 2.11240179)
  * clamp to [0, 255], truncate to u8, store B, G, R.
  * H and W even (the reference's reshape / repeat fail otherwise; here a ValueError), 2 .. 16384.

`Nv12Frame` entries are accepted wherever this package takes a BGR frame (FaceEmbedder.extract /
extract_batch, PersonDetector.detect / detect_batch, PrescanRunner's frame_at): they are uploaded as
NV12 (half the bytes of BGR) and converted on the device.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import PC_NV12_MAX_SIDE, Nv12Desc, check

K = tuple(np.float32(k) for k in (1.16438356, 1.79274107, 0.21324861, 0.53290933, 2.11240179))


def _check_size(H: int, W: int) -> None:
    if H < 2 or W < 2 or H > PC_NV12_MAX_SIDE or W > PC_NV12_MAX_SIDE or (H & 1) or (W & 1):
        raise ValueError(f"NV12 frame {H} x {W}: H and W must be even, 2 .. {PC_NV12_MAX_SIDE}")


class Nv12Frame:
    """One NV12 frame.

    Host form, Nv12Frame(data, H, W): `data` is what the reference's pipe delivers (bytes, memoryview
    or a u8 array): H rows of Y, y_stride apart (default W), then H/2 rows of interleaved U, V,
    uv_stride apart (default W), the UV plane starting at uv_offset (default H * y_stride).
    Device form, Nv12Frame.on_device(y_ptr, uv_ptr, H, W, y_stride, uv_stride): planes already in HBM.
    """

    __slots__ = ("H", "W", "y_stride", "uv_stride", "data", "uv_offset", "y_ptr", "uv_ptr", "_buf")

    def __init__(self, data, H: int, W: int, y_stride: Optional[int] = None, uv_stride: Optional[int] = None,
                 uv_offset: Optional[int] = None):
        self.H, self.W = int(H), int(W)
        _check_size(self.H, self.W)
        self.y_stride = self.W if y_stride is None else int(y_stride)
        self.uv_stride = self.W if uv_stride is None else int(uv_stride)
        if self.y_stride < self.W or self.uv_stride < self.W:
            raise ValueError(f"NV12 plane strides ({self.y_stride}, {self.uv_stride}) shorter than W = {self.W}")
        a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if a.dtype != np.uint8:
            raise ValueError("NV12 data must be bytes or a uint8 array")
        a = np.ascontiguousarray(a).reshape(-1)
        self.uv_offset = self.H * self.y_stride if uv_offset is None else int(uv_offset)
        if self.uv_offset < (self.H - 1) * self.y_stride + self.W:
            raise ValueError("NV12 UV plane overlaps the Y plane")
        need = self.uv_offset + (self.H // 2 - 1) * self.uv_stride + self.W
        if a.size < need:
            raise ValueError(f"NV12 frame {self.H} x {self.W}: {a.size} bytes, {need} needed")
        self.data = a
        self.y_ptr = self.uv_ptr = 0
        self._buf = None

    @classmethod
    def on_device(cls, y_ptr: int, uv_ptr: int, H: int, W: int, y_stride: Optional[int] = None,
                  uv_stride: Optional[int] = None, buf=None) -> "Nv12Frame":
        f = cls.__new__(cls)
        f.H, f.W = int(H), int(W)
        _check_size(f.H, f.W)
        f.y_stride = f.W if y_stride is None else int(y_stride)
        f.uv_stride = f.W if uv_stride is None else int(uv_stride)
        if f.y_stride < f.W or f.uv_stride < f.W or not y_ptr or not uv_ptr:
            raise ValueError("NV12 device frame: null plane or a stride shorter than W")
        f.data, f.uv_offset = None, 0
        f.y_ptr, f.uv_ptr, f._buf = int(y_ptr), int(uv_ptr), buf
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
        return self.W * self.H * 3 // 2

    def job(self, d_dst: int, dst_stride: Optional[int] = None) -> tuple:
        """The pc_nv12_to_bgr job (nv12_descs) of this device frame into d_dst (rows 3 W bytes apart by
        default)."""
        if not self.is_device:
            raise ValueError("a host NV12 frame is staged first (stage_nv12)")
        return (self.y_ptr, self.uv_ptr, self.H, self.W, self.y_stride, self.uv_stride, int(d_dst),
                3 * self.W if dst_stride is None else int(dst_stride))

    def planes(self) -> Tuple[np.ndarray, np.ndarray]:
        """(Y [H][W], UV [H/2][W]) u8 views of the host data."""
        if self.is_device:
            raise ValueError("a device NV12 frame has no host planes")
        H, W, a = self.H, self.W, self.data
        y = np.lib.stride_tricks.as_strided(a, (H, W), (self.y_stride, 1), writeable=False)
        uv = np.lib.stride_tricks.as_strided(a[self.uv_offset:], (H // 2, W), (self.uv_stride, 1), writeable=False)
        return y, uv


def nv12_to_bgr_numpy(frame: Nv12Frame) -> np.ndarray:
    """The operation of the module docstring in NumPy: float32, every operation rounded once."""
    y8, uv8 = frame.planes()
    y = y8.astype(np.float32)
    uv = uv8.astype(np.float32)
    u = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)
    c = y - np.float32(16.0)
    d = u - np.float32(128.0)
    e = v - np.float32(128.0)
    yc = K[0] * c
    out = np.empty((frame.H, frame.W, 3), np.float32)
    out[..., 0] = yc + K[4] * d
    out[..., 1] = (yc - K[2] * d) - K[3] * e
    out[..., 2] = yc + K[1] * e
    return np.clip(out, np.float32(0.0), np.float32(255.0), out=out).astype(np.uint8)


# ---- device ----
def nv12_descs(jobs: Sequence[Tuple[int, int, int, int, int, int, int, int]]):
    """pc_nv12_desc array of (y_ptr, uv_ptr, H, W, y_stride, uv_stride, dst_ptr, dst_stride) tuples."""
    descs = (Nv12Desc * max(1, len(jobs)))()
    for d, (yp, uvp, H, W, ys, uvs, dp, ds) in zip(descs, jobs):
        d.d_y, d.d_uv, d.H, d.W, d.y_stride, d.uv_stride, d.d_dst, d.dst_stride = yp, uvp, H, W, ys, uvs, dp, ds
    return descs


def convert_on_device(ctx, jobs) -> None:
    """One pc_nv12_to_bgr over `jobs` (see nv12_descs) on the context's stream."""
    if jobs:
        check(ctx.lib.pc_nv12_to_bgr(ctx.handle, nv12_descs(jobs), len(jobs)), ctx.handle, "nv12_to_bgr")


def stage_nv12(h2d, frame: Nv12Frame, d_dst: int, threads: int = 4) -> Nv12Frame:
    """A host NV12 frame -> d_dst packed (Y rows, then UV rows, W bytes each: 3 H / 2 rows) through the
    context's pinned staging ring (pc_frame_stage). Returns the device form of the frame."""
    H, W = frame.H, frame.W
    if frame.y_stride == frame.uv_stride and frame.uv_offset == H * frame.y_stride:
        a = np.lib.stride_tricks.as_strided(frame.data, (H * 3 // 2, W, 1), (frame.y_stride, 1, 1), writeable=False)
        h2d.stage_frame(a, d_dst, threads)
    else:
        y, uv = frame.planes()
        h2d.stage_frame(y[:, :, None], d_dst, threads)
        h2d.stage_frame(uv[:, :, None], d_dst + H * W, threads)
    return Nv12Frame.on_device(d_dst, d_dst + H * W, H, W, W, W)


def nv12_to_bgr(frame: Nv12Frame, ctx=None) -> np.ndarray:
    """H x W x 3 BGR u8 of an NV12 frame. ctx=None: the NumPy backend; a runtime.GpuContext: upload,
    pc_nv12_to_bgr, download (the same bytes)."""
    if ctx is None:
        return nv12_to_bgr_numpy(frame)
    H, W = frame.H, frame.W
    if frame.is_device:
        dev = frame
    else:
        dev = stage_nv12(ctx, frame, ctx.scratch("nv12_src", frame.packed_bytes).ptr)
    out = ctx.scratch("nv12_bgr", H * W * 3)
    convert_on_device(ctx, [dev.job(out.ptr)])
    return ctx.download(out.ptr, (H, W, 3), np.uint8)


_reader_ctx = None


def reader_nv12_to_bgr(self, raw) -> Optional[np.ndarray]:
    """Drop-in for FfmpegPipeReader._nv12_to_bgr (video_io.py:2888-2912), converting on the device:
    None when `raw` is shorter than W * H * 3 / 2 bytes, else the H x W x 3 BGR array. Install with
        video_io.FfmpegPipeReader._nv12_to_bgr = frames.reader_nv12_to_bgr
    The context is self._pc_ctx when the reader carries one, else a module-wide context on device 0."""
    global _reader_ctx
    h, w = int(self._h), int(self._w)
    need = (w * h * 3) // 2
    if len(raw) < need:
        return None
    ctx = getattr(self, "_pc_ctx", None)
    if ctx is None:
        if _reader_ctx is None or not _reader_ctx.handle:
            from .runtime import GpuContext
            _reader_ctx = GpuContext(0)
        ctx = _reader_ctx
    return nv12_to_bgr(Nv12Frame(np.frombuffer(raw, dtype=np.uint8, count=need), h, w), ctx)
