"""The NumPy backend of person_capture_amd.frames against the reference's own
FfmpegPipeReader._nv12_to_bgr (video_io.py:2888-2912), through the data tools/gen_golden_nv12.py
recorded from it: the SHA-256 of the exhaustive frame (every (Y, U, V) triple once) and one small
frame. Every comparison is ==."""
import hashlib

import numpy as np
import pytest

import nv12_cases
from person_capture_amd import frames


@pytest.fixture(scope="module")
def golden():
    with np.load(nv12_cases.GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def test_exhaustive_frame_has_every_triple_once():
    S = nv12_cases.EXHAUSTIVE_SIDE
    raw = nv12_cases.exhaustive_nv12()
    y = raw[:S * S].reshape(S, S).astype(np.int64)
    uv = raw[S * S:].reshape(S // 2, S).astype(np.int64)
    u = np.repeat(np.repeat(uv[:, 0::2], 2, 0), 2, 1)
    v = np.repeat(np.repeat(uv[:, 1::2], 2, 0), 2, 1)
    assert np.array_equal(np.sort(((y << 16) | (u << 8) | v).reshape(-1)), np.arange(1 << 24))


def test_numpy_backend_exhaustive_hash(golden):
    S = nv12_cases.EXHAUSTIVE_SIDE
    out = frames.nv12_to_bgr(frames.Nv12Frame(nv12_cases.exhaustive_nv12(), S, S))
    assert out.shape == (S, S, 3) and out.dtype == np.uint8
    assert hashlib.sha256(out.tobytes()).digest() == golden["exhaustive_sha256"].tobytes()


def test_numpy_backend_small_frame(golden):
    H, W = (int(x) for x in golden["small_hw"])
    raw = golden["small_raw"]
    assert np.array_equal(frames.nv12_to_bgr(frames.Nv12Frame(raw, H, W)), golden["small_bgr"])
    # bytes and memoryview are the pipe's types
    assert np.array_equal(frames.nv12_to_bgr(frames.Nv12Frame(raw.tobytes(), H, W)), golden["small_bgr"])
    assert np.array_equal(frames.nv12_to_bgr(frames.Nv12Frame(memoryview(raw.tobytes()), H, W)), golden["small_bgr"])


def test_numpy_backend_plane_strides(golden):
    """Padded plane strides and a gap between the planes give the packed frame's bytes."""
    H, W = (int(x) for x in golden["small_hw"])
    raw = golden["small_raw"]
    ys, uvs, gap = W + 5, W + 11, 7
    buf = np.full(H * ys + gap + (H // 2) * uvs, 0xEE, np.uint8)
    for r in range(H):
        buf[r * ys:r * ys + W] = raw[r * W:(r + 1) * W]
    for r in range(H // 2):
        o = H * ys + gap + r * uvs
        buf[o:o + W] = raw[(H + r) * W:(H + r + 1) * W]
    f = frames.Nv12Frame(buf, H, W, y_stride=ys, uv_stride=uvs, uv_offset=H * ys + gap)
    assert np.array_equal(frames.nv12_to_bgr(f), golden["small_bgr"])


@pytest.mark.parametrize("H,W", [(47, 64), (48, 63), (0, 64), (48, 16386), (1, 1)])
def test_bad_sizes_raise(H, W):
    with pytest.raises(ValueError):
        frames.Nv12Frame(np.zeros(max(1, W * max(H, 1) * 2), np.uint8), H, W)


def test_short_buffer_and_short_strides_raise():
    H, W = 48, 64
    with pytest.raises(ValueError):
        frames.Nv12Frame(np.zeros(W * H * 3 // 2 - 1, np.uint8), H, W)
    with pytest.raises(ValueError):
        frames.Nv12Frame(np.zeros(W * H * 2, np.uint8), H, W, y_stride=W - 1)
    with pytest.raises(ValueError):
        frames.Nv12Frame(np.zeros(W * H * 2, np.uint8), H, W, uv_stride=W - 2)
    with pytest.raises(ValueError):   # strides that need more bytes than there are
        frames.Nv12Frame(np.zeros(W * H * 3 // 2, np.uint8), H, W, y_stride=W + 16)
    with pytest.raises(ValueError):
        frames.Nv12Frame(np.zeros(W * H * 3, np.uint16), H, W)


def test_reader_returns_none_on_short_buffer():
    """FfmpegPipeReader._nv12_to_bgr's contract (video_io.py:2894-2896): a short read is None, before
    any device is touched."""
    class Reader:
        _h, _w = 48, 64
    assert frames.reader_nv12_to_bgr(Reader(), bytes(48 * 64 * 3 // 2 - 1)) is None
    assert frames.reader_nv12_to_bgr(Reader(), b"") is None
