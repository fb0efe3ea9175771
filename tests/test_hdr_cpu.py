"""The HDR conversion's NumPy backend (person_capture_amd/frames_hdr.py) against the reference's OWN
_eotf_pq / _eotf_hlg / _python_tonemap_to_bgr8 (video_io.py:3239-3291), through the data
tools/gen_golden_hdr.py recorded from them; HdrFrame's validation; the reader drop-ins. No GPU."""
import numpy as np
import pytest

import hdr_cases
from person_capture_amd import frames_hdr
from person_capture_amd.frames_hdr import HdrFrame

S = hdr_cases.SIDE


@pytest.fixture(scope="module")
def golden():
    with np.load(hdr_cases.GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def _frame(name, layout="planar_gbr"):
    rgb = hdr_cases.case_rgb(name)
    tr, t, peak = hdr_cases.case_params(name)
    if layout == "planar_gbr":
        return HdrFrame(hdr_cases.planar_gbr(rgb), S, S, tr, t, peak)
    return HdrFrame(np.stack((rgb[0], rgb[1], rgb[2]), axis=-1), S, S, tr, t, peak, layout="rgb")


@pytest.mark.parametrize("name", hdr_cases.CASE_NAMES)
def test_numpy_backend_against_reference(golden, name):
    """Every case: at most 1 LSB from the reference's recorded output, at most 5e-4 of the bytes differing
    (the reference's f32 np.power against the exactly rounded one). Both layouts of the same pixels give
    equal bytes."""
    ref = golden[name]
    assert ref.shape == (S, S, 3) and ref.size >= 196608
    got = frames_hdr.hdr_to_bgr(_frame(name))
    ok, mx, nbad = hdr_cases.within_cap(got, ref)
    print(name, "max diff", mx, "differing", nbad, "of", ref.size)
    assert ok, (name, mx, nbad)
    assert np.array_equal(frames_hdr.hdr_to_bgr(_frame(name, "rgb")), got)


def test_small_frame_and_host_forms(golden):
    """The small debugging frame: bytes, memoryview and array forms, and padded rows and planes."""
    H, W = (int(v) for v in golden["small_hw"])
    raw, ref = golden["small_raw"], golden["small_bgr"]
    got = frames_hdr.hdr_to_bgr(HdrFrame(raw, H, W, "pq", 200.0, 1000.0))
    assert hdr_cases.within_cap(got, ref)[0]
    assert np.array_equal(frames_hdr.hdr_to_bgr(HdrFrame(raw.tobytes(), H, W)), got)
    assert np.array_equal(frames_hdr.hdr_to_bgr(HdrFrame(memoryview(raw.tobytes()), H, W)), got)
    rs, gap = W + 5, 11
    buf = np.full(3 * (H * rs + gap), np.nan, np.float32)
    for p in range(3):
        for r in range(H):
            o = p * (H * rs + gap) + r * rs
            buf[o:o + W] = raw[(p * H + r) * W:(p * H + r + 1) * W]
    assert np.array_equal(frames_hdr.hdr_to_bgr(HdrFrame(buf, H, W, row_stride=rs, plane_stride=H * rs + gap)), got)
    planes = raw.reshape(3, H, W)
    hwc = np.full((H, W + 2, 3), np.nan, np.float32)
    hwc[:, :W] = np.stack((planes[2], planes[0], planes[1]), axis=-1)
    assert np.array_equal(frames_hdr.hdr_to_bgr(HdrFrame(hwc, H, W, layout="rgb", row_stride=3 * (W + 2))), got)
    f = HdrFrame(raw, H, W)
    assert f.shape == (H, W, 3) and f.ndim == 3 and f.size == H * W * 3 and not f.is_device


def test_validation():
    H, W = 6, 10
    z = np.zeros(3 * H * W, np.float32)
    HdrFrame(z, H, W)
    HdrFrame(z, 1, 1)
    for h, w in ((0, 4), (4, 0), (-2, 4), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError):
            HdrFrame(np.zeros(64, np.float32), h, w)
    with pytest.raises(ValueError):
        HdrFrame(z[:-1], H, W)                                  # short planar buffer
    with pytest.raises(ValueError):
        HdrFrame(z[:-1], H, W, layout="rgb")                    # short interleaved buffer
    with pytest.raises(ValueError):
        HdrFrame(z.tobytes()[:-2], H, W)                        # not whole floats
    with pytest.raises(ValueError):
        HdrFrame(z, H, W, row_stride=W - 1)
    with pytest.raises(ValueError):
        HdrFrame(z, H, W, layout="rgb", row_stride=3 * W - 1)
    with pytest.raises(ValueError):
        HdrFrame(z, H, W, row_stride=W + 1)                     # padded rows do not fit
    with pytest.raises(ValueError):
        HdrFrame(np.zeros(4 * H * W, np.float32), H, W, plane_stride=H * W - 1)   # planes overlap
    with pytest.raises(ValueError):
        HdrFrame(z.astype(np.float64), H, W)
    with pytest.raises(ValueError):
        HdrFrame(z.astype(np.float16), H, W)
    with pytest.raises(ValueError):
        HdrFrame(z, H, W, transfer="srgb")
    with pytest.raises(ValueError):
        HdrFrame(z, H, W, layout="bgr")
    for nits in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            HdrFrame(z, H, W, sdr_nits=nits)
        with pytest.raises(ValueError):
            HdrFrame(z, H, W, peak_nits=nits)
    with pytest.raises(ValueError):
        HdrFrame.on_device(0, 16, 32, H, W)
    with pytest.raises(ValueError):
        HdrFrame.on_device(18, 16, 32, H, W)                    # not 4-byte aligned
    with pytest.raises(ValueError):
        HdrFrame.on_device(16, 32, 48, H, W, pix_stride=2)
    with pytest.raises(ValueError):
        HdrFrame(z, H, W).job(16)                               # a host frame has no device job


class _Reader:
    """What FfmpegPipeReader.grab / retrieve do with one float frame (video_io.py:3005-3018, 3183-3192),
    with the module functions looked up where the drop-ins are installed."""

    def __init__(self, h, w, transfer, sdr_nits):
        self._h, self._w, self._transfer, self._sdr_nits = h, w, transfer, sdr_nits

    def frame(self, buf: bytes):
        planar = np.frombuffer(buf, dtype=np.float32).reshape(3, self._h, self._w)
        rgb = np.stack((planar[2], planar[0], planar[1]), axis=-1)
        if getattr(self, "_transfer", "") == "arib-std-b67":
            arr = frames_hdr.reader_eotf_hlg(rgb)
        else:
            arr = frames_hdr.reader_eotf_pq(rgb)
        return frames_hdr.reader_python_tonemap_to_bgr8(arr, peak_nits=1000.0,
                                                        target_nits=float(getattr(self, "_sdr_nits", 200.0)))


@pytest.mark.parametrize("transfer,name,nits", [("smpte2084", "pq", 203.0), ("arib-std-b67", "hlg", 100.0)])
def test_reader_drop_ins(transfer, name, nits):
    """The three drop-ins driven the way the unchanged reader drives them return what hdr_to_bgr_numpy
    returns for the pipe's bytes; the EOTF drop-ins compute nothing and record the transfer."""
    frames_hdr.set_reader_backend("numpy")
    try:
        H, W = 18, 26
        raw = np.random.default_rng(5).random(3 * H * W, dtype=np.float32)
        want = frames_hdr.hdr_to_bgr_numpy(HdrFrame(raw, H, W, name, nits, 1000.0))
        got = _Reader(H, W, transfer, nits).frame(raw.tobytes())
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want)
        tok = (frames_hdr.reader_eotf_hlg if name == "hlg" else frames_hdr.reader_eotf_pq)(
            np.zeros((H, W, 3), np.float32))
        assert isinstance(tok, HdrFrame) and tok.transfer == name and tok.layout == "rgb" and tok.shape == (H, W, 3)
        # a plain linear array takes transfer 'linear'
        lin = np.random.default_rng(6).random((H, W, 3), dtype=np.float32) * np.float32(0.05)
        want = frames_hdr.hdr_to_bgr_numpy(HdrFrame(lin, H, W, "linear", nits, 800.0, layout="rgb"))
        assert np.array_equal(frames_hdr.reader_python_tonemap_to_bgr8(lin, peak_nits=800.0, target_nits=nits), want)
    finally:
        frames_hdr.set_reader_backend(None)
    with pytest.raises(ValueError):
        frames_hdr.set_reader_backend("cpu")
