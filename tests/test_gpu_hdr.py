"""HDR frames on the device (csrc/pc_hdr.hip, person_capture_amd/frames_hdr.py) against the NumPy backend
(==, byte for byte) and against the outputs recorded from the reference's own _eotf_pq / _eotf_hlg /
_python_tonemap_to_bgr8 (video_io.py:3239-3291; 1 LSB, 5e-4 of the bytes: hdr_cases.within_cap)."""
import numpy as np
import pytest

import hdr_cases
from person_capture_amd import face_embedder as fe_mod
from person_capture_amd import frames, frames_hdr
from person_capture_amd._lib import PC_OK
from person_capture_amd.frames_hdr import HdrFrame

pytestmark = pytest.mark.gpu
PC_ERR_ARG = 1
S = hdr_cases.SIDE
GPU_CASES = [n for n, cls, _, t in hdr_cases.CASES if cls in ("boundary", "uniform") and t in (100.0, 203.0)]
assert len(GPU_CASES) == 12


@pytest.fixture(scope="module")
def golden():
    with np.load(hdr_cases.GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("layout", ["planar_gbr", "rgb"])
@pytest.mark.parametrize("name", GPU_CASES)
def test_cases_equal_numpy_backend_and_reference(gpu_ctx, golden, name, layout):
    """The boundary ramp (+-inf, -0.0, subnormals, the neighbourhoods of 0, 0.5 and 1, every decade) and the
    random frames, for pq, hlg and linear at 100 and 203 nits, from host frames of both layouts."""
    rgb = hdr_cases.case_rgb(name)
    tr, t, peak = hdr_cases.case_params(name)
    if layout == "planar_gbr":
        f = HdrFrame(hdr_cases.planar_gbr(rgb), S, S, tr, t, peak)
    else:
        f = HdrFrame(np.stack((rgb[0], rgb[1], rgb[2]), axis=-1), S, S, tr, t, peak, layout="rgb")
    ref = frames_hdr.hdr_to_bgr(f)
    got = frames_hdr.hdr_to_bgr(f, gpu_ctx)
    assert got.shape == (S, S, 3) and got.dtype == np.uint8
    bad = np.argwhere((got != ref).any(axis=2))
    if len(bad):   # a finding, not a tolerance: the sample and both values
        y, x = bad[0]
        print("first difference at", (y, x), "signal", rgb[:, y, x].tolist(), "device", got[y, x], "numpy", ref[y, x])
    assert len(bad) == 0, (name, len(bad), bad[:8])
    ok, mx, nbad = hdr_cases.within_cap(got, golden[name])
    print(name, layout, "against the reference: max diff", mx, "differing", nbad)
    assert ok, (name, mx, nbad)


# ---- mixed sizes, layouts and placements in one launch ----
_GEOM = [(1, 1), (1, 7), (5, 37), (33, 64), (270, 482), (540, 960)]
_TRANSFERS = ["pq", "hlg", "linear", "hlg", "pq", "hlg"]
_TARGETS = [100.0, 203.0, 200.0, 400.0, 203.0, 100.0]
_PEAKS = [1000.0, 1000.0, 600.0, 4000.0, 1000.0, 1000.0]


def _pad(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def geom_frames():
    """Per geometry: the (3, H, W) signal and the NumPy backend's bytes."""
    rng = np.random.default_rng(1313)
    sigs, refs = [], []
    for (H, W), tr, t, pk in zip(_GEOM, _TRANSFERS, _TARGETS, _PEAKS):
        s = rng.random((3, H, W), dtype=np.float32) * np.float32(1.1) - np.float32(0.05)
        if tr == "linear":
            s = (s * s) * np.float32(0.08)
        sigs.append(s)
        refs.append(frames_hdr.hdr_to_bgr(HdrFrame(hdr_cases.planar_gbr(s), H, W, tr, t, pk)))
    return sigs, refs


def _place(ctx, sig, H, W, pix_stride, off, packed):
    """The signal in device memory: (buffers, r_ptr, g_ptr, b_ptr, row_stride). packed: rows W pix_stride
    floats apart and every array an allocation of its own that ends with its last sample; else padded rows
    and (off) a base 4 bytes off a 16-byte boundary with an odd row stride."""
    if pix_stride == 3:
        hwc = np.stack((sig[0], sig[1], sig[2]), axis=-1)
        if packed:
            b = ctx.upload(hwc)
            assert b.nbytes == H * W * 12
            return [b], b.ptr, b.ptr + 4, b.ptr + 8, 3 * W
        base, rs = (1, _pad(3 * W, 4) + 5) if off else (0, _pad(3 * W, 4) + 4)
        host = np.full(base + H * rs + 4, np.float32(-7.0), np.float32)
        for r in range(H):
            host[base + r * rs:base + r * rs + 3 * W] = hwc[r].reshape(-1)
        b = ctx.upload(host)
        p = b.ptr + 4 * base
        return [b], p, p + 4, p + 8, rs
    if packed:
        bs = [ctx.upload(np.ascontiguousarray(sig[c])) for c in range(3)]
        assert all(b.nbytes == H * W * 4 for b in bs)
        return bs, bs[0].ptr, bs[1].ptr, bs[2].ptr, W
    base, rs = (1, _pad(W, 4) + 5) if off else (0, _pad(W, 4) + 4)
    plane = _pad(H * rs + 4, 4)
    host = np.full(base + 3 * plane, np.float32(-7.0), np.float32)
    for c, p in ((1, 0), (2, 1), (0, 2)):   # memory order G, B, R as on the pipe
        for r in range(H):
            o = base + p * plane + r * rs
            host[o:o + W] = sig[c][r]
    b = ctx.upload(host)
    q = b.ptr + 4 * base
    return [b], q + 8 * plane, q, q + 4 * plane, rs


@pytest.mark.parametrize("placement", ["aligned", "offset"])
def test_mixed_sizes_one_launch(gpu_ctx, geom_frames, placement):
    """Six sizes from 1 x 1 to 540 x 960, each as planes and as an interleaved array, with their own
    transfers and nits, in ONE pc_hdr_to_bgr: row strides larger than the row, dst_stride > 3 W with the row
    padding and 64 guard bytes around every destination prefilled with 0xA5 and required unchanged.
    'aligned': every pointer and stride a multiple of 16 bytes (16-byte loads, 12-byte stores, the scalar
    path for the W % 4 tails); 'offset': sample pointers 4 bytes and destinations 3 bytes off a 16-byte
    boundary, odd strides (the scalar path). The last frame's samples (packed) end on the last byte of
    allocations of their own."""
    sigs, refs = geom_frames
    off = placement == "offset"
    dst_off, dst_strides, geoms = [], [], []
    total = 64
    for ps in (1, 3):
        for (H, W) in _GEOM:
            ds = _pad(3 * W, 16) + 16 + (5 if off else 0)
            total = _pad(total, 16) + (3 if off else 0)
            dst_off.append(total)
            dst_strides.append(ds)
            geoms.append((H, W))
            total += H * ds + 64
    dst = gpu_ctx.alloc(total + 64)
    gpu_ctx.memset(dst.ptr, 0xA5, total + 64)
    keep, jobs = [], []
    for li, ps in enumerate((1, 3)):
        for k, ((H, W), sig) in enumerate(zip(_GEOM, sigs)):
            packed = k == len(_GEOM) - 1
            bufs, rp, gp, bp, rs = _place(gpu_ctx, sig, H, W, ps, off, packed)
            if not packed:
                assert rp % 16 == (4 if off else 0) and (rs * 4) % 16 == (4 if off else 0)
            keep.append(bufs)
            q = li * len(_GEOM) + k
            assert (dst.ptr + dst_off[q]) % 16 == (3 if off else 0)
            jobs.append((rp, gp, bp, H, W, ps, rs, dst.ptr + dst_off[q], dst_strides[q], _TRANSFERS[k], _TARGETS[k],
                         _PEAKS[k]))
    frames_hdr.convert_on_device(gpu_ctx, jobs)
    out = gpu_ctx.download(dst.ptr, (total + 64,), np.uint8)
    mask = np.ones(total + 64, bool)   # bytes that must still be 0xA5
    for q, ((H, W), o, ds) in enumerate(zip(geoms, dst_off, dst_strides)):
        rows = np.lib.stride_tricks.as_strided(out[o:], (H, 3 * W), (ds, 1))
        assert np.array_equal(rows.reshape(H, W, 3), refs[q % len(_GEOM)]), (q, H, W)
        for r in range(H):
            mask[o + r * ds:o + r * ds + 3 * W] = False
    assert (out[mask] == 0xA5).all()


def test_argument_handling(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    H, W = 4, 32
    sig = np.full(3 * H * W, np.float32(0.5), np.float32)
    src = gpu_ctx.upload(sig)
    dst = gpu_ctx.alloc(2 * H * W * 3)
    gpu_ctx.memset(dst.ptr, 0xA5, 2 * H * W * 3)
    names = ("r", "g", "b", "H", "W", "ps", "rs", "dst", "ds", "tr", "tn", "pn")
    good = (src.ptr + 8 * H * W, src.ptr, src.ptr + 4 * H * W, H, W, 1, W, dst.ptr, 3 * W, "pq", 200.0, 1000.0)

    def call(jobs, n=None):
        return lib.pc_hdr_to_bgr(h, frames_hdr.hdr_descs(jobs), len(jobs) if n is None else n)

    assert lib.pc_hdr_to_bgr(h, None, 0) == PC_OK
    assert call([good], 0) == PC_OK
    assert call([good], -1) == PC_ERR_ARG
    assert lib.pc_hdr_to_bgr(h, None, 1) == PC_ERR_ARG

    def with_(**kw):
        d = dict(zip(names, good))
        d.update(kw)
        return tuple(d[k] for k in names)

    nan, inf = float("nan"), float("inf")
    bad = [with_(r=0), with_(g=0), with_(b=0), with_(dst=0), with_(r=good[0] + 2), with_(g=good[1] + 1),
           with_(b=good[2] + 3), with_(H=0), with_(W=0), with_(H=-1), with_(H=16385), with_(W=16385),
           with_(rs=W - 1), with_(ps=3, rs=3 * W - 1), with_(ps=2), with_(ps=0), with_(ps=4), with_(ds=3 * W - 1),
           with_(tr=3), with_(tr=-1), with_(tn=0.0), with_(tn=-5.0), with_(tn=nan), with_(tn=inf), with_(pn=0.0),
           with_(pn=-1.0), with_(pn=nan), with_(pn=inf)]
    for b in bad:
        assert call([b]) == PC_ERR_ARG, b
        # nothing is staged or launched when a later frame of the batch is bad
        assert call([with_(dst=dst.ptr + H * W * 3), b]) == PC_ERR_ARG, b
    assert b"pc_hdr_to_bgr" in lib.pc_last_error(h)
    assert (gpu_ctx.download(dst.ptr, (2 * H * W * 3,), np.uint8) == 0xA5).all()
    assert call([good]) == PC_OK   # the context is still usable
    got = gpu_ctx.download(dst.ptr, (H, W, 3), np.uint8)
    assert np.array_equal(got, frames_hdr.hdr_to_bgr(HdrFrame(sig, H, W)))


def test_stage_hdr_row_blocks_and_padded_host_frames(gpu_ctx, geom_frames, monkeypatch):
    """stage_hdr: a host frame staged in many row blocks (the block size lowered to 64 KB: 33 rows of the
    270 x 482 frame a block), planes with padded rows and a gap between them (one staging per plane),
    and an interleaved array with padded rows, all equal to the NumPy backend."""
    sigs, refs = geom_frames
    k = _GEOM.index((270, 482))
    (H, W), sig, ref = _GEOM[k], sigs[k], refs[k]
    tr, t, pk = _TRANSFERS[k], _TARGETS[k], _PEAKS[k]
    monkeypatch.setattr(frames_hdr, "STAGE_BLOCK_BYTES", 64 << 10)
    packed = HdrFrame(hdr_cases.planar_gbr(sig), H, W, tr, t, pk)
    assert np.array_equal(frames_hdr.hdr_to_bgr(packed, gpu_ctx), ref)
    rs, gap = W + 3, 17
    buf = np.full(3 * (H * rs + gap), np.float32(-7.0), np.float32)
    for p, c in enumerate((1, 2, 0)):
        rows = np.lib.stride_tricks.as_strided(buf[p * (H * rs + gap):], (H, W), (4 * rs, 4))
        rows[:] = sig[c]
    padded = HdrFrame(buf, H, W, tr, t, pk, row_stride=rs, plane_stride=H * rs + gap)
    assert np.array_equal(frames_hdr.hdr_to_bgr(padded, gpu_ctx), ref)
    hwc = np.full((H, W + 1, 3), np.float32(-7.0), np.float32)
    hwc[:, :W] = np.stack((sig[0], sig[1], sig[2]), axis=-1)
    inter = HdrFrame(hwc, H, W, tr, t, pk, layout="rgb", row_stride=3 * (W + 1))
    assert np.array_equal(frames_hdr.hdr_to_bgr(inter, gpu_ctx), ref)


# ---- facades ----
def _soft_hdr(seed, H, W, transfer="hlg", layout="planar_gbr"):
    """A near-grey noise frame whose converted form is mid-grey noise over the whole u8 range, not clipped."""
    rng = np.random.default_rng(seed)
    lo, hi = (0.0, 0.72) if transfer == "hlg" else (0.3, 0.85)
    y = rng.random((H, W), dtype=np.float32)
    c = rng.random((3, H, W), dtype=np.float32) * np.float32(0.06) - np.float32(0.03)
    s = np.float32(lo) + np.float32(hi - lo) * y + c
    if layout == "rgb":
        return HdrFrame(np.stack((s[0], s[1], s[2]), axis=-1), H, W, transfer, 200.0, 1000.0, layout="rgb")
    return HdrFrame(hdr_cases.planar_gbr(s), H, W, transfer, 200.0, 1000.0)


def _soft_nv12(seed, H, W):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    raw[H * W:] = rng.integers(96, 160, H * W // 2, dtype=np.uint8)
    return frames.Nv12Frame(raw, H, W)


def _face_key(f):
    return (tuple(int(v) for v in f["bbox"]), f["feat"].tobytes(), float(f["quality"]))


def _batches(seed, H, W):
    """(all-BGR, the same as HdrFrames, HDR / BGR alternated), and a second batch with an NV12 frame in the
    middle as (all-BGR, [HDR, NV12, BGR])."""
    hd = [_soft_hdr(seed, H, W, "hlg"), _soft_hdr(seed + 1, H, W, "pq", "rgb"), _soft_hdr(seed + 2, H, W, "hlg", "rgb")]
    bgr = [frames_hdr.hdr_to_bgr(f) for f in hd]
    assert all(40 < b.mean() < 215 and (b == 255).mean() < 0.2 for b in bgr), [b.mean() for b in bgr]
    nv = _soft_nv12(seed + 3, H, W)
    return ((bgr, hd, [hd[0], bgr[1], hd[2]]), ([bgr[0], frames.nv12_to_bgr(nv), bgr[2]], [hd[0], nv, bgr[2]]))


def test_extract_batch_hdr_equals_bgr(gpu_ctx, monkeypatch):
    """FaceEmbedder.extract_batch (SCRFD-2.5g) over 3 frames given as HdrFrame, as hdr_to_bgr arrays, mixed,
    and in a BGR / NV12 / HDR mix: the same boxes, features, quality and policy state."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    first, second = _batches(170, 360, 640)
    st0 = fe.policy_state()

    def run(batch):
        fe.set_policy_state(st0)
        res = fe.extract_batch(batch, imgsz=320)
        return [[_face_key(f) for f in fr] for fr in res], fe.policy_state()

    runs = [run(b) for b in first]
    print("faces per frame", [len(fr) for fr in runs[0][0]])
    assert sum(len(fr) for fr in runs[0][0]) > 0
    assert runs[1] == runs[0] and runs[2] == runs[0]
    assert run(second[1]) == run(second[0])
    fe.set_policy_state(st0)
    assert [_face_key(f) for f in fe.extract(first[1][0], imgsz=320)] == runs[0][0][0]


def test_extract_batch_yolo_face_hdr_equals_bgr(gpu_ctx, monkeypatch):
    """The same on the YOLOv8-face backend (yolov8n-face)."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="yolov8n-face.pt", conf=0.05)
    assert fe.detector_backend == "yolo"
    first, second = _batches(175, 360, 640)

    def run(batch):
        return [[_face_key(f) for f in fr] for fr in fe.extract_batch(batch)]

    runs = [run(b) for b in first]
    print("faces per frame", [len(fr) for fr in runs[0]])
    assert runs[1] == runs[0] and runs[2] == runs[0]
    assert run(second[1]) == run(second[0])
    assert [_face_key(f) for f in fe.extract(first[1][2])] == runs[0][2]


def test_detect_batch_hdr_equals_bgr(gpu_ctx):
    from person_capture_amd.detectors import PersonDetector
    det = PersonDetector("yolov8n.pt", device="cuda")
    first, second = _batches(180, 360, 640)
    a = det.detect_batch(first[0], conf=0.05)
    assert det.detect_batch(first[1], conf=0.05) == a
    assert det.detect_batch(first[2], conf=0.05) == a
    assert det.detect_batch(second[1], conf=0.05) == det.detect_batch(second[0], conf=0.05)
    assert det.detect(first[1][1], conf=0.05) == a[1]
    print("persons per frame", [len(x) for x in a])


def test_prescan_hdr_equals_bgr(gpu_ctx, monkeypatch):
    """A PrescanRunner over 8 samples of 540 x 960 at prescan_max_width 416: HdrFrame samples, and a BGR /
    NV12 / HDR mix, give the BGR samples' records, spans, bank and final policy state."""
    from person_capture_amd.prescan import PrescanConfig, PrescanRunner
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    H, W, N = 540, 960, 8
    four = [_soft_hdr(190 + k, H, W, "hlg", "rgb" if k & 1 else "planar_gbr") for k in range(3)]
    nv = _soft_nv12(199, H, W)
    four_bgr = [frames_hdr.hdr_to_bgr(f, gpu_ctx) for f in four] + [frames.nv12_to_bgr(nv)]
    hd = [(four + [nv])[i // 2] for i in range(N)]
    bgr = [four_bgr[i // 2] for i in range(N)]
    mix = [bgr[i] if i % 3 == 0 else hd[i] for i in range(N)]
    bank = np.random.default_rng(9).standard_normal((2, 512)).astype(np.float32)
    cfg = PrescanConfig(prescan_stride=1, prescan_max_width=416, prescan_fd9_skip=False, face_quality_min=0.0,
                        prescan_fd_enter=2.5, prescan_fd_exit=3.0, prescan_fd_add=2.5,
                        prescan_add_cooldown_samples=2)
    st0 = fe.policy_state()

    def run(src):
        fe.set_policy_state(st0)
        r = PrescanRunner(fe, cfg, 4.0, N, ref_feat=bank, batch=8)
        spans, b = r.run(lambda i: src[i])
        return spans, b.tobytes(), [tuple(vars(x).items()) for x in r.records], fe.policy_state()

    base = run(bgr)
    print("spans", base[0], "faces", [dict(x)["n_faces"] for x in base[2]])
    assert sum(dict(x)["n_faces"] for x in base[2]) > 0
    assert run(hd) == base
    assert run(mix) == base


def test_extract_batch_16_frames_two_source_buffers(gpu_ctx, monkeypatch):
    """16 HdrFrames of 540 x 960 (7.5 MB of floats each) in one extract_batch: equal to the BGR run, through
    the two source scratch buffers only - 14 of the 16 copies go into a scratch an earlier frame of the call
    used, which is right only with the ordering edge from a conversion back to the next copy."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    H, W, N = 540, 960, 16
    hd = [_soft_hdr(300 + i, H, W, "pq" if i % 4 == 3 else "hlg", "rgb" if i & 1 else "planar_gbr") for i in range(N)]
    bgr = [frames_hdr.hdr_to_bgr(f, gpu_ctx) for f in hd]
    assert len({b.tobytes()[:4096] for b in bgr}) == N
    st0 = fe.policy_state()

    def run(batch):
        fe.set_policy_state(st0)
        res = fe.extract_batch(batch, imgsz=320)
        return [[_face_key(f) for f in fr] for fr in res], fe.policy_state()

    base = run(bgr)
    fe._hdr = frames_hdr.HdrStager(fe._ctx, fe._h2d, fe._stage_threads, key="t_hdr16_src")
    got = run(hd)
    print("faces per frame", [len(fr) for fr in base[0]], "scratch reuses", fe._hdr.reuses)
    assert got == base
    assert fe._hdr.reuses == N - 2
    srcs = [k for k in fe._ctx._bufs if k.startswith("t_hdr16_src")]
    assert sorted(srcs) == ["t_hdr16_src0", "t_hdr16_src1"]
    assert all(fe._ctx._bufs[k].nbytes == H * W * 12 for k in srcs)
