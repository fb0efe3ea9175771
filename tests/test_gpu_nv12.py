"""NV12 frames on the device (csrc/pc_nv12.hip, person_capture_amd/frames.py) against the NumPy backend,
which test_nv12_cpu.py pins to the reference's own FfmpegPipeReader._nv12_to_bgr (video_io.py:2888-2912).
Every comparison is ==."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import nv12_cases
from oracle import cv_ops
from person_capture_amd import face_embedder as fe_mod
from person_capture_amd import frames
from person_capture_amd._lib import PC_OK

pytestmark = pytest.mark.gpu
PC_ERR_ARG = 1


def _pad16(x):
    return (x + 15) // 16 * 16


class _Planes:
    """An NV12 frame laid out in one device buffer: base offset, plane strides."""

    def __init__(self, ctx, raw, H, W, ys, uvs, base):
        self.H, self.W, self.ys, self.uvs = H, W, ys, uvs
        self.uv_off = _pad16(base + H * ys) + base
        host = np.full(self.uv_off + (H // 2) * uvs + 16, 0x5A, np.uint8)
        for r in range(H):
            host[base + r * ys:base + r * ys + W] = raw[r * W:(r + 1) * W]
        for r in range(H // 2):
            o = self.uv_off + r * uvs
            host[o:o + W] = raw[(H + r) * W:(H + r + 1) * W]
        self.buf = ctx.upload(host)
        self.y_ptr, self.uv_ptr = self.buf.ptr + base, self.buf.ptr + self.uv_off
        self.frame = frames.Nv12Frame.on_device(self.y_ptr, self.uv_ptr, H, W, ys, uvs)


def _ref(raw, H, W):
    return frames.nv12_to_bgr(frames.Nv12Frame(raw, H, W))


def test_exhaustive_all_triples(gpu_ctx):
    """pc_nv12_to_bgr over all 2^24 (Y, U, V) triples equals the NumPy backend and hashes to the
    reference's output. This is the test a build with fused multiply-adds fails: 22 of the triples
    are at stake (their float sums round differently when the product is not rounded first)."""
    S = nv12_cases.EXHAUSTIVE_SIDE
    raw = nv12_cases.exhaustive_nv12()
    with np.load(nv12_cases.GOLDEN, allow_pickle=False) as g:
        sha = g["exhaustive_sha256"].tobytes()
    got = frames.nv12_to_bgr(frames.Nv12Frame(raw, S, S), gpu_ctx)
    assert got.shape == (S, S, 3) and got.dtype == np.uint8
    ref = _ref(raw, S, S)
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:8])
    assert hashlib.sha256(got.tobytes()).digest() == sha


_GEOM = [(2, 2), (2, 16), (16, 2), (6, 34), (10, 66), (270, 482), (1080, 1920)]


@pytest.fixture(scope="module")
def geom_frames():
    rng = np.random.default_rng(1212)
    raws = [nv12_cases.random_nv12(rng, H, W) for H, W in _GEOM]
    return raws, [_ref(r, H, W) for r, (H, W) in zip(raws, _GEOM)]


@pytest.mark.parametrize("layout", ["aligned", "offset"])
def test_mixed_sizes_one_launch(gpu_ctx, geom_frames, layout):
    """Seven frames from 2 x 2 to 1080 x 1920 in ONE pc_nv12_to_bgr: plane strides larger than W,
    dst_stride > 3 W with the row padding and 64 guard bytes behind every destination prefilled with
    0xA5 and required unchanged. 'aligned': every pointer and stride a multiple of 16 (16-byte path, byte
    path for the W % 16 tails); 'offset': planes 1 byte and destinations 3 bytes off a 16-byte boundary,
    odd strides (byte path). The last frame's planes (packed strides) end on the last byte of
    allocations of their own."""
    raws, refs = geom_frames
    off = layout == "offset"
    planes, jobs, dst_off, dst_strides = [], [], [], []
    total = 64
    for (H, W) in _GEOM:
        ds = _pad16(3 * W) + 16 + (5 if off else 0)
        total = _pad16(total) + (3 if off else 0)
        dst_off.append(total)
        dst_strides.append(ds)
        total += H * ds + 64
    dst = gpu_ctx.alloc(total + 64)
    gpu_ctx.memset(dst.ptr, 0xA5, total + 64)
    for k, ((H, W), raw) in enumerate(zip(_GEOM, raws)):
        if k == len(_GEOM) - 1:   # planes ending on the last byte of their allocations
            yb, uvb = gpu_ctx.upload(raw[:H * W].copy()), gpu_ctx.upload(raw[H * W:].copy())
            assert yb.nbytes == H * W and uvb.nbytes == H * W // 2
            planes.append((yb, uvb))
            jobs.append((yb.ptr, uvb.ptr, H, W, W, W, dst.ptr + dst_off[k], dst_strides[k]))
            continue
        ys, uvs = (_pad16(W) + 16, _pad16(W) + 32) if not off else (W + 3, W + 7)
        p = _Planes(gpu_ctx, raw, H, W, ys, uvs, 1 if off else 0)
        assert (p.y_ptr % 16, p.uv_ptr % 16) == ((1, 1) if off else (0, 0))
        planes.append(p)
        jobs.append((p.y_ptr, p.uv_ptr, H, W, ys, uvs, dst.ptr + dst_off[k], dst_strides[k]))
    frames.convert_on_device(gpu_ctx, jobs)
    out = gpu_ctx.download(dst.ptr, (total + 64,), np.uint8)
    mask = np.ones(total + 64, bool)   # bytes that must still be 0xA5
    for (H, W), ref, o, ds in zip(_GEOM, refs, dst_off, dst_strides):
        rows = np.lib.stride_tricks.as_strided(out[o:], (H, 3 * W), (ds, 1))
        assert np.array_equal(rows.reshape(H, W, 3), ref), (H, W)
        for r in range(H):
            mask[o + r * ds:o + r * ds + 3 * W] = False
    assert (out[mask] == 0xA5).all()


def test_argument_handling(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    H, W = 4, 32
    src = gpu_ctx.upload(np.zeros(W * H * 3 // 2, np.uint8))
    dst = gpu_ctx.alloc(2 * H * W * 3)
    gpu_ctx.memset(dst.ptr, 0xA5, 2 * H * W * 3)
    good = (src.ptr, src.ptr + H * W, H, W, W, W, dst.ptr, 3 * W)

    def call(jobs, n=None):
        return lib.pc_nv12_to_bgr(h, frames.nv12_descs(jobs), len(jobs) if n is None else n)

    assert lib.pc_nv12_to_bgr(h, None, 0) == PC_OK
    assert call([good], 0) == PC_OK
    assert call([good], -1) == PC_ERR_ARG
    assert lib.pc_nv12_to_bgr(h, None, 1) == PC_ERR_ARG

    def with_(**kw):
        names = ("y", "uv", "H", "W", "ys", "uvs", "dst", "ds")
        d = dict(zip(names, good))
        d.update(kw)
        return tuple(d[k] for k in names)

    bad = [with_(y=0), with_(uv=0), with_(dst=0), with_(H=3), with_(W=31), with_(H=0), with_(W=0), with_(H=16386),
           with_(W=16386), with_(ys=W - 1), with_(uvs=W - 2), with_(ds=3 * W - 1), with_(H=-2)]
    for b in bad:
        assert call([b]) == PC_ERR_ARG, b
        # nothing is staged or launched when a later frame of the batch is bad
        assert call([with_(dst=dst.ptr + H * W * 3), b]) == PC_ERR_ARG, b
    assert b"pc_nv12_to_bgr" in lib.pc_last_error(h)
    assert (gpu_ctx.download(dst.ptr, (2 * H * W * 3,), np.uint8) == 0xA5).all()
    assert call([good]) == PC_OK   # the context is still usable
    got = gpu_ctx.download(dst.ptr, (H, W, 3), np.uint8)
    assert np.array_equal(got, _ref(np.zeros(W * H * 3 // 2, np.uint8), H, W))
    # the fused downscales check their arguments the same way
    one = (C.c_void_p * 1)
    assert lib.pc_nv12_resize_area_fast_batch(h, one(src.ptr), one(src.ptr + H * W), one(dst.ptr), 1, H, W, W, W, 2, 2,
                                              H // 2 + 1, W // 2) == PC_ERR_ARG
    assert lib.pc_nv12_resize_area_fast_batch(h, one(src.ptr), one(0), one(dst.ptr), 1, H, W, W, W, 2, 2, H // 2,
                                              W // 2) == PC_ERR_ARG
    assert lib.pc_nv12_resize_area_fast_batch(h, one(src.ptr), one(src.ptr + H * W), one(dst.ptr), 1, H, W + 1, W + 1,
                                              W + 1, 2, 2, H // 2, W // 2) == PC_ERR_ARG


# (n, H, W, OH, OW, the cv::resize path)
_FUSED = [(1, 270, 480, 117, 208, "area"), (1, 96, 128, 48, 64, "area_fast"), (1, 90, 150, 30, 50, "area_fast"),
          (3, 540, 960, 234, 416, "area"), (1, 2160, 3840, 234, 416, "area")]


@pytest.fixture(scope="module")
def fused_refs():
    """Per shape: the frames' bytes and the oracle's INTER_AREA resize of the NumPy-converted frames."""
    from person_capture_amd import imageops
    out = {}
    for n, H, W, OH, OW, kind in _FUSED:
        assert imageops.resize_plan(H, W, (OW, OH), area=True)["kind"] == kind
        rng = np.random.default_rng(H * 31 + W)
        raws = [nv12_cases.random_nv12(rng, H, W) for _ in range(n)]
        out[(H, W)] = (raws, [cv_ops.resize(_ref(r, H, W), (OW, OH), 0, 0, cv_ops.INTER_AREA) for r in raws])
    return out


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("n,H,W,OH,OW,kind", _FUSED)
def test_fused_downscale(gpu_ctx, fused_refs, n, H, W, OH, OW, kind, layout):
    """pc_nv12_resize_area_batch / pc_nv12_resize_area_fast_batch equal pc_nv12_to_bgr followed by the BGR
    resize on the device, and the oracle's cv2.resize(INTER_AREA) of the NumPy-converted frame. 'offset':
    padded plane strides and bases 1 byte off a 16-byte boundary."""
    raws, refs = fused_refs[(H, W)]
    off = layout == "offset"
    ys, uvs = (W + 6, W + 10) if off else (W, W)
    planes = [_Planes(gpu_ctx, r, H, W, ys, uvs, 1 if off else 0) for r in raws]
    fused = fe_mod.dev_nv12_resize_batch(gpu_ctx, [p.frame for p in planes], [f"t_nv12_fused{i}" for i in range(n)],
                                         (OW, OH))
    got = [gpu_ctx.download(o.ptr, (OH, OW, 3), np.uint8) for o in fused]
    full = [gpu_ctx.alloc(H * W * 3) for _ in range(n)]
    frames.convert_on_device(gpu_ctx, [(p.y_ptr, p.uv_ptr, H, W, ys, uvs, b.ptr, 3 * W) for p, b in zip(planes, full)])
    two = fe_mod.dev_resize_batch(gpu_ctx, [fe_mod._DevImage(b.ptr, H, W, 3 * W) for b in full],
                                  [f"t_nv12_two{i}" for i in range(n)], (OW, OH))
    for g, t, ref in zip(got, two, refs):
        assert (t.H, t.W) == (OH, OW)
        assert np.array_equal(g, gpu_ctx.download(t.ptr, (OH, OW, 3), np.uint8))
        assert np.array_equal(g, ref)


# ---- facades ----
def _soft_nv12(seed, H, W):
    """A noise frame with moderate chroma, so that the converted frame is noise and not saturated."""
    rng = np.random.default_rng(seed)
    raw = nv12_cases.random_nv12(rng, H, W)
    raw[H * W:] = rng.integers(96, 160, H * W // 2, dtype=np.uint8)
    return frames.Nv12Frame(raw, H, W)


def _face_key(f):
    return (tuple(int(v) for v in f["bbox"]), f["feat"].tobytes(), float(f["quality"]))


def test_extract_batch_nv12_equals_bgr(gpu_ctx, monkeypatch):
    """FaceEmbedder.extract_batch over 3 frames given as Nv12Frame, as nv12_to_bgr arrays, and mixed:
    the same boxes, features, quality and policy state."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    nv = [_soft_nv12(70 + i, 360, 640) for i in range(3)]
    bgr = [frames.nv12_to_bgr(f) for f in nv]
    st0 = fe.policy_state()
    runs = []
    for batch in (bgr, nv, [nv[0], bgr[1], nv[2]]):
        fe.set_policy_state(st0)
        res = fe.extract_batch(batch, imgsz=320)
        runs.append(([[_face_key(f) for f in fr] for fr in res], fe.policy_state()))
    print("faces per frame", [len(fr) for fr in runs[0][0]])
    assert sum(len(fr) for fr in runs[0][0]) > 0
    assert runs[1] == runs[0] and runs[2] == runs[0]
    fe.set_policy_state(st0)
    one = fe.extract(nv[0], imgsz=320)
    assert [_face_key(f) for f in one] == runs[0][0][0]


def test_extract_batch_yolo_face_nv12_equals_bgr(gpu_ctx, monkeypatch):
    """The same on the YOLOv8-face backend (yolov8n-face): NV12, BGR and mixed entries give equal faces."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="yolov8n-face.pt", conf=0.05)
    assert fe.detector_backend == "yolo"
    nv = [_soft_nv12(75 + i, 360, 640) for i in range(3)]
    bgr = [frames.nv12_to_bgr(f) for f in nv]
    runs = [[[_face_key(f) for f in fr] for fr in fe.extract_batch(batch)]
            for batch in (bgr, nv, [bgr[0], nv[1], bgr[2]])]
    print("faces per frame", [len(fr) for fr in runs[0]])
    assert runs[1] == runs[0] and runs[2] == runs[0]
    assert [_face_key(f) for f in fe.extract(nv[2])] == runs[0][2]


def test_detect_batch_nv12_equals_bgr(gpu_ctx):
    from person_capture_amd.detectors import PersonDetector
    det = PersonDetector("yolov8n.pt", device="cuda")
    nv = [_soft_nv12(80 + i, 360, 640) for i in range(3)]
    bgr = [frames.nv12_to_bgr(f) for f in nv]
    a = det.detect_batch(bgr, conf=0.05)
    assert det.detect_batch(nv, conf=0.05) == a
    assert det.detect_batch([bgr[0], nv[1], bgr[2]], conf=0.05) == a
    assert det.detect(nv[1], conf=0.05) == a[1]
    print("persons per frame", [len(x) for x in a])


def test_prescan_nv12_equals_bgr(gpu_ctx, monkeypatch):
    """A PrescanRunner over 8 samples of 540 x 960 at prescan_max_width 416: NV12 samples, with the fused
    downscale off and on, give the BGR samples' records, spans, bank and final policy state."""
    from person_capture_amd.prescan import PrescanConfig, PrescanRunner
    monkeypatch.setenv("PERSON_CAPTURE_AMD_PRECISION", "f32")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ARCFACE", "iresnet50")
    fe = fe_mod.FaceEmbedder(ctx="cuda:0", yolo_model="scrfd_2.5g_bnkps", conf=0.5)
    H, W, N = 540, 960, 8
    nv = [_soft_nv12(90 + (i // 2), H, W) for i in range(N)]
    bgr = [frames.nv12_to_bgr(f) for f in nv]
    bank = np.random.default_rng(9).standard_normal((2, 512)).astype(np.float32)
    cfg = PrescanConfig(prescan_stride=1, prescan_max_width=416, prescan_fd9_skip=False, face_quality_min=0.0,
                        prescan_fd_enter=2.5, prescan_fd_exit=3.0, prescan_fd_add=2.5,
                        prescan_add_cooldown_samples=2)
    st0 = fe.policy_state()

    def run(src, fused):
        fe.set_policy_state(st0)
        r = PrescanRunner(fe, cfg, 4.0, N, ref_feat=bank, batch=8)
        r.nv12_fused = fused
        spans, b = r.run(lambda i: src[i])
        return spans, b.tobytes(), [tuple(vars(x).items()) for x in r.records], fe.policy_state()

    base = run(bgr, False)
    print("spans", base[0], "faces", [dict(x)["n_faces"] for x in base[2]])
    assert sum(dict(x)["n_faces"] for x in base[2]) > 0
    assert run(nv, False) == base
    assert run(nv, True) == base
