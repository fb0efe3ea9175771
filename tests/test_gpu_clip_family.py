"""The OpenCLIP ViT family on the GPU: B/32, B/16, L/14-336 and H/14 beside L/14.

* preprocessing at (224, 16), (224, 32) and (336, 14): pc_clip_prep_geom writes the patch matrix
  bit-exactly as Pillow + the oracle's patch order do, in the f32 and the centred f16x3 mode, and
  at (224, 14) byte for byte what pc_clip_prep writes.
* attention at op level against the device-semantics emulator, every net created under
  PERSON_CAPTURE_AMD_ATTN=stream so that the head-dim-64 shapes of at most 272 tokens run the new
  kernels too: the streaming f32-class kernels (f32 net, f16x3 split rows) within the project's 1e-5
  of max|ref|, the f16 matrix-core kernel within the error of mha_tokens<f16> plus the rounding of P
  to f16 (2^-10 max|v|).
* a head dim no kernel covers is refused with PC_ERR_FORMAT when the net is created.
* the towers at reduced depth (f32 and f16x3): unit embeddings within 1e-4 of the oracle; B/16 and
  B/32 (mha_tokens by default, like L/14) also under the switch.
* ReIDEmbedder(model_name="ViT-B-16" / "ViT-B-32") at full depth in f16, default dispatch and under
  the switch: cosine >= 0.99.
* PERSON_CAPTURE_AMD_ATTN=stream on ViT-L-14-d2 within 1e-4 of the oracle; without it the
  embeddings are bit for bit those of the commit before the family was added
  (tests/golden/clip_l14d2_before_family.npy).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import nets_torch as nt
from person_capture_amd import models_clip as mc
from person_capture_amd import program as pg
from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F16X3, PC_PREC_F32, CropDesc, check
from person_capture_amd.reid_embedder import ClipEngine, ReIDEmbedder, clip_weights
from person_capture_amd.runtime import Net
from program_emulator import run_program
from test_clip_family_cpu import _centred
from test_gpu_reid import CROPS

pytestmark = pytest.mark.gpu

PC_ERR_FORMAT = 4
TOL_X3 = 1e-5     # of max|ref|: the project's f16x3 bound (tests/test_gpu_reid_x3.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_l14d2_before_family.npy")


def _crop(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---- preprocessing ---------------------------------------------------------------------------
PREP_CROPS = [(300, 180), (97, 61), (336, 336), (1080, 400)]


def _prep_inputs(gpu_ctx):
    """The four crops plus one that is a view into a larger uploaded frame (row_stride > 3 W).
    Returns (host crops, CropDesc array, buffers to keep alive)."""
    crops = [_crop(40 + i, h, w) for i, (h, w) in enumerate(PREP_CROPS)]
    frame = _crop(45, 500, 640)
    view = frame[33:33 + 260, 101:101 + 333]
    bufs = [gpu_ctx.upload(c) for c in crops] + [gpu_ctx.upload(frame)]
    arr = (CropDesc * 5)()
    for i, c in enumerate(crops):
        arr[i].d_src, arr[i].H, arr[i].W, arr[i].row_stride = bufs[i].ptr, c.shape[0], c.shape[1], c.strides[0]
    arr[4].d_src, arr[4].H, arr[4].W, arr[4].row_stride = bufs[4].ptr + 33 * frame.strides[0] + 101 * 3, 260, 333, frame.strides[0]
    assert arr[4].row_stride > 3 * arr[4].W
    return crops + [view], arr, bufs


def _prep(gpu_ctx, prec, side, patch, arr, n):
    T, kp = (side // patch) ** 2 + 1, pg.cpad(3 * patch * patch)
    row, dt = (2 * kp, np.float16) if prec == PC_PREC_F16X3 else (kp, np.float32 if prec == PC_PREC_F32 else np.float16)
    out = gpu_ctx.alloc(n * T * row * np.dtype(dt).itemsize)
    check(gpu_ctx.lib.pc_clip_prep_geom(gpu_ctx.handle, prec, side, patch, arr, n, out.ptr), gpu_ctx.handle, "clip_prep_geom")
    return gpu_ctx.download(out.ptr, (n, T, row), dt)


@pytest.mark.parametrize("side,patch", [(224, 16), (224, 32), (336, 14)])
def test_prep_geom_bit_exact_vs_pillow(gpu_ctx, side, patch):
    crops, arr, _keep = _prep_inputs(gpu_ctx)
    K, kp = 3 * patch * patch, pg.cpad(3 * patch * patch)
    pil = [nt.clip_preprocess_pil(c, side) for c in crops]
    got = _prep(gpu_ctx, PC_PREC_F32, side, patch, arr, len(crops))
    for i, t in enumerate(pil):
        assert np.array_equal(got[i], nt.clip_patch_matrix(t, patch, kp)[0]), i
    cen = _prep(gpu_ctx, PC_PREC_F16X3, side, patch, arr, len(crops)).astype(np.float32)
    for i, t in enumerate(pil):
        assert np.array_equal(cen[i], _centred(t, patch, K, kp)[0]), i          # Pillow's u8 - 127.5, twice
        for half in (cen[i, :, :kp], cen[i, :, kp:]):
            assert not half[0].any() and not half[:, K:].any()
            assert np.abs(half[1:, :K]).min() >= 0.5                            # every pixel written


def test_prep_geom_224_14_equals_prep(gpu_ctx):
    crops, arr, _keep = _prep_inputs(gpu_ctx)
    n = len(crops)
    for prec, row, dt in ((PC_PREC_F32, 608, np.float32), (PC_PREC_F16, 608, np.float16), (PC_PREC_F16X3, 1216, np.float16)):
        out = gpu_ctx.alloc(n * 257 * row * np.dtype(dt).itemsize)
        check(gpu_ctx.lib.pc_clip_prep(gpu_ctx.handle, prec, arr, n, out.ptr), gpu_ctx.handle, "clip_prep")
        old = gpu_ctx.download(out.ptr, (n, 257, row), dt)
        new = _prep(gpu_ctx, prec, 224, 14, arr, n)
        assert old.tobytes() == new.tobytes(), prec


# ---- attention at op level ---------------------------------------------------------------------
CIN = 64
N_ATT, HEADS = 2, 2


def _lin(P, out, x, W, b):
    """1x1 conv over the token axis, W [cout][cin] (models_clip._lin without act / residual)."""
    cout, cin = W.shape
    cp = P.dims(x)[2]
    wp = np.zeros((pg.cpad(cout), cp), np.float32)
    wp[:cout, :cin] = W
    bias = np.zeros(pg.cpad(cout), np.float64)
    bias[:cout] = b
    P.conv(out, [(x, 1, 1, 1, 0, cin)], wp, cout, bias=bias)


def _attn_case(T, d, split):
    """qkv projection -> attention -> f32 projection. Returns (program, input, max|v| of the emulator's V)."""
    E = HEADS * d
    rng = np.random.default_rng(1000 * d + T)
    P = pg.Program(split=split)
    x_in = P.input_tensor(1, T, CIN)
    qkv = P.act(1, T, pg.cpad(3 * E))
    Wq, bq = _f16(rng.standard_normal((3 * E, CIN)) * CIN ** -0.5), rng.standard_normal(3 * E) * 0.1
    _lin(P, qkv, x_in, Wq, bq)
    a = P.act(1, T, pg.cpad(E))
    P.attention(a, qkv, HEADS, d)
    o = P.act(1, T, 32, is_f32=1)
    _lin(P, o, a, rng.standard_normal((32, E)) * E ** -0.5, np.zeros(32))
    P.outputs = [o]
    x = _f16(rng.standard_normal((N_ATT, 1, T, CIN)))
    v = x[:, 0].astype(np.float64) @ Wq[2 * E:].astype(np.float64).T + bq[2 * E:]
    return P, x, float(np.abs(v).max())


_REF = {}


def _emulator(T, d, split):
    """The emulator's output of a case, computed once per session and never modified."""
    key = (T, d, split)
    if key not in _REF:
        P, x, _ = _attn_case(T, d, split)
        (o,) = run_program(P, x)
        ref = o[:, :, 0].permute(0, 2, 1).numpy().copy()
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _device(gpu_ctx, T, d, split, precision):
    P, x, vmax = _attn_case(T, d, split)
    net = Net(gpu_ctx, P.serialize(), precision=precision, max_batch=N_ATT)
    dx = gpu_ctx.upload(x.astype(np.float32 if precision == PC_PREC_F32 else np.float16))
    net.run(dx.ptr, N_ATT)
    got = net.read_output(0, N_ATT)[:, 0]
    net.close()
    return got, vmax


# (577, 64): nine full key tiles and a one-key tile, nine full query blocks plus one query; (257, 80) and
# (50, 80): head dim 80 with a one-key last tile / one partial tile; (197, 64): ViT-B/16's token count.
# Head dim 64 with T <= 272 is mha_tokens' by default, so every case creates its net under
# PERSON_CAPTURE_AMD_ATTN=stream: (197, 64), and (257, 64) / (50, 64) (the shapes mha_tokens is tested at:
# a one-key last tile, one partial tile), then run the new kernels too.
ATT_SHAPES = [(577, 64), (257, 80), (50, 80), (197, 64)]
SWITCHED = [(257, 64), (50, 64)]


@pytest.mark.parametrize("T,d", ATT_SHAPES + SWITCHED)
@pytest.mark.parametrize("form", ["f32", "x3"])
def test_stream_attention_f32_class_vs_emulator(gpu_ctx, monkeypatch, T, d, form):
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", "stream")
    split = form == "x3"
    got, _ = _device(gpu_ctx, T, d, split, PC_PREC_F16 if split else PC_PREC_F32)
    ref = _emulator(T, d, split)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"stream attention {form} T={T} d={d}: max-abs / max|ref| {err:.2e}")
    assert err <= TOL_X3


def test_mfma_attention_f16_vs_emulator(gpu_ctx, monkeypatch):
    """Absolute error at the program's output. e0: mha_tokens<f16> (the default dispatch at head dim 64,
    T <= 272) against the emulator at (257, 64) and (50, 64). Rounding each P to f16 (relative 2^-11)
    moves a softmax-weighted mean of V by at most 2 * 2^-11 * max|v|, so the matrix-core kernel is held to
    e0 + 2^-10 * max|v|: the e0 of the same T where mha_tokens has one, the larger of the two elsewhere.
    The error is taken after the program's 32-channel projection (rows of norm about 1), as the op-level
    programs of this suite are built, so the derivation bounds the attention output and carries over to
    the measured figure only up to that projection; the figures printed sit near e0, far inside."""
    monkeypatch.delenv("PERSON_CAPTURE_AMD_ATTN", raising=False)
    e0 = {}
    for T in (257, 50):
        got, _ = _device(gpu_ctx, T, 64, False, PC_PREC_F16)
        e0[T] = float(np.abs(got - _emulator(T, 64, False)).max())
        print(f"mha_tokens<f16> T={T} d=64: max-abs {e0[T]:.3e}")
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", "stream")
    for T, d in SWITCHED + ATT_SHAPES:
        got, vmax = _device(gpu_ctx, T, d, False, PC_PREC_F16)
        e = float(np.abs(got - _emulator(T, d, False)).max())
        e_ref = e0[T] if (T, d) in SWITCHED else max(e0.values())
        bound = e_ref + 2.0 ** -10 * vmax
        print(f"mha_mfma T={T} d={d}: max-abs {e:.3e}, bound e0 {e_ref:.3e} + 2^-10 max|v| {vmax:.3f} = {bound:.3e}")
        assert e <= bound, (T, d)


def test_head_dim_48_refused_at_create(gpu_ctx):
    P, _, _ = _attn_case(50, 48, False)
    prog = P.serialize()
    for prec in (PC_PREC_F16, PC_PREC_F32):
        h = C.c_void_p()
        rc = gpu_ctx.lib.pc_net_create(gpu_ctx.handle, C.create_string_buffer(prog, len(prog)), len(prog), prec, 1, C.byref(h))
        if rc == 0:
            gpu_ctx.lib.pc_net_destroy(h)
        assert rc == PC_ERR_FORMAT


# ---- towers --------------------------------------------------------------------------------------
_TOWER_REF = {}


def _tower_crops():
    return [_crop(10 + i, h, w) for i, (h, w) in enumerate(CROPS[:4])]


def _ref_embed(name, crops):
    side = mc.clip_cfg(name)["image"]
    x = torch.stack([nt.clip_preprocess_pil(c, side) for c in crops])
    e = nt.clip_vit_forward(clip_weights(name, 0), name, x)
    return torch.nn.functional.normalize(e, dim=1).numpy()


def _tower_ref(name):
    if name not in _TOWER_REF:
        ref = _ref_embed(name, _tower_crops())
        ref.setflags(write=False)
        _TOWER_REF[name] = ref
    return _TOWER_REF[name]


def _embed(gpu_ctx, name, precision, crops, max_batch=4):
    eng = ClipEngine(gpu_ctx, clip_weights(name, 0), name, precision=precision, max_batch=max_batch)
    bufs = [gpu_ctx.upload(c) for c in crops]
    descs = [(b.ptr, c.shape[0], c.shape[1], c.strides[0]) for b, c in zip(bufs, crops)]
    d = gpu_ctx.alloc(len(crops) * eng.dim * 4)
    eng.embed_device(descs, d.ptr)
    got = gpu_ctx.download(d.ptr, (len(crops), eng.dim), np.float32)
    eng.embed_device(descs[2:3], d.ptr)
    one = gpu_ctx.download(d.ptr, (1, eng.dim), np.float32)
    eng.net.close()
    return got, one


# ViT-B/16 (197 tokens) and ViT-B/32 (50), head dim 64, run mha_tokens by default like ViT-L/14 and the
# streaming kernels under PERSON_CAPTURE_AMD_ATTN=stream; L/14-336 (577 tokens) and H/14 (head dim 80) always stream
TOWERS = [("ViT-B-16-d2", None), ("ViT-B-32-d2", None), ("ViT-L-14-336-d2", None), ("ViT-H-14-d2", None),
          ("ViT-B-16-d2", "stream"), ("ViT-B-32-d2", "stream")]


def _set_attn(monkeypatch, attn):
    if attn is None:
        monkeypatch.delenv("PERSON_CAPTURE_AMD_ATTN", raising=False)
    else:
        monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", attn)


@pytest.mark.parametrize("name,attn", TOWERS, ids=[n + ("-" + a if a else "") for n, a in TOWERS])
@pytest.mark.parametrize("prec", [PC_PREC_F32, PC_PREC_F16X3], ids=["f32", "x3"])
def test_family_tower_parity(gpu_ctx, monkeypatch, name, attn, prec):
    _set_attn(monkeypatch, attn)
    crops = _tower_crops()
    ref = _tower_ref(name)
    got, one = _embed(gpu_ctx, name, prec, crops)
    assert got.shape == ref.shape == (4, mc.clip_cfg(name)["out"])
    print(f"{name} prec {prec} attn {attn}: max-abs vs oracle {np.abs(got - ref).max():.2e}, "
          f"batch of 1 vs in a batch of 4 {np.abs(one[0] - got[2]).max():.2e}")
    assert np.abs(got - ref).max() < 1e-4
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    assert np.abs(one[0] - got[2]).max() < 1e-5


@pytest.mark.parametrize("name,attn", [("ViT-B-16", None), ("ViT-B-32", None), ("ViT-B-16", "stream"), ("ViT-B-32", "stream")],
                         ids=["ViT-B-16", "ViT-B-32", "ViT-B-16-stream", "ViT-B-32-stream"])
def test_reid_embedder_family_f16(gpu_ctx, monkeypatch, name, attn):
    """attn None: mha_tokens<f16> (the default at these towers' geometry); stream: the matrix-core kernel."""
    monkeypatch.setenv("PERSON_CAPTURE_AMD_REID_PRECISION", "f16")
    _set_attn(monkeypatch, attn)
    reid = ReIDEmbedder(device="cuda:0", model_name=name)
    assert reid.device == "cuda" and reid.dim == 512 and reid._engine.precision == PC_PREC_F16
    crops = [_crop(20 + i, h, w) for i, (h, w) in enumerate(CROPS[:2])]
    out = reid.extract([crops[0], None, np.zeros((0, 5, 3), np.uint8), crops[1]])
    assert len(out) == 2 and all(f.dtype == np.float32 and f.shape == (512,) for f in out)
    ref = _ref_embed(name, crops)
    for a, b in zip(out, ref):
        print(f"{name} f16 attn {attn}: cosine vs f32 oracle {float(np.dot(a, b)):.5f}")
        assert abs(np.linalg.norm(a) - 1.0) < 1e-4
        assert float(np.dot(a, b)) > 0.99
    assert reid.extract([]) == [] and reid.extract([None]) == []


# ---- the dispatch switch on the existing geometry ----------------------------------------------------
def test_attn_stream_switch_l14(gpu_ctx, monkeypatch):
    name = "ViT-L-14-d2"
    crops = _tower_crops()
    ref = _tower_ref(name)
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", "stream")
    got, _ = _embed(gpu_ctx, name, PC_PREC_F32, crops)
    print(f"{name} f32, PERSON_CAPTURE_AMD_ATTN=stream: max-abs vs oracle {np.abs(got - ref).max():.2e}")
    assert np.abs(got - ref).max() < 1e-4
    # unset: the dispatch, and every bit of the embeddings, of the commit before
    before = np.load(GOLDEN)    # [f32, f16, f16x3][4][768], written by that commit on an MI355X
    monkeypatch.delenv("PERSON_CAPTURE_AMD_ATTN")
    for i, prec in enumerate((PC_PREC_F32, PC_PREC_F16, PC_PREC_F16X3)):
        got, _ = _embed(gpu_ctx, name, prec, crops)
        assert got.tobytes() == before[i].tobytes(), prec
    monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", "default")      # any other word: the default too
    got, _ = _embed(gpu_ctx, name, PC_PREC_F16, crops)
    assert got.tobytes() == before[1].tobytes()
