"""f16x3 (split) ReID tower on the GPU, DESIGN.md §3.9.

* preprocessing: pc_clip_prep(PC_PREC_F16X3) writes the centred patch matrix twice per row,
  exactly Pillow's u8 pixels minus 127.5.
* split LayerNorm and split attention (pc_ops.hip SP forms) at op level against the
  device-semantics emulator, within the project's f16x3 bound (1e-5 of max|ref|).
* the tower (ViT-L/14 at reduced depth) and ReIDEmbedder (full depth) with
  PERSON_CAPTURE_AMD_REID_PRECISION=f16x3: unit embeddings within 1e-4 of the oracle.
* programs that mix plain and split tensors on LayerNorm / attention, and a 1216-wide CLIP
  input that is not flagged centred, are refused with PC_ERR_FORMAT before any launch.
"""
import ctypes as C

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
from test_clip_x3_cpu import centred_patch_matrix
from test_gpu_reid import CROPS

pytestmark = pytest.mark.gpu

PC_ERR_FORMAT = 4
TOL_X3 = 1e-5     # of max|ref|: the project's f16x3 bound (tests/test_gpu_bench_config.py, C2 f16x3)


def _crop(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_clip_prep_x3_centred_exact(gpu_ctx):
    crops = [_crop(i, h, w) for i, (h, w) in enumerate(CROPS)]
    bufs = [gpu_ctx.upload(c) for c in crops]
    arr = (CropDesc * len(crops))()
    for i, (c, b) in enumerate(zip(crops, bufs)):
        arr[i].d_src, arr[i].H, arr[i].W, arr[i].row_stride = b.ptr, c.shape[0], c.shape[1], c.strides[0]
    out = gpu_ctx.alloc(len(crops) * 257 * 1216 * 2)
    check(gpu_ctx.lib.pc_clip_prep(gpu_ctx.handle, PC_PREC_F16X3, arr, len(crops), out.ptr), gpu_ctx.handle, "clip_prep")
    got = gpu_ctx.download(out.ptr, (len(crops), 257, 1216), np.float16).astype(np.float32)
    for i, c in enumerate(crops):
        ref = centred_patch_matrix(nt.clip_preprocess_pil(c))[0]       # Pillow's u8 - 127.5, twice
        assert np.array_equal(got[i], ref), i
        for half in (got[i, :, :608], got[i, :, 608:]):
            assert not half[0].any() and not half[:, 588:].any()
            assert np.abs(half[1:, :588]).min() >= 0.5                 # every pixel written (x - 127.5 != 0)


# ---- op level: split LayerNorm / attention against the emulator -------------------------------
CIN = 64


def _lin(P, out, x, W, b):
    """1x1 conv over the token axis, W [cout][cin] (models_clip._lin without act / residual)."""
    cout, cin = W.shape
    cp = P.dims(x)[2]
    wp = np.zeros((pg.cpad(cout), cp), np.float32)
    wp[:cout, :cin] = W
    bias = np.zeros(pg.cpad(cout), np.float64)
    bias[:cout] = b
    P.conv(out, [(x, 1, 1, 1, 0, cin)], wp, cout, bias=bias)


def _run_vs_emulator(gpu_ctx, P, x):
    """x [N][1][T][CIN], exact in f16. Returns (device, emulator) outputs [N][T][C]."""
    N = x.shape[0]
    net = Net(gpu_ctx, P.serialize(), precision=PC_PREC_F16, max_batch=N)
    d = gpu_ctx.upload(x.astype(np.float16))
    net.run(d.ptr, N)
    got = net.read_output(0, N)[:, 0]
    (o,) = run_program(P, x)
    ref = o[:, :, 0].permute(0, 2, 1).numpy()
    net.close()
    return got, ref


# C: 128 a partial vector iteration (16 of 64 lanes), 1024 ViT-L's width, 100 rows that are no
# whole 16-byte vectors (the scalar `rows` form, with zero padding up to 128)
@pytest.mark.parametrize("Cw", [128, 1024, 100])
def test_split_layernorm_vs_emulator(gpu_ctx, Cw):
    N, T = 3, 257                      # M = 771 tokens: the last workgroup of 4 holds 3
    rng = np.random.default_rng(100 + Cw)
    P = pg.Program(split=True)
    x_in = P.input_tensor(1, T, CIN)
    e = P.act(1, T, pg.cpad(Cw))
    _lin(P, e, x_in, _f16(rng.standard_normal((Cw, CIN)) * CIN ** -0.5), rng.standard_normal(Cw) * 0.1)
    y = P.act(1, T, pg.cpad(Cw))
    P.layernorm(y, e, rng.uniform(0.8, 1.2, Cw).astype(np.float32), (rng.standard_normal(Cw) * 0.05).astype(np.float32),
                1e-5, add=rng.standard_normal((T, Cw)) * 0.3)
    o = P.act(1, T, 32, is_f32=1)
    _lin(P, o, y, rng.standard_normal((32, Cw)) * Cw ** -0.5, np.zeros(32))
    P.outputs = [o]
    assert P.tsplit[e] and P.tsplit[y]
    got, ref = _run_vs_emulator(gpu_ctx, P, _f16(rng.standard_normal((N, 1, T, CIN))))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"split layernorm C={Cw}: max-abs / max|ref| {err:.2e}")
    assert err <= TOL_X3


# T: 257 = 4 full query blocks + one query, per-wave key ranges of 65 (partial 16-key chunks);
# 50 = one partial block, key ranges 13, 13, 13, 11
@pytest.mark.parametrize("T", [257, 50])
def test_split_attention_vs_emulator(gpu_ctx, T):
    N, heads, d = 2, 2, 64
    E = heads * d
    rng = np.random.default_rng(200 + T)
    P = pg.Program(split=True)
    x_in = P.input_tensor(1, T, CIN)
    qkv = P.act(1, T, 3 * E)
    _lin(P, qkv, x_in, _f16(rng.standard_normal((3 * E, CIN)) * CIN ** -0.5), rng.standard_normal(3 * E) * 0.1)
    a = P.act(1, T, E)
    P.attention(a, qkv, heads, d)
    o = P.act(1, T, 32, is_f32=1)
    _lin(P, o, a, rng.standard_normal((32, E)) * E ** -0.5, np.zeros(32))
    P.outputs = [o]
    got, ref = _run_vs_emulator(gpu_ctx, P, _f16(rng.standard_normal((N, 1, T, CIN))))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"split attention T={T}: max-abs / max|ref| {err:.2e}")
    assert err <= TOL_X3


# ---- tower ----------------------------------------------------------------------------------
def _ref_embed(p, name, crops):
    x = torch.stack([nt.clip_preprocess_pil(c) for c in crops])
    e = nt.clip_vit_forward(p, name, x)
    return torch.nn.functional.normalize(e, dim=1).numpy()


def test_clip_tower_x3_parity(gpu_ctx):
    name = "ViT-L-14-d2"
    p = clip_weights(name, 0)
    # the crops are views into one uploaded frame: row_stride > W * 3
    frame = _crop(30, 1100, 1300)
    spots = [(5, 7), (320, 200), (400, 500), (11, 890)]
    views = [frame[y:y + h, x:x + w] for (y, x), (h, w) in zip(spots, CROPS[:4])]
    dframe = gpu_ctx.upload(frame)
    descs = [(dframe.ptr + y * frame.strides[0] + x * 3, h, w, frame.strides[0]) for (y, x), (h, w) in zip(spots, CROPS[:4])]
    assert all(rs > w * 3 for (_, _, w, rs) in descs)
    ref = _ref_embed(p, name, views)
    d = gpu_ctx.alloc(4 * 768 * 4)

    def embed(eng, dd):
        eng.embed_device(dd, d.ptr)
        return gpu_ctx.download(d.ptr, (len(dd), 768), np.float32)

    x3 = ClipEngine(gpu_ctx, p, name, precision=PC_PREC_F16X3, max_batch=4)
    assert x3.precision == PC_PREC_F16X3 and x3.net.precision == PC_PREC_F16
    got = embed(x3, descs)
    f32 = embed(ClipEngine(gpu_ctx, p, name, precision=PC_PREC_F32, max_batch=4), descs)
    print(f"x3 {name}: max-abs vs oracle {np.abs(got - ref).max():.2e}, vs device f32 {np.abs(got - f32).max():.2e} "
          f"(device f32 vs oracle {np.abs(f32 - ref).max():.2e})")
    assert np.abs(got - ref).max() < 1e-4
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    one = embed(x3, descs[2:3])
    print(f"x3 {name}: batch of 1 vs in a batch of 4 {np.abs(one[0] - got[2]).max():.2e}")
    assert np.abs(one[0] - got[2]).max() < 1e-5


def test_reid_embedder_vit_l14_x3(gpu_ctx, monkeypatch):
    monkeypatch.setenv("PERSON_CAPTURE_AMD_REID_PRECISION", "f16x3")
    reid = ReIDEmbedder(device="cuda:0")
    assert reid._engine.precision == PC_PREC_F16X3 and reid.dim == 768
    crops = [_crop(20 + i, h, w) for i, (h, w) in enumerate(CROPS[:2])]
    out = reid.extract([crops[0], None, np.zeros((0, 5, 3), np.uint8), crops[1]])
    assert len(out) == 2 and all(f.dtype == np.float32 and f.shape == (768,) for f in out)
    ref = _ref_embed(clip_weights("ViT-L-14", 0), "ViT-L-14", crops)
    err = max(float(np.abs(a - b).max()) for a, b in zip(out, ref))
    print(f"x3 ViT-L-14 (24 layers): max-abs vs oracle {err:.2e}")
    assert err < 1e-4
    assert reid.extract([]) == [] and reid.extract([None]) == []


# ---- rejections (pc_net_create / pc_clip_embed return before any launch) ---------------------
def _create_rc(gpu_ctx, P):
    prog = P.serialize()
    buf = C.create_string_buffer(prog, len(prog))
    h = C.c_void_p()
    rc = gpu_ctx.lib.pc_net_create(gpu_ctx.handle, buf, len(prog), PC_PREC_F16, 1, C.byref(h))
    if rc == 0:
        gpu_ctx.lib.pc_net_destroy(h)
    return rc


def _make_plain(P, t):
    """Turn split activation t of a split program into a plain f16 one of the same logical width."""
    P.tsplit[t] = 0
    P.tensors[t][3] //= 2
    P.tensors[t][4] //= 2
    P.vbufs[P.tensors[t][0]][0] //= 2


@pytest.mark.parametrize("op", ["layernorm", "attention"])
@pytest.mark.parametrize("plain", ["in", "out"])
def test_mixed_plain_split_rejected(gpu_ctx, op, plain):
    T, E = 50, 128
    rng = np.random.default_rng(7)
    P = pg.Program(split=True)
    x_in = P.input_tensor(1, T, CIN)
    cin = E if op == "layernorm" else 3 * E
    a = P.act(1, T, cin)
    _lin(P, a, x_in, _f16(rng.standard_normal((cin, CIN)) * 0.1), np.zeros(cin))
    b = P.act(1, T, E)
    if op == "layernorm":
        P.layernorm(b, a, np.ones(E, np.float32), np.zeros(E, np.float32))
    else:
        P.attention(b, a, 2, 64)
    o = P.act(1, T, 32, is_f32=1)
    _lin(P, o, b, rng.standard_normal((32, E)) * 0.1, np.zeros(32))
    P.outputs = [o]
    assert _create_rc(gpu_ctx, P) == 0            # both split: accepted
    _make_plain(P, a if plain == "in" else b)
    if plain == "out":                            # the last conv now reads a plain tensor: plain columns
        P.ops[-1][13] = P.arr(np.zeros((32, E), np.float32))
        P.ops[-1][15] = E
    assert _create_rc(gpu_ctx, P) == PC_ERR_FORMAT


def test_clip_embed_rejects_uncentred_1216(gpu_ctx):
    p = mc.synth_clip_vit("ViT-tiny-14", seed=1)
    P = mc.compile_clip_vit(p, "ViT-tiny-14", split=True)
    P.input_centered = False
    net = Net(gpu_ctx, P.serialize(), precision=PC_PREC_F16, max_batch=1)
    crop = _crop(1, 64, 64)
    dc = gpu_ctx.upload(crop)
    arr = (CropDesc * 1)()
    arr[0].d_src, arr[0].H, arr[0].W, arr[0].row_stride = dc.ptr, 64, 64, crop.strides[0]
    out = gpu_ctx.alloc(64 * 4)
    assert gpu_ctx.lib.pc_clip_embed(net.handle, arr, 1, C.c_void_p(out.ptr)) == PC_ERR_FORMAT
    net.close()
