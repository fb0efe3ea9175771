"""CPU checks of the f16x3 (split) ReID tower, DESIGN.md §3.9: the split compile of the
OpenCLIP ViT through the device-semantics emulator (hi/lo f16 storage, [hi, lo, hi] K walk)
against the literal oracle forward, the structure of the split program, and the words of
PERSON_CAPTURE_AMD_REID_PRECISION."""
import struct

import numpy as np
import pytest
import torch

from oracle import nets_torch as nt
from person_capture_amd import models_clip as mc
from person_capture_amd import reid_embedder as re_
from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F16X3, PC_PREC_F32
from program_emulator import run_program

NAME = "ViT-tiny-14"


@pytest.fixture(scope="module")
def tiny():
    return mc.synth_clip_vit(NAME, seed=1)


def centred_patch_matrix(t: torch.Tensor) -> np.ndarray:
    """The x3 device input of one preprocessed image: the u8 pixels (the exact inverse of
    ToTensor + Normalize) minus 127.5 in patch-matrix order, written twice -> [1][257][1216]."""
    mean = np.array(mc.CLIP_MEAN, np.float64).reshape(3, 1, 1)
    std = np.array(mc.CLIP_STD, np.float64).reshape(3, 1, 1)
    u8 = np.rint((t.numpy().astype(np.float64) * std + mean) * 255.0)
    assert u8.min() >= 0 and u8.max() <= 255
    half = nt.clip_patch_matrix(torch.from_numpy((u8 - 127.5).astype(np.float32)))   # [1][257][608]
    half[0, 0, :] = 0.0
    half[0, :, 588:] = 0.0
    return np.concatenate([half, half], axis=2)


def test_clip_x3_program_matches_oracle(tiny):
    """2e-5 of max|ref|: 5x the 3.6e-6 the centred form measures, below the 4.7e-5 of a raw
    0..255 input (cancellation in the patch embedding) and of a plain-f16 patch weight."""
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((300, 180), (224, 224))]
    xs = [nt.clip_preprocess_pil(im) for im in imgs]
    ref = nt.clip_vit_forward(tiny, NAME, torch.stack(xs)).numpy()
    P = mc.compile_clip_vit(tiny, NAME, split=True)
    x = np.concatenate([centred_patch_matrix(t)[:, None] for t in xs], axis=0)   # [N][1][257][1216]
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)           # exact in f16
    (o,) = run_program(P, x)
    got = o[:, :, 0, 0].numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"x3 {NAME} emulator vs oracle: rel max-abs {err:.2e}")
    assert err < 2e-5


def test_clip_x3_structure(tiny):
    P = mc.compile_clip_vit(tiny, NAME, split=True)
    assert P.tensors[P.input][1:4] == [1, 257, 1216] and P.tsplit[P.input] == 0 and P.input_centered
    words = struct.unpack_from("<8i", P.serialize())
    nbuf, inp = words[2], words[7]
    tw = struct.unpack_from("<8i", P.serialize(), (8 + 4 * nbuf + 8 * inp) * 4)
    assert tw[3] == 1216 and tw[7] == 2            # not split (bit 0), centred (bit 1)
    for i, (t, sp) in enumerate(zip(P.tensors, P.tsplit)):
        if i != P.input and not t[6]:
            assert sp == 1, i
    (out,) = P.outputs
    assert P.tensors[out][6] == 1 and P.tsplit[out] == 0


def test_clip_plain_compile_unchanged(tiny):
    a = mc.compile_clip_vit(tiny, NAME).serialize()
    assert a == mc.compile_clip_vit(tiny, NAME).serialize()
    assert a == mc.compile_clip_vit(tiny, NAME, split=False).serialize()
    P = mc.compile_clip_vit(tiny, NAME)
    assert P.tensors[P.input][1:4] == [1, 257, 608] and not P.input_centered and not any(P.tsplit)


@pytest.mark.parametrize("word,want", [("f16x3", PC_PREC_F16X3), ("X3", PC_PREC_F16X3), ("split", PC_PREC_F16X3),
                                       (None, PC_PREC_F32), ("f16", PC_PREC_F16), ("f32", PC_PREC_F32)])
def test_reid_precision_words(monkeypatch, word, want):
    if word is None:
        monkeypatch.delenv("PERSON_CAPTURE_AMD_REID_PRECISION", raising=False)
    else:
        monkeypatch.setenv("PERSON_CAPTURE_AMD_REID_PRECISION", word)
    assert re_._precision() == want
