"""CPU checks of the OpenCLIP ViT family: the towers with 16- and 32-pixel
patches and with head dim 80 compile into programs that match the literal oracle forward through
the device-semantics emulator (plain and f16x3 split), the FLOP count of the real towers is the
closed form, the towers out of scope are refused, and the ViT-tiny-14 program is byte for byte
what it was before the family was added."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import nets_torch as nt
from person_capture_amd import models_clip as mc
from person_capture_amd.program import cpad
from program_emulator import run_program

TINY = ["ViT-tiny-16", "ViT-tiny-32", "ViT-tiny-h80"]
IMGS = [(300, 180), (224, 224)]


def _inputs(name):
    c = mc.clip_cfg(name)
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in IMGS]
    return c, [nt.clip_preprocess_pil(im, c["image"]) for im in imgs]


def _centred(t, patch, K, kp):
    """The x3 device input of one preprocessed image (tests/test_clip_x3_cpu.centred_patch_matrix
    at any geometry): the u8 pixels minus 127.5 in patch-matrix order, written twice."""
    mean = np.array(mc.CLIP_MEAN, np.float64).reshape(3, 1, 1)
    std = np.array(mc.CLIP_STD, np.float64).reshape(3, 1, 1)
    u8 = np.rint((t.numpy().astype(np.float64) * std + mean) * 255.0)
    assert u8.min() >= 0 and u8.max() <= 255
    half = nt.clip_patch_matrix(torch.from_numpy((u8 - 127.5).astype(np.float32)), patch, kp)
    half[0, 0, :] = 0.0
    half[0, :, K:] = 0.0
    return np.concatenate([half, half], axis=2)


@pytest.mark.parametrize("name", TINY)
def test_family_program_matches_oracle(name):
    """1e-4 of max|ref|: the bound of tests/test_clip_cpu.py for ViT-tiny-14."""
    c, xs = _inputs(name)
    p = mc.synth_clip_vit(name, seed=1)
    ref = nt.clip_vit_forward(p, name, torch.stack(xs)).numpy()
    K = 3 * c["patch"] ** 2
    T = (c["image"] // c["patch"]) ** 2 + 1
    P = mc.compile_clip_vit(p, name)
    assert P.tensors[P.input][1:4] == [1, T, cpad(K)]
    x = np.concatenate([nt.clip_patch_matrix(t, c["patch"], cpad(K))[:, None] for t in xs], axis=0)
    (o,) = run_program(P, x)
    got = o[:, :, 0, 0].numpy()
    assert got.shape == ref.shape == (len(xs), c["out"])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name} emulator vs oracle: rel max-abs {err:.2e}")
    assert err < 1e-4


@pytest.mark.parametrize("name", TINY)
def test_family_x3_program_matches_oracle(name):
    """2e-5 of max|ref|: the bound of tests/test_clip_x3_cpu.py for ViT-tiny-14."""
    c, xs = _inputs(name)
    p = mc.synth_clip_vit(name, seed=1)
    ref = nt.clip_vit_forward(p, name, torch.stack(xs)).numpy()
    K = 3 * c["patch"] ** 2
    P = mc.compile_clip_vit(p, name, split=True)
    x = np.concatenate([_centred(t, c["patch"], K, cpad(K))[:, None] for t in xs], axis=0)
    assert P.tensors[P.input][1:4] == [1, x.shape[2], 2 * cpad(K)] and P.input_centered
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)           # exact in f16
    (o,) = run_program(P, x)
    got = o[:, :, 0, 0].numpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"x3 {name} emulator vs oracle: rel max-abs {err:.2e}")
    assert err < 2e-5


class _Zeros(dict):
    """Zero parameters of the right shapes, one shared array per shape (no synth: ViT-H/14 has
    0.6 G parameters)."""

    def __init__(self, name):
        super().__init__()
        c = mc.clip_cfg(name)
        self.c, self.cache = c, {}

    def __missing__(self, key):
        c, w = self.c, self.c["width"]
        tail = key.rsplit(".", 2)[-2:]
        if key == "visual.conv1.weight":
            shape = (w, 3, c["patch"], c["patch"])
        elif key == "visual.positional_embedding":
            shape = ((c["image"] // c["patch"]) ** 2 + 1, w)
        elif key == "visual.proj":
            shape = (w, c["out"])
        elif key.endswith("in_proj_weight"):
            shape = (3 * w, w)
        elif key.endswith("in_proj_bias"):
            shape = (3 * w,)
        elif tail == ["out_proj", "weight"]:
            shape = (w, w)
        elif tail == ["c_fc", "weight"]:
            shape = (c["mlp"], w)
        elif tail == ["c_fc", "bias"]:
            shape = (c["mlp"],)
        elif tail == ["c_proj", "weight"]:
            shape = (w, c["mlp"])
        else:                       # class embedding, LayerNorm weights / biases, the other biases
            shape = (w,)
        if shape not in self.cache:
            self.cache[shape] = np.zeros(shape, np.float32)
        return self.cache[shape]


@pytest.mark.parametrize("name", ["ViT-B-16", "ViT-H-14"])
def test_family_flops_closed_form(name):
    c = mc.clip_cfg(name)
    w, L = c["width"], c["layers"]
    T = (c["image"] // c["patch"]) ** 2 + 1
    K = 3 * c["patch"] ** 2
    per_layer = 2 * T * w * 3 * w + 4 * T * T * w + 2 * T * w * w + 4 * T * w * c["mlp"]
    total = 2 * T * K * w + L * per_layer + 2 * w * c["out"]
    P = mc.compile_clip_vit(_Zeros(name), name)
    assert P.flops_per_image == total


@pytest.mark.parametrize("name", ["ViT-g-14", "ViT-bigG-14", "RN50x64", "ViT-B-32-quickgelu"])
def test_out_of_scope_towers_refused(name):
    with pytest.raises(RuntimeError):
        mc.clip_cfg(name)


def test_family_table():
    want = {"ViT-B-32": (768, 12, 12, 3072, 512, 32, 224), "ViT-B-16": (768, 12, 12, 3072, 512, 16, 224),
            "ViT-L-14": (1024, 24, 16, 4096, 768, 14, 224), "ViT-L-14-336": (1024, 24, 16, 4096, 768, 14, 336),
            "ViT-H-14": (1280, 32, 16, 5120, 1024, 14, 224)}
    for name, row in want.items():
        c = mc.clip_cfg(name)
        assert tuple(c[k] for k in ("width", "layers", "heads", "mlp", "out", "patch", "image")) == row
        d2 = mc.clip_cfg(name + "-d2")
        assert d2.pop("layers") == 2 and all(d2[k] == c[k] for k in d2)
    assert mc.clip_cfg("ViT-tiny-h80")["width"] // mc.clip_cfg("ViT-tiny-h80")["heads"] == 80


# sha256 of compile_clip_vit(synth_clip_vit("ViT-tiny-14", seed=1), "ViT-tiny-14").serialize(), plain and
# split, computed on the commit before the family was added: the existing programs did not change
TINY14_SHA = {False: "94c773efb95b4bbaa9e08e314d80811feec3d320a830a9c4ba4b72229cec223c",
              True: "0d6c3245e958f1cc4f52501ce58308b5d91e8e43774f5c4236835fd7102e2e8e"}


@pytest.mark.parametrize("split", [False, True])
def test_tiny14_program_bytes_unchanged(split):
    p = mc.synth_clip_vit("ViT-tiny-14", seed=1)
    assert hashlib.sha256(mc.compile_clip_vit(p, "ViT-tiny-14", split=split).serialize()).hexdigest() == TINY14_SHA[split]
