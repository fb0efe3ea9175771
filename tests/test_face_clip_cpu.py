"""Host side of the OpenCLIP face mode (no GPU): the constructor still ends in RuntimeError where
there is no device, and the native path choice of pc_face_chips (pc_face_chip_plan) is
imageops.resize_plan's for the rectangle shapes tests/test_gpu_face_chips.py runs on the device."""
import pytest

from person_capture_amd import face_embedder as fe_mod
from person_capture_amd import imageops

SHAPES = [(224, 224), (336, 224), (224, 112), (448, 560), (150, 130), (112, 300), (1080, 700), (200, 90), (90, 200),
          (113, 40), (7, 113), (60, 50), (111, 112), (112, 112), (1, 1), (2, 3)]


def test_cpu_context_raises():
    with pytest.raises(RuntimeError):
        fe_mod.FaceEmbedder(ctx="cpu", yolo_model="scrfd_10g_bnkps", use_arcface=False)
    with pytest.raises(RuntimeError, match="YOLOv8-face"):
        fe_mod.FaceEmbedder(ctx="cpu", yolo_model="yolov8l-face.pt", use_arcface=False)
    with pytest.raises(RuntimeError):
        fe_mod.FaceEmbedder(ctx="cpu", yolo_model="scrfd_10g_bnkps", use_arcface=False, clip_model_name="RN50x64")


@pytest.mark.parametrize("H,W", SHAPES + [(16384, 16384), (1, 16384), (16384, 1), (113, 113), (223, 224), (112, 113)])
def test_chip_plan_is_resize_plan(H, W):
    want = imageops.resize_plan(H, W, (112, 112), area=max(H, W) > 112)
    got = imageops.chip_plan(H, W)
    assert got["kind"] == want["kind"]
    if want["kind"] == "area_fast":
        assert (got["isx"], got["isy"]) == (want["isx"], want["isy"])
    if want["kind"] == "linear":
        assert got["area_mode"] == want["area_mode"]


def test_chip_plan_covers_every_path():
    kinds = {}
    for H, W in SHAPES:
        p = imageops.chip_plan(H, W)
        k = p["kind"] + (str(p["area_mode"]) if p["kind"] == "linear" else "")
        kinds[k] = kinds.get(k, 0) + 1
    assert kinds == {"area_fast": 4, "area": 3, "linear1": 4, "linear0": 4, "copy": 1}


@pytest.mark.parametrize("H,W", [(0, 10), (10, 0), (16385, 10), (10, 16385), (-1, 5)])
def test_chip_plan_rejects_sizes_out_of_range(H, W):
    with pytest.raises(ValueError):
        imageops.chip_plan(H, W)
