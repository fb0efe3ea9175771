#!/usr/bin/env python3
"""Golden data of the HDR conversion, from the reference's OWN functions: _eotf_pq, _eotf_hlg, _oetf_bt709,
_hable_filmic and _python_tonemap_to_bgr8 are taken out of the reference's person_capture/video_io.py by AST
(the module itself does not import: av and imageio_ffmpeg are absent) and run with NumPy the way
FfmpegPipeReader.grab / retrieve call them (video_io.py:3005-3018, 3183-3192). Writes data only,
tests/golden/hdr_tonemap.npz:
  <case>               the reference's H x W x 3 BGR u8 output of every case of tests/hdr_cases.py (the inputs
                       are rebuilt from the cases' seeds, so only outputs are stored)
  small_raw / small_bgr / small_hw   one random 24 x 32 PQ frame at 200 nits, its planar G, B, R input floats
                       and output, for debugging
Before writing, every case is checked on the CPU against this package's NumPy backend under the caps of
hdr_cases (maximum difference 1 LSB, at most 5e-4 of the bytes). No reference source or bytecode is written
anywhere.

Run: python tools/gen_golden_hdr.py <root of the reference snapshot>
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import hdr_cases  # noqa: E402

NAMES = ("_eotf_pq", "_eotf_hlg", "_oetf_bt709", "_hable_filmic", "_python_tonemap_to_bgr8")


def reference_functions(ref_root: str) -> dict:
    """The five module-level functions of the reference's video_io.py, compiled from its AST in memory."""
    src = open(os.path.join(ref_root, "person_capture", "video_io.py"), encoding="utf-8").read()
    body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    if sorted(n.name for n in body) != sorted(NAMES):
        raise RuntimeError("the reference's video_io.py does not define " + ", ".join(NAMES))
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, "<video_io tone-map subset>", "exec"), ns)
    return {k: ns[k] for k in NAMES}


def reference_bgr(R: dict, rgb: np.ndarray, transfer: str, target_nits: float, peak_nits: float) -> np.ndarray:
    """What the reader does with one frame: rgb the (3, H, W) signal, restacked as grab restacks it."""
    hwc = np.stack((rgb[0], rgb[1], rgb[2]), axis=-1)
    with np.errstate(all="ignore"):
        lin = {"pq": R["_eotf_pq"], "hlg": R["_eotf_hlg"], "linear": lambda v: v}[transfer](hwc)
        return np.ascontiguousarray(R["_python_tonemap_to_bgr8"](lin, peak_nits=peak_nits, target_nits=target_nits))


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from person_capture_amd import frames_hdr
    R = reference_functions(sys.argv[1])
    out = {}
    for name in hdr_cases.CASE_NAMES:
        rgb = hdr_cases.case_rgb(name)
        tr, t, peak = hdr_cases.case_params(name)
        ref = reference_bgr(R, rgb, tr, t, peak)
        S = hdr_cases.SIDE
        assert ref.shape == (S, S, 3) and ref.dtype == np.uint8
        twin = frames_hdr.hdr_to_bgr(frames_hdr.HdrFrame(hdr_cases.planar_gbr(rgb), S, S, tr, t, peak))
        ok, mx, nbad = hdr_cases.within_cap(twin, ref)
        print(f"{name:22s} max diff {mx}  differing {nbad} of {ref.size} ({nbad / ref.size:.2e})")
        assert ok, name
        out[name] = ref
    H, W = 24, 32
    raw = np.random.default_rng(20261021).random(3 * H * W, dtype=np.float32)
    small = reference_bgr(R, np.stack([raw[2 * H * W:], raw[:H * W], raw[H * W:2 * H * W]]).reshape(3, H, W), "pq",
                          200.0, hdr_cases.PEAK_NITS)
    os.makedirs(os.path.dirname(hdr_cases.GOLDEN), exist_ok=True)
    np.savez_compressed(hdr_cases.GOLDEN, small_raw=raw, small_bgr=small, small_hw=np.array([H, W], np.int32), **out)
    size = os.path.getsize(hdr_cases.GOLDEN)
    print(len(out), "cases ->", hdr_cases.GOLDEN, size, "bytes")
    assert size < 900 * 1024


if __name__ == "__main__":
    main()
