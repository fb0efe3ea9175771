#!/usr/bin/env python3
"""Golden data of the NV12 conversion, from the reference's OWN function: FfmpegPipeReader._nv12_to_bgr
is taken out of the reference's person_capture/video_io.py by AST (the module itself does not import:
av and imageio_ffmpeg are absent) and run with NumPy. Writes data only, tests/golden/nv12.npz:
  exhaustive_sha256   SHA-256 of the BGR bytes of the canonical exhaustive frame (tests/nv12_cases.py:
                      all 2^24 (Y, U, V) triples, 4096 x 4096), as uint8[32]
  small_raw / small_bgr / small_hw   one random 48 x 64 frame, its input bytes and output, for debugging
No reference source or bytecode is written anywhere.

Run: python tools/gen_golden_nv12.py <root of the reference snapshot>
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nv12_cases  # noqa: E402


def reference_nv12_to_bgr(ref_root: str):
    src = open(os.path.join(ref_root, "person_capture", "video_io.py"), encoding="utf-8").read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name == "FfmpegPipeReader":
            body = [it for it in node.body if isinstance(it, ast.FunctionDef) and it.name == "_nv12_to_bgr"]
            cls = ast.ClassDef(name="FfmpegPipeReader", bases=[], keywords=[], body=body, decorator_list=[])
            mod = ast.Module(body=[cls], type_ignores=[])
            ast.fix_missing_locations(mod)
            ns = {"np": np}
            exec(compile(mod, "<video_io.FfmpegPipeReader subset>", "exec"), ns)
            return ns["FfmpegPipeReader"]
    raise RuntimeError("FfmpegPipeReader not found in the reference's video_io.py")


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    R = reference_nv12_to_bgr(sys.argv[1])

    def run(raw: np.ndarray, H: int, W: int) -> np.ndarray:
        r = R()
        r._h, r._w = H, W
        return r._nv12_to_bgr(raw.tobytes())

    S = nv12_cases.EXHAUSTIVE_SIDE
    big = run(nv12_cases.exhaustive_nv12(), S, S)
    assert big.shape == (S, S, 3) and big.dtype == np.uint8
    sha = hashlib.sha256(big.tobytes()).digest()
    H, W = 48, 64
    raw = nv12_cases.random_nv12(np.random.default_rng(20261021), H, W)
    small = run(raw, H, W)
    os.makedirs(os.path.dirname(nv12_cases.GOLDEN), exist_ok=True)
    np.savez_compressed(nv12_cases.GOLDEN, exhaustive_sha256=np.frombuffer(sha, np.uint8), small_raw=raw,
                        small_bgr=small, small_hw=np.array([H, W], np.int32))
    print("exhaustive sha256", sha.hex(), "->", nv12_cases.GOLDEN, os.path.getsize(nv12_cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
