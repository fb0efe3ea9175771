"""Inputs shared by the NV12 tests (test_nv12_cpu.py, test_gpu_nv12.py) and tools/gen_golden_nv12.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nv12.npz")
EXHAUSTIVE_SIDE = 4096


def exhaustive_nv12() -> np.ndarray:
    """The canonical exhaustive frame, 4096 x 4096, as the W * H * 3 / 2 bytes of the pipe: chroma cell
    k = cy * 2048 + cx holds the (u, v) pair k % 65536 (u = pair >> 8, v = pair & 255), so every pair is in
    64 cells; the four Y samples of the cell that is a pair's repetition rep = k // 65536 are
    4 rep + {0, 1, 2, 3} (top left, top right, bottom left, bottom right). Every (Y, U, V) triple occurs
    exactly once."""
    S = EXHAUSTIVE_SIDE
    k = np.arange((S // 2) * (S // 2), dtype=np.int64).reshape(S // 2, S // 2)
    pair, rep = k % 65536, k // 65536
    y = np.empty((S, S), np.uint8)
    y[0::2, 0::2] = 4 * rep
    y[0::2, 1::2] = 4 * rep + 1
    y[1::2, 0::2] = 4 * rep + 2
    y[1::2, 1::2] = 4 * rep + 3
    uv = np.empty((S // 2, S), np.uint8)
    uv[:, 0::2] = pair >> 8
    uv[:, 1::2] = pair & 255
    return np.concatenate([y.reshape(-1), uv.reshape(-1)])


def random_nv12(rng, H: int, W: int) -> np.ndarray:
    return rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
