"""Inputs shared by the HDR tests (test_hdr_cpu.py, test_gpu_hdr.py) and tools/gen_golden_hdr.py.

A case is one 256 x 256 frame (196 608 output bytes), rebuilt from its seed: the golden file holds the
reference's outputs only. The random classes draw 256 rows of 64 pixels and repeat each row four times
along x: 16 384 distinct random pixels a case, and an output the golden's deflate stores once."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdr_tonemap.npz")
SIDE = 256
PEAK_NITS = 1000.0   # what FfmpegPipeReader.retrieve passes (video_io.py:3187-3191)

# the caps of the twin / the device against the reference's recorded outputs: every differing byte differs
# by 1, and at most this share of a case's bytes differs (4 x the worst share measured, 24 of 196 608, to
# leave room for another NumPy build's powf)
MAX_LSB = 1
MAX_SHARE = 5e-4

# (name, input class, transfer, target_nits)
CASES = (
    [(f"{cls}_{tr}_{int(t)}", cls, tr, float(t)) for cls in ("boundary", "uniform") for tr in ("pq", "hlg", "linear")
     for t in (100, 203)]
    + [("code10_pq_200", "code10", "pq", 200.0), ("code10_hlg_400", "code10", "hlg", 400.0),
       ("limited_pq_400", "limited", "pq", 400.0), ("limited_hlg_200", "limited", "hlg", 200.0)]
)
CASE_NAMES = [c[0] for c in CASES]


def boundary_values() -> np.ndarray:
    """65 536 f32 samples: the specials (+-inf, -0.0, subnormal and tiny values, out-of-range values), every
    f32 within 2048 ulps of 0.5 and around 1, the decades from the smallest subnormal to 1 (where the linear
    transfer and the OETF's two branches live), and a ramp over the whole of [0, 1]."""
    one, half = np.float32(1.0), np.float32(0.5)
    special = np.array([np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1e-30, -1e-30, 1e-45, 1.5, 2.0, -0.25, -1.0, 3.0e38,
                        -3.0e38, 0.018, 0.0018, 1.0, 0.5, 0.75], np.float32)
    k = np.arange(-2048, 2049, dtype=np.float32)
    near_half = half + k * np.float32(2.0 ** -25)          # ulp(0.5-) = 2^-25
    near_one = one + np.arange(-4096, 513, dtype=np.float32) * np.float32(2.0 ** -24)
    decades = np.geomspace(1e-45, 1.0, 16384).astype(np.float32)
    rest = SIDE * SIDE - (special.size + near_half.size + near_one.size + decades.size)
    ramp = np.linspace(0.0, 1.0, rest, dtype=np.float64).astype(np.float32)
    v = np.concatenate([special, near_half, near_one, decades, ramp])
    assert v.size == SIDE * SIDE
    return v


def _tiled(rng_block: np.ndarray) -> np.ndarray:
    return np.tile(rng_block, (1, 1, 4))


def case_rgb(name: str) -> np.ndarray:
    """The (3, 256, 256) f32 R, G, B signal of a case."""
    _, cls, tr, _ = CASES[CASE_NAMES.index(name)]
    seed = 20261021 + CASE_NAMES.index(name)
    rng = np.random.default_rng(seed)
    n = SIDE * SIDE
    if cls == "boundary":
        v = boundary_values()
        i = np.arange(n)
        # top half grey (every value through all three channels at once), bottom half mixed
        g = np.where(i < n // 2, v, v[(i + n // 3) % n])
        b = np.where(i < n // 2, v, v[::-1])
        return np.stack([v, g, b]).reshape(3, SIDE, SIDE)
    if cls == "uniform":
        u = rng.random((3, SIDE, SIDE // 4), dtype=np.float32)
        if tr == "linear":   # linear light up to the peak (1000 nits), most of it in the curve's useful range
            u = (u * u) * (u * u) * np.float32(0.1)
        return _tiled(u)
    codes = rng.integers(0, 1024, (3, SIDE, SIDE // 4)).astype(np.float32)
    if cls == "code10":      # 10-bit full-range codes
        return _tiled(codes / np.float32(1023.0))
    if cls == "limited":     # 10-bit limited-range codes expanded: below 0 and above 1 at the ends
        return _tiled((codes - np.float32(64.0)) / np.float32(876.0))
    raise KeyError(cls)


def case_params(name: str):
    """(transfer, target_nits, peak_nits)."""
    _, _, tr, t = CASES[CASE_NAMES.index(name)]
    return tr, t, PEAK_NITS


def planar_gbr(rgb: np.ndarray) -> np.ndarray:
    """The pipe's bytes of a (3, H, W) R, G, B signal: planes G, B, R, as one flat f32 array."""
    return np.concatenate([rgb[1].reshape(-1), rgb[2].reshape(-1), rgb[0].reshape(-1)])


def within_cap(got: np.ndarray, ref: np.ndarray):
    """(ok, max |difference|, differing bytes) of two u8 arrays under MAX_LSB / MAX_SHARE."""
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    nbad = int(np.count_nonzero(d))
    mx = int(d.max()) if d.size else 0
    return (got.shape == ref.shape and mx <= MAX_LSB and nbad <= MAX_SHARE * ref.size), mx, nbad
