"""Inputs and plain restatements shared by the curator tests (test_curate_cpu.py, test_gpu_curate.py).
Not a test module."""
import functools

import numpy as np

# (h, w) of the metric crops: tiny odd sizes, no resize at the 256 limit, a non-integer ratio just
# above it, the 2x2 fast path, an integer x ratio with a non-integer y ratio (and 24 x 16 blocks for
# the 32 x 32 plane), 3 x 3 blocks, mixed ratios, the identity 32 x 32 resize, and planes one pixel
# wide / one pixel high.
SHAPES = [(33, 47), (97, 61), (256, 256), (257, 129), (512, 384), (768, 512), (768, 768), (640, 427), (32, 32),
          (8200, 32), (32, 8200)]


# (h, w, seed) of the images whose hash bits are compared: every shape, at a seed for which no
# coefficient of the hashed block lies within 1e-3 of the median (the tests assert that first)
PHASH_IMAGES = [(33, 47, 0), (97, 61, 1), (256, 256, 1), (257, 129, 0), (512, 384, 0), (768, 512, 0), (768, 768, 1),
                (640, 427, 1), (32, 32, 0), (8200, 32, 0), (32, 8200, 1), (97, 61, 2), (512, 384, 1)]


@functools.lru_cache(maxsize=None)
def image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """A smooth scene plus noise (so the 32 x 32 plane keeps low-frequency content)."""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = rng.uniform(0.5, 3.0, 6)
    ph = rng.uniform(0, 6.28, 6)
    base = np.stack([128 + 60 * np.sin(f[c] * 6.28 * xx / w + ph[c]) * np.cos(f[c + 3] * 6.28 * yy / h + ph[c + 3])
                     for c in range(3)], axis=-1)
    img = base + rng.normal(0, 25, (h, w, 3))
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def greedy_mmr(q, k, S, alpha, literal=True):
    """The reference's greedy MMR, restated: every step scores each remaining item with
    alpha q_i - (1 - alpha) max(0, max over the picked j of S[i][j]) in double precision and takes
    the greatest score, the first of equals in ascending index order. literal=True recomputes the
    maximum over all picked columns at every step; literal=False keeps it as a running maximum (for
    the sizes at which the literal form is too slow; both are compared at n = 300)."""
    n = len(q)
    k = min(int(k), n)
    q64 = np.asarray(q, np.float32).astype(np.float64)
    picked = []
    left = np.ones(n, bool)
    run = np.zeros(n, np.float64)
    for _ in range(k):
        if S is None or not picked:
            red = np.zeros(n, np.float64)
        elif literal:
            red = np.maximum(0.0, np.asarray(S)[:, picked].max(axis=1).astype(np.float64))
        else:
            red = run
        s = alpha * q64 - (1.0 - alpha) * red
        best, best_s = None, None
        for i in np.flatnonzero(left) if n <= 70 else ():
            if best is None or s[i] > best_s:
                best, best_s = int(i), s[i]
        if n > 70:
            best = int(np.argmax(np.where(left, s, -np.inf)))   # the first maximum: the walk above, vectorised
        picked.append(best)
        left[best] = False
        if S is not None and not literal:
            run = np.maximum(run, np.asarray(S)[:, best].astype(np.float64))
    return picked


def unit_rows(n, dim, seed, zero_rows=(), dup=()):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, dim)).astype(np.float32)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    for a, b in dup:
        F[b] = F[a]
    for z in zero_rows:
        F[z] = 0
    return F


# (n, k, alpha, flavour) of the ranking cases
MMR_CASES = [(1, 1, 0.75, "plain"), (2, 2, 0.75, "plain"), (2, 1, 0.0, "plain"), (65, 65, 0.75, "plain"),
             (65, 20, 0.0, "plain"), (65, 65, 1.0, "dup"), (65, 65, 0.75, "dup"), (65, 30, 0.75, "neg"),
             (300, 300, 0.75, "zero"), (300, 77, 0.75, "dup"), (300, 300, 0.0, "neg"), (300, 300, 1.0, "plain")]


def mmr_inputs(n, flavour, seed=3):
    """(S f32 [n][n] symmetric, q f32 [n]) of a ranking case: 'dup' has duplicate rows with equal q
    (ties go to the lower index), 'neg' has mostly negative similarities (clamped to 0), 'zero' has
    zero rows (items the reference gives None)."""
    rng = np.random.default_rng(seed + n)
    dup = [(0, n - 1), (n // 2, n // 3)] if flavour == "dup" and n >= 4 else []
    zero = [1, n - 2] if flavour == "zero" and n >= 4 else []
    F = unit_rows(n, 24 if flavour != "neg" else 3, seed + n, zero, dup)
    S = (F.astype(np.float64) @ F.astype(np.float64).T).astype(np.float32)
    S = np.maximum(S, S.T)
    if flavour == "neg":
        S = (S - np.float32(0.9)).astype(np.float32)
    q = rng.uniform(0, 1, n).astype(np.float32)
    if flavour == "dup":
        q = np.round(q * 4) / np.float32(4)      # many equal qualities
        for a, b in dup:
            q[b] = q[a]
    return S, q.astype(np.float32)
