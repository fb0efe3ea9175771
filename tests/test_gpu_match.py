"""pc_embed_finalize, pc_l2_normalize and pc_bank_match (pc_embed.hip) against float64 NumPy
restatements of match.fd_min and x / max(||x||, eps): every dim the face modes use (64, 512 and the
OpenCLIP 768 / 1024: per = dim / 64 = 1, 8, 12, 16 floats per lane), query counts that leave a
partial 8-query workgroup, banks of fewer rows than waves, the idx output (first maximal row, exact
ties included), the eps clamp, ld > dim, an empty bank and the dim rejection.

Tolerances: first-order worst-case bounds of the kernels' own summation order, u = 2^-24 (the
unit roundoff of f32; division and sqrt are correctly rounded, each one more u).

* The squared norm: a lane sums per squares (one rounding per term with a fused multiply-add, two
  without, nested: at most per roundings on any term), six xor-shuffle levels add six more. All terms
  are positive, so its relative error is at most (per + 6) u; the square root halves that and adds
  u, the division adds u: (0.5 per + 5) u relative on every normalised value. _tol_norm uses
  (0.5 per + 7) u: the 2 u on top cover the f32 rounding of eps and the second-order terms. With flip the sum of the two halves is rounded once
  (u on the value) and moves the norm by at most u more: one ulp = 2 u on top.
* fd: the normalised query carries (0.5 per + 5) u, the dot product's lane sum per u and its
  shuffles 6 u, each times sum |q_i b_i| <= ||q|| ||b|| = 1 for unit rows; 1 - max rounds by at most
  u |fd| <= 2 u: (1.5 per + 13) u absolute, _tol_fd uses (1.5 per + 14) u.

idx is compared with the f64 argmax for every query, none excluded, under the asserted
precondition that the f64 gap between the two largest similarities exceeds 2 _tol_fd: no rounding
the bound allows can then reorder them.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FILL = 0xB7
DIMS = [64, 512, 768, 1024]
NS = [1, 3, 4, 5, 8, 9, 17]
BS = [1, 2, 3, 4, 5, 64, 1025]
EPS_FACE = float(np.float32(1e-6))       # embed_finalize and bank_match clamp the norm at 1e-6f


def _tol_fd(dim):
    return (1.5 * (dim // 64) + 14) * U


def _tol_norm(dim, flip=False):
    return (0.5 * (dim // 64) + 7) * U + (2 * U if flip else 0.0)


# ---- references (f64) ---------------------------------------------------------------------------
def _ref_normalize(x, eps):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), eps)


def _ref_match(q, bank):
    """match.fd_min per query in f64: (fd, argmax, gap between the two largest similarities)."""
    sims = _ref_normalize(q, EPS_FACE) @ np.asarray(bank, np.float64).T
    top = np.sort(sims, axis=1)
    gap = top[:, -1] - top[:, -2] if sims.shape[1] > 1 else np.full(len(sims), np.inf)
    return 1.0 - sims.max(axis=1), sims.argmax(axis=1), gap


# ---- device calls, as engines.BankMatcher and the embedders make them ------------------------------
def _filled(ctx, nbytes):
    b = ctx.alloc(nbytes)
    ctx.memset(b.ptr, FILL, nbytes)
    return b


def _untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def _bank_match(ctx, q, bank, dim, want_rc0=True):
    """fd [n], idx [n] and the 16 floats / ints past each (which must keep the fill pattern)."""
    q = np.ascontiguousarray(q, np.float32)
    bank = np.ascontiguousarray(bank, np.float32)
    n, B = len(q), len(bank)
    dq = ctx.upload(q)
    db = ctx.upload(bank) if bank.size else ctx.alloc(16)
    dfd, didx = _filled(ctx, (n + 16) * 4), _filled(ctx, (n + 16) * 4)
    rc = ctx.lib.pc_bank_match(ctx.handle, C.c_void_p(dq.ptr), n, C.c_void_p(db.ptr), B, dim, C.c_void_p(dfd.ptr),
                               C.c_void_p(didx.ptr))
    fd = ctx.download(dfd.ptr, (n + 16,), np.float32)
    idx = ctx.download(didx.ptr, (n + 16,), np.int32)
    for b in (dq, db, dfd, didx):
        b.free()
    if not want_rc0:
        return rc, fd, idx
    assert rc == 0
    assert _untouched(fd[n:]) and _untouched(idx[n:])
    return fd[:n], idx[:n]


def _normalize(ctx, e, n, dim, flip=0, eps=None, want_rc0=True):
    """pc_embed_finalize (eps None) or pc_l2_normalize of e [rows][ld] -> [n][dim]."""
    e = np.ascontiguousarray(e, np.float32)
    ld = e.shape[1]
    de = ctx.upload(e)
    dout = _filled(ctx, (n * dim + 16) * 4)
    if eps is None:
        rc = ctx.lib.pc_embed_finalize(ctx.handle, C.c_void_p(de.ptr), ld, n, dim, flip, C.c_void_p(dout.ptr))
    else:
        rc = ctx.lib.pc_l2_normalize(ctx.handle, C.c_void_p(de.ptr), ld, n, dim, C.c_float(eps), C.c_void_p(dout.ptr))
    out = ctx.download(dout.ptr, (n * dim + 16,), np.float32)
    de.free()
    dout.free()
    if not want_rc0:
        return rc, out
    assert rc == 0
    assert _untouched(out[n * dim:])
    return out[:n * dim].reshape(n, dim)


def _unit_rows(rng, B, dim):
    b = rng.normal(size=(B, dim))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _queries(rng, n, dim):
    """Rows of norms spread over 0.1 .. 30 (log-uniform)."""
    q = rng.normal(size=(n, dim))
    q *= (0.1 * 300.0 ** rng.uniform(size=(n, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


# ---- bank_match: fd and idx ----------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("dim", DIMS)
def test_bank_match_fd_and_idx(gpu_ctx, dim, B):
    """n in NS: one to three workgroups, the last one partial except at 8; B < 4 leaves waves without a
    row (bi = -1), 5 and 1025 give the waves unequal shares."""
    rng = np.random.default_rng(dim * 7 + B)
    bank = _unit_rows(rng, B, dim)
    q_all = _queries(rng, sum(NS), dim)
    tol = _tol_fd(dim)
    worst, min_gap, at = 0.0, np.inf, 0
    for n in NS:
        q = q_all[at:at + n]
        at += n
        fd_ref, idx_ref, gap = _ref_match(q, bank)
        min_gap = min(min_gap, gap.min())
        assert np.all(gap > 2 * tol), f"n {n}: top-two gap {gap.min():.3g} within 2 tol"
        fd, idx = _bank_match(gpu_ctx, q, bank, dim)
        worst = max(worst, float(np.abs(fd.astype(np.float64) - fd_ref).max()))
        assert np.all(np.abs(fd.astype(np.float64) - fd_ref) <= tol), f"n {n}"
        assert np.array_equal(idx, idx_ref.astype(np.int32)), f"n {n}"
    print(f"dim {dim} B {B}: max |fd - ref| {worst:.3g} (tol {tol:.3g}), smallest top-two gap {min_gap:.3g}")


@pytest.mark.parametrize("rows", [(2, 5, 7), (1, 9)], ids=["three_waves", "one_wave"])
@pytest.mark.parametrize("dim", [512, 768])
def test_bank_match_exact_ties(gpu_ctx, dim, rows):
    """Bit-identical copies of the best row: the dot products are bit-equal, idx is the first of them
    (np.argmax). Rows 2, 5, 7 are swept by waves 2, 1, 3 (the cross-wave tie rule), rows 1 and 9 both by
    wave 1 (the strict > of the sweep)."""
    assert len({r % 4 for r in rows}) == (len(rows) if len(rows) == 3 else 1)
    rng = np.random.default_rng(dim + sum(rows))
    bank = _unit_rows(rng, 12, dim)
    best = bank[rows[0]].copy()
    for r in rows:
        bank[r] = best
    q = (best[None, :] * np.array([[0.2], [1.0], [7.0], [25.0], [3.0]]) + 0.002 * rng.normal(size=(5, dim))).astype(np.float32)
    fd_ref, _, _ = _ref_match(q, bank)
    sims = np.sort(_ref_normalize(q, EPS_FACE) @ bank.astype(np.float64).T, axis=1)
    assert all(bank[r].tobytes() == best.tobytes() for r in rows)
    assert np.all(sims[:, -len(rows)] - sims[:, -len(rows) - 1] > 0.5)      # the copies lead every other row by far
    fd, idx = _bank_match(gpu_ctx, q, bank, dim)
    assert np.all(np.abs(fd.astype(np.float64) - fd_ref) <= _tol_fd(dim))
    assert np.array_equal(idx, np.full(5, rows[0], np.int32)), idx


@pytest.mark.parametrize("dim", DIMS)
def test_bank_match_zero_and_tiny_queries(gpu_ctx, dim):
    """A zero row (every similarity 0: fd 1, idx 0) and a row of norm 1e-8 (divided by the 1e-6 clamp,
    not by its norm: similarities of a vector of norm 0.01) among ordinary ones."""
    rng = np.random.default_rng(dim + 1)
    bank = _unit_rows(rng, 5, dim)
    q = _queries(rng, 4, dim)
    q[1] = 0
    q[2] *= np.float32(1e-8) / np.float32(np.linalg.norm(q[2].astype(np.float64)))
    assert 0.9e-8 < np.linalg.norm(q[2].astype(np.float64)) < 1.1e-8
    fd_ref, idx_ref, gap = _ref_match(q, bank)
    assert fd_ref[1] == 1.0 and idx_ref[1] == 0 and 0.98 < fd_ref[2] < 1.02 and fd_ref[2] != 1.0
    keep = np.array([0, 2, 3])
    assert np.all(gap[keep] > 2 * _tol_fd(dim))
    fd, idx = _bank_match(gpu_ctx, q, bank, dim)
    print(f"dim {dim}: max |fd - ref| {np.abs(fd - fd_ref).max():.3g} (tol {_tol_fd(dim):.3g})")
    assert np.all(np.abs(fd.astype(np.float64) - fd_ref) <= _tol_fd(dim))
    assert fd[1] == 1.0
    assert np.array_equal(idx, idx_ref.astype(np.int32))


@pytest.mark.parametrize("dim", [64, 1024])
def test_bank_match_empty_bank(gpu_ctx, dim):
    """fd 9.0 (match.fd_min on an empty bank) and idx -1 (include/pcgpu.h), partial workgroup included."""
    q = _queries(np.random.default_rng(dim), 9, dim)
    fd, idx = _bank_match(gpu_ctx, q, np.zeros((0, dim), np.float32), dim)
    assert np.all(fd == np.float32(9.0)) and np.all(idx == -1)


# ---- embed_finalize / l2_normalize ------------------------------------------------------------------
def _padded(rows, ld):
    """rows [r][dim] inside [r][ld], the padding NaN: a value read from it poisons the row's output."""
    e = np.full((rows.shape[0], ld), np.nan, np.float32)
    e[:, :rows.shape[1]] = rows
    return e


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dim", DIMS)
def test_embed_finalize(gpu_ctx, dim, flip):
    """n = 9 (three workgroups of four rows, the last with one), ld = dim + 8, with a zero row, a row
    that the flip sum cancels to zero and a row of norm 1e-8 (the clamp: divided by 1e-6)."""
    n, ld = 9, dim + 8
    rng = np.random.default_rng(dim * 2 + flip)
    a = _queries(rng, n, dim)
    a[2] = 0
    a[5] *= np.float32(1e-8) / np.float32(np.linalg.norm(a[5].astype(np.float64)))
    rows = a
    x = a.astype(np.float64)
    if flip:
        b = _queries(rng, n, dim)
        b[2] = 0
        b[4] = -a[4]                       # cancels exactly
        b[5] = 0
        rows = np.concatenate([a, b])
        x = x + b.astype(np.float64)
    ref = _ref_normalize(x, EPS_FACE)
    assert np.all(ref[2] == 0) and 0.009 < np.linalg.norm(ref[5]) < 0.011
    assert not flip or np.all(ref[4] == 0)
    got = _normalize(gpu_ctx, _padded(rows, ld), n, dim, flip=flip)
    tol = _tol_norm(dim, flip)
    err = np.abs(got.astype(np.float64) - ref)
    nz = ref != 0
    print(f"dim {dim} flip {flip}: max relative error {(err[nz] / np.abs(ref[nz])).max() / U:.2f} u (tol {tol / U:.1f} u)")
    assert np.all(err <= tol * np.abs(ref))          # (zero rows: exactly zero)


@pytest.mark.parametrize("dim", DIMS)
def test_l2_normalize_eps_1e12(gpu_ctx, dim):
    """torch.nn.functional.normalize's eps: a row of norm 1e-8 is normalised to 1, one of 1e-13 is
    divided by 1e-12, a zero row stays zero; n = 5, ld = dim + 24."""
    n, ld, eps = 5, dim + 24, float(np.float32(1e-12))
    rng = np.random.default_rng(dim * 3)
    a = _queries(rng, n, dim)
    a[1] *= np.float32(1e-8) / np.float32(np.linalg.norm(a[1].astype(np.float64)))
    a[2] = 0
    a[3] *= np.float32(1e-13) / np.float32(np.linalg.norm(a[3].astype(np.float64)))
    ref = _ref_normalize(a, eps)
    norms = np.linalg.norm(ref, axis=1)
    assert abs(norms[1] - 1) < 1e-9 and norms[2] == 0 and 0.09 < norms[3] < 0.11
    got = _normalize(gpu_ctx, _padded(a, ld), n, dim, eps=eps)
    tol = _tol_norm(dim)
    err = np.abs(got.astype(np.float64) - ref)
    nz = ref != 0
    print(f"dim {dim}: max relative error {(err[nz] / np.abs(ref[nz])).max() / U:.2f} u (tol {tol / U:.1f} u)")
    assert np.all(err <= tol * np.abs(ref))


# ---- rejected dims ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 1088])
def test_rejected_dims_write_nothing(gpu_ctx, dim):
    """dim % 64 != 0 or dim > 1024: a non-zero status from all three calls, nothing written."""
    rng = np.random.default_rng(dim)
    q = _queries(rng, 5, dim)
    rc, fd, idx = _bank_match(gpu_ctx, q, _unit_rows(rng, 3, dim), dim, want_rc0=False)
    assert rc != 0 and _untouched(fd) and _untouched(idx)
    rc, out = _normalize(gpu_ctx, np.concatenate([q, q]), 5, dim, flip=1, want_rc0=False)
    assert rc != 0 and _untouched(out)
    rc, out = _normalize(gpu_ctx, q, 5, dim, eps=1e-12, want_rc0=False)
    assert rc != 0 and _untouched(out)
    # the context still works
    fd, idx = _bank_match(gpu_ctx, _queries(rng, 2, 64), _unit_rows(rng, 3, 64), 64)
    assert np.all(np.isfinite(fd)) and np.all((idx >= 0) & (idx < 3))
