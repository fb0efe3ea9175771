"""The curator kernels (pc_curate.hip) through the C ABI and the Python surface: pc_crop_metrics
against the NumPy backend (every integer and both planes equal, the DCT block within one f32
rounding of an f64 reference), pc_sim_matrix against an f64 product, pc_mmr_order against a plain
restatement of the reference's greedy loop."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.fft

from person_capture_amd import _lib, curate
from person_capture_amd._lib import check

from curate_cases import MMR_CASES, PHASH_IMAGES, SHAPES, greedy_mmr, image, mmr_inputs, unit_rows

pytestmark = pytest.mark.gpu

COEF_TOL = 2.0 ** -22


@functools.lru_cache(maxsize=None)
def backend(h, w, seed):
    return curate.crop_metrics_batch([image(h, w, seed)], keep_planes=True)[0]


def assert_same(dev, ref, what):
    for f in ("w", "h", "w2", "h2", "sum_g2", "sum_lap", "sum_lap2"):
        assert getattr(dev, f) == getattr(ref, f), (what, f)
    for f in ("hist", "row_sum", "col_sum"):
        assert np.array_equal(getattr(dev, f), getattr(ref, f)), (what, f)
    for p in ("gray", "g2", "p32"):
        assert np.array_equal(dev.planes[p], ref.planes[p]), (what, p)
    want = scipy.fft.dctn(ref.planes["p32"].astype(np.float64), norm="ortho")[:8, :8]
    assert np.all(np.abs(dev.coef.astype(np.float64) - want) <= COEF_TOL * np.maximum(1.0, np.abs(want))), what
    # derived values: equal as floats (same integers through the same host expressions)
    assert dev.sharpness == ref.sharpness and dev.exposure == ref.exposure and dev.black_border == ref.black_border
    assert dev.lap_var == ref.lap_var


def run_desc_batch(ctx, crops):
    """pc_crop_metrics on crops given as (image, row_stride, byte offset of the base pointer): the
    raw ABI call with buffers from pc_crop_metrics_layout."""
    n = len(crops)
    bufs, items = [], []
    for img, stride, shift in crops:
        h, w = img.shape[:2]
        host = np.zeros(h * stride + 64, np.uint8)
        rows = np.lib.stride_tricks.as_strided(host[shift:], (h, w * 3), (stride, 1))
        rows[:] = img.reshape(h, w * 3)
        d = ctx.upload(host)
        bufs.append(d)
        items.append(curate.DeviceCrop(d.ptr + shift, h, w, stride))
    return curate.crop_metrics_batch(items, ctx=ctx, keep_planes=True)


def test_crop_metrics_all_shapes(gpu_ctx):
    """One batch with every shape, one crop with row_stride > 3 w and one whose base pointer is 3 bytes
    past a 16-byte boundary (the byte-load path)."""
    crops = [(image(h, w, 0), 3 * w, 0) for h, w in SHAPES]
    crops.append((image(97, 61, 0), 3 * 61 + 29, 0))
    crops.append((image(512, 384, 0), 3 * 384 + 16, 3))
    crops.append((image(640, 427, 0), 3 * 427, 3))
    got = run_desc_batch(gpu_ctx, crops)
    assert len(got) == len(crops)
    for (img, _, _), m in zip(crops, got):
        assert_same(m, backend(img.shape[0], img.shape[1], 0), img.shape)


def test_crop_metrics_batch_of_1_and_33_and_phash(gpu_ctx):
    one = curate.crop_metrics_batch([image(257, 129, 0)], ctx=gpu_ctx, keep_planes=True)
    assert len(one) == 1
    assert_same(one[0], backend(257, 129, 0), "batch of 1")
    keys = [(h, w, s) for s in range(3) for h, w in SHAPES]
    assert len(keys) == 33 and set(PHASH_IMAGES) <= set(keys)
    got = curate.crop_metrics_batch([image(*k) for k in keys], ctx=gpu_ctx, keep_planes=True)
    for k, m in zip(keys, got):
        assert_same(m, backend(*k), k)
        if k in PHASH_IMAGES:
            want = scipy.fft.dctn(m.planes["p32"].astype(np.float64), norm="ortho")[:8, :8]
            assert curate.phash_margin(want) > 1e-3, k
            assert m.phash == backend(*k).phash == curate.phash_from_coef(want.astype(np.float32)), k


def test_crop_metrics_argument_checks(gpu_ctx):
    descs, tabs, starts = curate.build_descs([(640, 427)])
    descs[0].row_stride = 3 * 427
    off, sb, ob = curate.metrics_layout(descs, 1)
    assert sb > 0 and ob >= _lib.CURATE_RECORD_BYTES + 4 * (640 + 427)
    bad = (_lib.CurateDesc * 1)()
    C.memmove(bad, descs, C.sizeof(bad))
    bad[0].w2 += 1
    with pytest.raises(ValueError):
        curate.metrics_layout(bad, 1)
    C.memmove(bad, descs, C.sizeof(bad))
    bad[0].w = 31
    with pytest.raises(ValueError):
        curate.metrics_layout(bad, 1)
    # too small an output buffer: PC_ERR_ARG before anything is launched
    d = gpu_ctx.alloc(max(sb, ob))
    descs[0].d_src, descs[0].row_stride = d.ptr, 3 * 427
    dct = curate.dct_table()
    rc = gpu_ctx.lib.pc_crop_metrics(gpu_ctx.handle, descs, 1, tabs.ctypes.data_as(C.c_void_p), len(tabs),
                                     starts.ctypes.data_as(C.c_void_p), len(starts), dct.ctypes.data_as(C.c_void_p),
                                     C.c_void_p(d.ptr), sb, C.c_void_p(d.ptr), ob - 16)
    assert rc == 1
    # a table index past the source axis: refused on the host
    tabs2 = tabs.copy()
    tabs2["si"][-1] = 100000
    rc = gpu_ctx.lib.pc_crop_metrics(gpu_ctx.handle, descs, 1, tabs2.ctypes.data_as(C.c_void_p), len(tabs2),
                                     starts.ctypes.data_as(C.c_void_p), len(starts), dct.ctypes.data_as(C.c_void_p),
                                     C.c_void_p(d.ptr), sb, C.c_void_p(d.ptr), ob)
    assert rc == 1
    with pytest.raises(ValueError):
        curate.crop_metrics_batch([np.zeros((20, 40, 3), np.uint8)], ctx=gpu_ctx)
    d.free()


# ---- similarity ----
def dev_sim(ctx, F):
    n, dim = F.shape
    d_F = ctx.upload(F)
    d_S = ctx.alloc(4 * n * n)
    ctx.memset(d_S.ptr, 0xFF, 4 * n * n)
    check(ctx.lib.pc_sim_matrix(ctx.handle, C.c_void_p(d_F.ptr), n, dim, C.c_void_p(d_S.ptr)), ctx.handle, "sim")
    S = ctx.download(d_S.ptr, (n, n), np.float32)
    d_F.free()
    d_S.free()
    return S


@pytest.mark.parametrize("n,dim", [(1, 512), (65, 77), (300, 512), (257, 1280)])
def test_sim_matrix(gpu_ctx, n, dim):
    zero = (0,) if n == 1 else (3, n - 1)
    F = unit_rows(n, dim, 11 + n, zero_rows=() if n == 1 else zero)
    S = dev_sim(gpu_ctx, F)
    ref = F.astype(np.float64) @ F.astype(np.float64).T
    tol = dim * 2.0 ** -24             # gamma_dim, with sum |a_i b_i| <= 1 for unit rows
    assert np.all(np.abs(S.astype(np.float64) - ref) <= tol)
    assert np.array_equal(S, S.T)
    live = np.ones(n, bool)
    if n > 1:
        live[list(zero)] = False
        assert not S[list(zero)].any() and not S[:, list(zero)].any()     # exact zeros
        assert not np.signbit(S[list(zero)]).any()
    assert np.all(np.abs(np.diag(S)[live].astype(np.float64) - 1.0) <= tol)
    assert dev_sim(gpu_ctx, F).tobytes() == S.tobytes()


def test_sim_matrix_limits(gpu_ctx):
    assert gpu_ctx.lib.pc_sim_matrix(gpu_ctx.handle, None, 8193, 8, None) == 1
    assert gpu_ctx.lib.pc_mmr_order(gpu_ctx.handle, None, None, 8193, 1, 0.75, None) == 1
    assert gpu_ctx.lib.pc_mmr_order(gpu_ctx.handle, None, None, 5, 6, 0.75, None) == 1
    with pytest.raises(ValueError):
        curate.mmr_select_with_q(np.zeros(8193, np.float32), 1, None, ctx=gpu_ctx)


# ---- MMR ----
def dev_mmr(ctx, S, q, k, alpha):
    n = len(q)
    d_S = ctx.upload(np.ascontiguousarray(S, np.float32))
    d_q = ctx.upload(np.ascontiguousarray(q, np.float32))
    d_o = ctx.alloc(4 * k)
    check(ctx.lib.pc_mmr_order(ctx.handle, C.c_void_p(d_S.ptr), C.c_void_p(d_q.ptr), n, k, float(alpha),
                               C.c_void_p(d_o.ptr)), ctx.handle, "mmr")
    out = ctx.download(d_o.ptr, (k,), np.int32).tolist()
    for d in (d_S, d_q, d_o):
        d.free()
    return out


@pytest.mark.parametrize("n,k,alpha,flavour", MMR_CASES)
def test_mmr_order_cases(gpu_ctx, n, k, alpha, flavour):
    """The CPU test's cases on the CPU test's matrices (ties, negative similarities, zero rows)."""
    S, q = mmr_inputs(n, flavour)
    assert dev_mmr(gpu_ctx, S, q, k, alpha) == greedy_mmr(q, k, S, alpha)


@pytest.mark.parametrize("n,dim,k,alpha", [(65, 77, 65, 0.75), (300, 512, 300, 0.75), (300, 512, 40, 0.0),
                                           (1025, 64, 1025, 0.75), (2049, 32, 2049, 0.75), (2049, 32, 100, 1.0)])
def test_mmr_order_on_device_sim(gpu_ctx, n, dim, k, alpha):
    """pc_mmr_order on the device's own S (downloaded), duplicates and zero rows included; n = 1025 and
    2049 go past one item per thread."""
    F = unit_rows(n, dim, 21 + n, zero_rows=(2, n - 3), dup=((0, n - 1), (n // 2, 5)))
    q = np.random.default_rng(n).uniform(0, 1, n).astype(np.float32)
    q[n - 1] = q[0]
    S = dev_sim(gpu_ctx, F)
    assert dev_mmr(gpu_ctx, S, q, k, alpha) == greedy_mmr(q, k, S, alpha, literal=n <= 300)


# ---- Python surface ----
def test_python_surface(gpu_ctx):
    imgs = [image(97, 61, 1), image(640, 427, 1), image(256, 256, 1)]
    dev = curate.crop_metrics_batch(imgs, ctx=gpu_ctx)
    cpu = curate.crop_metrics_batch(imgs)
    for a, b in zip(dev, cpu):
        assert (a.phash, a.sharpness, a.exposure, a.black_border) == (b.phash, b.sharpness, b.exposure, b.black_border)
        assert a.sum_lap2 == b.sum_lap2 and np.array_equal(a.hist, b.hist)
    for n, k, alpha, flavour in MMR_CASES[3:]:
        S, q = mmr_inputs(n, flavour)
        assert curate.mmr_select_with_q(q, k, S, alpha, ctx=gpu_ctx) == curate.mmr_select_with_q(q, k, S, alpha)
    S, q = mmr_inputs(65, "plain")
    assert curate.mmr_select_with_q(q, 65, None, 0.75, ctx=gpu_ctx) == curate.mmr_select_with_q(q, 65, None, 0.75)
    # a matrix that is not symmetric still reads sim_mat[i, picked]
    A = np.random.default_rng(4).uniform(-1, 1, (65, 65)).astype(np.float32)
    assert curate.mmr_select_with_q(q, 65, A, 0.5, ctx=gpu_ctx) == greedy_mmr(q, 65, A, 0.5)
    # mmr_rank: similarity and ranking without S leaving the device
    F = unit_rows(300, 77, 9, zero_rows=(7,))
    q = np.random.default_rng(9).uniform(0, 1, 300).astype(np.float32)
    order, S = curate.mmr_rank(F, q, alpha=0.75, ctx=gpu_ctx, return_sim=True)
    assert order == greedy_mmr(q, 300, S, 0.75) and curate.mmr_rank(F, q, k=9, ctx=gpu_ctx) == order[:9]
    # the default context serves the reference's names
    curate.set_default_context(gpu_ctx)
    try:
        assert curate.phash64(imgs[0]) == cpu[0].phash and curate.sharpness_norm(imgs[1]) == cpu[1].sharpness
    finally:
        curate.set_default_context(None)
