"""The float64 references of the non-GEMM ops (net_op_refs.py) against torch in f64, on the shapes and
data of the device tests (net_op_cases.py), and the CPU emulator of the programs against the references
within f32 rounding. After this the references can be trusted without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import net_op_cases as nc
import net_op_refs as R
from program_emulator import run_program


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(x, np.float64), (0, 3, 1, 2))))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("geom", nc.POOL_GEOMS)
@pytest.mark.parametrize("data", nc.POOL_DATA)
def test_maxpool_ref_vs_torch(geom, data):
    H, W, k, s, p = geom
    x = nc.pool_values(np.random.default_rng(1), (3, H, W, 8), data)
    assert (x < 0).all() or data != "negative"
    ref = R.maxpool(x, k, s, p)
    assert np.array_equal(ref, _nhwc(F.max_pool2d(_nchw(x), k, s, p)))
    assert np.isfinite(ref).all()
    if data == "negative":        # a pool that padded with 0 would answer 0 at the border
        assert (ref < 0).all()


@pytest.mark.parametrize("shape", [(3, 3, 5, 8), (3, 1, 1, 40), (1, 6, 10, 4)])
def test_upsample_ref_vs_torch(shape):
    x = np.random.default_rng(2).standard_normal(shape)
    assert np.array_equal(R.upsample2(x), _nhwc(F.interpolate(_nchw(x), scale_factor=2.0, mode="nearest")))


@pytest.mark.parametrize("case", nc.layernorm_cases(), ids=lambda c: c.name)
def test_layernorm_ref_vs_torch(case):
    C = case.C
    x = torch.from_numpy(np.asarray(case.val[..., :C], np.float64))
    if case.add is not None:
        x = x + torch.from_numpy(case.add.astype(np.float64))[None, None]
    ref = F.layer_norm(x, (C,), torch.from_numpy(case.gamma.astype(np.float64)), torch.from_numpy(case.beta.astype(np.float64)),
                       float(np.float32(case.eps))).numpy()
    got = case.exp[0]
    assert np.abs(got[..., :C] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert not got[..., C:].any()
    for (n, t), kind in case.kinds.items():      # a constant row answers beta
        if kind == "constant" and case.add is None:
            assert np.abs(got[n, 0, t, :C] - case.beta).max() <= case.bound[n, 0, t, :C].max()


@pytest.mark.parametrize("run", nc.att_runs(), ids=lambda r: "-".join(map(str, r)))
def test_attention_ref_vs_torch(run):
    case = nc.att_case(*run)
    E, d, heads = case.E, case.d, case.heads
    N, T = case.val.shape[0], case.val.shape[2]
    x = torch.from_numpy(np.asarray(case.val[:, 0], np.float64))
    q, k, v = (x[..., i * E:(i + 1) * E].reshape(N, T, heads, d).transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(d), -1) @ v).transpose(1, 2).reshape(N, T, E).numpy()
    got = case.exp[0][:, 0]
    assert np.abs(got[..., :E] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert not got[..., E:].any()
    # what the constructed kinds are built to answer
    for (n, h), kind in case.kinds.items():
        o = got[n, :, h * d:(h + 1) * d]
        vv = case.val[n, 0, :, 2 * E + h * d:2 * E + (h + 1) * d]
        kk = case.val[n, 0, :, E + h * d]
        if kind == "winner":
            assert np.abs(o - vv[int(np.argmax(kk))]).max() < 1e-9
        elif kind == "tie" and T >= 2:
            i, j = np.flatnonzero(kk == 100.0)
            assert np.abs(o - (vv[i] + vv[j]) / 2).max() < 1e-9
        elif kind == "flat":
            assert np.abs(o - vv.mean(0)).max() < 1e-12


def test_winner_placements_cover_every_form():
    """Every kernel form meets a winning key first, last in a partial chunk or tile, at key 63 and at key 64."""
    seen = {form: set() for form in nc.ATT_FORMS}
    for run in nc.att_runs():
        case = nc.att_case(*run)
        E, d, T = case.E, case.d, run[1]
        for (n, h), kind in case.kinds.items():
            if kind == "winner":
                kk = case.val[n, 0, :, E + h * d]
                assert (kk == 100.0).sum() == 1 and (np.delete(kk, np.argmax(kk)) <= 60).all()
                seen[run[0]] |= nc.att_winner_placements(T, int(np.argmax(kk)))
    for form, got in seen.items():
        assert got == {"first", "last", "63", "64"}, (form, got)


def test_split_rule():
    v = np.random.default_rng(3).standard_normal(4096).astype(np.float32) * 100
    hi, lo = R.split(v)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    assert np.array_equal(hi, v.astype(np.float16))
    s = R.unsplit(hi, lo)
    assert np.abs(s - v).max() <= 2.0 ** -22 * np.abs(v).max()
    exact = (np.arange(-2048, 2048) / 64.0).astype(np.float32)          # f16 values: lo = 0, the sum is the value
    hi, lo = R.split(exact)
    assert not lo.any() and np.array_equal(R.unsplit(hi, lo), exact.astype(np.float64))


# ---- the emulator against the references, on the programs of the device tests -----------------------
F32_REL = 2.0 ** -21     # a few f32 roundings of the value itself


def _emulate(case):
    outs = run_program(case.P, np.asarray(case.storage(), np.float32))
    return [o.permute(0, 2, 3, 1).numpy().astype(np.float64) for o in outs]


@pytest.mark.parametrize("case", nc.pool_cases() + nc.upsample_cases(), ids=lambda c: c.name)
def test_emulator_exact_ops(case):
    for got, exp in zip(_emulate(case), case.exp):
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("case", nc.layernorm_cases(), ids=lambda c: c.name)
def test_emulator_layernorm(case):
    outs = _emulate(case)
    err = np.abs(outs[0] - case.exp[0])
    assert (err <= case.bound + F32_REL * np.abs(case.exp[0])).all(), (err / np.maximum(case.bound, 1e-30)).max()
    if len(outs) > 1:
        assert np.array_equal(outs[1], case.exp[1])


@pytest.mark.parametrize("run", [r for r in nc.att_runs() if r[1] in (1, 17, 65, 273)], ids=lambda r: "-".join(map(str, r)))
def test_emulator_attention(run):
    case = nc.att_case(*run)
    outs = _emulate(case)
    err = np.abs(outs[0] - case.exp[0])
    vmax = np.abs(case.val).max()
    assert np.isfinite(outs[0]).all() and (err <= 1e-5 * vmax).all(), err.max()
