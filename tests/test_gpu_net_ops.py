"""The net executor's non-GEMM kernels at op level, against the float64 references of net_op_refs.py:
the four max pools (pc_conv.hip), upsample2_nhwc, the LayerNorm forms and absmax_f16 / pc_net_calibrate
(pc_ops.hip). The programs, inputs and expectations are net_op_cases.py's (checked on the CPU against
torch in f64 by test_net_op_refs_cpu.py); every case is a few thousand elements.

* max pool and upsample: bit-equal to the reference, in every declared channel of every output -
  including the slices of a shared buffer that the op must leave as the identity conv wrote them.
  Split outputs: hi + lo equals the reference and hi = f16(m).
* LayerNorm: within the bound net_op_cases.ln_bound derives (its docstring) per element; channels
  [C, width) exactly zero; no NaN. Measured maxima are printed beside the bound (-s shows them).
* pc_net_calibrate: the reported abs-max of every conv-written f16 tensor equals, as f32 bits, max |x| of the
  device's own downloaded output; every other tensor reads 0.
* three programs with bad geometry are refused by pc_net_create with PC_ERR_FORMAT (none is ever run).
"""
import ctypes as C

import numpy as np
import pytest

import net_op_cases as nc
import net_op_refs as R
from net_op_device import MAX_BATCH, assert_bit_equal, assert_split_storage, halves, run_case
from person_capture_amd._lib import PC_PREC_F16
from plan_geometry_cases import geometry_cases

pytestmark = pytest.mark.gpu

PC_ERR_FORMAT = 4


@pytest.mark.parametrize("case", nc.pool_cases(), ids=lambda c: c.name)
def test_maxpool_bit_equal(gpu_ctx, case):
    outs, _ = run_case(gpu_ctx, case)
    for i, exp in enumerate(case.exp):
        assert_bit_equal(case, i, outs[i], exp)


@pytest.mark.parametrize("case", nc.upsample_cases(), ids=lambda c: c.name)
def test_upsample_bit_equal(gpu_ctx, case):
    outs, _ = run_case(gpu_ctx, case)
    for i, exp in enumerate(case.exp):
        assert_bit_equal(case, i, outs[i], exp)


@pytest.mark.parametrize("case", nc.layernorm_cases(), ids=lambda c: c.name)
def test_layernorm_vs_f64(gpu_ctx, case):
    """Bound: net_op_cases.ln_bound (derived there from the kernels' f32 arithmetic, per element)."""
    outs, _ = run_case(gpu_ctx, case)
    hi, lo = halves(case, 0, outs[0])
    got = hi.astype(np.float64) if lo is None else R.unsplit(hi, lo)
    Cn, exp, bound = case.C, case.exp[0], case.bound
    assert np.isfinite(got).all(), case.name
    err = np.abs(got - exp)
    worst = {}
    for (n, t), kind in case.kinds.items():
        r = (err[n, 0, t, :Cn] / bound[n, 0, t, :Cn]).max()
        if r >= worst.get(kind, (-1,))[0]:
            worst[kind] = (r, err[n, 0, t, :Cn].max(), bound[n, 0, t, :Cn][np.argmax(err[n, 0, t, :Cn])])
    print(f"{case.name}: " + "; ".join(f"{k} max err {e:.2e} (bound there {b:.2e}, worst err/bound {r:.3f})"
                                       for k, (r, e, b) in sorted(worst.items())))
    assert (err[..., :Cn] <= bound[..., :Cn]).all(), case.name
    # the zero tail, in both halves of a split output
    assert not hi[..., Cn:].any() and (lo is None or not lo[..., Cn:].any()), case.name
    if lo is not None:
        assert_split_storage(hi, lo)
        assert_bit_equal(case, 1, outs[1], case.exp[1])            # the identity conv in front was exact


@pytest.mark.parametrize("case", nc.calib_cases(), ids=lambda c: c.name)
def test_calibrate_absmax_exact(gpu_ctx, case):
    outs, absmax = run_case(gpu_ctx, case, calibrate=True)
    P = case.P
    assert absmax.shape == (len(P.tensors),)
    seen = {}
    for t, what in case.measured.items():
        vb, _, _, Ct, _, coff, _ = P.tensors[t]
        # the program output that holds this tensor's buffer; a split tensor's figure is its hi half
        i = next(i for i, o in enumerate(P.outputs) if P.tensors[o][0] == vb)
        h = Ct // 2 if P.tsplit[t] else Ct
        x = outs[i][..., coff:coff + h].astype(np.float32)
        want = np.float32(np.abs(x).max())
        seen[what] = (x.flat[np.argmax(np.abs(x))], absmax[t])
        assert absmax[t].view(np.uint32) == want.view(np.uint32), (case.name, what, absmax[t], want)
    print(f"{case.name}: " + ", ".join(f"{k}: extreme {v:g}, abs-max {m:g}" for k, (v, m) in seen.items()))
    assert seen["negative maximum"][0] == -6.75 and seen["negative maximum"][1] == 6.75
    if "near 300" in seen:
        assert seen["near 300"][1] == 288.0
        assert seen["near 0.01"][1] == 4.5 * 2.0 ** -9               # its own largest: it does not see its neighbour
    for t in range(len(P.tensors)):
        if t not in case.measured:
            assert absmax[t] == 0.0, (case.name, t, absmax[t])


def test_bad_geometry_refused_by_net_create(gpu_ctx):
    """pc_net_create runs the same decoder as pc_net_plan: nothing is allocated or launched for these."""
    cases = geometry_cases()
    for name in ("layernorm_c4096", "pool_c6", "attention_qkv_narrow"):
        prog = cases[name][0].serialize()
        buf = C.create_string_buffer(prog, len(prog))
        h = C.c_void_p()
        rc = gpu_ctx.lib.pc_net_create(gpu_ctx.handle, buf, len(prog), PC_PREC_F16, MAX_BATCH, C.byref(h))
        if rc == 0:
            gpu_ctx.lib.pc_net_destroy(h)
        assert rc == PC_ERR_FORMAT, (name, rc)
        assert cases[name][1] in gpu_ctx.lib.pc_last_error(gpu_ctx.handle).decode()
