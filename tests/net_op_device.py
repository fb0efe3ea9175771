"""Running a net_op_cases.Case on the device and reading its outputs as stored: shared by
test_gpu_net_ops.py and test_gpu_attention_edges.py."""
import numpy as np

import net_op_refs as R
from person_capture_amd._lib import PC_PREC_F16, PC_PREC_F32
from person_capture_amd.runtime import Net

MAX_BATCH = 4        # the cases run N = 3 images (or 1) on a net of 4


def run_case(ctx, case, calibrate=False):
    """-> (the raw storage [N][H][W][cs] of every program output, pc_net_calibrate's abs-max per tensor or None)."""
    net = Net(ctx, case.P.serialize(), precision=PC_PREC_F32 if case.f32 else PC_PREC_F16, max_batch=MAX_BATCH)
    try:
        d = ctx.upload(case.storage())
        absmax = None
        if calibrate:
            absmax = net.calibrate(d.ptr, case.N, n_tensors=len(case.P.tensors))
        else:
            net.run(d.ptr, case.N)
        outs = []
        for i in range(len(case.P.outputs)):
            ptr, (H, W, _, cs, is_f32) = net.output(i)
            outs.append(ctx.download(ptr, (case.N, H, W, cs), np.float32 if is_f32 else np.float16))
    finally:
        net.close()
    return outs, absmax


def halves(case, i, raw):
    """(hi, lo) of output i as stored (lo None for a plain tensor), over the tensor's logical channels."""
    t = case.P.outputs[i]
    assert raw.shape[-1] == case.P.tensors[t][4]
    if case.P.tsplit[t]:
        h = case.P.tensors[t][3] // 2
        return raw[..., :h], raw[..., h:2 * h]
    return raw[..., :case.P.tensors[t][3]], None


def assert_bit_equal(case, i, raw, exp):
    hi, lo = halves(case, i, raw)
    assert hi.shape == exp.shape, (hi.shape, exp.shape)
    if lo is None:
        assert np.array_equal(hi.astype(np.float64), exp), f"{case.name}: output {i}"
        return
    assert np.array_equal(R.unsplit(hi, lo), exp), f"{case.name}: output {i}: hi + lo"
    assert np.array_equal(hi, R.split(exp)[0]), f"{case.name}: output {i}: hi = f16(m)"


def assert_split_storage(hi, lo):
    """hi = f16(v), lo = f16(v - hi): |lo| is at most half an ulp of hi, which is at most 2^-11 |hi| (2^-25 below
    the normal range). (hi = f16(hi + lo) itself does not follow: a lo that rounded up to exactly half an ulp
    makes the sum a tie.)"""
    assert (np.abs(lo.astype(np.float64)) <= np.maximum(2.0 ** -11 * np.abs(hi.astype(np.float64)), 2.0 ** -25)).all()
