"""The attention kernels at the attention output itself (no projection behind it), against the float64
reference net_op_refs.attention: mha_tokens<float | f16 | float, SP> (pc_ops.hip), mha_stream<SP, 64 | 80> and
mha_mfma<64 | 80> (pc_attn.hip).

qkv is the net input of width 3E + 32 and the output tensor is E + 32 wide, so both pixel strides exceed the
data; the split forms read an exact identity conv of the input and write a split output read as hi + lo.
Every run holds one (image, head) pair per data kind (net_op_cases.ATT_KINDS): random-normal, one winning
key (logit 100, the others <= 60; net_op_cases.ATT_WINNER puts it first, last in a partial chunk or tile, at key
63 and at key 64 for every kernel form), two tied keys in different waves or tiles, logits ramping up (the running
maximum moves at every chunk) and down, and all logits equal. T covers: waves without a key (T <= 48 in
mha_stream, T < 4 in mha_tokens), T = 1, the tile and query-block edge 64 / 65, and the dispatch edge
272 / 273 between the resident and the streaming forms. The T = 65 runs with three heads and three images
give every (image, head) data of its own: the block -> (image, head, query block) decoding.

Bounds: net_op_cases.att_bound (derived in its docstring): 1e-5 max|v| for random-normal data on the f32-class
forms, the constructed kinds from the f32 logit rounding, __expf and the accumulation over T keys, plus half an
f16 ulp for f16 outputs, 2^-22 relative for split outputs, and for mha_mfma 2^-10 max|v| (P in f16) and
T 2^-25 max|v| (P in the f16 subnormals). No output is NaN or inf. Measured maxima are printed per data kind."""
import numpy as np
import pytest

import net_op_cases as nc
import net_op_refs as R
from net_op_device import assert_bit_equal, assert_split_storage, halves, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", nc.att_runs(), ids=lambda r: f"{r[0]}-T{r[1]}-h{r[2]}-n{r[3]}")
def test_attention_vs_f64(gpu_ctx, monkeypatch, run):
    case = nc.att_case(*run)
    # read when the net is created (pc_net.h Tuning::attn_stream)
    if case.stream:
        monkeypatch.setenv("PERSON_CAPTURE_AMD_ATTN", "stream")
    else:
        monkeypatch.delenv("PERSON_CAPTURE_AMD_ATTN", raising=False)
    outs, _ = run_case(gpu_ctx, case)
    hi, lo = halves(case, 0, outs[0])
    got = hi.astype(np.float64) if lo is None else R.unsplit(hi, lo)
    E, d = case.E, case.d
    assert np.isfinite(got).all(), case.name
    err = np.abs(got - case.exp[0])
    line = []
    for (n, h), kind in sorted(case.kinds.items()):
        sl = slice(h * d, (h + 1) * d)
        e, b = err[n, 0, :, sl], case.bound[n, 0, :, sl]
        line.append(f"[{n},{h}] {kind} {e.max():.2e} / {b.flat[np.argmax(e)]:.2e}")
        assert (e <= b).all(), (case.name, n, h, kind, e.max(), b.flat[np.argmax(e)])
    kernel = nc.ATT_FORMS[case.form][3] if run[1] <= 272 else "the streaming form of this storage"
    print(f"{case.name} ({kernel}): max err / bound there: " + "; ".join(line))
    # the 32 channels beyond E stay as the buffer was created: the kernels write heads * d channels
    assert not hi[..., E:].any() and (lo is None or not lo[..., E:].any()), case.name
    if lo is not None:
        assert_split_storage(hi, lo)
        assert_bit_equal(case, 1, outs[1], case.exp[1])            # the identity conv in front was exact
