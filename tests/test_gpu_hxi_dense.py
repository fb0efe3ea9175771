"""conv_hxi's split 14x14x256 and 28x28x128 forms without padding columns in their pixel fragments
(pc_conv_hxi.hip HxiGeom DENSE and the pitch-29 form, PC_HXI_DENSE, the default) against
the pitch enumeration (PC_HXI_DENSE=0). Every output pixel keeps its accumulation order and its epilogue,
so the net output is compared byte for byte: per-layer launches (PC_CONV_HXI=59: codes 502 / 503) and
chained ones (123: code 300 for the 14x14 runs), eagerly and through one graph replay.

The net is test_gpu_hxi_chain.py's: a synthetic IResNet-34 split program (10 14x14x256 layers, 6 28x28x128
ones; residuals, PReLU and the border-class bias of the folded pre-BN convs, at the image's borders and at
the interior rows of the 28x28 form's 7-row blocks), created for 192 images and run at 33 and 37, the
smallest batches that take the one-image forms."""
import numpy as np
import pytest

from person_capture_amd import models
from person_capture_amd._lib import PC_PREC_F16

pytestmark = pytest.mark.gpu

MAXB = 192
B0 = 33
CHAINED, UNCHAINED = "123", "59"


def _input(gpu_ctx, batch, seed):
    x = np.zeros((batch, 112, 112, 4), np.float16)
    x[..., :3] = np.random.default_rng(seed).uniform(-127.5, 127.5, (batch, 112, 112, 3))
    return gpu_ctx.upload(x)


def _run(gpu_ctx, monkeypatch, P, d, batch, mask, dense):
    """(output bytes of an eager run, its profile codes, output bytes of a graph replay)"""
    from person_capture_amd.runtime import Net
    monkeypatch.setenv("PC_CONV_HXI", mask)
    monkeypatch.setenv("PC_HXI_DENSE", dense)
    monkeypatch.delenv("PC_HXI_CHAIN_MAX", raising=False)
    monkeypatch.delenv("PC_HXI28_OCC", raising=False)
    net = Net(gpu_ctx, P.serialize(), PC_PREC_F16, max_batch=MAXB)
    try:
        net.profile(True)
        net.run(d.ptr, batch)
        codes = [int(r[4]) for r in net.profile_ops()]
        net.profile(False)
        eager = net.read_output(0, batch).copy().view(np.uint8)
        net.set_graph(True)
        net.run(d.ptr, batch)      # capture + first launch
        net.run(d.ptr, batch)      # replay
        replay = net.read_output(0, batch).copy().view(np.uint8)
        return eager, codes, replay
    finally:
        net.close()


@pytest.fixture(scope="module")
def r34():
    return models.compile_iresnet(models.synth_iresnet(34, seed=21), 34, split=True)


@pytest.mark.parametrize("mask", [CHAINED, UNCHAINED])
@pytest.mark.parametrize("batch", [B0, B0 + 4])
def test_hxi_dense_bit_identical(gpu_ctx, monkeypatch, r34, batch, mask):
    d = _input(gpu_ctx, batch, seed=batch)
    try:
        ref, ref_codes, ref_replay = _run(gpu_ctx, monkeypatch, r34, d, batch, mask, "0")
        got, codes, replay = _run(gpu_ctx, monkeypatch, r34, d, batch, mask, "1")
    finally:
        d.free()
    # the switch changes no plan: the same kernels' codes, and the forms in question did run
    assert codes == ref_codes
    assert codes.count(503) == 6, codes
    if mask == CHAINED:
        assert codes.count(300) >= 2 and 502 not in codes, codes
    else:
        assert codes.count(502) == 10 and 300 not in codes, codes
    assert np.array_equal(ref_replay, ref)
    assert np.array_equal(got, ref)
    assert np.array_equal(replay, ref)
