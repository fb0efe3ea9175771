"""Chained conv_hxi launches (pc_conv_hxi.hip conv_hxi_chain, PC_CONV_HXI bit 6): the runs of
14x14x256 and 7x7x512 f16x3 layers of an IResNet as one launch per run, one image per workgroup, against the
same plan with a launch per layer (the mask without bit 6). Every layer runs conv_hxi's own code, so the net
output is compared byte for byte: with no cap on the layers per launch (PC_HXI_CHAIN_MAX=0), with a cap of 1 (every layer a
chained launch of its own) and of 3 (launches that begin on a conv2 whose residual the previous launch wrote,
and that end on a conv1), eagerly and through graph replay.

Batches: the smallest one that takes the one-image-per-workgroup forms - one more than the largest small-batch
plan class, which the reference fixture reads back from the planner's profile codes - and an odd one a few rows
larger. IResNet-34 is the smallest depth with two or more identity blocks at 14x14 (5: a run of 10 layers, and
2 at 7x7: a run of 4); IResNet-100 (runs of 58 and 4) runs once."""
import numpy as np
import pytest

from person_capture_amd import models
from person_capture_amd._lib import PC_PREC_F16

pytestmark = pytest.mark.gpu

MAXB = 192          # the max-batch plans take conv_hxi from 192 images; the small classes end at 32
B0 = 33
CHAINED, UNCHAINED = "123", "59"


def _program(depth, seed):
    return models.compile_iresnet(models.synth_iresnet(depth, seed=seed), depth, split=True)


def _input(gpu_ctx, batch, seed):
    x = np.zeros((batch, 112, 112, 4), np.float16)
    x[..., :3] = np.random.default_rng(seed).uniform(-127.5, 127.5, (batch, 112, 112, 3))
    return gpu_ctx.upload(x)


def _run(gpu_ctx, monkeypatch, P, d, batch, mask, cap=None, graph=False):
    """(output bytes, profile codes of an eager run, graph-replayed output bytes or None, chain_info()[0])"""
    from person_capture_amd.runtime import Net
    monkeypatch.setenv("PC_CONV_HXI", mask)
    if cap is None:
        monkeypatch.delenv("PC_HXI_CHAIN_MAX", raising=False)
    else:
        monkeypatch.setenv("PC_HXI_CHAIN_MAX", str(cap))
    net = Net(gpu_ctx, P.serialize(), PC_PREC_F16, max_batch=MAXB)
    try:
        net.profile(True)
        net.run(d.ptr, batch)
        codes = [int(r[4]) for r in net.profile_ops()]
        net.profile(False)
        eager = net.read_output(0, batch).copy().view(np.uint8)
        replay = None
        if graph:
            net.set_graph(True)
            net.run(d.ptr, batch)      # capture + first launch
            net.run(d.ptr, batch)      # replay
            replay = net.read_output(0, batch).copy().view(np.uint8)
        return eager, codes, replay, net.chain_info()[0]
    finally:
        net.close()


@pytest.fixture(scope="module")
def r34():
    return _program(34, seed=21)


@pytest.fixture(scope="module")
def unchained34(gpu_ctx, r34):
    """Per batch: the per-layer plan's output bytes and profile codes (computed once, shared by the cases)."""
    cache = {}

    def get(monkeypatch, batch):
        if batch not in cache:
            d = _input(gpu_ctx, batch, seed=batch)
            try:
                cache[batch] = _run(gpu_ctx, monkeypatch, r34, d, batch, UNCHAINED)
            finally:
                d.free()
        return cache[batch]
    return get


def test_smallest_batch_of_the_one_image_forms(gpu_ctx, monkeypatch, r34):
    """B0 - 1 images still run the small-batch forms (codes 506 / 508), B0 the one-image forms (502 / 505)."""
    d = _input(gpu_ctx, B0, seed=1)
    try:
        below = _run(gpu_ctx, monkeypatch, r34, d, B0 - 1, UNCHAINED)[1]
        at = _run(gpu_ctx, monkeypatch, r34, d, B0, UNCHAINED)[1]
    finally:
        d.free()
    assert below.count(506) == 10 and below.count(508) == 4 and not {502, 505} & set(below), below
    assert at.count(502) == 10 and at.count(505) == 4 and not {506, 508} & set(at), at


@pytest.mark.parametrize("cap", [0, 1, 3])     # (PC_HXI_CHAIN_MAX; 0: no cap)
@pytest.mark.parametrize("batch", [B0, B0 + 4])
def test_hxi_chain_bit_identical(gpu_ctx, monkeypatch, r34, unchained34, batch, cap):
    ref, ref_codes, _, ref_chains = unchained34(monkeypatch, batch)
    n14, n7 = ref_codes.count(502), ref_codes.count(505)
    assert (n14, n7) == (10, 4) and 300 not in ref_codes and ref_chains == 0, ref_codes
    d = _input(gpu_ctx, batch, seed=batch)
    try:
        got, codes, replay, chains = _run(gpu_ctx, monkeypatch, r34, d, batch, CHAINED, cap, graph=True)
    finally:
        d.free()
    per = cap or max(n14, n7)
    want = -(-n14 // per) + -(-n7 // per)          # launches: each run cut into pieces of at most `cap` layers
    assert codes.count(300) == want and not {502, 505} & set(codes), codes
    # (the further layers of a launch leave a marker each, code 301: no time, no FLOPs)
    assert codes.count(301) == n14 + n7 - want and len(codes) == len(ref_codes)
    # every other op keeps its record
    assert [c for c in codes if c not in (300, 301)] == [c for c in ref_codes if c not in (502, 505)]
    assert chains == 0                              # (pc_net_chain_info counts the resident f16 chains only)
    assert np.array_equal(got, ref)
    assert np.array_equal(replay, ref)


def test_hxi_chain_iresnet100(gpu_ctx, monkeypatch):
    """The depth with the 58-layer run: uncapped, two chained launches (58 + 4 layers) for 62 per-layer ones."""
    P = _program(100, seed=22)
    d = _input(gpu_ctx, B0, seed=3)
    try:
        ref, ref_codes, _, _ = _run(gpu_ctx, monkeypatch, P, d, B0, UNCHAINED)
        got, codes, replay, chains = _run(gpu_ctx, monkeypatch, P, d, B0, CHAINED, cap=0, graph=True)
    finally:
        d.free()
    assert ref_codes.count(502) == 58 and ref_codes.count(505) == 4 and 300 not in ref_codes, ref_codes
    assert codes.count(300) == 2 and codes.count(301) == 60 and not {502, 505} & set(codes) and chains == 0, codes
    assert np.array_equal(got, ref) and np.array_equal(replay, ref)
