"""The network planner on the CPU (pc_net_plan: decode, validate and plan a program under the current
environment, no device): malformed programs are refused with PC_ERR_FORMAT, and the kernel choices that
carry the bit-identity contract of the plan classes are the documented ones.

A plan record is (op kind, kernel code, form, K-row bytes, split-K, igemm cfg); code and form are what
pc_net_profile_ops reports for a per-layer launch (pcgpu.h)."""
import ctypes as C

import numpy as np
import pytest

from person_capture_amd import _lib, models
from person_capture_amd import program as pg
from person_capture_amd._lib import PC_PREC_F16
from plan_geometry_cases import geometry_cases as _geometry_cases
from plan_geometry_cases import valid_geometry_programs as _valid_geometry_programs

PC_ERR_FORMAT = 4   # pcgpu.h
KIND, CODE, FORM, ROWB, SPLITK, CFG = range(6)
# channel tile of every igemm cfg (pc_conv.hip launch_rowb)
CFG_BC = [128, 128, 64, 64, 96, 32, 32, 128, 256, 256, 64, 96, 32, 128]


def _plan(blob, max_batch, prec=PC_PREC_F16, nbytes=None):
    """-> (class batch sizes, plans[class][op][6]) with class 0 the max-batch plan, or (-status, message)."""
    lib = _lib.load()
    words = np.frombuffer(blob, np.int32, 8)
    nops = int(words[5])
    cls = np.zeros(16, np.int32)
    plans = np.zeros((17, max(nops, 1), 6), np.int32)
    err = C.create_string_buffer(256)
    i32p = C.POINTER(C.c_int32)
    k = lib.pc_net_plan(blob, len(blob) if nbytes is None else nbytes, prec, max_batch, cls.ctypes.data_as(i32p), 16,
                        plans.ctypes.data_as(i32p), max(nops, 1), err, 256)
    if k < 0:
        return k, err.value.decode()
    return [int(b) for b in cls[:k - 1]], plans[:k, :nops]


# ---- malformed programs ---------------------------------------------------------------------------
def _two_convs():
    P = pg.Program()
    x = P.input_tensor(16, 16, 64)
    y = P.act(16, 16, 64)
    z = P.act(16, 16, 64)
    rng = np.random.default_rng(0)
    for a, b in ((x, y), (y, z)):
        w = pg.pack_conv_weights([rng.standard_normal((64, 64, 3, 3)) * 0.05], [64], 64)
        P.conv(b, [(a, 3, 3, 1, 1, 64)], w, 64, bias=np.zeros(64), act=pg.ACT_RELU)
    P.outputs = [z]
    return P.serialize(), (x, y, z)


def _ops_at(blob):
    h = np.frombuffer(blob, np.int32, 8)
    return 8 + int(h[2]) * 4 + int(h[3]) * 8 + int(h[4]) * 4 + int(h[6])


def _edit(blob, op, edits=None, record=None):
    w = np.frombuffer(blob, np.int32).copy()
    at = _ops_at(blob) + 32 * op
    if record is not None:
        w[at:at + 32] = 0
        w[at:at + len(record)] = record
    for k, v in (edits or {}).items():
        w[at + k] = v
    return w.tobytes()


def test_valid_base_program_plans():
    blob, _ = _two_convs()
    cls, plans = _plan(blob, 8)
    assert cls == [1] and plans.shape == (2, 2, 6) and (plans[:, :, KIND] == pg.OP_CONV).all()
    assert (plans[:, :, SPLITK] == 1).all()


BAD = 99   # no such tensor / array


def _malformed_cases():
    blob, (x, y, z) = _two_convs()
    eps = int(np.float32(1e-5).view(np.int32))
    return {
        "conv_input_tensor": _edit(blob, 1, {3: BAD}),
        "conv_output_tensor": _edit(blob, 1, {1: BAD}),
        "conv_residual_tensor": _edit(blob, 1, {21: BAD, 22: pg.RES_SAME}),
        "conv_negative_tensor": _edit(blob, 1, {3: -2}),
        "stem_tensor": _edit(blob, 1, record=[pg.OP_STEM, z, BAD, 3, 3, 1, 1, 0, 64, 1, -1, 0, 64, 3]),
        "maxpool_tensor": _edit(blob, 1, record=[pg.OP_MAXPOOL, BAD, y, 3, 1, 1]),
        "upsample_tensor": _edit(blob, 1, record=[pg.OP_UPSAMPLE, z, BAD]),
        "layernorm_tensor": _edit(blob, 1, record=[pg.OP_LAYERNORM, BAD, y, 1, 1, -1, 0, eps, 64]),
        "attention_tensor": _edit(blob, 1, record=[pg.OP_ATTENTION, z, BAD, 1, 64]),
        "conv_weight_array": _edit(blob, 0, {13: 999}),
        "conv_bias_array": _edit(blob, 0, {17: 999}),
        "layernorm_array": _edit(blob, 1, record=[pg.OP_LAYERNORM, z, y, 999, 1, -1, 0, eps, 64]),
        "nseg_3": _edit(blob, 0, {2: 3}),
        "nseg_0": _edit(blob, 0, {2: 0}),
        "unknown_kind": _edit(blob, 1, {0: 77}),
        "negative_splitk": _edit(blob, 1, {24: -4}),
    }


@pytest.mark.parametrize("name", sorted(_malformed_cases()))
def test_malformed_program_is_refused(name):
    k, msg = _plan(_malformed_cases()[name], 8)
    assert k == -PC_ERR_FORMAT, (k, msg)
    assert msg


# ---- geometry the kernels would follow outside their tensors (plan_geometry_cases.py) ---------------
@pytest.mark.parametrize("name", sorted(_valid_geometry_programs()))
def test_geometry_bases_plan(name):
    """The programs the geometry cases below are cut from are themselves accepted."""
    r = _plan(_valid_geometry_programs()[name].serialize(), 4)
    assert not isinstance(r[0], int), r


@pytest.mark.parametrize("name", sorted(_geometry_cases()))
def test_bad_geometry_is_refused(name):
    P, words = _geometry_cases()[name]
    k, msg = _plan(P.serialize(), 4)
    assert k == -PC_ERR_FORMAT, (k, msg)
    assert msg and words in msg, msg


# ---- every program the project compiles is accepted --------------------------------------------------
def _project_programs():
    """(name, build) of every compiler's programs, synthetic weights: plain / split / c8 where the family has
    them, and the op-level programs of net_op_cases.py. Built on demand (the towers' weights are large)."""
    from person_capture_amd import models_clip as mc
    from person_capture_amd import models_yolo as my
    out = []
    for depth in (18, 50, 100):
        for kw in ({}, {"split": True}, {"c8": True}):
            out.append((f"iresnet{depth}-{'-'.join(kw) or 'plain'}",
                        lambda depth=depth, kw=kw: models.compile_iresnet(models.synth_iresnet(depth, seed=0, calibrate=False), depth, **kw)))
    for v in ("2.5g", "10g"):
        for D in (320, 640):
            for split in (False, True):
                out.append((f"scrfd{v}-{D}-{'split' if split else 'plain'}",
                            lambda v=v, D=D, split=split: models.compile_scrfd(models.synth_scrfd(v, seed=0, calibrate=False), v, D, split=split)))
    out.append(("yolov8n", lambda: my.compile_yolov8(my.synth_yolov8("n", seed=0, calibrate=False), "n", 384, 640)))
    out.append(("yolov8n-face", lambda: my.compile_yolov8(my.synth_yolov8_face("n", seed=0, calibrate=False), "n", 384, 640,
                                                          nc=1, kpt=(5, 3))))
    for name in sorted(mc.CLIP_CFGS):
        if mc.CLIP_CFGS[name]["layers"] > 2:
            continue      # the family's full-depth rows: the -d2 rows are the same shapes per layer
        for split in (False, True):
            out.append((f"{name}-{'split' if split else 'plain'}",
                        lambda name=name, split=split: mc.compile_clip_vit(mc.synth_clip_vit(name, seed=0), name, split=split)))
    return out


@pytest.mark.parametrize("name", [n for n, _ in _project_programs()])
def test_every_compiled_program_plans(name):
    P = dict(_project_programs())[name]()
    precs = [PC_PREC_F16] if P.split else [PC_PREC_F16, _lib.PC_PREC_F32]
    for prec in precs:
        r = _plan(P.serialize(), 8, prec)
        assert not isinstance(r[0], int), (name, prec, r)


def test_every_op_level_program_plans():
    import net_op_cases as nc
    for case in nc.all_cases():
        r = _plan(case.P.serialize(), 4, _lib.PC_PREC_F32 if case.f32 else PC_PREC_F16)
        assert not isinstance(r[0], int), (case.name, r)


def test_truncated_op_table_is_refused():
    blob, _ = _two_convs()
    k, msg = _plan(blob, 8, nbytes=(_ops_at(blob) + 32 + 7) * 4)   # ends inside the second record
    assert k == -PC_ERR_FORMAT and "truncated" in msg


# ---- IResNet-100 f16x3 ----------------------------------------------------------------------------
HXI = {502: 58, 503: 24, 505: 4}      # conv_hxi 14x14x256 / 28x28x128 / 7x7x512 layers
HXI_SMALL = {502: 506, 503: 507, 505: 508}


@pytest.fixture(scope="module")
def r100x3():
    return models.compile_iresnet(models.synth_iresnet(100, seed=0, calibrate=False), 100, split=True).serialize()


def test_iresnet100_x3_classes_and_hxi(r100x3, monkeypatch):
    monkeypatch.delenv("PC_CONV_HXI", raising=False)
    cls, plans = _plan(r100x3, 512)
    assert cls == [1, 4, 16, 32, 64, 128, 256]
    top = plans[0]
    for code, n in HXI.items():
        assert int((top[:, CODE] == code).sum()) == n, code
    # the <= 32-image classes run those ops on the small-batch forms
    for c, b in enumerate(cls, start=1):
        if b > 32:
            continue
        for code, small in HXI_SMALL.items():
            assert (plans[c][top[:, CODE] == code, CODE] == small).all(), (b, code)


def test_iresnet100_x3_hxi_off(r100x3, monkeypatch):
    monkeypatch.setenv("PC_CONV_HXI", "0")
    _, plans = _plan(r100x3, 512)
    assert not np.isin(plans[:, :, CODE], [502, 503, 505, 506, 507, 508]).any()


# ---- SCRFD-10G f16x3 ------------------------------------------------------------------------------
def test_scrfd10g_x3_neck_convs():
    P = models.compile_scrfd(models.synth_scrfd("10g", seed=0, calibrate=False), "10g", 640, split=True)
    cls, plans = _plan(P.serialize(), 64)
    assert cls == [1, 4, 16]
    neck = [i for i, w in enumerate(P.ops)
            if w[0] == pg.OP_CONV and w[2] == 1 and w[4] == 3 and w[5] == 3 and w[6] == 1 and
            P.dims(w[3]) == (20, 20, 224) and P.dims(w[1]) == (20, 20, 224)]
    assert neck
    for c in (1, 2, 3):
        assert (plans[c][neck, CODE] == 504).all(), plans[c][neck]
    assert ((plans[0][neck, CODE] >= 100) & (plans[0][neck, CODE] < 200) & (plans[0][neck, FORM] & 1 == 1)).all()


# ---- the PC_CONV_CFG cascade ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_nets():
    return [(models.compile_scrfd(models.synth_scrfd("2.5g", seed=0, calibrate=False), "2.5g", 320), 64),
            (models.compile_iresnet(models.synth_iresnet(50, seed=0, calibrate=False), 50), 256)]


@pytest.mark.parametrize("k", range(14))
def test_forced_igemm_cfg_disables_the_other_kernels(plain_nets, monkeypatch, k):
    for name in ("PC_CONV_HALO", "PC_CONV_FAST", "PC_CONV_T2D", "PC_CONV_HX"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("PC_CONV_CFG", str(k))
    forced = 0
    for P, max_batch in plain_nets:
        _, plans = _plan(P.serialize(), max_batch)
        convs = [i for i, w in enumerate(P.ops) if w[0] == pg.OP_CONV]
        fits = [i for i in convs if P.ops[i][14] % CFG_BC[k] == 0]
        forced += len(fits)
        for pl in plans:
            assert (pl[convs, CODE] == -1).all()          # igemm: not halo / fast / t2d / hx / chain
            assert (pl[fits, CFG] == k).all() and (pl[fits, FORM] == k).all()
    assert forced   # (the tile divides some conv's npad in one of the nets)


# ---- f16c8 IResNet --------------------------------------------------------------------------------
def _family(code, form):
    """The K order a conv accumulates in: the fused split tiles' (conv_fast SX / C8 and the halo kernels,
    which walk K in their order), t2d's, or the plain tiles' virtual [hi, lo, hi] blocks."""
    if code >= 500 or (100 <= code < 200 and form & 1):
        return "fused"
    return "t2d" if 200 <= code < 300 else "plain"


@pytest.fixture(scope="module")
def r50c8():
    return models.compile_iresnet(models.synth_iresnet(50, seed=0, calibrate=False), 50, c8=True)


@pytest.mark.parametrize("rowb", [None, "64", "128"])
def test_iresnet_c8_one_row_width_and_family(r50c8, monkeypatch, rowb):
    if rowb is None:
        monkeypatch.delenv("PC_C8_ROWB", raising=False)
    else:
        monkeypatch.setenv("PC_C8_ROWB", rowb)
    P = r50c8
    cls, plans = _plan(P.serialize(), 512)
    assert len(cls) >= 5
    c8_convs = [i for i, w in enumerate(P.ops) if w[0] == pg.OP_CONV and P.tc8[w[3]]]
    assert c8_convs
    assert (plans[:, c8_convs, ROWB] == (128 if rowb == "128" else 64)).all()
    assert ((plans[:, c8_convs, CODE] >= 600) & (plans[:, c8_convs, CODE] < 700)).all()
    split_convs = [i for i, w in enumerate(P.ops) if w[0] == pg.OP_CONV and P.tsplit[w[3]]]
    for i in split_convs:
        fam = {_family(int(pl[i, CODE]), int(pl[i, FORM])) for pl in plans}
        assert len(fam) == 1, (i, fam)
        if plans[0][i, SPLITK] == 1:
            assert fam == {"fused"}, (i, fam)
