"""A head-only YOLOv8 stand-in for the post-processing tests (tests/test_gpu_yolo_nms.py).

pc_yolo_detect / pc_yolo_pose_detect need a net with a 4-channel [Hp][Wp] input and three f32
outputs at strides 8, 16 and 32 of 64 + nc (+ 3 nkpt) channels. This builds the smallest
program.Program with that interface: a 3x3 stride-2 stem, four 16-channel 3x3 stride-2 convs
(strides 4, 8, 16, 32) and one plain 1x1 f32 head per level, nc = 1, so every anchor is a
class-0 candidate and the heads are under the test's control:

* box: the DFL bias profile peaks at `box` bins, so boxes are about 2 * box strides wide
  (small boxes: thousands survive the NMS; large boxes: a few hundred);
* feature 0 of every level is a positive average of the frame (brightness), and the class
  logit rises with it: a bright region scores high, a black one about 0.03; the other
  features are seeded random convs that spread logits, DFL bins and keypoints per anchor.

The stride-8 receptive field is 15 px, so the interior anchors of a constant 64-px tile see
identical inputs: exact ties in score and box shape.
"""
import ctypes as C

import numpy as np

from person_capture_amd import models_yolo as my
from person_capture_amd import program as pg
from person_capture_amd._lib import PC_PREC_F32, YoloLetterboxDesc, YoloScale, check
from person_capture_amd.engines import opencv_vresize_simd_end
from person_capture_amd.runtime import Net

FEAT = 16
CLS_GAIN, CLS_BIAS, CLS_MIX = 4.0, 0.5, 0.45
DFL_SHARP, DFL_MIX = 1.2, 0.12
KPT_MIX = 0.25


def _silu(x):
    return x / (1.0 + np.exp(-x))


def head_program(Hp: int, Wp: int, nkpt: int = 0, box: float = 1.0, seed: int = 0) -> pg.Program:
    assert Hp % 32 == 0 and Wp % 32 == 0
    rng = np.random.default_rng(seed)
    c, cp = FEAT, pg.cpad(FEAT)
    P = pg.Program()
    xin = P.input_tensor(Hp, Wp, 4)
    # stem: feature 0 = silu(4 * mean RGB of the 3x3 window), the rest random
    w4 = np.zeros((c, 3, 3, 4))
    w4[1:, :, :, :3] = rng.normal(0.0, np.sqrt(2.0 / 27.0), (c - 1, 3, 3, 3))
    w4[0, :, :, :3] = 4.0 / 27.0
    t = P.act(Hp // 2, Wp // 2, cp)
    P.stem(t, xin, w4, np.zeros(c), stride=2, pad=1, act=pg.ACT_SILU)
    v0 = _silu(4.0 * 0.5)            # feature 0 on a mid-grey frame, tracked per level
    heads = []
    for lvl, s in enumerate((4, 8, 16, 32)):
        w = rng.normal(0.0, np.sqrt(2.0 / (9.0 * c)), (c, c, 3, 3))
        w[0] = 0.0
        w[0, 0] = 1.2 / 9.0
        y = P.act(Hp // s, Wp // s, cp)
        P.conv(y, [(t, 3, 3, 2, 1, c)], pg.pack_conv_weights([w], [cp], cp), c, bias=np.zeros(cp), act=pg.ACT_SILU)
        t = y
        v0 = _silu(1.2 * v0)
        if s == 4:
            continue
        ctot = 64 + 1 + 3 * nkpt
        wh = np.zeros((ctot, c, 1, 1))
        bh = np.zeros(ctot)
        wh[:64, 1:, 0, 0] = rng.normal(0.0, DFL_MIX, (64, c - 1))
        bh[:64] = np.tile(-DFL_SHARP * np.abs(np.arange(16) - box), 4)
        wh[64, 0, 0, 0] = CLS_GAIN / v0
        wh[64, 1:, 0, 0] = rng.normal(0.0, CLS_MIX, c - 1)
        bh[64] = CLS_BIAS - CLS_GAIN
        wh[65:, 1:, 0, 0] = rng.normal(0.0, KPT_MIX, (3 * nkpt, c - 1))
        npad = pg.cpad(ctot)
        o = P.act(Hp // s, Wp // s, npad, is_f32=1)
        P.conv(o, [(t, 1, 1, 1, 0, c)], pg.pack_conv_weights([wh], [cp], npad), ctot, bias=pg.pad_vec(bh, npad),
               act=pg.ACT_NONE)
        heads.append(P.view(o, 0, ctot))
    P.outputs = heads
    return P


# ---- frames (BGR u8) -----------------------------------------------------------
def noise_frame(H, W, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (H, W, 3), dtype=np.uint8)


def tiled_frame(H, W, seed, tile=64, lo=96, hi=256, levels=8):
    """Constant-colour tiles, each channel one of `levels` values in [lo, hi)."""
    rng = np.random.default_rng(seed)
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    vals = (lo + rng.integers(0, levels, (th, tw, 3)) * ((hi - lo) // levels)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(vals, tile, axis=0), tile, axis=1)[:H, :W])


def split_frame(H, W, seed, strip):
    """Noise with the last `strip` rows black: their anchors score lowest and no box of the
    bright part reaches far into them."""
    f = noise_frame(H, W, seed)
    f[H - strip:] = 0
    return f


def dark_frame(H, W):
    return np.zeros((H, W, 3), np.uint8)


# ---- device driver -------------------------------------------------------------
class HeadEngine:
    """The head program at one canvas on the device, driven through pc_yolo_detect /
    pc_yolo_pose_detect as the detectors drive the real nets."""

    def __init__(self, ctx, Hp, Wp, nkpt=0, box=1.0, seed=0, max_batch=1):
        self.ctx, self.Hp, self.Wp, self.nkpt, self.max_batch = ctx, Hp, Wp, nkpt, max_batch
        self.program = head_program(Hp, Wp, nkpt, box, seed)
        self.net = Net(ctx, self.program.serialize(), precision=PC_PREC_F32, max_batch=max_batch)

    def detect(self, frames, imgsz, conf, iou, max_det):
        """Returns per frame a dict: dets [k][5], kpts [k][nkpt][3] or None, count, ncand and the
        device's three head tensors of this run."""
        n = len(frames)
        ctx = self.ctx
        d = (YoloLetterboxDesc * n)()
        sc = (YoloScale * n)()
        kpad = (C.c_float * (2 * n))()
        srcs = []
        for i, fr in enumerate(frames):
            H, W = fr.shape[:2]
            new_w, new_h, top, left, Hp, Wp = my.letterbox_geometry(H, W, imgsz)
            assert (Hp, Wp) == (self.Hp, self.Wp)
            fr = np.ascontiguousarray(fr)
            srcs.append(ctx.upload(fr))
            d[i].d_src, d[i].H, d[i].W, d[i].row_stride = srcs[-1].ptr, H, W, fr.strides[0]
            d[i].new_w, d[i].new_h, d[i].top, d[i].left = new_w, new_h, top, left
            d[i].scale_x, d[i].scale_y = 1.0 / (float(new_w) / W), 1.0 / (float(new_h) / H)
            d[i].simd_end = opencv_vresize_simd_end(new_w * 3)
            d[i].identity = 1 if (new_w, new_h) == (W, H) else 0
            gain, px, py = my.scale_geometry(Hp, Wp, H, W)
            sc[i].gain, sc[i].pad_x, sc[i].pad_y, sc[i].W0, sc[i].H0 = gain, float(px), float(py), float(W), float(H)
            kpad[2 * i], kpad[2 * i + 1] = (Wp - W * gain) / 2, (Hp - H * gain) / 2
        dd = ctx.alloc(n * max_det * 5 * 4)
        dc = ctx.alloc(n * 4)
        dn = ctx.alloc(n * 4)
        ctx.memset(dd.ptr, 0xFF, n * max_det * 5 * 4)
        if self.nkpt:
            dk = ctx.alloc(n * max_det * self.nkpt * 3 * 4)
            check(ctx.lib.pc_yolo_pose_detect(self.net.handle, d, n, self.Hp, self.Wp, C.c_float(conf), C.c_float(iou),
                                              sc, kpad, max_det, self.nkpt, C.c_void_p(dd.ptr), C.c_void_p(dk.ptr),
                                              C.c_void_p(dc.ptr), C.c_void_p(dn.ptr)), ctx.handle, "yolo_pose_detect")
        else:
            check(ctx.lib.pc_yolo_detect(self.net.handle, d, n, self.Hp, self.Wp, C.c_float(conf), C.c_float(iou), sc,
                                         max_det, C.c_void_p(dd.ptr), C.c_void_p(dc.ptr), C.c_void_p(dn.ptr)),
                  ctx.handle, "yolo_detect")
        cnt = ctx.download(dc.ptr, (n,), np.int32)
        ncand = ctx.download(dn.ptr, (n,), np.int32)
        dets = ctx.download(dd.ptr, (n, max_det, 5), np.float32)
        kp = ctx.download(dk.ptr, (n, max_det, self.nkpt, 3), np.float32) if self.nkpt else None
        heads = [self.net.read_output(i, n) for i in range(3)]
        out = []
        for i in range(n):
            k = int(cnt[i])
            assert 0 <= k <= max_det
            out.append({"dets": dets[i, :k].copy(), "kpts": kp[i, :k].copy() if self.nkpt else None, "count": k,
                        "ncand": int(ncand[i]), "heads": [h[i] for h in heads]})
        return out
