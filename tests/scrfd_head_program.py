"""A head-only SCRFD stand-in for the post-processing tests (tests/test_gpu_scrfd_nms.py).

pc_scrfd_detect needs a net with a DxD NHWC4 input ((x - 127.5) / 128, RGB) and three f32 outputs
at strides 8, 16 and 32 of 30 channels: cls(2) | bbox(8) | kps(20), two anchors per location
(models.compile_scrfd). This builds the smallest program.Program with that interface: a 3x3
stride-2 stem, four 16-channel 3x3 stride-2 convs (strides 4, 8, 16, 32) and one plain 1x1 f32
head per level, with the heads under the test's control:

* feature 0 of every level is a positive average of the frame (brightness), and both class logits
  rise with it: a black frame scores about 0.03, a mid-grey one about 0.62, a bright one higher;
* the bbox bias is `box` strides for all four distances, so boxes are about 2 * box strides wide
  (small boxes: thousands survive the NMS; large boxes: a few hundred);
* the other features are seeded random convs that spread logits, distances and landmarks per anchor.

The stride-8 receptive field is 15 px, so the interior anchors of a constant 64-px tile see
identical inputs: exact ties in score and box shape between neighbouring locations. With
shared=True anchor 1 of every location gets anchor 0's class and bbox weights (not its landmark
weights): two candidates of one score and one box, IoU 1, told apart by their landmarks alone.
"""
import ctypes as C

import numpy as np

from person_capture_amd import program as pg
from person_capture_amd._lib import PC_PREC_F32, LetterboxDesc, check
from person_capture_amd.engines import make_letterbox_desc
from person_capture_amd.runtime import Net

FEAT = 16
CLS_GAIN, CLS_BIAS, CLS_MIX = 4.0, 0.5, 0.45
BOX_MIX, KPT_MIX = 0.12, 0.25
FILL = 0xA5                                  # byte the driver prefills dets / kps with
GUARD = 64                                   # rows past the end of dets / kps, prefilled too


def _silu(x):
    return x / (1.0 + np.exp(-x))


def head_program(D: int, box: float = 2.0, seed: int = 0, shared: bool = False) -> pg.Program:
    assert D % 32 == 0
    rng = np.random.default_rng(seed)
    c, cp = FEAT, pg.cpad(FEAT)
    P = pg.Program()
    xin = P.input_tensor(D, D, 4)
    # stem: feature 0 = silu(2 * (mean of the 3x3 RGB window) + 2): 0 on black, silu(2) on mid-grey
    w4 = np.zeros((c, 3, 3, 4))
    w4[1:, :, :, :3] = rng.normal(0.0, np.sqrt(2.0 / 27.0), (c - 1, 3, 3, 3))
    w4[0, :, :, :3] = 2.0 / 27.0
    b4 = np.zeros(c)
    b4[0] = 2.0
    t = P.act(D // 2, D // 2, cp)
    P.stem(t, xin, w4, b4, stride=2, pad=1, act=pg.ACT_SILU)
    v0 = _silu(2.0)                  # feature 0 on a mid-grey frame, tracked per level
    heads = []
    for s in (4, 8, 16, 32):
        w = rng.normal(0.0, np.sqrt(2.0 / (9.0 * c)), (c, c, 3, 3))
        w[0] = 0.0
        w[0, 0] = 1.2 / 9.0
        y = P.act(D // s, D // s, cp)
        P.conv(y, [(t, 3, 3, 2, 1, c)], pg.pack_conv_weights([w], [cp], cp), c, bias=np.zeros(cp), act=pg.ACT_SILU)
        t = y
        v0 = _silu(1.2 * v0)
        if s == 4:
            continue
        wh = np.zeros((30, c, 1, 1))
        bh = np.zeros(30)
        wh[0:2, 0, 0, 0] = CLS_GAIN / v0
        wh[0:2, 1:, 0, 0] = rng.normal(0.0, CLS_MIX, (2, c - 1))
        bh[0:2] = CLS_BIAS - CLS_GAIN
        wh[2:10, 1:, 0, 0] = rng.normal(0.0, BOX_MIX, (8, c - 1))
        bh[2:10] = box
        wh[10:30, 1:, 0, 0] = rng.normal(0.0, KPT_MIX, (20, c - 1))
        if shared:
            wh[1] = wh[0]
            wh[6:10] = wh[2:6]
        npad = pg.cpad(30)
        o = P.act(D // s, D // s, npad, is_f32=1)
        P.conv(o, [(t, 1, 1, 1, 0, c)], pg.pack_conv_weights([wh], [cp], npad), 30, bias=pg.pad_vec(bh, npad),
               act=pg.ACT_NONE)
        heads.append(P.view(o, 0, 30))
    P.outputs = heads
    return P


# ---- frames (BGR u8) -----------------------------------------------------------
def noise_frame(H, W, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (H, W, 3), dtype=np.uint8)


def tiled_frame(H, W, seed, tile=64, lo=32, hi=224, levels=8):
    """Constant-colour tiles, each channel one of `levels` values in [lo, hi)."""
    rng = np.random.default_rng(seed)
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    vals = (lo + rng.integers(0, levels, (th, tw, 3)) * ((hi - lo) // levels)).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(vals, tile, axis=0), tile, axis=1)[:H, :W])


def dark_frame(H, W):
    return np.zeros((H, W, 3), np.uint8)


def split_frame(H, W, seed, bright_cols):
    """Noise in the first `bright_cols` columns, black in the rest: only the anchors of the bright
    part can reach a threshold well above the black score."""
    f = noise_frame(H, W, seed)
    f[:, bright_cols:] = 0
    return f


# ---- device driver -------------------------------------------------------------
class HeadEngine:
    """The head program at one D on the device, driven through pc_scrfd_detect as ScrfdEngine
    drives the real nets."""

    def __init__(self, ctx, D=640, box=2.0, seed=0, shared=False, max_batch=1):
        self.ctx, self.D, self.max_batch = ctx, D, max_batch
        self.program = head_program(D, box, seed, shared)
        self.net = Net(ctx, self.program.serialize(), precision=PC_PREC_F32, max_batch=max_batch)
        self.anchors = 2 * sum((D // s) ** 2 for s in (8, 16, 32))

    def detect(self, frames, det_thresh, nms_thresh, max_det):
        """One pc_scrfd_detect launch over `frames`. Returns per frame a dict: the whole dets
        [max_det][5] and kps [max_det][10] buffers (prefilled with FILL bytes before the call),
        count, ncand, det_scale and the device's three head tensors of this run; the last frame's
        dict also has "guard": the GUARD rows allocated past the end of both buffers."""
        n = len(frames)
        ctx = self.ctx
        descs, scales, srcs = [], [], []
        for fr in frames:
            fr = np.ascontiguousarray(fr)
            srcs.append(ctx.upload(fr))
            d, s = make_letterbox_desc(srcs[-1].ptr, fr.shape[0], fr.shape[1], fr.strides[0], self.D)
            descs.append(d)
            scales.append(s)
        arr = (LetterboxDesc * n)(*descs)
        sc = (C.c_float * n)(*[float(s) for s in scales])
        rows = n * max_det + GUARD
        dd = ctx.alloc(rows * 5 * 4)
        dk = ctx.alloc(rows * 10 * 4)
        dc = ctx.alloc(n * 4)
        dn = ctx.alloc(n * 4)
        ctx.memset(dd.ptr, FILL, rows * 5 * 4)
        ctx.memset(dk.ptr, FILL, rows * 10 * 4)
        ctx.memset(dc.ptr, FILL, n * 4)
        ctx.memset(dn.ptr, FILL, n * 4)
        check(ctx.lib.pc_scrfd_detect(self.net.handle, arr, n, self.D, C.c_float(det_thresh), C.c_float(nms_thresh),
                                      sc, max_det, C.c_void_p(dd.ptr), C.c_void_p(dk.ptr), C.c_void_p(dc.ptr),
                                      C.c_void_p(dn.ptr)), ctx.handle, "scrfd_detect")
        cnt = ctx.download(dc.ptr, (n,), np.int32)
        ncand = ctx.download(dn.ptr, (n,), np.int32)
        dets = ctx.download(dd.ptr, (rows, 5), np.float32)
        kps = ctx.download(dk.ptr, (rows, 10), np.float32)
        heads = [self.net.read_output(i, n) for i in range(3)]
        for b in (dd, dk, dc, dn, *srcs):
            b.free()
        out = [{"dets": dets[i * max_det:(i + 1) * max_det], "kps": kps[i * max_det:(i + 1) * max_det],
                "count": int(cnt[i]), "ncand": int(ncand[i]), "det_scale": float(np.float32(scales[i])),
                "heads": [h[i] for h in heads]} for i in range(n)]
        out[-1]["guard"] = (dets[n * max_det:], kps[n * max_det:])
        return out
