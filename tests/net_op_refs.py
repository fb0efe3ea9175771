"""float64 references of the network's non-GEMM ops (pc_conv.hip max pools, pc_ops.hip upsample /
LayerNorm, the three attention kernels) - plain NumPy, no torch, no device.

Every function takes NHWC arrays holding the values as the device stores them (f16 and f32 values
are exact in f64) and returns f64. tests/test_net_op_refs_cpu.py checks them against torch in f64."""
import numpy as np


def maxpool(x, k, s, p):
    """[N][H][W][C] -> [N][OH][OW][C], OH = (H + 2p - k) // s + 1; padding never wins (-inf)."""
    x = np.asarray(x, np.float64)
    N, H, W, C = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.full((N, H + 2 * p, W + 2 * p, C), -np.inf)
    xp[:, p:p + H, p:p + W] = x
    y = np.full((N, OH, OW, C), -np.inf)
    for kh in range(k):
        for kw in range(k):
            y = np.maximum(y, xp[:, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s])
    return y


def upsample2(x):
    """Nearest-neighbour x2: y[n, oh, ow] = x[n, oh // 2, ow // 2]."""
    x = np.asarray(x, np.float64)
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def layernorm(x, C, gamma, beta, eps, add=None):
    """LayerNorm over channels [0, C) of every pixel of x [N][H][W][>= C]: two-pass, population variance.
    add [H*W][C] (the positional table, one row per pixel of an image) is added first. -> [N][H][W][C]."""
    x = np.asarray(x, np.float64)[..., :C]
    N, H, W, _ = x.shape
    if add is not None:
        x = x + np.asarray(add, np.float64).reshape(1, H, W, C)
    mean = x.sum(-1, keepdims=True) / C
    d = x - mean
    var = (d * d).sum(-1, keepdims=True) / C
    return d / np.sqrt(var + np.float64(np.float32(eps))) * np.asarray(gamma, np.float64)[:C] + np.asarray(beta, np.float64)[:C]


def attention(qkv, heads, d):
    """qkv [N][T][>= 3E], E = heads * d: q | k | v, head-major inside each -> [N][T][E],
    softmax(q k^T / sqrt(d)) v per (image, head), the softmax max-subtracted."""
    qkv = np.asarray(qkv, np.float64)
    N, T = qkv.shape[:2]
    E = heads * d
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(N, T, heads, d).transpose(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(0, 1, 3, 2)) / np.sqrt(np.float64(d))
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    o = (e / e.sum(-1, keepdims=True)) @ v
    return o.transpose(0, 2, 1, 3).reshape(N, T, E)


def split(v):
    """The f16x3 storage rule: hi = f16(v), lo = f16(v - hi), of the f32 value v. -> (hi, lo) as f16."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def unsplit(hi, lo):
    """hi + lo in f64 (exact)."""
    return np.asarray(hi, np.float64) + np.asarray(lo, np.float64)
