"""The smallest programs that reach each non-GEMM kernel of the net executor, with their inputs and
their float64 expectations (net_op_refs.py). Shared by the CPU checks of the references and of the
planner (test_net_op_refs_cpu.py, test_plan_cpu.py) and by the device tests (test_gpu_net_ops.py,
test_gpu_attention_edges.py).

A case is a Case: the Program, the net's element type, the input as the device stores it, and per
program output the expected logical values [N][H][W][C] in f64 (a split tensor's C counts one half;
channel padding the op promises to zero is part of the expectation), plus what the case's own test
needs (bounds, per-(image, head) kinds).

Direct programs: the op reads the net input and writes a program output, so the error is the op's
alone. Where a fully written buffer is needed (concatenation buffers, views, split inputs) an exact
1x1 identity conv of the input fills it: every product is a value times 1 (or 2^-12) and at most two
terms are non-zero, so the f32 accumulation is exact in any order."""
import numpy as np

import net_op_refs as R
from person_capture_amd import program as pg

U = 2.0 ** -24          # f32 unit roundoff
LO = 2.0 ** -12         # weight of the second input half in a split program's identity conv


class Case:
    def __init__(self, name, P, f32, x, exp, **kw):
        self.name, self.P, self.f32, self.x, self.exp = name, P, f32, x, exp
        self.__dict__.update(kw)

    @property
    def N(self):
        return self.x.shape[0]

    def storage(self):
        """The input in the net's element type."""
        return np.ascontiguousarray(self.x, np.float32 if self.f32 else np.float16)


def ident(P, out, x, C, stride=1, lo=None, scale=1.0):
    """Exact 1x1 conv: out[c] = scale * x[c] (+ 2^-12 * x[lo + c]), c < C; x is the plain net input."""
    cp = P.dims(x)[2]
    w = np.zeros((pg.cpad(C), cp), np.float32)
    w[np.arange(C), np.arange(C)] = scale
    if lo is not None:
        w[np.arange(C), lo + np.arange(C)] = LO
    P.conv(out, [(x, 1, 1, stride, 0, cp)], w, C)


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def lo_part(rng, shape):
    """The second input half of a split program: multiples of 1/8 in [-1, 1]; times 2^-12 it sits below
    the f16 ulp of every first-half value >= 2^-2 in magnitude, and a + 2^-12 b is exact in f32."""
    return rng.integers(-8, 9, shape) / 8.0


# ---- max pool --------------------------------------------------------------------------------------
POOL_GEOMS = [(7, 5, 3, 2, 1), (9, 6, 5, 1, 2), (6, 4, 2, 2, 0), (1, 1, 3, 2, 1)]   # H, W, k, s, p
POOL_DATA = ["negative", "mixed", "corner"]
# f32: maxpool_nhwc<float>; f16c32: maxpool_nhwc_f16x8; f16c12 (8 does not divide C) and f16view (a view 8
# bytes into a 16-byte vector) fail maxpool_launch's vector test: maxpool_nhwc<f16>; split: maxpool_split_f16x8
POOL_FORMS = ["f32", "f16c32", "f16c12", "f16view", "split"]


def pool_values(rng, shape, data):
    """Multiples of 1/64 with 1 <= |v| <= 4 (exact in f16, never 0); 'corner': the per-channel maximum of
    every image sits in pixel (H - 1, 0)."""
    v = rng.integers(64, 257, shape) / 64.0
    if data == "negative":
        return -v
    v = v * rng.choice([-1.0, 1.0], shape)
    if data == "corner":
        v[:, -1, 0, :] = 5.0 + (np.arange(shape[3]) % 4) * 0.25
    return v


def pool_case(form, geom, data, N=3):
    H, W, k, s, p = geom
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    rng = np.random.default_rng([11, POOL_FORMS.index(form), H, k, POOL_DATA.index(data)])
    name = f"pool-{form}-{H}x{W}k{k}s{s}p{p}-{data}"
    if form in ("f32", "f16c32", "f16c12"):
        C = {"f32": 8, "f16c32": 32, "f16c12": 12}[form]
        xv = pool_values(rng, (N, H, W, C), data)
        P = pg.Program()
        x = P.input_tensor(H, W, C)
        y = P.act(OH, OW, C)
        P.maxpool(y, x, k, s, p)
        P.outputs = [y]
        return Case(name, P, form == "f32", xv, [R.maxpool(xv, k, s, p)])
    if form == "f16view":
        xv = pool_values(rng, (N, H, W, 32), data)
        P = pg.Program()
        x = P.input_tensor(H, W, 32)
        Z = P.act(H, W, 32)
        ident(P, Z, x, 32)
        y = P.act(OH, OW, 8)
        P.maxpool(y, P.view(Z, 4, 8), k, s, p)
        P.outputs = [y, Z]
        return Case(name, P, False, xv, [R.maxpool(xv[..., 4:12], k, s, p), xv])
    assert form == "split"
    a, b = pool_values(rng, (N, H, W, 32), data), lo_part(rng, (N, H, W, 32))
    P = pg.Program(split=True)
    x = P.input_tensor(H, W, 64)
    e = P.act(H, W, 32)
    ident(P, e, x, 32, lo=32)
    y = P.act(OH, OW, 32)
    P.maxpool(y, e, k, s, p)
    P.outputs = [y, e]
    v = a + b * LO
    return Case(name, P, False, np.concatenate([a, b], -1), [R.maxpool(v, k, s, p), v])


def sppf_case(N=3):
    """SPPF: three k5 s1 p2 pools, each from slice j into slice j + 1 of one 4 x 32-channel buffer."""
    H, W = 9, 6
    xv = pool_values(np.random.default_rng(12), (N, H, W, 32), "mixed")
    P = pg.Program()
    x = P.input_tensor(H, W, 32)
    Z = P.act(H, W, 128)
    ident(P, P.view(Z, 0, 32), x, 32)
    exp = [xv]
    for j in range(3):
        P.maxpool(P.view(Z, 32 * (j + 1), 32), P.view(Z, 32 * j, 32), 5, 1, 2)
        exp.append(R.maxpool(exp[-1], 5, 1, 2))
    P.outputs = [Z]
    return Case("pool-sppf", P, False, xv, [np.concatenate(exp, -1)])


def pool_cases():
    return [pool_case(f, g, d) for f in POOL_FORMS for g in POOL_GEOMS for d in POOL_DATA] + [sppf_case()]


# ---- upsample --------------------------------------------------------------------------------------
def _up_values(rng, shape):
    return rng.integers(-512, 513, shape) / 64.0 + 1.0 / 128


def up_direct_case(f32, C, H, W, N=3, coff=0, cin=None):
    """Input (a view at channel offset coff of a cin-wide net input) -> its own output tensor."""
    cin = cin or C
    xv = _up_values(np.random.default_rng([13, C, H, coff, int(f32)]), (N, H, W, cin))
    P = pg.Program()
    x = P.input_tensor(H, W, cin)
    y = P.act(2 * H, 2 * W, C)
    P.upsample2(y, P.view(x, coff, C) if (coff or cin != C) else x)
    P.outputs = [y]
    return Case(f"up-{'f32' if f32 else 'f16'}-c{C}-{H}x{W}" + (f"-from{coff}of{cin}" if cin != C else ""), P, f32, xv,
                [R.upsample2(xv[..., coff:coff + C])])


def up_into_view_case(f32, N=3):
    """40 channels of a 3x5 map (a stride-2 identity conv of the input) into the view at offset 32 of a
    96-channel 6x10 buffer the identity conv wrote before: its other 56 channels come back unchanged.
    N * 4 * 15 * (40 / V) threads: no multiple of 256 in either type."""
    xv = _up_values(np.random.default_rng([14, int(f32)]), (N, 6, 10, 96))
    P = pg.Program()
    x = P.input_tensor(6, 10, 96)
    Z = P.act(6, 10, 96)
    ident(P, Z, x, 96)
    S = P.act(3, 5, 40)
    ident(P, S, x, 40, stride=2)
    P.upsample2(P.view(Z, 32, 40), S)
    P.outputs = [Z]
    exp = xv.copy()
    exp[..., 32:72] = R.upsample2(xv[:, ::2, ::2, :40])
    return Case(f"up-{'f32' if f32 else 'f16'}-into-view", P, f32, xv, [exp])


def upsample_cases():
    return [up_direct_case(False, 8, 3, 5), up_direct_case(False, 40, 1, 1), up_direct_case(False, 40, 3, 5),
            up_direct_case(True, 4, 3, 5), up_direct_case(True, 4, 1, 1), up_direct_case(False, 8, 3, 5, coff=8, cin=24),
            up_direct_case(True, 4, 3, 5, coff=8, cin=24), up_into_view_case(False), up_into_view_case(True)]


# ---- LayerNorm -------------------------------------------------------------------------------------
# layernorm_launch takes the `vec` kernel when V | C, V | both pixel strides (V = 4 floats / 8 halves per
# 16 bytes), C / V <= 64 * LN_NIT and every pointer is 16-byte aligned; else the `rows` kernel.
#   (form, C, input width, output width)                      kernel
LN_SHAPES = [
    ("f32", 32, 32, 32),          # layernorm_vec<float>: 8 of 64 lanes hold a vector
    ("f32", 1280, 1280, 1280),    # layernorm_vec<float>: five vector rounds (ViT-H)
    ("f32", 2048, 2048, 2048),    # layernorm_vec<float>: the limit, all eight rounds full
    ("f32", 104, 128, 128),       # layernorm_vec<float>: zero tail [104, 128)
    ("f32", 50, 64, 64),          # layernorm_rows<float>: 4 does not divide 50
    ("f16", 32, 32, 32),          # layernorm_vec<f16>
    ("f16", 1024, 1024, 1024),    # layernorm_vec<f16>: two vector rounds
    ("f16", 104, 128, 128),       # layernorm_vec<f16>: zero tail
    ("f16", 100, 128, 128),       # layernorm_rows<f16>: 8 does not divide 100
    ("split", 104, 128, 128),     # layernorm_vec<f16, SP>: zero tail in both halves
]
LN_KINDS = ["normal", "mean100", "spike", "constant", "normal"]
LN_PAD = 1e4     # what the input's channels beyond C hold when the input is the net input


def _ln_rows(rng, form, kind, C):
    """One token's C values as stored (f32, or exact in f16) and, for the split form, its second half."""
    b = np.zeros(C)
    if kind == "constant":
        return np.full(C, 3.0), b
    if kind == "mean100":     # spread 0.1 in f32 storage; steps of 0.25 (exact at 100 in f16) in f16 storage
        a = 100.0 + (0.1 * rng.standard_normal(C) if form == "f32" else 0.25 * rng.integers(-4, 5, C))
        return np.asarray(a, np.float32).astype(np.float64), lo_part(rng, C) if form == "split" else b
    a = rng.standard_normal(C)
    if kind == "spike":
        a[3] = 1000.0 * (1.0 + abs(a[3]))
        return (np.asarray(a, np.float32).astype(np.float64) if form == "f32" else f16r(a)), b
    a = np.asarray(a, np.float32).astype(np.float64) if form == "f32" else f16r(a)
    return a, lo_part(rng, C) if form == "split" else b


def ln_bound(xs, C, gamma, beta, eps, form):
    """|device - f64 reference| per element of a token's row xs (f64, after the table was added).

    The kernels (pc_ops.hip layernorm_vec / layernorm_rows) compute, in f32 with u = 2^-24:
      s = sum x (per lane at most ceil(C / 64) sequential adds, then 6 butterfly levels), mean = s / C:
        |mean - mean*| <= (D + 1) u A with D = ceil(C / 64) + 6 the adds on the longest path and
        A = max |x|; the table add rounds each x once more: u A.  -> dm = (D + 2) u A
      d = x - mean (u |d| each), q = sum d^2 (all terms positive: relative (D + 2) u), var = q / C + eps,
      rstd = 1 / sqrt(var) (two correctly rounded ops, 2 u; half the variance's relative error). The mean's
      error enters the variance at second order: dm^2 / (var + eps).
        -> relative error of rstd  r = ((D + 5) / 2 + 2) u + dm^2 / (2 (var + eps))
      y = d * rstd * gamma + beta: three more roundings.
    Together  |dy| <= rstd |gamma| dm + |d rstd gamma| (r + 3 u) + u |y|, and the store adds half an f16 ulp
    (2^-11 |y|, 2^-25 below the normal range) for f16 outputs or 2^-22 |y| for split outputs."""
    xs = np.asarray(xs, np.float64)
    D = -(-C // 64) + 6
    A = np.abs(xs).max()
    mean = xs.sum() / C
    d = xs - mean
    var = (d * d).sum() / C
    rstd = 1.0 / np.sqrt(var + eps)
    dm = (D + 2) * U * A
    r = ((D + 5) / 2 + 2) * U + dm * dm / (2 * (var + eps))
    t = np.abs(d * rstd * gamma)
    y = np.abs(d * rstd * gamma + beta)
    bound = rstd * np.abs(gamma) * dm + t * (r + 3 * U) + U * y
    if form == "f16":
        bound = bound + np.maximum(2.0 ** -11 * (y + bound), 2.0 ** -25)
    elif form == "split":
        bound = bound + 2.0 ** -22 * (y + bound)
    return bound


def ln_case(shape, table, eps, N=3, T=5):
    form, C, win, wout = shape
    rng = np.random.default_rng([15, LN_SHAPES.index(shape), int(table), N, T])
    gamma = rng.uniform(0.8, 1.2, C).astype(np.float32)
    beta = (0.05 * rng.standard_normal(C)).astype(np.float32)
    # T rows of clearly different values: row t sits near 10 (t + 1)
    add = (10.0 * (1 + np.arange(T))[:, None] + rng.standard_normal((T, C))).astype(np.float32) if table else None
    a = np.full((N, 1, T, win), 0.0 if form == "split" else LN_PAD)
    b = np.zeros((N, 1, T, win))
    kinds = {}
    for n in range(N):
        for t in range(T):
            kinds[n, t] = LN_KINDS[(n + t + (T == 1)) % len(LN_KINDS)] if T > 1 else "mean100"
            a[n, 0, t, :C], b[n, 0, t, :C] = _ln_rows(rng, form, kinds[n, t], C)
    P = pg.Program(split=form == "split")
    if form == "split":
        x = P.input_tensor(1, T, 2 * win)
        e = P.act(1, T, win)
        ident(P, e, x, win, lo=win)
        src, xv, v = e, np.concatenate([a, b], -1), a + b * LO
    else:
        src = x = P.input_tensor(1, T, win)
        xv = v = a
    y = P.act(1, T, wout)
    P.layernorm(y, src, gamma, beta, eps, add=add)
    P.outputs = [y] + ([e] if form == "split" else [])
    exp = np.zeros((N, 1, T, wout))
    exp[..., :C] = R.layernorm(v, C, gamma, beta, eps, add)
    bound = np.zeros_like(exp)
    for n in range(N):
        for t in range(T):
            xs = np.asarray(v[n, 0, t, :C], np.float64) + (np.asarray(add[t], np.float64) if table else 0.0)
            bound[n, 0, t, :C] = ln_bound(xs, C, gamma.astype(np.float64), beta.astype(np.float64),
                                          float(np.float32(eps)), form)
    name = f"ln-{form}-c{C}in{win}-{'table' if table else 'plain'}-eps{eps:g}-{N}x{T}"
    return Case(name, P, form == "f32", xv, [exp] + ([v] if form == "split" else []), bound=bound, kinds=kinds,
                form=form, C=C, beta=beta, gamma=gamma, add=add, eps=eps, val=v)


def layernorm_cases():
    out = []
    for sh in LN_SHAPES:
        out += [ln_case(sh, table, eps) for table in (True, False) for eps in (1e-5, 1e-6)]
        out.append(ln_case(sh, sh[1] % 3 == 0, 1e-5, N=1, T=1))
    return out


# ---- calibration -----------------------------------------------------------------------------------
def calib_case(split, H, W, N=3):
    """Convs writing: a plain f16 tensor with cout < npad whose largest value is negative; two views of one
    buffer, one near 300 and one near 0.01 (plain program only: a split tensor has no channel views); an is_f32
    tensor; and a LayerNorm reading the first. measured: the tensor ids whose abs-max the run must report."""
    rng = np.random.default_rng([16, int(split), H, W])
    xv = rng.integers(-255, 256, (N, H, W, 32)) / 64.0
    xv[0, 0, 0, 5] = 4.5            # the largest magnitude of channels [0, 20) is positive here ...
    P = pg.Program(split=split)
    x = P.input_tensor(H, W, 32)
    t1 = P.act(H, W, 32)
    w = np.zeros((32, 32), np.float32)
    w[np.arange(20), np.arange(20)] = -1.5     # ... and negative in t1
    P.conv(t1, [(x, 1, 1, 1, 0, 32)], w, 20)
    measured = {t1: "negative maximum"}
    outs = [t1]
    if not split:
        Z = P.act(H, W, 64)
        big, small = P.view(Z, 0, 32), P.view(Z, 32, 32)
        ident(P, big, x, 32, scale=64.0)
        ident(P, small, x, 32, scale=2.0 ** -9)
        measured[big], measured[small] = "near 300", "near 0.01"
        outs.append(Z)
    f = P.act(H, W, 32, is_f32=1)
    ident(P, f, x, 32)
    ln = P.act(H, W, 32)
    P.layernorm(ln, t1, np.ones(20, np.float32), np.zeros(20, np.float32))
    P.outputs = outs + [f, ln]
    return Case(f"calib-{'split' if split else 'plain'}-{H}x{W}", P, False, xv, None, measured=measured)


def calib_cases():
    return [calib_case(s, H, W) for s in (False, True) for (H, W) in ((5, 7), (1, 1))]


# ---- attention -------------------------------------------------------------------------------------
ATT_KINDS = ["normal", "winner", "tie", "ramp_up", "ramp_down", "flat"]
ATT_PAD = 7.0        # the qkv pixel's channels beyond 3E
# (storage, head dim, needs PERSON_CAPTURE_AMD_ATTN=stream, kernel)
ATT_FORMS = {
    "tokens_f32": ("f32", 64, False, "mha_tokens<float>"),
    "tokens_f16": ("f16", 64, False, "mha_tokens<f16>"),
    "tokens_sp": ("split", 64, False, "mha_tokens<float, SP>"),
    "stream_f32_64": ("f32", 64, True, "mha_stream<false, 64>"),
    "stream_sp_64": ("split", 64, True, "mha_stream<true, 64>"),
    "mfma_64": ("f16", 64, True, "mha_mfma<64>"),
    "stream_f32_80": ("f32", 80, False, "mha_stream<false, 80>"),
    "stream_sp_80": ("split", 80, False, "mha_stream<true, 80>"),
    "mfma_80": ("f16", 80, False, "mha_mfma<80>"),
}
ATT_T_RESIDENT = [1, 3, 5, 64, 65, 272]
ATT_T_STREAM = [1, 16, 17, 49, 64, 65, 129]
# Where the winning key sits, per T: the k-th "winner" head of a run takes entry k (the last entry again after
# that). Every form meets all four placements: first (T = 5 resident, 16 streaming), last in a partial chunk or
# tile (T = 3, 272 resident: key ranges of 1 and 68 per wave; T = 17, 49, 129 streaming; 273), key 63 (T = 64, and
# the second winner of the nine-head run at T = 65) and key 64 (T = 65). att_winner_placements() names them and
# test_net_op_refs_cpu.py asserts the cover per form.
ATT_WINNER = {1: [0], 3: [2], 5: [0], 16: [0], 17: [16], 49: [48], 64: [63], 65: [64, 63], 129: [128], 272: [271],
              273: [272]}
ATT_T_LAST_PARTIAL = (3, 17, 49, 129, 272, 273)


def att_winner_placements(T, pos):
    """The named placements a winner at key pos of T keys covers."""
    out = set()
    if pos == 0 and T > 1:
        out.add("first")
    if pos == T - 1 and T in ATT_T_LAST_PARTIAL:
        out.add("last")
    if pos in (63, 64):
        out.add(str(pos))
    return out


def att_runs():
    """(form, T, heads, N) of every attention run. heads = 2 and N = 3 give six (image, head) pairs, one per
    data kind; the T = 65 run with heads = 3 and N = 3 has nine, every one with data of its own. T = 273 at
    d = 64 is run without the environment variable: the default dispatch must stream it."""
    runs = []
    for form, (st, d, stream, _) in ATT_FORMS.items():
        for T in (ATT_T_STREAM if (stream or d == 80) else ATT_T_RESIDENT):
            runs.append((form, T, 2, 3))
        runs.append((form, 65, 3, 3))
    runs += [("tokens_f32", 273, 2, 3), ("tokens_f16", 273, 2, 3), ("tokens_sp", 273, 1, 2)]
    return runs


def _att_head(rng, kind, T, d, st, resident, salt, occ):
    """q, k, v [T][d] of one (image, head) and the largest |logit|. The constructed kinds put small integers on
    dim 0 of q and k (and an image-dependent constant pair on dim 1, which shifts every logit alike): at d = 64
    the products, their sum and the scale 1/8 are exact, so the device and the reference see the same logits."""
    rnd = (lambda s: np.asarray(rng.standard_normal(s), np.float32).astype(np.float64)) if st == "f32" else \
        (lambda s: f16r(rng.standard_normal(s)))
    v = rnd((T, d))
    if kind == "normal" or (kind == "tie" and T < 2):
        return rnd((T, d)), rnd((T, d)), v
    q, k = np.zeros((T, d)), np.zeros((T, d))
    q[:, 0] = 8.0
    q[:, 1], k[:, 1] = 1.0, float(salt % 5)
    if kind == "winner":     # one logit of 100, every other <= 60; the winner where ATT_WINNER puts it
        k[:, 0] = rng.integers(-60, 61, T)
        k[ATT_WINNER[T][min(occ, len(ATT_WINNER[T]) - 1)], 0] = 100.0
    elif kind == "tie":      # two identical key rows in different waves (resident) or tiles (streaming)
        k[:, 0] = rng.integers(-60, 61, T)
        i, j = (63, 64) if (T > 64 and not resident) else (0, T - 1)
        k[i, 0] = k[j, 0] = 100.0
    elif kind == "ramp_up":
        k[:, 0] = np.arange(T)
    elif kind == "ramp_down":
        k[:, 0] = np.arange(T)[::-1]
    return q, k, v


def att_bound(kind, st, d, T, mfma, vmax, out, lmax):
    """|device - f64 reference| at the attention output, with u = 2^-24 and vmax = max |v| of the head.

    random-normal data, f32-class forms: the project's 1e-5 vmax (TOL_X3). Constructed data:
      logits: exact at d = 64. At d = 80 the scale is inexact: q * scale, the one non-zero product per dim and
        the two-term sum round once each, 3 u lmax (lmax = max |logit|) absolute on a logit, that much relative
        on its weight and on the normaliser: 2 * 3 u lmax vmax.
      __expf(x) = exp2(x log2 e): the argument's rounding is |x| u relative on the result, the exp2 itself
        1 ulp; arguments that matter have |x| <= 20 (a weight below e^-20 adds < 2.1e-9 vmax per key, T of them
        at most: the tail term), so 24 u per exponential. A term passes through at most 4 that matter: its own,
        the rescale of a later chunk (twice before its weight is below e^-20 on the steepest ramp) and the
        combine; numerator and normaliser both: 8 * 24 u vmax.
      accumulation: a wave sums at most ceil(T / 4) + 16 keys sequentially, the combine 4 more, the division
        and the product 4: 2 (ceil(T / 4) + 24) u vmax for numerator and normaliser.
    Stores: f16 outputs half an ulp (2^-11 |out|, 2^-25 below the normal range); split outputs 2^-22 |out|.
    mha_mfma: P is rounded to f16 before PV, 2^-10 vmax (tests/test_gpu_clip_family.py), and P values in the
    f16 subnormal range lose up to 2^-25 each: T 2^-25 vmax."""
    if kind == "normal":
        b = 1e-5 * vmax
    else:
        logit = 0.0 if d == 64 else 2 * 3 * U * lmax
        b = (logit + 8 * 24 * U + 2 * (-(-T // 4) + 24) * U + T * 2.1e-9) * vmax
    if mfma:
        b = b + (2.0 ** -10 + T * 2.0 ** -25) * vmax
    out = np.abs(out)
    if st == "f16":
        return b + np.maximum(2.0 ** -11 * (out + b), 2.0 ** -25)
    if st == "split":
        return b + 2.0 ** -22 * (out + b)
    return b + 0 * out


def att_case(form, T, heads, N):
    st, d, stream, _ = ATT_FORMS[form]
    resident = form.startswith("tokens") and T <= 272
    E = heads * d
    wq, wo = 3 * E + 32, E + 32        # both pixel strides exceed the data
    rng = np.random.default_rng([17, list(ATT_FORMS).index(form), T, heads, N])
    a = np.full((N, 1, T, wq), ATT_PAD)
    b = np.zeros((N, 1, T, wq))
    kinds, lmax = {}, {}
    # six pairs: every kind once; nine pairs (three heads): the kinds cycle from "winner", which comes twice
    ti = 1 if heads == 3 else (ATT_T_RESIDENT + ATT_T_STREAM + [273]).index(T)
    winners = 0
    for n in range(N):
        for h in range(heads):
            kind = kinds[n, h] = ATT_KINDS[(n * heads + h + ti) % len(ATT_KINDS)]
            q, k, v = _att_head(rng, kind, T, d, st, resident, n * heads + h + ti, winners)
            winners += kind == "winner"
            for i, m in enumerate((q, k, v)):
                a[n, 0, :, i * E + h * d:i * E + (h + 1) * d] = m
            if st == "split":      # second halves: v always, q and k of the random-normal heads only
                b[n, 0, :, 2 * E + h * d:2 * E + (h + 1) * d] = lo_part(rng, (T, d))
                if kind == "normal":
                    b[n, 0, :, h * d:(h + 1) * d] = lo_part(rng, (T, d))
                    b[n, 0, :, E + h * d:E + (h + 1) * d] = lo_part(rng, (T, d))
            lmax[n, h] = np.abs((q @ k.T) / np.sqrt(d)).max()
    P = pg.Program(split=st == "split")
    if st == "split":
        x = P.input_tensor(1, T, 2 * wq)
        qkv = P.act(1, T, wq)
        ident(P, qkv, x, wq, lo=wq)
        xv, val = np.concatenate([a, b], -1), a + b * LO
    else:
        qkv = x = P.input_tensor(1, T, wq)
        xv = val = a
    o = P.act(1, T, wo)
    P.attention(o, qkv, heads, d)
    P.outputs = [o] + ([qkv] if st == "split" else [])
    exp = np.zeros((N, 1, T, wo))
    exp[:, 0, :, :E] = R.attention(val[:, 0], heads, d)
    bound = np.zeros_like(exp)
    for (n, h), kind in kinds.items():
        sl = slice(h * d, (h + 1) * d)
        vmax = np.abs(val[n, 0, :, 2 * E + h * d:2 * E + (h + 1) * d]).max()
        bound[n, 0, :, sl] = att_bound(kind, st, d, T, form.startswith("mfma") or (form == "tokens_f16" and T > 272),
                                       vmax, exp[n, 0, :, sl], lmax[n, h])
    return Case(f"attn-{form}-T{T}-h{heads}-n{N}", P, st == "f32", xv, [exp] + ([val] if st == "split" else []),
                bound=bound, kinds=kinds, form=form, stream=stream, E=E, d=d, heads=heads, val=val)


# ---- every program of this file (the planner must accept them all) ----------------------------------
def all_cases():
    return pool_cases() + upsample_cases() + layernorm_cases() + calib_cases() + [att_case(*r) for r in att_runs()]
