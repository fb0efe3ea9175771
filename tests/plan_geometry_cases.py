"""Programs whose tensors or op geometry a kernel would follow outside its tensors, one per rule of
pc_program.cpp check_tensor / check_geometry, and the accepted programs they are cut from. Built with
program.py; shared by test_plan_cpu.py (pc_net_plan, no device) and test_gpu_net_ops.py (pc_net_create)."""
import numpy as np

from person_capture_amd import program as pg


def _shape(P, t, **kw):
    """Edit tensor t of a Program: H, W, C, cs, coff, is_f32 (its buffer grows with it unless keep_buf)."""
    T = P.tensors[t]
    keep = kw.pop("keep_buf", False)
    for k, v in kw.items():
        T[{"H": 1, "W": 2, "C": 3, "cs": 4, "coff": 5, "is_f32": 6}[k]] = v
    if T[0] >= 0 and not keep:
        P.vbufs[T[0]][0] = max(P.vbufs[T[0]][0], T[1] * T[2] * T[4])
        if "is_f32" in kw:
            P.vbufs[T[0]][1] = kw["is_f32"]
    return P


def _pool_prog(C=8, k=3, s=2, p=1, oh=4, ow=3, view=None):
    P = pg.Program()
    x = P.input_tensor(7, 5, 16)
    y = P.act(oh, ow, C)
    P.maxpool(y, P.view(x, *view) if view else P.view(x, 0, C), k, s, p)
    P.outputs = [y]
    return P


def _up_prog(C=8, oh=6, ow=10, view=None, wide=16):
    P = pg.Program()
    x = P.input_tensor(3, 5, wide)
    y = P.act(oh, ow, C)
    P.upsample2(y, P.view(x, *view) if view else P.view(x, 0, C))
    P.outputs = [y]
    return P


def _ln_prog(C=64, win=64, wout=64, T=5, tout=5, rows=5, ngamma=None, nbeta=None, table=True, split=False):
    P = pg.Program(split=split)
    x = P.input_tensor(1, T, win)
    y = P.act(1, tout, wout)
    P.layernorm(y, x, np.ones(ngamma or C, np.float32), np.zeros(nbeta or C, np.float32), 1e-5,
                add=np.zeros((rows, C), np.float32) if table else None)
    P.ops[-1][8] = C
    P.outputs = [y]
    return P


def _attn_prog(wq=192, wo=64, heads=1, T=5, tout=5, qview=None, oview=None):
    P = pg.Program()
    x = P.input_tensor(1, T, wq)
    y = P.act(1, tout, wo)
    P.attention(P.view(y, *oview) if oview else y, P.view(x, *qview) if qview else x, heads, 64)
    P.outputs = [y]
    return P


def _conv_prog(res_mode=pg.RES_UP2, rh=8, bias_mode=pg.BIAS_CHANNEL):
    """x 16x16 -> t (3x3 s1 p1, bias, PReLU slopes) -> o (1x1, a residual r that no op writes)."""
    P = pg.Program()
    x = P.input_tensor(16, 16, 32)
    t, o = P.act(16, 16, 32), P.act(16, 16, 32)
    r = P.act(rh, rh, 32)
    P.conv(t, [(x, 3, 3, 1, 1, 32)], np.zeros((32, 288), np.float32), 32,
           bias=np.zeros(32 * (9 if bias_mode == pg.BIAS_BORDER9 else 1)), bias_mode=bias_mode, slope=np.ones(32), act=pg.ACT_PRELU)
    P.conv(o, [(t, 1, 1, 1, 0, 32)], np.zeros((32, 32), np.float32), 32, bias=np.zeros(32), res=r, res_mode=res_mode)
    P.outputs = [o]
    return P


def _stem_prog():
    P = pg.Program()
    x = P.input_tensor(16, 16, 4)
    y = P.act(8, 8, 32)
    P.stem(y, x, np.zeros((32, 3, 3, 4), np.float32), np.zeros(32, np.float32), 2, 1)
    P.outputs = [y]
    return P


def _short(P, word, n, op=0):
    """The array that word `word` of op `op` names, cut to n floats."""
    P.arrays[P.ops[op][word]] = np.zeros(n, np.float32)
    return P


def valid_geometry_programs():
    return {"pool": _pool_prog(), "pool_view": _pool_prog(C=4, view=(4, 4)), "up": _up_prog(), "up_view": _up_prog(view=(8, 8)),
            "ln": _ln_prog(), "ln_plain": _ln_prog(table=False), "ln_2048": _ln_prog(C=2048, win=2048, wout=2048),
            "ln_narrow": _ln_prog(C=40, win=64, wout=64), "attn": _attn_prog(), "attn_wide": _attn_prog(wq=224, wo=96),
            "attn_view": _attn_prog(wq=208, qview=(8, 192)), "conv_up2": _conv_prog(),
            "conv_same": _conv_prog(pg.RES_SAME, 16), "conv_border": _conv_prog(bias_mode=pg.BIAS_BORDER9),
            "stem": _stem_prog()}


def geometry_cases():
    """name -> (program, words of the message): one case per rule of pc_program.cpp check_tensor / check_geometry."""
    two = lambda: _two_convs_program()
    c = {}
    # every tensor
    c["tensor_h0"] = (_shape(two()[0], 1, H=0), "tensor: H, W and C")
    c["tensor_coff_negative"] = (_shape(_pool_prog(C=4, view=(4, 4)), 2, coff=-4), "tensor: channel slice")
    c["tensor_slice_past_stride"] = (_shape(_pool_prog(C=4, view=(4, 4)), 2, coff=14), "tensor: channel slice")
    c["tensor_larger_than_buffer"] = (_shape(two()[0], 1, H=17, keep_buf=True), "tensor: larger than its buffer")
    c["tensor_is_f32_not_its_buffers"] = (_shape(two()[0], 1, is_f32=1, keep_buf=True), "tensor: is_f32")
    # element types of the stem and the non-GEMM ops
    c["pool_is_f32_out"] = (_shape(_pool_prog(), 1, is_f32=1), "max pool: reads and writes the net's element type")
    c["upsample_is_f32_out"] = (_shape(_up_prog(), 1, is_f32=1), "upsample: reads and writes the net's element type")
    c["layernorm_is_f32_out"] = (_shape(_ln_prog(), 1, is_f32=1), "layernorm: reads and writes the net's element type")
    c["stem_is_f32_in"] = (_shape(_stem_prog(), 0, is_f32=1), "stem: reads the net's element type")
    c["attention_is_f32_out"] = (_shape(_attn_prog(), 1, is_f32=1), "attention: reads and writes the net's element type")
    # max pool
    c["pool_k0"] = (_pool_prog(k=0), "max pool: window")
    c["pool_stride0"] = (_pool_prog(s=0), "max pool: window")
    c["pool_pad_over_half"] = (_pool_prog(p=2, oh=5, ow=4), "max pool: window")
    c["pool_wrong_output_size"] = (_pool_prog(oh=4, ow=4), "max pool: the output size")
    c["pool_output_narrower"] = (_shape(_pool_prog(), 1, C=4, cs=4), "max pool: input and output must have the same channels")
    c["pool_c6"] = (_shape(_shape(_pool_prog(), 1, C=6, cs=8), 2, C=6), "max pool: channels, pixel strides and offsets")
    c["pool_cs6"] = (_shape(_pool_prog(C=4), 1, cs=6), "max pool: channels, pixel strides and offsets")
    c["pool_coff2"] = (_pool_prog(C=4, view=(2, 4)), "max pool: channels, pixel strides and offsets")
    # upsample
    c["upsample_4x4_from_3x5"] = (_up_prog(oh=4, ow=4), "upsample: the output must be twice")
    c["upsample_c4_f16"] = (_up_prog(C=4), "upsample: channels, pixel strides and offsets")
    c["upsample_cs12_f16"] = (_up_prog(wide=12), "upsample: channels, pixel strides and offsets")
    c["upsample_coff4_f16"] = (_up_prog(view=(4, 8)), "upsample: channels, pixel strides and offsets")
    # LayerNorm
    c["layernorm_c0"] = (_ln_prog(C=64, table=False, ngamma=64), "layernorm: 1 <= C <= 2048")
    c["layernorm_c0"][0].ops[-1][8] = 0
    c["layernorm_c4096"] = (_ln_prog(C=4096, win=4096, wout=4096), "layernorm: 1 <= C <= 2048")
    c["layernorm_output_4096"] = (_ln_prog(C=64, wout=4096), "layernorm: 1 <= C <= 2048")
    c["layernorm_wider_than_input"] = (_ln_prog(C=64, win=32), "layernorm: C wider than its input or output")
    c["layernorm_wider_than_output"] = (_ln_prog(C=64, wout=32), "layernorm: C wider than its input or output")
    c["layernorm_pixels_differ"] = (_ln_prog(tout=6), "layernorm: input and output must have the same pixels")
    c["layernorm_gamma_8_for_64"] = (_ln_prog(ngamma=8), "layernorm: gamma and beta")
    c["layernorm_gamma_8_for_64"][0].ops[-1][8] = 64
    c["layernorm_beta_short"] = (_ln_prog(nbeta=63), "layernorm: gamma and beta")
    c["layernorm_table_rows_0"] = (_ln_prog(), "layernorm: the positional table")
    c["layernorm_table_rows_0"][0].ops[-1][6] = 0
    c["layernorm_table_rows_not_pixels"] = (_ln_prog(rows=4), "layernorm: the positional table")
    c["layernorm_table_short"] = (_short(_ln_prog(), 5, 5 * 64 - 1), "layernorm: the positional table")
    # attention
    c["attention_qkv_narrow"] = (_attn_prog(wq=128), "attention: 3 * heads * d wider")
    c["attention_output_narrow"] = (_attn_prog(wo=32), "attention: 3 * heads * d wider")
    c["attention_tokens_differ"] = (_attn_prog(tout=6), "attention: input and output must have the same tokens")
    c["attention_qkv_stride_196"] = (_attn_prog(wq=196, qview=(0, 192)), "attention: pixel strides")
    c["attention_output_stride_68"] = (_attn_prog(wo=68, oview=(0, 64)), "attention: pixel strides")
    c["attention_offset_8_bytes"] = (_attn_prog(wq=208, qview=(4, 192)), "attention: tensor offsets")
    # conv
    c["conv_output_size"] = (_shape(_conv_prog(), 1, H=15), "conv: the output size")
    c["conv_residual_same_other_size"] = (_conv_prog(pg.RES_SAME, 8), "conv: a same-size residual")
    c["conv_residual_up2_not_half"] = (_conv_prog(pg.RES_UP2, 7), "conv: an upsampled residual")
    c["conv_residual_mode_3"] = (_conv_prog(), "conv: the residual mode")
    c["conv_residual_mode_3"][0].ops[1][22] = 3
    c["conv_weights_short"] = (_short(_conv_prog(), 13, 32 * 288 - 1), "conv: the weight array")
    c["conv_bias_short"] = (_short(_conv_prog(), 17, 31), "conv: the bias array")
    c["conv_border_bias_npad"] = (_short(_conv_prog(bias_mode=pg.BIAS_BORDER9), 17, 32), "conv: the bias array")
    c["conv_slopes_short"] = (_short(_conv_prog(), 19, 31), "conv: the slope array")
    return c


def _two_convs_program():
    P = pg.Program()
    x = P.input_tensor(16, 16, 64)
    y, z = P.act(16, 16, 64), P.act(16, 16, 64)
    for a, b in ((x, y), (y, z)):
        P.conv(b, [(a, 3, 3, 1, 1, 64)], np.zeros((64, 576), np.float32), 64, bias=np.zeros(64), act=pg.ACT_RELU)
    P.outputs = [z]
    return P, (x, y, z)
