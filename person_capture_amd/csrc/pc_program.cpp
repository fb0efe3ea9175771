// Program decoder: the serialized network (person_capture_amd/program.py) -> NetDesc, validated. The only
// code that reads op records by word position (pc_net.h OpWord); everything after it works on the typed ops
// and may index the tensor, buffer and array tables with any id it finds there.
#include <string.h>
#include <algorithm>
#include "pc_net.h"

namespace pc {

namespace {
struct Decoder {
  const NetDesc& d;
  std::string& err;
  bool bad(const char* what) {
    err = std::string("malformed program: ") + what;
    return false;
  }
  bool tensor(int t, bool optional = false) {
    return (optional && t == -1) || (t >= 0 && t < (int)d.tens.size()) || bad("tensor id out of range");
  }
  bool array(int a, bool optional = false) {
    return (optional && a == -1) || (a >= 0 && a < (int)d.arrays.size()) || bad("array id out of range");
  }

  bool decode_op(const int32_t* w, NetOp& op) {
    memset(&op, 0, sizeof(op));
    op.kind = w[kWKind];
    switch (op.kind) {
      case OP_CONV: {
        ConvOp& c = op.conv;
        c.out = w[kWOut];
        c.nseg = w[kWConvNseg];
        if (c.nseg < 1 || c.nseg > 2) return bad("conv segments must be 1 or 2");
        if (!tensor(c.out)) return false;
        for (int s = 0; s < c.nseg; ++s) {
          const int32_t* sw = w + kWConvSeg + kWConvSegWords * s;
          c.seg[s] = ConvSegOp{sw[0], sw[1], sw[2], sw[3], sw[4], 0};
          if (!tensor(c.seg[s].x)) return false;
          if (c.seg[s].KH < 1 || c.seg[s].KW < 1 || c.seg[s].stride < 1 || c.seg[s].pad < 0)
            return bad("conv window");
          // algorithmic MACs count the true input channels (padded lanes excluded by the program)
          c.seg[s].cin_true = w[kWConvCinTrue + s] > 0 ? w[kWConvCinTrue + s] : d.tens[c.seg[s].x].C;
        }
        c.w = w[kWConvW]; c.npad = w[kWConvNpad]; c.ktot = w[kWConvKtot]; c.cout = w[kWConvCout];
        c.bias = w[kWConvBias]; c.bias_mode = w[kWConvBiasMode];
        c.slope = w[kWConvSlope]; c.act = w[kWConvAct];
        c.res = w[kWConvRes]; c.res_mode = w[kWConvResMode];
        c.act_after_res = w[kWConvActAfterRes];
        if (w[kWConvSplitk] < 0 || w[kWConvSplitk] > 64) return bad("conv split-K out of range");
        c.splitk = w[kWConvSplitk] > 1 ? w[kWConvSplitk] : 1;
        c.cout_true = w[kWConvCoutTrue] > 0 ? w[kWConvCoutTrue] : c.cout;
        if (c.npad <= 0 || c.ktot <= 0 || c.cout <= 0 || c.cout > c.npad) return bad("conv weight dims");
        return array(c.w) && array(c.bias, true) && array(c.slope, true) && tensor(c.res, true);
      }
      case OP_STEM: {
        StemOp& s = op.stem;
        s = StemOp{w[kWOut], w[kWIn], w[kWStemKH], w[kWStemKW], w[kWStemStride], w[kWStemPad], w[kWStemW],
                   w[kWStemCout], w[kWStemBias], w[kWStemSlope], w[kWStemAct], w[kWStemCpad],
                   w[kWStemCinTrue] > 0 ? w[kWStemCinTrue] : 3};
        if (s.KH < 1 || s.KW < 1 || s.stride < 1 || s.pad < 0 || s.cout <= 0) return bad("stem window");
        return tensor(s.out) && tensor(s.x) && array(s.w) && array(s.bias) && array(s.slope, true);
      }
      case OP_MAXPOOL:
        op.pool = PoolOp{w[kWOut], w[kWIn], w[kWPoolK], w[kWPoolStride], w[kWPoolPad]};
        return tensor(op.pool.out) && tensor(op.pool.x);
      case OP_UPSAMPLE:
        op.up = UpsampleOp{w[kWOut], w[kWIn]};
        return tensor(op.up.out) && tensor(op.up.x);
      case OP_LAYERNORM: {
        LayerNormOp& l = op.ln;
        l = LayerNormOp{w[kWOut], w[kWIn], w[kWLnGamma], w[kWLnBeta], w[kWLnAdd], w[kWLnRows], 0.f, w[kWLnC]};
        memcpy(&l.eps, &w[kWLnEps], 4);
        return tensor(l.out) && tensor(l.x) && array(l.gamma) && array(l.beta) && array(l.add, true);
      }
      case OP_ATTENTION:
        op.attn = AttnOp{w[kWOut], w[kWIn], w[kWAttnHeads], w[kWAttnHeadDim]};
        return tensor(op.attn.out) && tensor(op.attn.x);
      default:
        return bad("unknown op type");
    }
  }
};

// Every tensor lies inside its buffer: a pixel holds its channel slice, the buffer holds every pixel,
// and tensor and buffer agree on the element type. (buf -1: the net input, the caller's memory.)
const char* check_tensor(const NetDesc& d, const NetTensor& t) {
  if (t.buf < -1) return "malformed program: tensor: buffer id out of range";
  if (t.H < 1 || t.W < 1 || t.C < 1) return "malformed program: tensor: H, W and C must be at least 1";
  if (t.coff < 0 || (long long)t.coff + t.C > t.cs) return "malformed program: tensor: channel slice [coff, coff + C) outside the pixel stride";
  if (t.buf >= 0) {
    const NetBuf& b = d.bufs[t.buf];
    if ((long long)t.H * t.W * t.cs > b.elems) return "malformed program: tensor: larger than its buffer";
    if ((t.is_f32 != 0) != (b.is_f32 != 0)) return "malformed program: tensor: is_f32 differs from its buffer's";
  }
  return nullptr;
}

// The shape rules of every op, from the kernels' own indexing (pc_conv.hip max pools, pc_ops.hip, pc_attn.hip,
// pc_conv_common.h epilogue): a program that passes reads and writes inside its tensors. nullptr: fine.
const char* check_geometry(const NetDesc& d, const NetOp& op) {
  const int k = op.kind;
  auto cnt = [&](int a) { return d.arrays[a].cnt; };
  // the window's output size, in 64 bits (every operand comes from the file); -1: the window does not fit
  auto out_dim = [](long long in, long long win, long long stride, long long pad) {
    return in + 2 * pad < win ? -1LL : (in + 2 * pad - win) / stride + 1;
  };
  const NetTensor& Y = d.tens[op.out()];
  if (k == OP_CONV) {
    const ConvOp& c = op.conv;
    for (int s = 0; s < c.nseg; ++s) {
      const ConvSegOp& g = c.seg[s];
      const NetTensor& X = d.tens[g.x];
      if (Y.H != out_dim(X.H, g.KH, g.stride, g.pad) || Y.W != out_dim(X.W, g.KW, g.stride, g.pad))
        return "conv: the output size does not follow from a segment's input and window";
    }
    if (c.res >= 0) {
      const NetTensor& R = d.tens[c.res];
      if (c.res_mode == RES_SAME && (R.H != Y.H || R.W != Y.W)) return "conv: a same-size residual must have the output's size";
      // the epilogue reads residual pixel (oh >> 1, ow >> 1)
      if (c.res_mode == RES_UP2 && (R.H != ((long long)Y.H + 1) / 2 || R.W != ((long long)Y.W + 1) / 2))
        return "conv: an upsampled residual must have half the output's size, rounded up";
      if (c.res_mode != RES_SAME && c.res_mode != RES_UP2) return "conv: the residual mode must be same-size (1) or upsampled (2)";
    }
    if (cnt(c.w) < (long long)c.npad * c.ktot) return "conv: the weight array holds fewer than npad * ktot floats";
    if (c.bias >= 0 && cnt(c.bias) < (long long)c.npad * (c.bias_mode == BIAS_BORDER9 ? 9 : 1))
      return "conv: the bias array holds fewer than npad floats (9 * npad in border mode)";
    if (c.slope >= 0 && cnt(c.slope) < c.npad) return "conv: the slope array holds fewer than npad floats";
    return nullptr;
  }
  const NetTensor& X = d.tens[op.io.x];
  // the stem and the four non-GEMM kernels read and write the net's own element type
  if (!d.f32 && (X.is_f32 || (k != OP_STEM && Y.is_f32))) {
    switch (k) {
      case OP_STEM: return "stem: reads the net's element type, not an is_f32 tensor of an f16 net";
      case OP_MAXPOOL: return "max pool: reads and writes the net's element type, not an is_f32 tensor of an f16 net";
      case OP_UPSAMPLE: return "upsample: reads and writes the net's element type, not an is_f32 tensor of an f16 net";
      case OP_LAYERNORM: return "layernorm: reads and writes the net's element type, not an is_f32 tensor of an f16 net";
      default: return "attention: reads and writes the net's element type, not an is_f32 tensor of an f16 net";
    }
  }
  const int xc = X.split ? X.C / 2 : X.C, yc = Y.split ? Y.C / 2 : Y.C;   // logical widths
  const int V = d.f32 ? 4 : 8;                                            // elements of a 16-byte vector
  if (k == OP_MAXPOOL) {
    const PoolOp& p = op.pool;
    if (p.k < 1 || p.stride < 1 || p.pad < 0 || p.pad > p.k / 2) return "max pool: window needs k >= 1, stride >= 1 and 0 <= pad <= k / 2";
    if (Y.H != out_dim(X.H, p.k, p.stride, p.pad) || Y.W != out_dim(X.W, p.k, p.stride, p.pad))
      return "max pool: the output size does not follow from the input and the window";
    if (Y.C != X.C) return "max pool: input and output must have the same channels";
    if (xc % 4 || X.cs % 4 || Y.cs % 4 || X.coff % 4 || Y.coff % 4) return "max pool: channels, pixel strides and offsets must be multiples of 4";
  } else if (k == OP_UPSAMPLE) {
    if (Y.H != 2LL * X.H || Y.W != 2LL * X.W) return "upsample: the output must be twice the input's height and width";
    if (std::min(X.C, Y.C) % V || X.cs % V || Y.cs % V || X.coff % V || Y.coff % V)
      return "upsample: channels, pixel strides and offsets must be whole 16-byte vectors";
  } else if (k == OP_LAYERNORM) {
    const LayerNormOp& l = op.ln;
    if (l.C < 1 || l.C > 2048 || yc > 2048) return "layernorm: 1 <= C <= 2048 and an output of at most 2048 channels";
    if (l.C > xc || l.C > yc) return "layernorm: C wider than its input or output tensor";
    if ((long long)X.H * X.W != (long long)Y.H * Y.W) return "layernorm: input and output must have the same pixels";
    if (cnt(l.gamma) < l.C || cnt(l.beta) < l.C) return "layernorm: gamma and beta must hold C floats";
    if (l.add >= 0 && (l.rows < 1 || l.rows != (long long)X.H * X.W || cnt(l.add) < (long long)l.rows * l.C))
      return "layernorm: the positional table must hold one row of C floats per pixel of an image";
  } else if (k == OP_ATTENTION) {
    const AttnOp& a = op.attn;
    const long long E = (long long)a.heads * a.head_dim;
    if (3 * E > xc || E > yc) return "attention: 3 * heads * d wider than the qkv tensor, or heads * d wider than the output";
    if ((long long)X.H * X.W != (long long)Y.H * Y.W) return "attention: input and output must have the same tokens";
    if (X.cs % 8 || Y.cs % V) return "attention: pixel strides must be multiples of 8 (qkv) and of 4 (f32) or 8 (f16) elements (output)";
    if (X.coff % V || Y.coff % V) return "attention: tensor offsets must be aligned to 16 bytes";
  }
  return nullptr;
}
}  // namespace

int decode_program(const void* prog, size_t nbytes, int precision, int max_batch, NetDesc& d, std::string& err) {
  auto fail = [&](int code, const char* msg) { err = msg; return code; };
  if (!prog || max_batch <= 0) return fail(PC_ERR_ARG, "pc_net_create: bad arguments");
  const int32_t* P = (const int32_t*)prog;
  const size_t nw = nbytes / 4;
  if (nw < 8 || P[0] != 0x544E4350 || P[1] != 1) return fail(PC_ERR_FORMAT, "bad program magic/version");
  d = NetDesc();
  d.f32 = precision == PC_PREC_F32;
  d.max_batch = max_batch;
  const int nbuf = P[2], nten = P[3], narr = P[4], nop = P[5], nout = P[6];
  d.in_tensor = P[7];
  size_t pos = 8;
  if (nbuf < 0 || nten < 0 || narr < 0 || nop < 0 || nout < 0 ||
      pos + (size_t)nbuf * 4 + (size_t)nten * 8 + (size_t)narr * 4 + nout + (size_t)nop * kOpWords > nw)
    return fail(PC_ERR_FORMAT, "truncated program");
  for (int i = 0; i < nbuf; ++i, pos += 4)
    d.bufs.push_back(NetBuf{(long long)(uint32_t)P[pos] | ((long long)P[pos + 1] << 32), P[pos + 2]});
  for (int i = 0; i < nten; ++i, pos += 8) {
    NetTensor t{P[pos], P[pos + 1], P[pos + 2], P[pos + 3], P[pos + 4], P[pos + 5], P[pos + 6], P[pos + 7] & 1};
    t.c8 = (P[pos + 7] >> 2) & 1;
    if (i == d.in_tensor && (P[pos + 7] & 2)) d.in_centered = 1;
    if (t.buf >= nbuf) return fail(PC_ERR_FORMAT, "malformed program: buffer id out of range");
    d.tens.push_back(t);
  }
  for (int i = 0; i < narr; ++i, pos += 4)
    d.arrays.push_back(NetArray{(long long)(uint32_t)P[pos] | ((long long)P[pos + 1] << 32),
                                (long long)(uint32_t)P[pos + 2] | ((long long)P[pos + 3] << 32)});
  for (int i = 0; i < nout; ++i) d.outs.push_back(P[pos++]);
  d.words.assign(P + pos, P + pos + (size_t)nop * kOpWords);
  pos += (size_t)nop * kOpWords;
  d.data = (const float*)(P + pos);
  d.ndata = nw - pos;
  if (d.in_tensor < 0 || d.in_tensor >= nten) return fail(PC_ERR_FORMAT, "malformed program: input tensor id out of range");
  for (int o : d.outs)
    if (o < 0 || o >= nten) return fail(PC_ERR_FORMAT, "malformed program: output tensor id out of range");
  for (const NetArray& a : d.arrays)
    if (a.off < 0 || a.cnt < 0 || (size_t)(a.off + a.cnt) > d.ndata) return fail(PC_ERR_FORMAT, "array out of range");
  for (const NetBuf& b : d.bufs)
    if (b.elems < 0) return fail(PC_ERR_FORMAT, "malformed program: buffer size");
  for (const NetTensor& t : d.tens)
    if (const char* why = check_tensor(d, t)) return fail(PC_ERR_FORMAT, why);
  Decoder dec{d, err};
  d.ops.resize(nop);
  for (int i = 0; i < nop; ++i)
    if (!dec.decode_op(&d.words[(size_t)i * kOpWords], d.ops[i])) return PC_ERR_FORMAT;

  // f16x3 split tensors: f16 nets only; convs, the fused stem, the max pool,
  // LayerNorm and attention (both tensors split) read or write them
  for (auto& t : d.tens)
    if (t.split && (d.f32 || t.is_f32 || t.buf < 0 || t.C % 16 || t.cs != t.C))
      return fail(PC_ERR_FORMAT, "split tensor: f16 net, dense [hi | lo] activation buffer");
  // f16c8 tensors: split storage of whole 32-channel blocks, written by convs and the fused stem,
  // read by convs (conv_fast C8) and as a conv residual
  for (auto& t : d.tens)
    if (t.c8 && (!t.split || (t.C / 2) % 32)) return fail(PC_ERR_FORMAT, "f16c8 tensor: split storage of 32-channel blocks");
  for (auto& op : d.ops) {
    const int k = op.kind;
    // attention: a head dim one of the kernels covers (pc_ops.hip mha_tokens, pc_attn.hip)
    if (k == OP_ATTENTION && (op.attn.heads <= 0 || !attention_head_dim_ok(op.attn.head_dim)))
      return fail(PC_ERR_FORMAT, "attention: head dims 64 and 80 are implemented");
    if (k == OP_CONV || k == OP_STEM) continue;   // (a stem reads the plain net input; plan_stem checks its output)
    const NetTensor &Y = d.tens[op.io.out], &X = d.tens[op.io.x];
    if (Y.c8 || X.c8) return fail(PC_ERR_FORMAT, "op cannot read or write f16c8 tensors");
    // LayerNorm / attention: both tensors split (pc_ops.hip SP forms) or neither
    if ((k == OP_MAXPOOL && (Y.split != X.split || (X.split && Y.C != X.C))) ||
        (k == OP_UPSAMPLE && (Y.split || X.split)) ||
        ((k == OP_LAYERNORM || k == OP_ATTENTION) && Y.split != X.split))
      return fail(PC_ERR_FORMAT, "op cannot read or write split tensors");
    // split LayerNorm / attention: the logical width fits one half of either tensor
    if ((k == OP_LAYERNORM || k == OP_ATTENTION) && Y.split) {
      const int cin = k == OP_LAYERNORM ? op.ln.C : 3 * op.attn.heads * op.attn.head_dim;
      const int cout = k == OP_LAYERNORM ? op.ln.C : op.attn.heads * op.attn.head_dim;
      if (cin <= 0 || cin > X.C / 2 || cout > Y.C / 2)
        return fail(PC_ERR_FORMAT, "split layernorm / attention wider than its tensors' halves");
    }
  }
  for (auto& op : d.ops)
    if (op.kind == OP_STEM && d.tens[op.stem.x].split) return fail(PC_ERR_FORMAT, "op cannot read or write split tensors");
  for (auto& op : d.ops)
    if (const char* why = check_geometry(d, op)) return fail(PC_ERR_FORMAT, why);
  return PC_OK;
}

}  // namespace pc
