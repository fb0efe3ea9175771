// The network executor. A network arrives as a serialized "program" (person_capture_amd/program.py):
// buffers, NHWC tensor views, float arrays and a flat op list. pc_net_create decodes it (pc_program.cpp),
// plans it (pc_plan.cpp: a kernel and tile per conv and plan class, no device involved), then allocates and
// uploads what the plans need; a run resolves views to device pointers for its batch and launches the
// kernels in order on the context stream; optionally the whole run is captured into a HIP graph.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>
#include "pc_net_dev.h"

namespace pc {
hipError_t conv_launch(int f32, int rowb, int cfg, const ConvParams& p, hipStream_t s);
hipError_t conv_halo_launch(int f32, int cfg, const ConvParams& p, hipStream_t s);
hipError_t conv_fast_launch(int f32, int rowb, int cfg, const ConvParams& p, int wg_layout, hipStream_t s);
hipError_t conv_hx_launch(const ConvParams& p, int wlds, hipStream_t s);
hipError_t conv_hxg_launch(const ConvParams& p, int small, hipStream_t s);
hipError_t conv_hxi_launch(const ConvParams& p, int small, int occ1_28, int dense, hipStream_t s);
int conv_hxi_chain_ok(const ConvParams& p);
hipError_t conv_hxi_chain_launch(const void* d_layers, int nl, int HW, int N, int dense, hipStream_t s);
hipError_t conv_t2d_launch(const ConvParams& p, int variant, hipStream_t s);
hipError_t conv_chain_launch(const void* x, int xcs, void* y, int ycs, const void* blk_dev, int nblk, int N, int H,
                             int W, long long ktot, int dbg, hipStream_t s);
size_t conv_chain_block_bytes();
int stem_fused_ok(int f32, int cin, int cin_true, int KH, int KW, int npad, int cwrite, int ycs, int ycoff);
hipError_t stem_fused_launch(const StemParams& p, const void* wpk, const float* bias, const float* slope, int npad,
                             int cwrite, hipStream_t s);
hipError_t splitk_finish_launch(int f32, const ConvParams& p, hipStream_t s);
hipError_t absmax_f16_launch(const void* x, long long npix, int C, int cs, unsigned* out, hipStream_t s);
hipError_t stem_launch(int f32, const StemParams& p, hipStream_t s);
hipError_t maxpool_launch(int f32, const PoolParams& p, hipStream_t s);
hipError_t stem_im2col_launch(int f32, const StemParams& p, int cin_true, void* col, hipStream_t s);
// pc_ops.hip
struct UpsampleParams { const void* x; int N, H, W, C, xcs; void* y; int ycs; };
hipError_t upsample2_launch(int f32, const UpsampleParams& p, hipStream_t s);
struct LayerNormParams {
  const void* x; int xcs; void* y; int ycs; int M, C, cwrite;
  const float* gamma; const float* beta; const float* add; int rows; float eps; int xlo, ylo;
};
hipError_t layernorm_launch(int f32, const LayerNormParams& p, hipStream_t s);
struct AttnParams { const void* qkv; int qcs; void* out; int ocs; int N, T, heads; float scale; int qlo, olo; };
hipError_t attention_launch(int f32, const AttnParams& p, int head_dim, int stream_form, hipStream_t s);
}  // namespace pc

using namespace pc;

// bytes from a tensor's base to the zero tail of the buffer that holds it
static unsigned tensor_zero_off(const pc_net* n, int t) {
  const NetTensor& T = n->tens[t];
  const int es = esize(n, T.is_f32);
  const size_t end = T.buf < 0 ? n->in_img_bytes * n->max_batch : (size_t)n->bufs[T.buf].elems * n->max_batch * es;
  return (unsigned)(end - (size_t)T.coff * es);
}

static int upload(pc_ctx* c, void** d, const void* h, size_t bytes, const char* what) {
  if (hipMalloc(d, bytes) != hipSuccess || hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) != hipSuccess)
    return fail(c, PC_ERR_HIP, std::string(what) + " upload failed");
  return PC_OK;
}

// The MFMA stem's weights, repacked [npad][32], tap-major, channel-minor, with its bias and slopes
static int upload_stem(pc_net* n, const StemOp& op, StemPlan& st) {
  pc_ctx* c = n->ctx;
  const int KH = op.KH, KW = op.KW, cout = op.cout, cin_true = st.cin_true, esz = n->f32 ? 4 : 2;
  const float* hw = n->data + n->arrays[op.w].off;
  std::vector<float> wf((size_t)st.npad * 32, 0.f), b(st.npad, 0.f), sl(st.npad, 0.f);
  for (int co = 0; co < cout; ++co)
    for (int t = 0; t < KH * KW; ++t)
      for (int ci = 0; ci < cin_true; ++ci) wf[(size_t)co * 32 + t * cin_true + ci] = hw[((size_t)co * KH * KW + t) * 4 + ci];
  const float* hb = n->data + n->arrays[op.bias].off;
  for (int co = 0; co < cout; ++co) b[co] = hb[co];
  if (op.slope >= 0) {
    const float* hs = n->data + n->arrays[op.slope].off;
    for (int co = 0; co < cout; ++co) sl[co] = hs[co];
  }
  int rc;
  if (st.split) {   // rows of 64: K 0-31 W_hi, 32-63 W_lo = f16(W - W_hi)
    std::vector<_Float16> h((size_t)st.npad * 64);
    for (int co = 0; co < st.npad; ++co)
      for (int k = 0; k < 32; ++k) {
        const float v = wf[(size_t)co * 32 + k];
        const _Float16 hi = (_Float16)v;
        h[(size_t)co * 64 + k] = hi;
        h[(size_t)co * 64 + 32 + k] = (_Float16)(v - (float)hi);
      }
    rc = upload(c, &st.w, h.data(), h.size() * 2, "stem weight");
  } else if (n->f32) {
    rc = upload(c, &st.w, wf.data(), wf.size() * 4, "stem weight");
  } else {
    std::vector<_Float16> h(wf.size());
    for (size_t k = 0; k < wf.size(); ++k) h[k] = (_Float16)wf[k];
    rc = upload(c, &st.w, h.data(), h.size() * esz, "stem weight");
  }
  if (rc == PC_OK) rc = upload(c, (void**)&st.bias, b.data(), st.npad * 4, "stem bias");
  if (rc == PC_OK && op.slope >= 0) rc = upload(c, (void**)&st.slope, sl.data(), st.npad * 4, "stem slope");
  return rc;
}

// Runs of IResNet identity blocks that the resident chain kernel (pc_conv_chain.hip) can
// execute as one launch: conv1 = 3x3/s1 over X with the border-class bias and PReLU,
// conv2 = 3x3/s1 over conv1's output + bias + residual X, 256 channels, images of at
// most 199 pixels, f16. Every tensor between the chain's first input and its last output
// must be read only inside the chain (the kernel never writes them).
static int plan_chains(pc_net* n) {
  n->chain_at.assign(n->ops.size(), -1);
  n->chain_min_batch = n->tune.chain_min_batch;
  if (n->f32 || !n->tune.chain) return PC_OK;
  if ((size_t)conv_chain_block_bytes() != sizeof(ChainBlockH)) return fail(n->ctx, PC_ERR_HIP, "chain block layout");
  const int nt = (int)n->tens.size();
  std::vector<int> uses(nt, 0);
  for (auto& op : n->ops) for_each_input(op, [&](int t) { uses[t]++; });
  for (int o : n->outs) uses[o] += 1000;
  // a one-segment 3x3 / stride 1 / pad 1 conv of 256 -> 256 channels over tensor X, no split-K, act before the residual
  auto conv3x3_256 = [&](const NetOp& op, int X) {
    const ConvOp& a = op.conv;
    return op.kind == OP_CONV && a.nseg == 1 && a.seg[0].x == X && a.seg[0].KH == 3 && a.seg[0].KW == 3 &&
           a.seg[0].stride == 1 && a.seg[0].pad == 1 && a.npad == 256 && a.cout == 256 && a.bias >= 0 &&
           a.act_after_res == 0 && a.splitk == 1;
  };
  auto is_block = [&](size_t i, int X) -> int {   // output tensor of the block at ops i, i+1, or -1
    if (i + 1 >= n->ops.size()) return -1;
    const ConvOp &a = n->ops[i].conv, &b = n->ops[i + 1].conv;
    if (!conv3x3_256(n->ops[i], X) || a.bias_mode != BIAS_BORDER9 || a.slope < 0 || a.act != ACT_PRELU || a.res >= 0)
      return -1;
    const int Y1 = a.out;
    if (!conv3x3_256(n->ops[i + 1], Y1) || b.bias_mode != BIAS_CHANNEL || b.act != ACT_NONE || b.res != X ||
        b.res_mode != RES_SAME || a.ktot != b.ktot)
      return -1;
    const NetTensor &TX = n->tens[X], &T1 = n->tens[Y1], &T2 = n->tens[b.out];
    if (TX.is_f32 || T1.is_f32 || T2.is_f32 || TX.buf < 0 || T2.buf < 0) return -1;
    if (TX.C != 256 || T1.C != 256 || T2.C != 256 || T1.H != TX.H || T1.W != TX.W || T2.H != TX.H || T2.W != TX.W)
      return -1;
    if (!conv_chain_fits(TX.H, TX.W, TX.C, a.npad, a.ktot)) return -1;
    if (uses[Y1] != 1) return -1;   // conv1's output feeds conv2 only
    return b.out;
  };
  for (size_t i = 0; i + 1 < n->ops.size();) {
    const int X = n->ops[i].kind == OP_CONV ? n->ops[i].conv.seg[0].x : -1;
    int out = X >= 0 ? is_block(i, X) : -1;
    if (out < 0) { ++i; continue; }
    ChainPlan ch;
    ch.first = (int)i;
    ch.in_t = X;
    ch.nblk = 1;
    ch.ktot = n->ops[i].conv.ktot;
    // X is read twice by the first block (conv1 input and residual); later block inputs
    // must be read by their block only
    while (uses[out] == 2) {
      const int nxt = is_block(i + 2 * ch.nblk, out);
      if (nxt < 0) break;
      out = nxt;
      ch.nblk++;
    }
    ch.out_t = out;
    const NetTensor &TX = n->tens[X], &TY = n->tens[out];
    const bool alias_ok = TX.buf != TY.buf || (TX.cs == TY.cs && TX.coff == TY.coff);
    if (ch.nblk < 2 || !alias_ok || (TX.cs & 7) || (TY.cs & 7) || (TX.coff & 7) || (TY.coff & 7)) {
      i += 2 * ch.nblk;
      continue;
    }
    std::vector<ChainBlockH> hb(ch.nblk);
    // weight layout of the kernel's register stream (tuning: PC_CHAIN_WL): 0 the convs'
    // own [256][ktot] rows; 1 / 2 repacked fragment-major, 1 KiB per (K-step j, channel
    // group g, row block a) holding W[g*64 + a*16 + (l & 15)][j*32 + (l >> 4)*8 .. +7] at
    // +16*l, ordered [j][g][a] (1) or [g][a][j] (2)
    ch.wl = n->tune.chain_wl;
    const size_t cbytes = (size_t)72 * 256 * 64;
    if (ch.wl) {
      HIPCHK(n->ctx, hipMalloc(&ch.d_wpack, cbytes * 2 * ch.nblk));
      n->chains.push_back(ch);   // (owned by the net from here: an error below frees it with the net)
      const long long ktot = ch.ktot;
      std::vector<_Float16> src((size_t)256 * ktot), dst(cbytes / 2);
      for (int cv = 0; cv < 2 * ch.nblk; ++cv) {
        HIPCHK(n->ctx, hipMemcpy(src.data(), n->dev_arrays[n->ops[i + cv].conv.w], src.size() * 2, hipMemcpyDeviceToHost));
        for (int j = 0; j < 72; ++j)
          for (int g = 0; g < 4; ++g)
            for (int a = 0; a < 4; ++a)
              for (int l = 0; l < 64; ++l) {
                const _Float16* sp = &src[(size_t)(g * 64 + a * 16 + (l & 15)) * ktot + j * 32 + (l >> 4) * 8];
                const size_t blk1k = ch.wl == 1 ? ((size_t)j * 4 + g) * 4 + a : ((size_t)g * 4 + a) * 72 + j;
                _Float16* dp = &dst[(blk1k * 64 + l) * 8];
                for (int e = 0; e < 8; ++e) dp[e] = sp[e];
              }
        HIPCHK(n->ctx, hipMemcpy((char*)ch.d_wpack + cbytes * cv, dst.data(), cbytes, hipMemcpyHostToDevice));
      }
    } else {
      n->chains.push_back(ch);
    }
    for (int k = 0; k < ch.nblk; ++k) {
      const ConvOp &a = n->ops[i + 2 * k].conv, &b = n->ops[i + 2 * k + 1].conv;
      const void* w1 = ch.wl ? (const void*)((char*)ch.d_wpack + cbytes * (2 * k)) : n->dev_arrays[a.w];
      const void* w2 = ch.wl ? (const void*)((char*)ch.d_wpack + cbytes * (2 * k + 1)) : n->dev_arrays[b.w];
      hb[k] = ChainBlockH{w1, (const float*)n->dev_arrays[a.bias], (const float*)n->dev_arrays[a.slope], w2,
                          (const float*)n->dev_arrays[b.bias]};
      ch.flops_per_image += n->plans[i + 2 * k].flops_per_image + n->plans[i + 2 * k + 1].flops_per_image;
    }
    n->chains.back().flops_per_image = ch.flops_per_image;
    int rc = upload(n->ctx, &n->chains.back().d_blk, hb.data(), hb.size() * sizeof(ChainBlockH), "chain blocks");
    if (rc) return rc;
    n->chain_at[i] = (int)n->chains.size() - 1;
    i += 2 * ch.nblk;
  }
  return PC_OK;
}

static void conv_params(pc_net* n, size_t i, const ConvPlan& pl, int N, ConvParams& p);

// The chained launches of every plan class (PC_CONV_HXI bit 6): see find_hxi_runs. The layers' kernel
// parameters do not depend on the batch (the kernel takes it from its grid), so each class's array is
// built and uploaded here, once.
static int plan_hxi_runs(pc_net* n) {
  n->hxi_runs.clear();
  // (PC_CONV_DBG strips phases of the per-layer kernels: phase splits measure those)
  if (n->f32 || !(n->tune.hxi_mask & 64) || n->tune.conv_dbg_set) return PC_OK;
  const int nops = (int)n->ops.size();
  std::vector<int32_t> elig(nops);
  std::vector<int32_t> outs(n->outs.begin(), n->outs.end());
  n->hxi_runs.resize(1 + n->plans_cls.size());
  for (size_t k = 0; k < n->hxi_runs.size(); ++k) {
    const std::vector<ConvPlan>& plans = k ? n->plans_cls[k - 1] : n->plans;
    HxiRuns& R = n->hxi_runs[k];
    R.at.assign(nops, -1);
    std::vector<ConvParams> params(nops);
    bool any = false;
    for (int i = 0; i < nops; ++i) {
      elig[i] = 0;
      if (n->ops[i].kind != OP_CONV || (plans[i].hx != 3 && plans[i].hx != 6) || plans[i].splitk != 1) continue;
      const ConvOp& op = n->ops[i].conv;
      // every tensor a layer touches lives in a buffer and has the map's geometry (H W cs elements per image), so
      // tensors that share a buffer overlap image by image only - a workgroup's layers never touch another
      // image's bytes, whichever layer the other workgroups are at
      const NetTensor &X = n->tens[op.seg[0].x], &Y = n->tens[op.out];
      bool ok = X.buf >= 0 && Y.buf >= 0 && X.split && Y.split && X.H == Y.H && X.W == Y.W && X.cs == Y.cs;
      if (ok && op.res >= 0) {
        const NetTensor& T = n->tens[op.res];
        ok = T.buf >= 0 && T.H == Y.H && T.W == Y.W && T.cs == Y.cs;
      }
      if (!ok) continue;
      conv_params(n, i, plans[i], 0, params[i]);
      elig[i] = conv_hxi_chain_ok(params[i]);
      any = any || elig[i];
    }
    if (!any) continue;
    std::vector<std::pair<int, int>> launches;
    find_hxi_runs(n->words.data(), nops, elig.data(), outs.data(), (int)outs.size(), n->tune.hxi_chain_max, launches);
    std::vector<ConvParams> packed;
    for (auto& l : launches) {
      HxiRun r;
      r.first = l.first;
      r.nl = l.second;
      r.hw = n->tens[n->ops[l.first].out()].H;
      r.param_off = packed.size();
      for (int i = l.first; i < l.first + l.second; ++i) {
        packed.push_back(params[i]);
        r.flops_per_image += n->plans[i].flops_per_image;
      }
      R.at[l.first] = (int)R.runs.size();
      R.runs.push_back(r);
    }
    int rc = upload(n->ctx, &R.d_params, packed.data(), packed.size() * sizeof(ConvParams), "conv_hxi chain parameters");
    if (rc) return rc;
  }
  return PC_OK;
}

// OCP e4m3fn encoding (round to nearest even, saturating at +-448): the host side of the f16c8
// weight bytes; the device encodes activations with v_cvt_pk_fp8_f32 (pc_conv_common.h f8_pack8)
static uint8_t e4m3_encode(float v) {
  const uint8_t sgn = std::signbit(v) ? 0x80 : 0;
  const float a = std::fabs(v);
  if (!(a == a)) return 0x7f;
  if (a >= 448.f) return sgn | 0x7e;
  int e2 = 0;
  std::frexp(a, &e2);
  int E = e2 - 1;                                 // a in [2^E, 2^(E+1))
  if (a == 0.f || E < -6) {                       // subnormals: steps of 2^-9
    const int q = (int)std::nearbyint(std::ldexp(a, 9));
    return sgn | (uint8_t)q;                      // q == 8 is the smallest normal's encoding
  }
  int q = (int)std::nearbyint(std::ldexp(a, 3 - E));   // 8 .. 16
  if (q == 16) { q = 8; ++E; }
  if (E > 8 || (E == 8 && q > 14)) return sgn | 0x7e;
  return sgn | (uint8_t)(((E + 7) << 3) | (q - 8));
}

// Fragment-ordered copy of a fused f16x3 conv's weights (conv_fast WG, conv_hx64): K tiles of 32
// channels in the fused tiles' order at 64-byte rows (segment, group of 64 hi channels, tap row, tap
// column, 32-channel block; ConvSeg::gt); per tile
// npad / 16 row blocks of [W_hi, W_lo] fragments, each 64 lanes x 8 f16 (lane l: row l & 15,
// channels 8 (l >> 4) .. +8), so a wave's fragment read is one contiguous KiB.
static int pack_wfrag(pc_net* n, const ConvOp& op, const float* wf, void** out) {
  const int npad = op.npad;
  const long long ktot = op.ktot;
  if (op.nseg == 1 && !n->tens[op.seg[0].x].split) {
    // plain f16 (conv_hxi's plain form): K tiles of 32 channels tap-major (tap row, tap column,
    // 32-channel block: conv_fast's plain K order), per tile npad / 16 row blocks of W fragments
    const int C = n->tens[op.seg[0].x].C, KH = op.seg[0].KH, KW = op.seg[0].KW;
    if (C % 32 || (long long)KH * KW * C != ktot || npad % 16) return fail(n->ctx, PC_ERR_FORMAT, "wfrag: plain K layout");
    const long long nkt = (long long)KH * KW * (C / 32), tile_elems = (long long)(npad / 16) * 512;
    std::vector<_Float16> h((size_t)(nkt * tile_elems));
    for (long long kt = 0; kt < nkt; ++kt)
      for (int rb = 0; rb < npad / 16; ++rb)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const long long row = rb * 16 + (l & 15), k = kt * 32 + (l >> 4) * 8 + j;
            h[(size_t)(kt * tile_elems + ((long long)rb * 64 + l) * 8 + j)] = (_Float16)wf[row * ktot + k];
          }
    return upload(n->ctx, out, h.data(), h.size() * 2, "wfrag");
  }
  long long nkt = 0, k0 = 0;
  for (int sg = 0; sg < op.nseg; ++sg) {
    const NetTensor& X = n->tens[op.seg[sg].x];
    if (!X.split || (X.C / 2) % 32) return fail(n->ctx, PC_ERR_FORMAT, "wfrag: split inputs of 32-channel blocks");
    nkt += (long long)op.seg[sg].KH * op.seg[sg].KW * (X.C / 2 / 32);
    k0 += (long long)op.seg[sg].KH * op.seg[sg].KW * 3 * (X.C / 2);
  }
  if (k0 != ktot || npad % 16) return fail(n->ctx, PC_ERR_FORMAT, "wfrag: K layout");
  const long long tile_elems = (long long)(npad / 16) * 2 * 512;
  std::vector<_Float16> h((size_t)(nkt * tile_elems));
  long long kt = 0;
  k0 = 0;
  for (int sg = 0; sg < op.nseg; ++sg) {
    const int cp = n->tens[op.seg[sg].x].C / 2, KH = op.seg[sg].KH, KW = op.seg[sg].KW;
    const int gt = cp % 64 == 0 ? 2 : 1;   // the fused tiles' channel groups at 64-byte K rows
    for (int g0 = 0; g0 < cp / 32; g0 += gt)
      for (int th = 0; th < KH; ++th)
        for (int tw = 0; tw < KW; ++tw)
          for (int cb = g0; cb < g0 + gt; ++cb, ++kt) {
            const long long kbase = k0 + (long long)(th * KW + tw) * 3 * cp + cb * 32;
            for (int rb = 0; rb < npad / 16; ++rb)
              for (int hf = 0; hf < 2; ++hf)
                for (int l = 0; l < 64; ++l)
                  for (int j = 0; j < 8; ++j) {
                    const long long row = rb * 16 + (l & 15);
                    const long long k = kbase + (hf ? 2 * cp : 0) + (l >> 4) * 8 + j;
                    h[(size_t)(kt * tile_elems + ((long long)(rb * 2 + hf) * 64 + l) * 8 + j)] = (_Float16)wf[row * ktot + k];
                  }
          }
    k0 += (long long)KH * KW * 3 * cp;
  }
  return upload(n->ctx, out, h.data(), h.size() * 2, "wfrag");
}

// f16c8 conv weights: the program holds the split form [W_hi, W_hi, W_lo] per tap and
// segment; the W_lo block's bytes become, per 32 input channels, [W_hi8 x 32 | W_lo8 x 32] (e4m3 of
// W_hi * 2^sh and W_lo * 2^sl, one exponent pair per conv). *wf8s gets their E8M0 scales.
static int pack_c8_weights(pc_net* n, const ConvOp& op, const float* wf, long long cnt, std::vector<_Float16>& h,
                           int* wf8s) {
  const int npad = op.npad;
  const long long ktot = op.ktot;
  if ((long long)npad * ktot != cnt) return fail(n->ctx, PC_ERR_FORMAT, "f16c8 weights: array size");
  float mh = 0.f, ml = 0.f;
  struct Blk { long long k0; int cp, taps; };
  std::vector<Blk> segs;
  long long k0 = 0;
  for (int sg = 0; sg < op.nseg; ++sg) {
    const NetTensor& X = n->tens[op.seg[sg].x];
    if (!X.c8) return fail(n->ctx, PC_ERR_FORMAT, "f16c8 weights: non-f16c8 segment");
    const int cp = X.C / 2, taps = op.seg[sg].KH * op.seg[sg].KW;
    segs.push_back({k0, cp, taps});
    k0 += (long long)taps * 3 * cp;
  }
  if (k0 != ktot) return fail(n->ctx, PC_ERR_FORMAT, "f16c8 weights: K layout");
  for (const Blk& b : segs)
    for (int r = 0; r < npad; ++r)
      for (int t = 0; t < b.taps; ++t) {
        const float* row = wf + (long long)r * ktot + b.k0 + (long long)t * 3 * b.cp;
        for (int c = 0; c < b.cp; ++c) {
          mh = std::max(mh, std::fabs(row[c]));
          ml = std::max(ml, std::fabs(row[2 * b.cp + c]));
        }
      }
  // the largest magnitude of each half lands in [224, 448)
  const int sh = mh > 0.f ? (int)std::floor(std::log2(448.f / mh)) : 0;
  const int sl = ml > 0.f ? (int)std::floor(std::log2(448.f / ml)) : 0;
  if (127 - sh < 1 || 127 - sh > 254 || 127 - sl < 1 || 127 - sl > 254)
    return fail(n->ctx, PC_ERR_FORMAT, "f16c8 weights: scale out of range");
  for (const Blk& b : segs)
    for (int r = 0; r < npad; ++r)
      for (int t = 0; t < b.taps; ++t) {
        const long long base = (long long)r * ktot + b.k0 + (long long)t * 3 * b.cp;
        uint8_t* dst = reinterpret_cast<uint8_t*>(&h[base + 2 * b.cp]);
        for (int c = 0; c < b.cp; ++c) {
          dst[(c >> 5) * 64 + (c & 31)] = e4m3_encode(std::ldexp(wf[base + c], sh));
          dst[(c >> 5) * 64 + 32 + (c & 31)] = e4m3_encode(std::ldexp(wf[base + 2 * b.cp + c], sl));
        }
      }
  *wf8s = (127 - sh) | ((127 - sl) << 8);
  return PC_OK;
}

// Step 3 of pc_net_create: everything the plans need on the device
static int materialise(pc_net* n) {
  pc_ctx* c = n->ctx;
  const int narr = (int)n->arrays.size(), max_batch = n->max_batch;
  // which arrays are conv weights (uploaded in the activation dtype)
  std::vector<int> is_w(narr, 0), c8_op(narr, -1);
  n->wf8s.assign(n->ops.size(), 0);
  for (size_t i = 0; i < n->ops.size(); ++i) {
    if (n->ops[i].kind != OP_CONV) continue;
    const ConvOp& op = n->ops[i].conv;
    is_w[op.w] = 1;
    if (n->tens[op.seg[0].x].c8) c8_op[op.w] = (int)i;
  }
  n->dev_arrays.assign(narr, nullptr);
  int rc = PC_OK;
  for (int i = 0; i < narr; ++i) {
    const long long off = n->arrays[i].off, cnt = n->arrays[i].cnt;
    if (is_w[i] && !n->f32) {
      std::vector<_Float16> h(cnt);
      for (long long k = 0; k < cnt; ++k) h[k] = (_Float16)n->data[off + k];
      if (c8_op[i] >= 0 && (rc = pack_c8_weights(n, n->ops[c8_op[i]].conv, n->data + off, cnt, h, &n->wf8s[c8_op[i]])))
        return rc;
      if (hipMalloc(&n->dev_arrays[i], cnt * 2 + 16) != hipSuccess ||
          hipMemcpy(n->dev_arrays[i], h.data(), cnt * 2, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, PC_ERR_HIP, "weight upload failed");
    } else if (hipMalloc(&n->dev_arrays[i], cnt * 4 + 16) != hipSuccess ||
               hipMemcpy(n->dev_arrays[i], n->data + off, cnt * 4, hipMemcpyHostToDevice) != hipSuccess) {
      return fail(c, PC_ERR_HIP, "array upload failed");
    }
  }
  n->buf_d.assign(n->bufs.size(), nullptr);
  for (size_t i = 0; i < n->bufs.size(); ++i) {
    const NetBuf& b = n->bufs[i];
    const size_t bytes = (size_t)b.elems * max_batch * ((b.is_f32 || n->f32) ? 4 : 2) + kZeroTail;
    // the conv loader addresses activations with 32-bit offsets
    if (bytes >= (1ull << 32)) return fail(c, PC_ERR_ARG, "activation buffer exceeds 4 GiB; lower max_batch");
    if (hipMalloc(&n->buf_d[i], bytes) != hipSuccess) return fail(c, PC_ERR_HIP, "activation buffer allocation failed");
    hipMemset(n->buf_d[i], 0, bytes);  // channel padding lanes and the zero tail must read as zero
  }
  const NetTensor& I = n->tens[n->in_tensor];
  n->in_img_bytes = (size_t)I.H * I.W * I.cs * esize(n, I.is_f32);
  bool conv_reads_input = false;
  for (auto& op : n->ops)
    if (op.kind == OP_CONV)
      for (int s = 0; s < op.conv.nseg; ++s)
        if (n->tens[op.conv.seg[s].x].buf < 0) conv_reads_input = true;
  if (conv_reads_input) {
    const size_t bytes = n->in_img_bytes * max_batch + kZeroTail;
    if (bytes >= (1ull << 32)) return fail(c, PC_ERR_ARG, "input buffer exceeds 4 GiB; lower max_batch");
    if (hipMalloc(&n->in_copy, bytes) != hipSuccess) return fail(c, PC_ERR_HIP, "input copy allocation failed");
    hipMemset(n->in_copy, 0, bytes);
  }
  for (size_t i = 0; i < n->ops.size(); ++i)
    if (n->ops[i].kind == OP_STEM && n->stems[i].use_mfma && (rc = upload_stem(n, n->ops[i].stem, n->stems[i]))) return rc;
  // fragment-ordered weights for the convs any plan runs on the WG form
  n->wfrag.assign(n->ops.size(), nullptr);
  for (size_t i = 0; i < n->ops.size(); ++i) {
    if (n->ops[i].kind != OP_CONV) continue;
    bool wg = n->plans[i].wg || n->plans[i].hx;   // (the halo-staged kernel reads the same copy)
    for (auto& pc : n->plans_cls) wg = wg || pc[i].wg || pc[i].hx;
    const ConvOp& op = n->ops[i].conv;
    if (wg && (rc = pack_wfrag(n, op, n->data + n->arrays[op.w].off, &n->wfrag[i]))) return rc;
  }
  if (n->stem_col_bytes) {
    if (hipMalloc(&n->stem_col, n->stem_col_bytes) != hipSuccess) return fail(c, PC_ERR_HIP, "stem im2col workspace");
    hipMemset(n->stem_col, 0, n->stem_col_bytes);
  }
  if (n->partial_bytes && hipMalloc((void**)&n->partial, n->partial_bytes) != hipSuccess)
    return fail(c, PC_ERR_HIP, "split-K workspace");
  return PC_OK;
}

extern "C" int pc_net_create(pc_ctx* c, const void* prog, size_t nbytes, int precision, int max_batch, pc_net** out) {
  if (!c || !prog || !out || max_batch <= 0) return fail(c, PC_ERR_ARG, "pc_net_create: bad arguments");
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  pc_net* n = new pc_net();
  n->ctx = c;
  n->tune = tuning_from_env();
  std::string err;
  int rc = decode_program(prog, nbytes, precision, max_batch, *n, err);   // 1. decode and validate
  if (rc == PC_OK) rc = plan_net(*n, n->tune, *n, err);                   // 2. plan (no device)
  if (rc != PC_OK) fail(c, rc, err);
  if (rc == PC_OK) rc = materialise(n);                                   // 3. allocate and upload
  if (rc == PC_OK) rc = plan_chains(n);                                   // 4. launches that need device addresses
  if (rc == PC_OK) rc = plan_hxi_runs(n);
  n->data = nullptr;   // (the caller's blob)
  n->ndata = 0;
  if (rc != PC_OK) {
    pc_net_destroy(n);
    return rc;
  }
  *out = n;
  return PC_OK;
}

extern "C" int pc_net_destroy(pc_net* n) {
  if (!n) return PC_OK;
  hipSetDevice(n->ctx->device);
  hipStreamSynchronize(n->ctx->stream);
  for (auto& kv : n->graphs) hipGraphExecDestroy(kv.second);
  if (n->cap_stream) hipStreamDestroy(n->cap_stream);
  if (n->d_absmax) hipFree(n->d_absmax);
  for (void* a : n->dev_arrays) if (a) hipFree(a);
  for (void* a : n->wfrag) if (a) hipFree(a);
  for (void* b : n->buf_d) if (b) hipFree(b);
  if (n->partial) hipFree(n->partial);
  if (n->prep) hipFree(n->prep);
  if (n->in_copy) hipFree(n->in_copy);
  for (auto& st : n->stems) {
    if (st.w) hipFree(st.w);
    if (st.bias) hipFree(st.bias);
    if (st.slope) hipFree(st.slope);
  }
  if (n->stem_col) hipFree(n->stem_col);
  for (auto& R : n->hxi_runs) if (R.d_params) hipFree(R.d_params);
  for (auto& ch : n->chains) {
    if (ch.d_blk) hipFree(ch.d_blk);
    if (ch.d_wpack) hipFree(ch.d_wpack);
  }
  delete n;
  return PC_OK;
}

static int prof_event(pc_net* n, int* idx) {
  if (n->ev_used == n->ev_pool.size()) {
    hipEvent_t e;
    HIPCHK(n->ctx, hipEventCreate(&e));
    n->ev_pool.push_back(e);
  }
  *idx = (int)n->ev_used++;
  HIPCHK(n->ctx, hipEventRecord(n->ev_pool[*idx], n->ctx->stream));
  return PC_OK;
}

// start a profile record: an op's end event is the next op's start event (open_ev), else a new one
static int prof_begin(pc_net* n, bool prof, int open_ev, ProfRec& rec) {
  if (!prof) return PC_OK;
  if (open_ev >= 0) {
    rec.a = open_ev;
    return PC_OK;
  }
  return prof_event(n, &rec.a);
}

// plan class of a run of N images (-1: the max-batch plans)
static int plan_class(const pc_net* n, int N) {
  for (size_t c = 0; c < n->cls_batch.size(); ++c)
    if (N <= n->cls_batch[c]) return (int)c;
  return -1;
}

// The kernel parameters of conv op i under plan pl for N images (tensor addresses as they are now: a
// tensor that is the net input follows pc_net::cur_input)
static void conv_params(pc_net* n, size_t i, const ConvPlan& pl, int N, ConvParams& p) {
  pc_ctx* c = n->ctx;
  const ConvOp& op = n->ops[i].conv;
  memset(&p, 0, sizeof(p));
  const NetTensor& Y = n->tens[op.out];
  p.nseg = op.nseg;
  const int bke = pl.rowb / (n->f32 ? 4 : 2);
  int kt = 0;
  for (int sg = 0; sg < p.nseg; ++sg) {
    const ConvSegOp& g = op.seg[sg];
    const NetTensor& X = n->tens[g.x];
    ConvSeg& S = p.seg[sg];
    S.x = tensor_ptr(n, g.x);
    S.zero_off = tensor_zero_off(n, g.x);
    S.H = X.H; S.W = X.W; S.C = X.C; S.cs = X.cs;
    S.KH = g.KH; S.KW = g.KW; S.stride = g.stride; S.pad = g.pad;
    S.cblk = X.C / bke;
    if (X.c8) S.f8s = (127 - X.e_lo) | ((127 - X.e_hi) << 8);
    if (X.split && pl.sx) {   // fused split tiles: the hi blocks; lo block = hi block + vwrap
      S.cblk = S.cblk / 2;
      S.vwrap = S.cblk;
      // channel groups of 64 hi channels where they divide the channels (ConvSeg::gt)
      S.gt = (X.C / 2) % 64 == 0 ? 64 / bke : 1;
    } else if (X.split) {     // virtual channel blocks [hi, lo, hi] (pc_common.h ConvSeg::vwrap)
      S.vwrap = S.cblk;
      S.cblk = S.cblk / 2 * 3;
    }
    S.kt = S.KH * S.KW * S.cblk;
    kt += S.kt;
  }
  p.w = n->dev_arrays[op.w];
  p.ktot = op.ktot;
  p.N = N; p.OH = Y.H; p.OW = Y.W; p.M = N * Y.H * Y.W;
  p.npad = op.npad;
  p.cout = op.cout;
  p.cwrite = std::min(Y.split ? Y.C / 2 : Y.C, p.npad);
  p.ysplit = Y.split ? Y.C / 2 : 0;
  p.y = tensor_ptr(n, op.out);
  p.ycs = Y.cs;
  p.out_f32 = Y.is_f32 && !n->f32 ? 1 : (n->f32 ? 1 : 0);
  p.bias = op.bias >= 0 ? (const float*)n->dev_arrays[op.bias] : nullptr;
  p.bias_mode = op.bias >= 0 ? op.bias_mode : 0;
  p.slope = op.slope >= 0 ? (const float*)n->dev_arrays[op.slope] : nullptr;
  p.act = op.act;
  p.res = op.res >= 0 ? tensor_ptr(n, op.res) : nullptr;
  p.res_mode = op.res >= 0 ? op.res_mode : 0;
  if (op.res >= 0) {
    const NetTensor& R = n->tens[op.res];
    p.rcs = R.cs; p.rH = R.H; p.rW = R.W;
    p.rsplit = R.split ? R.C / 2 : 0;
  }
  p.act_after_res = op.act_after_res;
  p.kt_total = kt;
  p.sx = pl.sx;
  p.c8 = pl.c8;
  p.wf8s = n->wf8s[i];
  p.wfrag = pl.wg || pl.hx ? n->wfrag[i] : nullptr;
  if (Y.c8) {
    p.yc8 = 1;
    p.ylo_mul = std::ldexp(1.f, Y.e_lo);
    p.yhi_mul = std::ldexp(1.f, Y.e_hi);
  }
  if (op.res >= 0 && n->tens[op.res].c8) {
    p.rc8 = 1;
    p.rlo_inv = std::ldexp(1.f, -n->tens[op.res].e_lo);
  }
  p.splitk = pl.splitk;
  p.partial = n->partial;
  p.zero = c->zero;
  p.dbg = n->tune.conv_dbg;
}

static void stem_params(pc_net* n, const StemOp& op, int N, StemParams& p) {
  memset(&p, 0, sizeof(p));
  const NetTensor &X = n->tens[op.x], &Y = n->tens[op.out];
  p.x = tensor_ptr(n, op.x);
  p.N = N; p.H = X.H; p.W = X.W; p.cin = X.C; p.xcs = X.cs;
  p.OH = Y.H; p.OW = Y.W; p.KH = op.KH; p.KW = op.KW; p.stride = op.stride; p.pad = op.pad;
  p.w = (const float*)n->dev_arrays[op.w];
  p.cout = op.cout;
  p.bias = (const float*)n->dev_arrays[op.bias];
  p.slope = op.slope >= 0 ? (const float*)n->dev_arrays[op.slope] : nullptr;
  p.act = op.act;
  p.ycs = Y.cs;
  p.cpad = op.cpad;
  p.y = tensor_ptr(n, op.out);
  p.ysplit = Y.split ? Y.C / 2 : 0;
  if (Y.c8) {
    p.yc8 = 1;
    p.ylo_mul = std::ldexp(1.f, Y.e_lo);
    p.yhi_mul = std::ldexp(1.f, Y.e_hi);
  }
}

// the 1x1 conv over the im2col rows of an unfused MFMA stem
static void stem_conv_params(pc_net* n, const StemPlan& st, const StemParams& p, const NetTensor& Y, int N, ConvParams& q) {
  memset(&q, 0, sizeof(q));
  q.nseg = 1;
  ConvSeg& S = q.seg[0];
  S.x = n->stem_col;
  S.H = Y.H; S.W = Y.W; S.C = 32; S.cs = 32;
  S.KH = 1; S.KW = 1; S.stride = 1; S.pad = 0;
  S.cblk = 1; S.kt = 1;
  S.zero_off = (unsigned)((size_t)N * Y.H * Y.W * 32 * (n->f32 ? 4 : 2));
  q.w = st.w; q.ktot = 32;
  q.N = N; q.OH = Y.H; q.OW = Y.W; q.M = N * Y.H * Y.W;
  q.npad = st.npad; q.cout = p.cout; q.cwrite = std::min(Y.C, st.npad);
  q.y = p.y; q.ycs = Y.cs; q.out_f32 = n->f32 ? 1 : (Y.is_f32 ? 1 : 0);
  q.bias = st.bias; q.bias_mode = BIAS_CHANNEL;
  q.slope = st.slope; q.act = p.act;
  q.kt_total = 1; q.splitk = 1;
}

static void pool_params(pc_net* n, const PoolOp& op, int N, PoolParams& p) {
  const NetTensor &X = n->tens[op.x], &Y = n->tens[op.out];
  p.x = tensor_ptr(n, op.x); p.N = N; p.H = X.H; p.W = X.W; p.C = X.C; p.xcs = X.cs;
  p.y = tensor_ptr(n, op.out); p.OH = Y.H; p.OW = Y.W; p.ycs = Y.cs;
  p.k = op.k; p.stride = op.stride; p.pad = op.pad;
  p.split = X.split;
  if (X.split) p.C = X.C / 2;   // the hi half; lo at +C (the decoder checked Y.split == X.split)
}

static void upsample_params(pc_net* n, const UpsampleOp& op, int N, UpsampleParams& p) {
  const NetTensor &X = n->tens[op.x], &Y = n->tens[op.out];
  p.x = tensor_ptr(n, op.x); p.N = N; p.H = X.H; p.W = X.W; p.C = std::min(X.C, Y.C); p.xcs = X.cs;
  p.y = tensor_ptr(n, op.out); p.ycs = Y.cs;
}

static void layernorm_params(pc_net* n, const LayerNormOp& op, int N, LayerNormParams& p) {
  const NetTensor &X = n->tens[op.x], &Y = n->tens[op.out];
  p.x = tensor_ptr(n, op.x); p.xcs = X.cs;
  p.y = tensor_ptr(n, op.out); p.ycs = Y.cs;
  p.M = N * X.H * X.W; p.C = op.C; p.cwrite = Y.C;
  p.xlo = p.ylo = 0;
  if (X.split) { p.xlo = X.C / 2; p.ylo = p.cwrite = Y.C / 2; }   // (the decoder checked Y.split == X.split)
  p.gamma = (const float*)n->dev_arrays[op.gamma];
  p.beta = (const float*)n->dev_arrays[op.beta];
  p.add = op.add >= 0 ? (const float*)n->dev_arrays[op.add] : nullptr;
  p.rows = op.add >= 0 ? op.rows : 1;
  p.eps = op.eps;
}

static void attn_params(pc_net* n, const AttnOp& op, int N, AttnParams& p) {
  const NetTensor &Q = n->tens[op.x], &O = n->tens[op.out];
  p.qkv = tensor_ptr(n, op.x); p.qcs = Q.cs;
  p.out = tensor_ptr(n, op.out); p.ocs = O.cs;
  p.N = N; p.T = Q.H * Q.W; p.heads = op.heads;
  p.scale = 1.0f / sqrtf((float)op.head_dim);
  p.qlo = Q.split ? Q.C / 2 : 0;
  p.olo = O.split ? O.C / 2 : 0;
}

static int run_ops(pc_net* n, int N, hipStream_t s) {
  pc_ctx* c = n->ctx;
  const Tuning& tu = n->tune;
  // eager runs are profiled; a captured run records no events (its replays are not profiled)
  const bool prof = n->prof && !n->capturing;
  if (n->in_copy)
    HIPCHK(c, hipMemcpyAsync(n->in_copy, n->cur_input, n->in_img_bytes * N, hipMemcpyDeviceToDevice, s));
  // one event per op boundary: an op's end event is the next op's start event
  int open_ev = -1, rc;
  const int cls = plan_class(n, N);
  for (size_t i = 0; i < n->ops.size(); ++i) {
    const NetOp& op = n->ops[i];
    if (n->chain_at[i] >= 0 && N >= n->chain_min_batch) {
      // a run of identity blocks as one resident-chain launch (pc_conv_chain.hip)
      const ChainPlan& ch = n->chains[n->chain_at[i]];
      ProfRec rec{-1, -1, OP_CONV, ch.flops_per_image * N, (int)i, 300};
      if ((rc = prof_begin(n, prof, open_ev, rec))) return rc;
      const NetTensor &TX = n->tens[ch.in_t], &TY = n->tens[ch.out_t];
      // dbg: the weight layout, the weight path (1: LDS-DMA weight ring, measured faster than the register
      // stream) and PC_CONV_DBG's phase bits
      const int dbg = (ch.wl << 8) | (tu.chain_mode << 10) | (tu.conv_dbg & 7);
      HIPCHK(c, conv_chain_launch(tensor_ptr(n, ch.in_t), TX.cs, tensor_ptr(n, ch.out_t), TY.cs, ch.d_blk, ch.nblk, N,
                                  TX.H, TX.W, ch.ktot, dbg, s));
      if (prof) {
        if ((rc = prof_event(n, &rec.b))) return rc;
        n->recs.push_back(rec);
        open_ev = rec.b;
      }
      i += 2 * ch.nblk - 1;
      continue;
    }
    const HxiRuns* hr = n->hxi_runs.empty() ? nullptr : &n->hxi_runs[cls + 1];
    const HxiRun* run = hr && !n->calib && !hr->runs.empty() && hr->at[i] >= 0 ? &hr->runs[hr->at[i]] : nullptr;
    // (a chained conv_hxi launch is one timed record: its first op, its layers' FLOPs, kernel code 300)
    ProfRec rec{-1, -1, op.kind, run ? run->flops_per_image * N : op.kind == OP_CONV ? n->plans[i].flops_per_image * N : 0.0,
                (int)i, run ? 300 : -1};
    if ((rc = prof_begin(n, prof, open_ev, rec))) return rc;
    if (run) {
      rec.small = cls;
      HIPCHK(c, conv_hxi_chain_launch(static_cast<const ConvParams*>(hr->d_params) + run->param_off, run->nl, run->hw, N, tu.hxi_dense, s));
      i += run->nl - 1;
    } else if (op.kind == OP_CONV) {
      const ConvPlan& pl = cls >= 0 ? n->plans_cls[cls][i] : n->plans[i];
      rec.small = cls;
      ConvParams p;
      conv_params(n, i, pl, N, p);
      if (pl.hx >= 3 && pl.hx != 5) {
        HIPCHK(c, conv_hxi_launch(p, pl.hx >= 7, tu.hxi28_occ1, tu.hxi_dense, s));
      } else if (pl.hx == 2 || pl.hx == 5) {
        HIPCHK(c, conv_hxg_launch(p, pl.hx == 5, s));
      } else if (pl.hx) {
        HIPCHK(c, conv_hx_launch(p, tu.hx64_wlds, s));
      } else if (pl.t2d >= 0) {
        HIPCHK(c, conv_t2d_launch(p, pl.t2d, s));
      } else if (pl.fast >= 0) {
        HIPCHK(c, conv_fast_launch(n->f32, pl.rowb, pl.fast, p, tu.wg_layout, s));
      } else if (pl.halo >= 0) {
        HIPCHK(c, conv_halo_launch(n->f32, pl.halo, p, s));
      } else {
        HIPCHK(c, conv_launch(n->f32, pl.rowb, pl.cfg, p, s));
      }
      if (pl.splitk > 1) {
        HIPCHK(c, splitk_finish_launch(n->f32, p, s));
      }
    } else if (op.kind == OP_STEM) {
      StemParams p;
      stem_params(n, op.stem, N, p);
      const NetTensor &X = n->tens[op.stem.x], &Y = n->tens[op.stem.out];
      const StemPlan& st = n->stems[i];
      const int st_cwrite = std::min(Y.split ? Y.C / 2 : Y.C, st.npad);
      // fused gather + MFMA stem (pc_stem.hip) unless PC_STEM_UNFUSED was set
      // (stem_fused stores f16: an f32 output tensor inside an f16 net takes the unfused path)
      const bool fused = st.use_mfma && !tu.stem_unfused && !Y.is_f32 &&
                         stem_fused_ok(n->f32, X.C, st.cin_true, p.KH, p.KW, st.npad, st_cwrite, Y.cs, Y.coff) &&
                         X.cs % 4 == 0 && (reinterpret_cast<uintptr_t>(p.x) & 7) == 0 &&
                         (reinterpret_cast<uintptr_t>(p.y) & 15) == 0;
      if (st.split && !fused) return fail(c, PC_ERR_FORMAT, "split stem: the fused kernel cannot run this op");
      if (fused) {
        rec.kind = OP_CONV;
        rec.flops = n->plans[i].flops_per_image * N;
        HIPCHK(c, stem_fused_launch(p, st.w, st.bias, st.slope, st.npad, st_cwrite, s));
      } else if (!st.use_mfma) {
        HIPCHK(c, stem_launch(n->f32, p, s));
      } else {
        HIPCHK(c, stem_im2col_launch(n->f32, p, st.cin_true, n->stem_col, s));
        if (prof) {   // im2col counts as "other", the MFMA part as a conv launch
          if ((rc = prof_event(n, &rec.b))) return rc;
          n->recs.push_back(rec);
          const int b = rec.b;
          rec = ProfRec{b, -1, OP_CONV, n->plans[i].flops_per_image * N, (int)i};
        }
        ConvParams q;
        stem_conv_params(n, st, p, Y, N, q);
        // the statically scheduled kernel's 64x256 tile when it divides the channels
        if (st.npad % 64 == 0 && conv_fast_valid(4, st.rowb) && !tu.stem_generic)
          HIPCHK(c, conv_fast_launch(n->f32, st.rowb, 4, q, tu.wg_layout, s));
        else
          HIPCHK(c, conv_launch(n->f32, st.rowb, st.cfg, q, s));
      }
    } else if (op.kind == OP_MAXPOOL) {
      PoolParams p;
      pool_params(n, op.pool, N, p);
      HIPCHK(c, maxpool_launch(n->f32, p, s));
    } else if (op.kind == OP_UPSAMPLE) {
      UpsampleParams p;
      upsample_params(n, op.up, N, p);
      HIPCHK(c, upsample2_launch(n->f32, p, s));
    } else if (op.kind == OP_LAYERNORM) {
      LayerNormParams p;
      layernorm_params(n, op.ln, N, p);
      HIPCHK(c, layernorm_launch(n->f32, p, s));
    } else if (op.kind == OP_ATTENTION) {
      AttnParams p;
      attn_params(n, op.attn, N, p);
      HIPCHK(c, attention_launch(n->f32, p, op.attn.head_dim, tu.attn_stream, s));
    }
    if (n->calib && (op.kind == OP_CONV || op.kind == OP_STEM)) {   // pc_net_calibrate: max |x| of the op's output
      const NetTensor& Y = n->tens[op.out()];
      if (!Y.is_f32 && !n->f32)
        HIPCHK(c, absmax_f16_launch(tensor_ptr(n, op.out()), (long long)N * Y.H * Y.W, Y.split ? Y.C / 2 : Y.C, Y.cs,
                                    reinterpret_cast<unsigned*>(n->d_absmax) + op.out(), s));
    }
    if (prof) {
      if ((rc = prof_event(n, &rec.b))) return rc;
      n->recs.push_back(rec);
      open_ev = rec.b;
      // the other layers of a chained launch: a marker each (code 301, no time, no FLOPs - the launch's record
      // carries both), so a profiled run still has a record per op
      for (int k = 1; run && k < run->nl; ++k)
        n->recs.push_back(ProfRec{rec.b, rec.b, OP_CONV, 0.0, rec.op + k, 301, cls});
    }
  }
  return PC_OK;
}

// f16c8 scale calibration: one eager run over N images records every conv / stem
// output's largest magnitude; each f16c8 tensor then gets e_hi with max * 2^e_hi in
// [448 / 2^(headroom+1), 448 / 2^headroom) and e_lo = e_hi + 11 (|lo| <= 2^-11 |x|). The
// activations may grow 2^headroom times past the calibration before the e4m3 bytes saturate.
extern "C" int pc_net_calibrate(pc_net* n, const void* d_in, int N, int headroom_log2, float* h_absmax) {
  if (!n || !d_in || N <= 0 || N > n->max_batch || headroom_log2 < 0 || headroom_log2 > 8) return PC_ERR_ARG;
  pc_ctx* c = n->ctx;
  std::lock_guard<std::mutex> lk(n->graph_mu);
  const size_t nt = n->tens.size();
  if (!n->d_absmax) HIPCHK(c, hipMalloc((void**)&n->d_absmax, nt * 4));
  HIPCHK(c, hipMemsetAsync(n->d_absmax, 0, nt * 4, c->stream));
  n->cur_input = d_in;
  n->calib = 1;
  const int rc = run_ops(n, N, c->stream);
  n->calib = 0;
  if (rc) return rc;
  std::vector<float> mx(nt);
  HIPCHK(c, hipMemcpyAsync(mx.data(), n->d_absmax, nt * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t t = 0; t < nt; ++t) {
    NetTensor& T = n->tens[t];
    if (h_absmax) h_absmax[t] = mx[t];
    if (!T.c8 || !(mx[t] > 0.f) || !std::isfinite(mx[t])) continue;
    const int e = (int)std::floor(std::log2(448.f / mx[t])) - headroom_log2;
    if (127 - e < 1 || 127 - (e + 11) < 1 || 127 - e > 254) return fail(c, PC_ERR_FORMAT, "f16c8 scale out of range");
    T.e_hi = e;
    T.e_lo = e + 11;
  }
  // captured graphs hold the old scales as kernel arguments
  for (auto& kv : n->graphs) hipGraphExecDestroy(kv.second);
  n->graphs.clear();
  return PC_OK;
}

extern "C" int pc_net_profile(pc_net* n, int enable) {
  if (!n) return PC_ERR_ARG;
  HIPCHK(n->ctx, hipStreamSynchronize(n->ctx->stream));
  n->prof = enable ? 1 : 0;
  n->ev_used = 0;
  n->recs.clear();
  return PC_OK;
}

extern "C" int pc_net_profile_read(pc_net* n, double* out) {
  if (!n || !out) return PC_ERR_ARG;
  HIPCHK(n->ctx, hipStreamSynchronize(n->ctx->stream));
  double conv_ms = 0, other_ms = 0, flops = 0;
  int conv_n = 0, other_n = 0;
  for (const ProfRec& r : n->recs) {
    float ms = 0.f;
    HIPCHK(n->ctx, hipEventElapsedTime(&ms, n->ev_pool[r.a], n->ev_pool[r.b]));
    if (r.kind == OP_CONV) { conv_ms += ms; conv_n++; flops += r.flops; }
    else { other_ms += ms; other_n++; }
  }
  out[0] = conv_ms; out[1] = conv_n; out[2] = flops; out[3] = other_ms; out[4] = other_n;
  return PC_OK;
}

// Per-record detail of the profiled runs: 6 doubles per record
// [op index, kind, ms, flops, kernel, form]: the kernel and form of a per-layer conv launch as
// plan_kernel_code / plan_kernel_form (pc_net.h) give them; 300 the resident chain or a chained conv_hxi
// launch, 301 a further layer of the chained launch before it (0 ms, 0 flops); returns the count.
extern "C" int pc_net_profile_ops(pc_net* n, double* out, int max_recs) {
  if (!n || !out) return -PC_ERR_ARG;
  HIPCHK(n->ctx, hipStreamSynchronize(n->ctx->stream));
  int k = 0;
  for (const ProfRec& r : n->recs) {
    if (k >= max_recs) break;
    float ms = 0.f;
    HIPCHK(n->ctx, hipEventElapsedTime(&ms, n->ev_pool[r.a], n->ev_pool[r.b]));
    double* o = out + 6 * k++;
    const bool conv = r.op >= 0 && n->ops[r.op].kind == OP_CONV;
    o[0] = r.op; o[1] = r.kind; o[2] = ms; o[3] = r.flops;
    const ConvPlan* pl = conv ? (r.small >= 0 ? &n->plans_cls[r.small][r.op] : &n->plans[r.op]) : nullptr;
    o[4] = r.code >= 0 ? r.code : conv ? plan_kernel_code(*pl) : -1;
    // (a chain record's [5] is the generic tile of its first conv, as before)
    o[5] = !conv ? -1 : r.code >= 0 ? pl->cfg : plan_kernel_form(*pl);
  }
  return k;
}

extern "C" int pc_net_run(pc_net* n, const void* d_in, int N) {
  if (!n || !d_in) return PC_ERR_ARG;
  pc_ctx* c = n->ctx;
  if (N <= 0 || N > n->max_batch) return fail(c, PC_ERR_ARG, "batch out of range");
  n->cur_input = d_in;
  // (profiling runs eagerly: the per-op HIP events are the point of it)
  if (!n->use_graph || N > n->graph_max_batch || n->prof) return run_ops(n, N, c->stream);
  // Graphs are captured on a stream private to the net, never on the context stream: a context
  // (and its stream) is shared by every FaceEmbedder of the process, and work another host thread
  // enqueued there during an open capture would be recorded into this graph (not run now, replayed
  // later) or invalidate it. Capturing executes nothing, so the private stream needs no ordering
  // with the context stream; the instantiated graph is launched on the context stream. The lock
  // serialises capture and the graph table of one net between host threads.
  std::lock_guard<std::mutex> lk(n->graph_mu);
  auto key = std::make_pair(N, d_in);
  auto it = n->graphs.find(key);
  if (it == n->graphs.end()) {
    // (bounded: a graph per (batch, input) pair; callers with many batch sizes start over at 256)
    if (n->graphs.size() >= 256) {
      HIPCHK(c, hipStreamSynchronize(c->stream));   // (launched graphs may still run)
      for (auto& kv : n->graphs) hipGraphExecDestroy(kv.second);
      n->graphs.clear();
    }
    if (!n->cap_stream) HIPCHK(c, hipStreamCreateWithFlags(&n->cap_stream, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    HIPCHK(c, hipStreamBeginCapture(n->cap_stream, hipStreamCaptureModeThreadLocal));
    n->capturing = 1;
    int rc = run_ops(n, N, n->cap_stream);
    n->capturing = 0;
    hipError_t e = hipStreamEndCapture(n->cap_stream, &g);
    if (rc != PC_OK || e != hipSuccess) {   // a failed capture leaves no graph behind
      if (g) hipGraphDestroy(g);
      if (rc != PC_OK) return rc;
      return fail(c, PC_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
    }
    hipGraphExec_t ge;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) return fail(c, PC_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(e));
    it = n->graphs.emplace(key, ge).first;
  }
  HIPCHK(c, hipGraphLaunch(it->second, c->stream));
  return PC_OK;
}

extern "C" int pc_net_set_graph(pc_net* n, int enable) {
  if (!n) return PC_ERR_ARG;
  n->use_graph = enable ? 1 : 0;
  return PC_OK;
}
extern "C" int pc_net_set_graph_max_batch(pc_net* n, int32_t max_batch) {
  if (!n || max_batch < 1) return PC_ERR_ARG;
  n->graph_max_batch = max_batch;
  return PC_OK;
}

extern "C" int pc_net_input_dims(pc_net* n, int32_t* d) {
  if (!n || !d) return PC_ERR_ARG;
  const NetTensor& T = n->tens[n->in_tensor];
  d[0] = T.H; d[1] = T.W; d[2] = T.C; d[3] = T.cs;
  return PC_OK;
}
extern "C" int pc_net_num_outputs(pc_net* n) { return n ? (int)n->outs.size() : -1; }
extern "C" int pc_net_output(pc_net* n, int idx, void** d_ptr, int32_t* dims) {
  if (!n || idx < 0 || idx >= (int)n->outs.size()) return PC_ERR_ARG;
  const int t = n->outs[idx];
  const NetTensor& T = n->tens[t];
  if (d_ptr) *d_ptr = tensor_ptr(n, t);
  if (dims) { dims[0] = T.H; dims[1] = T.W; dims[2] = T.C; dims[3] = T.cs; dims[4] = (T.is_f32 || n->f32) ? 1 : 0; }
  return PC_OK;
}
extern "C" int pc_net_chain_info(pc_net* n, int32_t* min_batch, int32_t* per_round) {
  if (!n) return -PC_ERR_ARG;
  int ncu = 256;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, n->ctx->device) != hipSuccess || ncu <= 0)
    ncu = 256;
  if (min_batch) *min_batch = n->chain_min_batch;
  if (per_round) *per_round = ncu;
  return (int)n->chains.size();
}
extern "C" int pc_net_set_chain_min_batch(pc_net* n, int32_t min_batch) {
  if (!n) return -PC_ERR_ARG;
  const int v = min_batch <= 0 ? (1 << 30) : min_batch;
  if (v != n->chain_min_batch) {
    // captured graphs replay the launch schedule of their capture (chain or per-conv)
    hipStreamSynchronize(n->ctx->stream);
    for (auto& kv : n->graphs) hipGraphExecDestroy(kv.second);
    n->graphs.clear();
  }
  n->chain_min_batch = v;
  return 0;
}
extern "C" int pc_net_stats(pc_net* n, double* flops, int32_t* launches) {
  if (!n) return PC_ERR_ARG;
  if (flops) *flops = n->flops_per_image;
  if (launches) *launches = n->launches;
  return PC_OK;
}
