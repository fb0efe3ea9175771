// The planner: which kernel, tile and K-row width every conv of a program runs on, per plan class.
// Pure host logic over a decoded program (NetDesc) and the switches (Tuning): no device, no HIP types.
// Kernel choices carry the bit-identity contract of extract() / extract_batch(): every plan class of a
// conv accumulates in one order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "pc_net.h"

namespace pc {

// ---------------------------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------------------------
Tuning tuning_from_env() {
  Tuning t;
  auto given = [](const char* name) { return getenv(name) != nullptr; };
  auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  auto is = [&](const char* name, int v) { return given(name) && num(name, 0) == v; };

  // The override cascade. Forcing one kernel family means "test that family", so it disables the families
  // that would otherwise take the conv from it, in the planner's order of precedence
  // (igemm < halo < conv_fast < t2d < hx):
  //   PC_CONV_CFG=k   igemm tile k where it divides npad; halo, conv_fast, t2d and hx off unless given themselves
  //   PC_CONV_HALO    0 off, k + 1 halo tile k; conv_fast, t2d and hx off unless given themselves
  //   PC_CONV_FAST    0 off, k + 1 conv_fast tile k; t2d and hx off unless given themselves
  //   PC_CONV_T2D     0 off, 2 wherever it can run; hx off
  //   PC_T2D_SPLIT64, PC_SPLIT_FUSED (any value): hx off
  //   PC_CONV_HX=0    hx off
  const bool cfg = given("PC_CONV_CFG"), halo = given("PC_CONV_HALO"), fast = given("PC_CONV_FAST"),
             t2d = given("PC_CONV_T2D");
  if (cfg) {
    const int f = num("PC_CONV_CFG", -1);
    t.cfg_force = f >= 0 && f < kNumConvCfgs ? f : -1;
  }
  t.halo_force = halo ? num("PC_CONV_HALO", 0) : (cfg ? 0 : -1);
  t.fast_force = fast ? num("PC_CONV_FAST", 0) : (cfg || halo ? 0 : -1);
  t.t2d_mode = t2d ? num("PC_CONV_T2D", 0) : (cfg || halo || fast ? 0 : 1);
  t.hx_allowed = !is("PC_CONV_HX", 0) && !fast && !cfg && !halo && !t2d && !given("PC_T2D_SPLIT64") &&
                 !given("PC_SPLIT_FUSED");
  t.split_fused = !is("PC_SPLIT_FUSED", 0);

  t.rowb_set = given("PC_CONV_ROWB");
  t.rowb64 = is("PC_CONV_ROWB", 64);
  t.t2d_flags = (is("PC_T2D_SPLIT", 0) ? kT2dSplitOff : 0) | (given("PC_T2D_SPLIT64") ? kT2dSplit64 : 0) |
                (given("PC_T2D_NARROW") ? kT2dNarrow : 0) | (given("PC_T2D_NBUF3") ? kT2dNbuf3 : 0) |
                (given("PC_T2D_128") ? kT2d128 : 0) | (is("PC_T2D_128", 8) ? kT2d128x8 : 0);
  t.hxg_mask = num("PC_CONV_HXG", 3);
  t.hxi_mask = num("PC_CONV_HXI", kHxiDefaultMask);
  t.small_tiles = !is("PC_SMALL_TILES", 0);
  t.small_splitk = given("PC_SMALL_SPLITK");
  t.small_plans = !given("PC_NO_SMALL_PLANS");
  t.c8_rowb = is("PC_C8_ROWB", 128) ? 128 : 64;
  t.sx_wg = !is("PC_SX_WG", 0);
  t.stem_direct = given("PC_STEM_DIRECT");

  t.chain = !is("PC_CHAIN", 0);
  if (given("PC_CHAIN_MIN")) t.chain_min_batch = std::max(1, num("PC_CHAIN_MIN", 0));
  t.chain_wl = is("PC_CHAIN_WL", 2) ? 2 : 0;
  if (given("PC_CHAIN_MODE")) t.chain_mode = num("PC_CHAIN_MODE", 0) ? 1 : 0;
  if (given("PC_HXI_CHAIN_MAX")) t.hxi_chain_max = std::max(0, num("PC_HXI_CHAIN_MAX", 0));
  t.hxi28_occ1 = is("PC_HXI28_OCC", 1);
  if (given("PC_HXI_DENSE")) t.hxi_dense = is("PC_HXI_DENSE", 1) ? kHxiDense14 | kHxiDense28 : num("PC_HXI_DENSE", 0) & (kHxiDense14 | kHxiDense28);

  t.conv_dbg_set = given("PC_CONV_DBG");
  t.conv_dbg = num("PC_CONV_DBG", 0);
  if (const char* e = getenv("PERSON_CAPTURE_AMD_ATTN")) t.attn_stream = strcmp(e, "stream") == 0;
  t.stem_unfused = given("PC_STEM_UNFUSED");
  t.stem_generic = given("PC_STEM_GENERIC");
  t.hx64_wlds = !is("PC_HX64_WLDS", 0);
  t.wg_layout = num("PC_WG_LAYOUT", 1) != 0;
  return t;
}

// ---------------------------------------------------------------------------------------------
// one conv
// ---------------------------------------------------------------------------------------------
namespace {

// tile configuration (pc_conv.hip launch_rowb): channel tile BC must divide npad
const int cfg_bc[kNumConvCfgs] = {128, 128, 64, 64, 96, 32, 32, 128, 256, 256, 64, 96, 32, 128};
const int cfg_bp[kNumConvCfgs] = {128, 64, 256, 128, 128, 256, 128, 256, 128, 256, 512, 256, 512, 128};

// The facts about a conv and its tensors that the kernel families ask for, each computed once
struct ConvShape {
  const ConvOp* op;
  const NetTensor *X, *Y, *R;   // first segment's input, output, residual (or null)
  int esz;                      // activation element size
  int rowb;                     // widest K row every segment's channels allow: 128 or 64 bytes
  int max_batch;
  long long plan_batch;
  bool small;                   // a small-batch plan class (<= 64 images)
  long long Mimg, M;            // output pixels per image / of plan_batch images (overflow checks use max_batch)
  bool any_split;               // any input, the output or the residual is f16x3
  bool all_split;               // every input is f16x3 (f16 net)
  bool in_c8, out_c8;           // f16c8 inputs / output or residual
  // one segment, 3x3 / stride 1 / pad 1, output of the input's size
  bool same3x3;
  bool in_split, out_split;     // X / Y in the plain f16x3 form (split, not f16c8; dense by the decoder's check)
  int cin, cout;                // logical channels of X / Y (one half of a split tensor)
  bool res_ok_split;            // no residual, or a same-size f16x3 one (not f16c8, not upsampled)
  bool res_ok_plain;            // no residual, or a same-size plain f16 one
  bool fits32;                  // X's byte offsets at max_batch, with the zero tail, fit 32 bits
  long long tiles(int c) const { return (M + cfg_bp[c] - 1) / cfg_bp[c] * (op->npad / cfg_bc[c]); }
};

int fail(std::string& err, const char* msg) {
  err = msg;
  return PC_ERR_FORMAT;
}

int conv_shape(const NetDesc& d, const ConvOp& op, long long plan_batch, bool small, ConvShape& s, std::string& err) {
  s.op = &op;
  s.X = &d.tens[op.seg[0].x];
  s.Y = &d.tens[op.out];
  s.R = op.res >= 0 ? &d.tens[op.res] : nullptr;
  const NetTensor &X = *s.X, &Y = *s.Y;
  s.esz = d.f32 ? 4 : 2;
  s.max_batch = d.max_batch;
  s.plan_batch = plan_batch;
  s.small = small;
  s.rowb = 128;
  s.any_split = Y.split != 0 || (s.R && s.R->split);
  s.all_split = !d.f32;
  int nc8 = 0;
  for (int sg = 0; sg < op.nseg; ++sg) {
    const NetTensor& T = d.tens[op.seg[sg].x];
    // a split input's K tile must not straddle its hi and lo halves: the tile divides C / 2
    const int cl = T.split ? T.C / 2 : T.C;
    s.any_split = s.any_split || T.split;
    s.all_split = s.all_split && T.split;
    nc8 += T.c8;
    if ((cl * s.esz) % 128) s.rowb = 64;
    if ((cl * s.esz) % 64) return fail(err, "conv input channels not a multiple of the K tile");
    if ((size_t)T.C * s.esz + 128 > kZeroTail) return fail(err, "conv input wider than the zero tail");
    if (T.split && (d.f32 || T.is_f32 || T.cs != T.C))
      return fail(err, "split tensors are dense f16 [hi | lo] pixels of an f16 net");
  }
  // f16c8 inputs: every segment f16c8, conv_fast's C8 tiles only
  s.in_c8 = nc8 > 0;
  s.out_c8 = Y.c8 || (s.R && s.R->c8);
  if (s.in_c8 && nc8 != op.nseg) return fail(err, "conv mixes f16c8 and other input segments");
  s.Mimg = (long long)Y.H * Y.W;
  s.M = s.Mimg * plan_batch;   // tile choice for this batch
  const ConvSegOp& g = op.seg[0];
  s.same3x3 = op.nseg == 1 && g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && X.H == Y.H && X.W == Y.W;
  s.in_split = X.split && !X.c8;
  s.out_split = Y.split && !Y.c8;
  s.cin = X.split ? X.C / 2 : X.C;
  s.cout = Y.split ? Y.C / 2 : Y.C;
  s.res_ok_split = !s.R || (op.res_mode != RES_UP2 && s.R->split && !s.R->c8);
  s.res_ok_plain = !s.R || (op.res_mode != RES_UP2 && !s.R->split && !s.R->is_f32);
  s.fits32 = (double)X.H * X.W * d.max_batch * X.cs * s.esz + kZeroTail < 4294967296.0;
  return PC_OK;
}

// A family claims the conv: the families planned before it let go. (rowb and cfg stay: the K-row width
// shapes the kernel parameters of every family, pc_net.cpp conv_params.)
enum Family { kHalo, kFast, kT2d, kHx, kSplitK };
void take(ConvPlan& pl, Family f, int v) {
  pl.halo = pl.fast = pl.t2d = -1;
  pl.sx = 0;
  switch (f) {
    case kHalo: pl.halo = v; break;
    case kFast: pl.fast = v; break;
    case kT2d: pl.t2d = v; break;
    case kHx: pl.hx = v; break;
    case kSplitK: pl.splitk = v; break;
  }
}

// The generic implicit-GEMM kernel (pc_conv.hip): every conv has a tile here
int plan_igemm(const ConvShape& s, const Tuning& tu, ConvPlan& pl, std::string& err) {
  const int npad = s.op->npad;
  // Tile choice, from single-conv measurements on MI355X (tools/probe_conv.py,
  // DESIGN.md §3.1): 8-wave tiles with 64x64 or 128x64 per wave whenever the grid has
  // enough tiles; the 4-wave tiles for small grids.
  int cfg = -1;
  auto fits = [&](int c, long long min_tiles) { return npad % cfg_bc[c] == 0 && s.tiles(c) >= min_tiles; };
  if (fits(9, 192)) cfg = 9;                 // 256x256, npad % 256
  else if (fits(7, 192)) cfg = 7;            // 128x256
  else if (fits(13, 192)) cfg = 13;          // 128x128 (8 waves)
  else if (npad % 128 && fits(11, 128)) cfg = 11;   // 96x256
  else if (npad % 128 && fits(10, 128)) cfg = 10;   // 64x512
  else if (npad % 64 && fits(12, 128)) cfg = 12;    // 32x512
  else if (npad % 128 == 0) cfg = s.tiles(0) >= 256 ? 0 : 1;
  else if (npad % 96 == 0) cfg = 4;
  else if (npad % 64 == 0) cfg = s.tiles(2) >= 512 ? 2 : 3;
  else if (npad % 32 == 0) cfg = s.tiles(5) >= 512 ? 5 : 6;
  else return fail(err, "conv npad must be a multiple of 32");
  if (tu.cfg_force >= 0 && npad % cfg_bc[tu.cfg_force] == 0) cfg = tu.cfg_force;   // testing / tuning override
  pl.rowb = tu.rowb64 ? 64 : s.rowb;   // (tuning: force 64-byte K-tiles)
  pl.cfg = cfg;
  pl.M_per_image = s.Mimg;
  pl.splitk = s.op->splitk;
  return PC_OK;
}

// Stride-1 "same" convs (the bulk of both trunks) run on the halo kernel
// (pc_conv_halo.hip): the input run of a pixel tile is staged once per channel chunk
// and every tap reads it from LDS. PC_CONV_HALO=0 disables, =k+1 forces cfg k.
// (a forced igemm tile (PC_CONV_CFG) without PC_CONV_HALO means "test that tile")
void plan_halo(const ConvShape& s, const Tuning& tu, ConvPlan& pl) {
  const ConvOp& op = *s.op;
  const NetTensor &X = *s.X, &Y = *s.Y;
  const int KH = op.seg[0].KH, KW = op.seg[0].KW, npad = op.npad, force = tu.halo_force;
  const bool ok = !s.any_split && op.nseg == 1 && pl.splitk == 1 && op.seg[0].stride == 1 && KH == KW &&
                  op.seg[0].pad * 2 + 1 == KH && X.H == Y.H && X.W == Y.W && KH * KW <= 32 &&
                  (double)s.M * X.cs * s.esz < 4294967296.0 - 65536.0 && force != 0;
  if (!ok) return;
  auto htiles = [&](int hc) {
    int bc = 0, bp = 0;
    conv_halo_tile(hc, &bc, &bp);
    return npad % bc ? 0LL : (s.M + bp - 1) / bp * (npad / bc);
  };
  auto hok = [&](int hc) { return htiles(hc) > 0 && conv_halo_fits(hc, KH, KW, X.W); };
  int hc = -1;
  if (force > 0) {
    if (hok(force - 1)) hc = force - 1;
  } else {
    // largest tile whose grid still covers the CUs; smaller tiles otherwise
    static const int order[] = {0, 1, 2, 3, 4};
    for (int k : order)
      if (hok(k) && htiles(k) >= 192) { hc = k; break; }
    if (hc < 0)
      for (int k : {2, 4, 3, 1, 0})
        if (hok(k)) { hc = k; break; }
  }
  if (hc >= 0) {
    take(pl, kHalo, hc);
    pl.rowb = 64;   // the halo kernel steps K by one 64-byte LDS row
  }
}

// The statically scheduled kernel (pc_conv_fast.hip) takes every conv it can run:
// no split-K, offsets within 32 bits. Tile choice: fewest rounds of workgroups over
// the 256 CUs (one workgroup per CU), then the per-tile cost factor measured on
// MI355X (bigger wave tiles stage fewer LDS bytes per MFMA).
// PC_CONV_FAST=0 disables, =k+1 forces tile k.
// f16x3 split inputs on conv_fast: fused tiles (a (tap, hi block) with its lo block and both
// weight halves, pc_conv_fast.hip SX) where two stages of the doubled tile fit the LDS.
// PC_SPLIT_FUSED=0: walk the virtual [hi, lo, hi] blocks as plain tiles instead.
// rowb: the K-row width plan_igemm settled on (the halo kernel's own 64-byte rows do not count)
int plan_fast(const NetDesc& d, const ConvShape& s, const Tuning& tu, int rowb, ConvPlan& pl, std::string& err) {
  const ConvOp& op = *s.op;
  const int npad = op.npad, nseg = op.nseg, esz = s.esz;
  const long long M = s.M;
  if (s.in_c8 && (op.splitk > 1 || d.f32 || !tu.split_fused))
    return fail(err, "f16c8 convs run on conv_fast's fused C8 tiles only (no split-K)");
  const bool try_sx = s.all_split && pl.splitk == 1 && tu.split_fused;
  const int force = tu.fast_force;
  bool ok = pl.splitk == 1 && force != 0;
  // odd multiples of 32 channels (96, 160, 224: SCRFD trunks) run faster on the generic
  // kernel's 96x256 / 32x512 tiles (measured per layer, tools/probe_layers.py scrfd)
  if (force < 0 && npad > 32 && npad % 64 == 32 && !try_sx) ok = false;
  for (int sg = 0; sg < nseg && ok; ++sg) {
    const NetTensor& X = d.tens[op.seg[sg].x];
    if ((double)X.H * X.W * d.max_batch * X.cs * esz + kZeroTail >= 4294967296.0) ok = false;
  }
  if ((double)npad * op.ktot * esz >= 4294967296.0) ok = false;
  if (!ok) return PC_OK;
  // (15-19: small-batch tiles, latency-bound K loops: a second round of them costs about
  // as much as the first, hence the high factor of the smallest)
  static const double cost[] = {1.0, 1.12, 1.12, 1.3, 1.3, 1.3, 1.15, 1.45, 1.3, 1.0, 0.9, 1.3, 1.6, 1.0, 1.0,
                                1.9, 1.6, 1.6, 3.0, 1.9, 1.3, 1.55};
  static const int occ[] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1};   // workgroups per CU
  static_assert(sizeof(cost) / sizeof(cost[0]) == sizeof(occ) / sizeof(occ[0]), "tile tables");
  // fused split tiles: the 128x512 tile (8 waves of 64x128) ran ArcFace-x3's 28x28x128 at 464 us
  // against 233 for the 128x256 tile at the same estimate (profiles/r05n_sx_tile_sweep.txt)
  // (and the 64x128 small tile: ArcFace-x3's 28x28x128 at 12 rows 28.0 us against 34.5 for the 32x256
  // tile the plain factor picks, profiles/r06n_small_tile_sweep.txt)
  auto sxcost = [&](int k) { return k == 9 ? 2.2 : k == 16 ? 1.4 : cost[k]; };
  int best = -1, best_rowb = rowb, sx = 0;
  double best_t = 0;
  bool rows256 = s.small && !d.f32 && !s.any_split && rowb == 128 && !tu.rowb_set;
  for (int sg = 0; sg < nseg && rows256; ++sg) rows256 = (d.tens[op.seg[sg].x].C * esz) % 256 == 0;
  // the small-batch tiles: small-batch plans only, unless one is forced (PC_SMALL_TILES=0: A/B)
  auto small_tile_off = [&](int k) {
    return k >= kFastSmallCfg0 && k <= kFastSmallCfg1 && (!s.small || !tu.small_tiles) && force <= 0;
  };
  for (int k = 0; k < conv_fast_num_cfgs(); ++k) {
    int bc = 0, bp = 0;
    conv_fast_tile(k, &bc, &bp);
    // cfgs 10 and 14 run on 64-byte K rows only; the small-batch tiles 15-17 take 256-byte
    // rows where every segment's channels allow (half the barrier-separated K tiles)
    const int rb = (k == 10 || k == 14) ? 64 : (k >= 15 && k <= 17 && rows256) ? 256 : rowb;
    if (npad % bc || !conv_fast_valid(k, rb)) continue;
    if (force > 0 && k != force - 1) continue;
    if (small_tile_off(k)) continue;
    const long long t = (M + bp - 1) / bp * (npad / bc);
    const double rounds = (double)((t + 256 * occ[k] - 1) / (256 * occ[k]));
    const double est = rounds * bc * bp * occ[k] * cost[k];
    if (best < 0 || est < best_t) { best = k; best_t = est; best_rowb = rb; }
  }
  if (try_sx) {   // the same choice among the tiles that can stage fused split tiles
    int bsx = -1, bsx_rowb = rowb;
    double bsx_t = 0;
    for (int k = 0; k < conv_fast_num_cfgs(); ++k) {
      int bc = 0, bp = 0;
      conv_fast_tile(k, &bc, &bp);
      if (npad % bc || (force > 0 && k != force - 1)) continue;
      if (small_tile_off(k)) continue;
      for (int rb : {rowb, 64}) {
        // f16c8 inputs: tiles with the LDS epilogue, at ONE K-row width for every plan of the
        // net (Tuning::c8_rowb; PC_C8_ROWB for tuning): the row width orders the f16 and block-scaled
        // MFMAs of a K tile, so a conv's output would otherwise depend on its batch class
        if (s.in_c8 && (!conv_fast_valid_c8(k, rb) || rb != tu.c8_rowb)) continue;
        if (s.out_c8 && !conv_fast_valid_c8(k, rb)) continue;   // f16c8 output / residual: LDS epilogue
        if (!conv_fast_valid_sx(k, rb)) continue;
        const long long t = (M + bp - 1) / bp * (npad / bc);
        // the 2-wave whole-width tiles (20, 21) need two workgroups per CU to keep their K loop fed:
        // a grid under one per CU ran SCRFD-x3's 20x20x224 at b32 in 124 us against 76.5 on the 32x256
        // tile (12), at b64 130 vs 162 (profiles/r06ap_tile_sweep.txt)
        const double est = (double)((t + 255) / 256) * bc * bp * sxcost(k) * ((k == 20 || k == 21) && t < 256 ? 2.0 : 1.0);
        if (bsx < 0 || est < bsx_t) { bsx = k; bsx_t = est; bsx_rowb = rb; }
        break;
      }
    }
    if (bsx >= 0) { best = bsx; best_rowb = bsx_rowb; sx = 1; }
    else if (s.in_c8) best = -1;
  }
  if (best >= 0) {
    take(pl, kFast, best);
    pl.rowb = best_rowb;
    pl.sx = sx;
    pl.c8 = sx && s.in_c8 ? 1 : 0;
  }
  return PC_OK;
}

// 3x3 stride-1 convs over 32/64 channels run on the 2-D block kernel with register-
// resident weights (pc_conv_t2d.hip, f16) when its 16-pixel-wide blocks cover the
// image with little waste. PC_CONV_T2D=0 disables, =2 forces wherever it can run.
void plan_t2d(const NetDesc& d, const ConvShape& s, const Tuning& tu, ConvPlan& pl) {
  const ConvOp& op = *s.op;
  const NetTensor &X = *s.X, &Y = *s.Y;
  const int mode = tu.t2d_mode;
  // split (f16x3): split input -> split output (and split residual, if any) only
  const int sp = X.split ? 1 : 0;
  const bool split_ok = !sp ? !s.any_split
                            : (Y.split && !Y.c8 && !s.in_c8 && (!s.R || (s.R->split && !s.R->c8)) &&
                               Y.C / 2 >= 8 && (Y.C / 2) % 8 == 0);
  const int var = (mode > 0 && !d.f32 && op.nseg == 1 && pl.splitk == 1 && X.H == Y.H && X.W == Y.W && split_ok)
                      ? conv_t2d_select(s.cin, op.npad, op.seg[0].KH, op.seg[0].KW, op.seg[0].stride, op.seg[0].pad,
                                        op.act, Y.is_f32, Y.cs, Y.coff, sp, tu.t2d_flags)
                      : -1;
  if (var >= 0 && op.ktot >= (sp ? 27LL : 9LL) * s.cin && s.fits32 && (double)s.M < 2147483647.0) {
    const int th = conv_t2d_rows(var);
    const double cover = (double)Y.H * Y.W / ((double)((Y.H + th - 1) / th * th) * ((Y.W + 15) / 16 * 16));
    if (mode == 2 || cover >= 0.75) take(pl, kT2d, var);   // the variant, fixed at plan time (conv_t2d_launch runs exactly it)
  }
}

// the f16x3 form the halo-staged kernels run: split C -> C channels, 3x3 "same", K = [hi, hi, lo] x 9 taps
bool split_same3x3(const ConvShape& s) {
  return s.same3x3 && s.in_split && s.out_split && s.Y->C == s.X->C && s.op->npad == s.cin &&
         s.op->ktot == 27 * s.cin && s.res_ok_split && s.fits32;
}

// f16x3 64 -> 64 channel 3x3 layers on the halo-staged split kernel (pc_conv_hx.hip: 160x160x64
// b64 524 vs 632 us on conv_fast's fused tile) where its grid fills the CUs; it accumulates in the
// fused tiles' order (round 6), so plan classes choose freely. PC_CONV_HX=0 disables; the tuning
// overrides of the other kernels too.
void plan_hx64(const ConvShape& s, ConvPlan& pl) {
  const NetTensor& Y = *s.Y;
  // (its 16x12 blocks at two per CU; a grid of fewer blocks - a per-frame extract()'s 40x40 maps -
  // keeps the fused tiles: the same accumulation order, so the classes stay bit-identical)
  if (split_same3x3(s) && s.cin == 64 && s.plan_batch * ((Y.H + 11) / 12) * ((Y.W + 15) / 16) >= 256) take(pl, kHx, 1);
}

// 96 -> 96 channel layers (SCRFD's 80x80 / 40x40 / 20x20 x96 trunk) on conv_hxg<96, 96>: one
// workgroup per CU, every output channel per wave, the halo staged per 32-channel group
// (PC_CONV_HXG=0 disables, for A/B)
// (and SCRFD's 20x20x224 neck layers, small-batch form only)
void plan_hxg(const ConvShape& s, const Tuning& tu, ConvPlan& pl) {
  const NetTensor& Y = *s.Y;
  const bool c224 = s.cin == 224 && Y.H == 20 && s.plan_batch <= 16;
  if (!split_same3x3(s) || !(s.cin == 96 || c224)) return;
  // (one 16x20 block per CU; smaller grids - a single frame's 80x80 map is 20 blocks - take the
  // small-batch form, 16x4 blocks x 32 channels (PC_CONV_HXG bit 1; 80x80 / 40x40 maps, 20x20 in the plans
  // for <= 16 frames; SCRFD-x3 at one frame 1.20 -> 0.98 ms, profiles/r06bm_*), or the fused
  // tiles: bit-identical, conv_hxg walks K and the MFMA passes in their order)
  if (s.plan_batch * ((Y.H + 19) / 20) * ((Y.W + 15) / 16) >= 128 && (tu.hxg_mask & 1) && !c224) take(pl, kHx, 2);
  else if ((tu.hxg_mask & 2) && (Y.H >= 40 || s.plan_batch <= 16)) take(pl, kHx, 5);   // (profile code 504)
}

// IResNet's 14x14x256 and 28x28x128 layers on the image-resident conv_hxi (pc_conv_hxi.hip) at
// batches that give every CU a workgroup (plans for >= 192 / 64 images): bit-identical to the fused
// tiles the smaller plan classes run (same K order, MFMA order and epilogue arithmetic).
// PC_CONV_HXI is a mask of the shapes it takes: bit 0 14x14x256, bit 1 28x28x128 (f16x3), bits 2 / 3 the
// same shapes of plain f16 nets, bit 4 the f16x3 7x7x512, bit 5 the small-batch forms, bit 6 runs of
// the one-image split forms (14x14x256, 7x7x512) as chained launches (plan_hxi_runs; default 123: all but
// plain 14x14x256, which the resident chain beats). ArcFace-x3
// b256 per layer, interleaved on one box: 28x28x128 187.5 vs 224.2 us on the 128x256 WG tile,
// 14x14x256 149.3 vs 151.5 on the 256x224 one; C3 962 vs 930 frames/s with the embed quantum at 128
// faces (256 rows = one round of one-image workgroups; at 383 rows, 1.5 rounds, 876: the quantum
// follows, face_embedder.py), profiles/r06e_*
//
// plain f16 nets (BASELINE C2's fp16 ArcFace): bits 2 / 3 = 14x14x256 / 28x28x128 (tap-major K: the
// plain tiles' and the resident chain's order, bit-identical). f16 ArcFace b256, one box (r06m):
// 28x28x128 72.8 us/launch vs 94.0 on tile cfg 14 (C2 f16 7.64 vs 8.17 ms); 14x14x256 65 us x 58 =
// 3.77 ms vs 3.34 for the resident chain, so bit 2 stays opt-in (profiles/r06m_*)
void plan_hxi_plain(const ConvShape& s, const Tuning& tu, ConvPlan& pl) {
  const NetTensor &X = *s.X, &Y = *s.Y;
  const int m = tu.hxi_mask;
  if (s.same3x3 && !X.split && !X.c8 && !X.is_f32 && !Y.split && !Y.is_f32 && !Y.c8 && X.cs == X.C && Y.cs == Y.C &&
      Y.C == X.C && s.op->npad == X.C && X.W == X.H && s.op->ktot == 9 * X.C && s.res_ok_plain &&
      (((m & 4) && X.C == 256 && X.H == 14 && s.plan_batch >= 192) ||
       ((m & 8) && X.C == 128 && X.H == 28 && s.plan_batch >= 64)) &&
      s.fits32)
    take(pl, kHx, X.C == 256 ? 3 : 4);
}

void plan_hxi_split(const ConvShape& s, const Tuning& tu, ConvPlan& pl) {
  const NetTensor& X = *s.X;
  const int m = tu.hxi_mask, hc = X.C / 2;
  const long long b = s.plan_batch;
  // (bit 4: the f16x3 7x7x512 stage, one image per workgroup at pitch 9)
  // (bit 5, default on: the small-batch forms, 32 channels of 7 rows per workgroup, in the plans for <= 32
  // images - a per-frame extract()'s rows; the f16x3 shapes. ArcFace-x3 at 12 rows, one box: 14x14x256
  // 29.9 vs 31.3 us on the 64x64 tile, 28x28x128 20.7 vs 27.6, 7x7x512 35.6 vs 56.6; profiles/r06bh_*)
  const bool hxs_shape = (m & 32) && b <= 32 && ((hc == 256 && X.H == 14) || (hc == 128 && X.H == 28) || (hc == 512 && X.H == 7));
  const bool hxi_shape = ((m & 1) && hc == 256 && X.H == 14 && b >= 192) || ((m & 2) && hc == 128 && X.H == 28 && b >= 64) ||
                         ((m & 16) && hc == 512 && X.H == 7 && b >= 192) || hxs_shape;
  if (hxi_shape && split_same3x3(s) && X.W == X.H)
    take(pl, kHx, (hc == 256 ? 3 : hc == 128 ? 4 : 6) + (hxs_shape ? (hc == 512 ? 3 : 4) : 0));   // (profile codes 502 / 503 / 505, small 506-508)
}

// small-batch plan: a long-K conv of a few images fills a fraction of the CUs (a 14x14x256
// conv of 12 rows: 56 workgroups of 2304-long K) - split K over the generic kernel so the
// grid covers them; the partials are finished by splitk_finish with the full epilogue.
// Opt-in (PC_SMALL_SPLITK=1): split-K sums in another order, so a frame's results would
// depend on the batch it ran in, and extract() / extract_batch() are bit-identical by
// contract (tests/test_gpu_face_embedder.py::test_extract_single_matches_batch).
void plan_small_splitk(const NetDesc& d, const ConvShape& s, const Tuning& tu, int igemm_rowb, ConvPlan& pl) {
  if (!(s.small && pl.splitk == 1 && !d.f32 && !s.any_split && tu.small_splitk)) return;
  const long long t = s.tiles(pl.cfg);
  const int ktiles = (int)(s.op->ktot * s.esz / igemm_rowb);
  if (t < 192 && ktiles >= 16) {
    int sk = (int)std::min<long long>(8, std::max<long long>(2, 384 / std::max<long long>(1, t)));
    sk = std::min(sk, ktiles / 4);
    if (sk >= 2) {
      take(pl, kSplitK, sk);
      pl.rowb = igemm_rowb;
    }
  }
}

int plan_conv(const NetDesc& d, const Tuning& tu, const ConvOp& op, long long plan_batch, bool small, ConvPlan& pl,
              std::string& err) {
  ConvShape s;
  int rc = conv_shape(d, op, plan_batch, small, s, err);
  if (rc) return rc;
  pl = ConvPlan();
  // in the order of precedence: a later family takes the conv from an earlier one
  if ((rc = plan_igemm(s, tu, pl, err))) return rc;
  const int igemm_rowb = pl.rowb;
  plan_halo(s, tu, pl);
  if ((rc = plan_fast(d, s, tu, igemm_rowb, pl, err))) return rc;
  plan_t2d(d, s, tu, pl);
  if (tu.hx_allowed && !d.f32 && op.nseg == 1 && pl.splitk == 1) {
    plan_hx64(s, pl);
    plan_hxg(s, tu, pl);
    plan_hxi_plain(s, tu, pl);
    plan_hxi_split(s, tu, pl);
  }
  plan_small_splitk(d, s, tu, igemm_rowb, pl);

  const NetTensor& Y = *s.Y;
  if (s.in_c8) {   // nothing else runs f16c8 inputs
    if (pl.fast < 0 || !pl.c8) return fail(err, "no conv_fast C8 tile fits this f16c8 conv");
    pl.halo = pl.t2d = -1;
    pl.hx = 0;
    pl.splitk = 1;
  }
  // (and only by those with the LDS epilogue: the per-fragment epilogue of the 96 / 224-channel tiles
  // has no f8 region handling)
  if (s.out_c8 && (pl.fast < 0 || !pl.sx || pl.t2d >= 0 || pl.hx || pl.halo >= 0 || !conv_fast_valid_c8(pl.fast, pl.rowb)))
    return fail(err, "f16c8 outputs and residuals are written / read by conv_fast's fused LDS-epilogue tiles only");
  // fused f16x3 tiles of 64-byte K rows on the WG form where it is instantiated (PC_SX_WG=0: staged
  // weights, for A/B). Same K order and pass order as the staged form: bit-identical outputs.
  pl.wg = pl.fast >= 0 && pl.sx && !pl.c8 && pl.rowb == 64 && pl.splitk == 1 && pl.t2d < 0 && !pl.hx && pl.halo < 0 &&
          conv_fast_valid_wg(pl.fast) && tu.sx_wg;
  if (s.cout > op.npad) return fail(err, "conv output tensor wider than npad");
  if (Y.split && (Y.is_f32 || Y.cs != Y.C || (Y.C / 2) % 8))
    return fail(err, "split conv output must be a dense f16 [hi | lo] tensor");
  // split-K reads split inputs (the K iterator's virtual blocks) into f32 partials; the finish
  // kernel writes plain tensors only (the f16x3 IResNet's FC: split 7x7x512 -> f32 embedding)
  if (pl.splitk > 1 && (Y.split || (s.R && s.R->split))) return fail(err, "split-K into a split output");
  return PC_OK;
}

// Stem as im2col + 1x1 MFMA conv when the window fits one 32-element K row
// (3x3x3 = 27). Weights are repacked [npad][32], tap-major, channel-minor (pc_net.cpp upload_stem).
int plan_stem(const NetDesc& d, const Tuning& tu, const StemOp& op, StemPlan& st, size_t& col_bytes, std::string& err) {
  const NetTensor &X = d.tens[op.x], &Y = d.tens[op.out];
  if (Y.split && (d.f32 || op.KH * op.KW * op.cin_true > 32 || X.C != 4 || Y.is_f32))
    return fail(err, "split stem output needs the fused f16 stem");
  if (!Y.split && (tu.stem_direct || op.KH * op.KW * op.cin_true > 32 || X.C != 4)) return PC_OK;   // direct kernel
  const int esz = d.f32 ? 4 : 2;
  st.use_mfma = 1;
  st.cin_true = op.cin_true;
  st.split = Y.split;
  st.npad = (std::max(op.cout, Y.split ? Y.C / 2 : Y.C) + 31) / 32 * 32;
  st.rowb = 32 * esz;   // one K-tile of exactly 32 elements
  const long long M = (long long)Y.H * Y.W * d.max_batch;
  st.cfg = st.npad % 128 == 0 ? 7 : (st.npad % 64 == 0 ? 10 : 12);
  col_bytes = std::max(col_bytes, (size_t)M * 32 * esz + 256);
  return PC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the whole net
// ---------------------------------------------------------------------------------------------
int plan_net(const NetDesc& d, const Tuning& tu, NetPlan& out, std::string& err) {
  out = NetPlan();
  const size_t nops = d.ops.size();
  const int max_batch = d.max_batch;
  out.plans.resize(nops);
  // Small-batch classes 1, 4, 16, 32, 64 images up to a quarter of max_batch: a per-frame
  // extract() runs SCRFD on 1 image and ArcFace on 2 x its faces (2-30 rows); a net of 64
  // (SCRFD) keeps 1 / 4 / 16, so its 32-frame C3 chunks stay on the max-batch tiles (r03:
  // the 16-image tiles at 32 images cost 0.4 ms per step).
  if (max_batch > 2 && tu.small_plans) {
    for (int b : {1, 4, 16, 32, 64})
      if (b <= std::max(1, max_batch / 4)) out.cls_batch.push_back(b);
    // f16x3 nets (ArcFace-x3 runs 256-row calls on a 512-row net: C3's 128-face quantum with flips):
    // plans for 128 rows and half the max batch too - a tile chosen for 512 rows runs 256 at half a
    // round (7x7x512: 248 vs 185 us, profiles/r05n_sx_tile_sweep.txt). Their convs keep the one K
    // order of every class (the fused tiles' K-row width is fixed per conv), so results stay bit-identical.
    bool has_split = false;
    for (auto& t : d.tens) has_split = has_split || t.split;
    if (has_split && max_batch >= 256)
      for (int b : {128, max_batch / 2})
        if (b > out.cls_batch.back()) out.cls_batch.push_back(b);
  }
  out.plans_cls.assign(out.cls_batch.size(), std::vector<ConvPlan>(nops));
  out.stems.resize(nops);
  size_t part = 0;
  for (size_t i = 0; i < nops; ++i) {
    const NetOp& op = d.ops[i];
    const NetTensor& Y = d.tens[op.out()];
    int rc = PC_OK;
    if (op.kind == OP_CONV) {
      const ConvOp& c = op.conv;
      ConvPlan& pl = out.plans[i];
      if ((rc = plan_conv(d, tu, c, max_batch, false, pl, err))) return rc;
      // small batches (per-frame extract: one frame's faces, prescan samples) get their own
      // tile choice: the max-batch tiles would leave most CUs idle
      for (size_t k = 0; k < out.cls_batch.size(); ++k) {
        ConvPlan& sp = out.plans_cls[k][i];
        if ((rc = plan_conv(d, tu, c, out.cls_batch[k], out.cls_batch[k] <= 64, sp, err))) return rc;
        if (sp.splitk > 1)
          part = std::max(part, (size_t)((long long)sp.splitk * sp.M_per_image * out.cls_batch[k] * c.npad * 4));
      }
      if (pl.splitk > 1) part = std::max(part, (size_t)((long long)pl.splitk * pl.M_per_image * max_batch * c.npad * 4));
      double macs = 0.0;
      // algorithmic MACs: real output channels x real taps x input channels
      for (int s = 0; s < c.nseg; ++s)
        macs += (double)Y.H * Y.W * c.cout_true * c.seg[s].KH * c.seg[s].KW * c.seg[s].cin_true;
      out.flops_per_image += 2.0 * macs;
      pl.flops_per_image = 2.0 * macs;
      out.launches += pl.splitk > 1 ? 2 : 1;
    } else if (op.kind == OP_STEM) {
      const StemOp& s = op.stem;
      const double fl = 2.0 * Y.H * Y.W * s.cout * s.KH * s.KW * s.cin_true;
      out.flops_per_image += fl;
      if ((rc = plan_stem(d, tu, s, out.stems[i], out.stem_col_bytes, err))) return rc;
      out.plans[i].flops_per_image = fl;
      out.launches += out.stems[i].use_mfma ? 2 : 1;
    } else if (op.kind == OP_ATTENTION) {
      const NetTensor& Q = d.tens[op.attn.x];
      const double T = (double)Q.H * Q.W;
      out.flops_per_image += 4.0 * T * T * op.attn.heads * op.attn.head_dim;
      out.launches += 1;
    } else {
      out.launches += 1;
    }
  }
  out.partial_bytes = part;
  return PC_OK;
}

int plan_kernel_code(const ConvPlan& pl) {
  return pl.hx            ? 499 + pl.hx   // 500 conv_hx64, 501 conv_hxg, 502 / 503 / 505 conv_hxi 14x14 / 28x28 / 7x7, 506-508 their small-batch forms
         : pl.c8          ? 600 + pl.fast
         : pl.t2d >= 0    ? 200 + pl.t2d
         : pl.fast >= 0   ? 100 + pl.fast
                          : pl.halo;
}

int plan_kernel_form(const ConvPlan& pl) {
  const bool fastk = !pl.hx && pl.t2d < 0 && pl.fast >= 0;
  return fastk ? (pl.sx ? 1 : 0) + (pl.wg ? 2 : 0) + (pl.rowb == 128 ? 4 : 0) : pl.cfg;
}

// ---------------------------------------------------------------------------------------------
// chained conv_hxi launches
// ---------------------------------------------------------------------------------------------
// Chained conv_hxi launches (pc_conv_hxi.hip conv_hxi_chain): the launches that cover the ops marked in
// `elig` (the convs a plan class runs on the one-image-per-workgroup split forms), as (first op, layers)
// pairs in program order. A run is a maximal stretch of consecutive marked ops in which
//  * each op's one input is the previous op's output, and a residual is a tensor written earlier in the
//    program (inside the run or before it) - so within a launch a workgroup reads only what it wrote itself;
//  * no tensor written inside the run, but the last op's, is read by an op outside it (or is a net output):
//    the run ends where such a tensor is written (IResNet: at a block's conv2, never at a conv1).
// A run of L layers is then cut into launches of at most `cap` layers (cap <= 0: one launch); these cuts
// fall anywhere - a kernel boundary orders the launches like the per-layer ones.
// Pure host logic over the program's raw op words (hand-made ones too, which the decoder would not pass:
// the words it needs, by the OpWord names), exported for tests/test_hxi_runs_cpu.py.
void find_hxi_runs(const int32_t* ops, int nops, const int32_t* elig, const int32_t* outs, int nouts,
                   int cap, std::vector<std::pair<int, int>>& launches) {
  launches.clear();
  auto W = [&](int i) { return ops + (size_t)i * kOpWords; };
  auto out_of = [&](int i) { return W(i)[kWOut]; };
  auto conv1 = [&](int i) { return W(i)[kWKind] == OP_CONV && W(i)[kWConvNseg] == 1; };   // a one-segment conv
  int nt = 0;
  auto reads = [&](int i, auto&& fn) {
    const int32_t* w = W(i);
    if (w[kWKind] == OP_CONV) {
      for (int sg = 0; sg < w[kWConvNseg] && sg < 2; ++sg) fn(w[kWConvSeg + kWConvSegWords * sg]);
      if (w[kWConvRes] >= 0) fn(w[kWConvRes]);
    } else {
      fn(w[kWIn]);
    }
  };
  for (int i = 0; i < nops; ++i) {
    nt = std::max(nt, out_of(i) + 1);
    reads(i, [&](int t) { nt = std::max(nt, t + 1); });
  }
  for (int k = 0; k < nouts; ++k) nt = std::max(nt, outs[k] + 1);
  const int kNever = -1, kAlways = 1 << 30;
  std::vector<int> last_use(nt, kNever), producer(nt, kNever);
  for (int i = 0; i < nops; ++i) {
    reads(i, [&](int t) { if (t >= 0) last_use[t] = std::max(last_use[t], i); });
    if (out_of(i) >= 0) producer[out_of(i)] = i;
  }
  for (int k = 0; k < nouts; ++k) if (outs[k] >= 0) last_use[outs[k]] = kAlways;
  auto res_ok = [&](int i) { const int r = W(i)[kWConvRes]; return r < 0 || producer[r] < i; };
  auto follows = [&](int i) {   // op i continues a run that holds op i - 1
    return elig[i] && conv1(i) && W(i)[kWConvSeg] == out_of(i - 1) && res_ok(i);
  };
  for (int f = 0; f < nops;) {
    if (!elig[f] || !conv1(f) || !res_ok(f)) { ++f; continue; }
    int e = f;
    while (e + 1 < nops && follows(e + 1)) ++e;
    // the longest prefix [f, j] whose inner tensors are all read for the last time inside it
    int j = e;
    for (; j > f; --j) {
      bool ok = true;
      for (int i = f; i < j && ok; ++i) ok = last_use[out_of(i)] <= j;
      if (ok) break;
    }
    const int L = j - f + 1, step = cap > 0 ? cap : L;
    for (int o = 0; o < L; o += step) launches.emplace_back(f + o, std::min(step, L - o));
    f = j + 1;
  }
}

}  // namespace pc

using namespace pc;

extern "C" int pc_plan_hxi_runs(const int32_t* ops, int n_ops, const int32_t* eligible, const int32_t* outs,
                                int n_outs, int cap, int32_t* runs, int max_runs) {
  if (!ops || !eligible || n_ops < 0 || (n_outs > 0 && !outs) || (max_runs > 0 && !runs)) return -PC_ERR_ARG;
  std::vector<std::pair<int, int>> l;
  find_hxi_runs(ops, n_ops, eligible, outs, n_outs, cap, l);
  for (size_t k = 0; k < l.size() && (int)k < max_runs; ++k) {
    runs[2 * k] = l[k].first;
    runs[2 * k + 1] = l[k].second;
  }
  return (int)l.size();
}

extern "C" int pc_net_plan(const void* prog, size_t nbytes, int precision, int max_batch, int32_t* cls_batch_out,
                           int max_cls, int32_t* plans_out, int max_ops, char* err_out, int err_len) {
  std::string err;
  NetDesc d;
  NetPlan P;
  int rc = decode_program(prog, nbytes, precision, max_batch, d, err);
  if (rc == PC_OK) rc = plan_net(d, tuning_from_env(), P, err);
  const int ncls = 1 + (int)P.cls_batch.size(), nops = (int)d.ops.size();
  if (rc == PC_OK && ((ncls - 1 > max_cls) || nops > max_ops || (ncls > 1 && !cls_batch_out) || (nops && !plans_out))) {
    rc = PC_ERR_ARG;
    err = "pc_net_plan: output arrays too small";
  }
  if (err_out && err_len > 0) snprintf(err_out, err_len, "%s", err.c_str());
  if (rc != PC_OK) return -rc;
  for (int c = 1; c < ncls; ++c) cls_batch_out[c - 1] = P.cls_batch[c - 1];
  for (int c = 0; c < ncls; ++c)
    for (int i = 0; i < nops; ++i) {
      const ConvPlan& pl = c ? P.plans_cls[c - 1][i] : P.plans[i];
      int32_t* o = plans_out + ((size_t)c * max_ops + i) * PC_PLAN_WORDS;
      const bool conv = d.ops[i].kind == OP_CONV;
      o[0] = d.ops[i].kind;
      o[1] = conv ? plan_kernel_code(pl) : -1;
      o[2] = conv ? plan_kernel_form(pl) : -1;
      o[3] = conv ? pl.rowb : 0;
      o[4] = conv ? pl.splitk : 0;
      o[5] = conv ? pl.cfg : -1;
    }
  return ncls;
}
