// The network executor's host-only side: the decoded program (pc_program.cpp), the tuning switches and
// the plans (pc_plan.cpp). No HIP types here: everything in this header runs on a machine without a
// device (pc_net_plan, tests/test_plan_cpu.py). The device state of a net is pc_net_dev.h's pc_net.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/pcgpu.h"
#include "pc_enums.h"

namespace pc {

enum { OP_CONV = 1, OP_STEM = 2, OP_MAXPOOL = 3, OP_UPSAMPLE = 4, OP_LAYERNORM = 5, OP_ATTENTION = 6 };

// Word positions of the 32-word op records (person_capture_amd/program.py writes the same table):
//   every op   [0] kind  [1] output tensor
//   CONV       [2] segments (1 or 2)  [3 + 5s .. 7 + 5s] segment s: input tensor, KH, KW, stride, pad
//              [13] weights  [14] npad  [15] ktot  [16] cout  [17] bias (-1: none)  [18] bias mode
//              [19] PReLU slopes (-1: none)  [20] act  [21] residual tensor (-1: none)  [22] residual mode
//              [23] act after residual  [24] split-K (0 / 1: none)  [25 + s] true input channels of segment s
//              [27] true output channels for the FLOP count (0: cout)
//   STEM       [2] input  [3] KH  [4] KW  [5] stride  [6] pad  [7] weights  [8] cout  [9] bias
//              [10] PReLU slopes (-1: none)  [11] act  [12] channels written  [13] true input channels (0: 3)
//   MAXPOOL    [2] input  [3] k  [4] stride  [5] pad
//   UPSAMPLE   [2] input
//   LAYERNORM  [2] input  [3] gamma  [4] beta  [5] positional table (-1: none)  [6] its rows  [7] eps (f32 bits)
//              [8] channels
//   ATTENTION  [2] qkv  [3] heads  [4] head dim
// Only decode_op (pc_program.cpp) and find_hxi_runs (raw words by contract) read records by position.
enum OpWord {
  kWKind = 0, kWOut = 1, kWIn = 2,
  kWConvNseg = 2, kWConvSeg = 3, kWConvSegWords = 5, kWConvW = 13, kWConvNpad = 14, kWConvKtot = 15, kWConvCout = 16,
  kWConvBias = 17, kWConvBiasMode = 18, kWConvSlope = 19, kWConvAct = 20, kWConvRes = 21, kWConvResMode = 22,
  kWConvActAfterRes = 23, kWConvSplitk = 24, kWConvCinTrue = 25, kWConvCoutTrue = 27,
  kWStemKH = 3, kWStemKW = 4, kWStemStride = 5, kWStemPad = 6, kWStemW = 7, kWStemCout = 8, kWStemBias = 9,
  kWStemSlope = 10, kWStemAct = 11, kWStemCpad = 12, kWStemCinTrue = 13,
  kWPoolK = 3, kWPoolStride = 4, kWPoolPad = 5,
  kWLnGamma = 3, kWLnBeta = 4, kWLnAdd = 5, kWLnRows = 6, kWLnEps = 7, kWLnC = 8,
  kWAttnHeads = 3, kWAttnHeadDim = 4,
  kOpWords = 32,
};

// Tensor and array ids are validated by the decoder: in range, -1 ("none") only in the fields marked so.
struct ConvSegOp { int x, KH, KW, stride, pad, cin_true; };
struct ConvOp {
  int out, nseg;
  ConvSegOp seg[2];
  int w, npad, ktot, cout;
  int bias, bias_mode;        // bias -1: none
  int slope, act;             // slope -1: none
  int res, res_mode;          // res -1: none
  int act_after_res;
  int splitk;                 // >= 1
  int cout_true;
};
struct StemOp { int out, x, KH, KW, stride, pad, w, cout, bias, slope, act, cpad, cin_true; };   // slope -1: none
struct PoolOp { int out, x, k, stride, pad; };
struct UpsampleOp { int out, x; };
struct LayerNormOp { int out, x, gamma, beta, add, rows; float eps; int C; };   // add -1: none
struct AttnOp { int out, x, heads, head_dim; };
struct NetOp {
  int kind;
  union {
    struct { int out, x; } io;   // every kind but CONV: the output and the one input (the structs' first fields)
    ConvOp conv;
    StemOp stem;
    PoolOp pool;
    UpsampleOp up;
    LayerNormOp ln;
    AttnOp attn;
  };
  int out() const { return io.out; }   // (ConvOp starts with `out` too)
};

struct NetBuf { long long elems; int is_f32; };
// split: f16x3 tensor (detector precision mode): C physical channels = [hi | lo],
// C / 2 each; the lo half of a pixel is C / 2 elements after its hi half
// c8: f16c8 tensor: split storage whose second half holds, per 32
// channels, the e4m3 bytes [lo8 | hi8]; lo8 = e4m3(lo * 2^e_lo), hi8 = e4m3(hi * 2^e_hi) with
// per-tensor exponents set by pc_net_calibrate (provisional values before it)
struct NetTensor { int buf, H, W, C, cs, coff, is_f32, split; int c8 = 0, e_lo = 15, e_hi = 4; };
struct NetArray { long long off, cnt; };   // in floats, into NetDesc::data

// A decoded, validated program
struct NetDesc {
  int f32 = 0;
  int max_batch = 0;
  int in_tensor = 0;
  int in_centered = 0;        // the input is the centred image x - 127.5 (program input tensor flag bit 1)
  std::vector<NetBuf> bufs;
  std::vector<NetTensor> tens;
  std::vector<NetArray> arrays;
  std::vector<int> outs;
  std::vector<NetOp> ops;
  std::vector<int32_t> words;   // the op records as they came (find_hxi_runs)
  const float* data = nullptr;  // the program's float data: borrowed, valid while the caller's blob is
  size_t ndata = 0;
};

// Every activation buffer is followed by kZeroTail zero bytes: a padding tap of the
// implicit-GEMM loader reads one K-tile row (any channel block of the pixel stride)
// from there, so the tail covers the widest pixel row a conv reads.
static const size_t kZeroTail = 65536;

// Parses and validates a program: PC_OK, or PC_ERR_FORMAT / PC_ERR_ARG with a message in err that names the op
// kind and the rule. "Validated" covers, after it returns PC_OK:
//  * ids: every tensor, buffer and array id of every op indexes its table;
//  * tensors (check_tensor): H, W, C >= 1, the channel slice inside the pixel stride, every pixel inside the
//    buffer, is_f32 as the buffer's; the split / f16c8 storage rules;
//  * geometry (check_geometry): what each kernel's own indexing assumes - the pool and conv output sizes, the
//    doubled upsample, LayerNorm's C against both tensors, its arrays and the kernel's 2048-channel limit,
//    attention's widths, token counts and 16-byte alignment, residual sizes, array lengths, and the element
//    type the non-GEMM kernels and the stem move (include/pcgpu.h lists the refusals).
// So a decoded program reads and writes inside its tensors and arrays. What the planner still decides (tile
// fits, split-K, which conv family can take a layer) is plan_net's, with its own PC_ERR_FORMAT messages.
int decode_program(const void* prog, size_t nbytes, int precision, int max_batch, NetDesc& d, std::string& err);
template <typename F>
static inline void for_each_input(const NetOp& op, F&& fn) {   // the tensors an op reads
  if (op.kind == OP_CONV) {
    for (int s = 0; s < op.conv.nseg; ++s) fn(op.conv.seg[s].x);
    if (op.conv.res >= 0) fn(op.conv.res);
  } else {
    fn(op.io.x);
  }
}

// The tuning / testing switches, read from the environment once: when a net (tuning_from_env, at the top of
// pc_net_create and pc_net_plan) or a context (PC_AREA_DIRECT, pc_ctx_create) is created. A switch changed
// later does not reach an existing net: its plans, its captured graphs and its launches stay consistent.
// DESIGN.md §3.11 lists the variables.
struct Tuning {
  // --- conv planner: the resolved override cascade (tuning_from_env) ---
  int cfg_force = -1;         // PC_CONV_CFG: igemm tile wherever it divides npad (-1: the planner's choice)
  int rowb64 = 0;             // PC_CONV_ROWB=64: 64-byte K rows
  int rowb_set = 0;           // PC_CONV_ROWB given at all: no 256-byte rows on the small-batch tiles
  int halo_force = -1;        // -1 planner's choice, 0 off, k + 1: halo tile k
  int fast_force = -1;        // -1 planner's choice, 0 off, k + 1: conv_fast tile k
  int t2d_mode = 1;           // 0 off, 1 where its blocks cover the image, 2 wherever it can run
  int t2d_flags = 0;          // T2dFlags (conv_t2d_select)
  int split_fused = 1;        // PC_SPLIT_FUSED=0: no fused f16x3 tiles (SX) on conv_fast
  int hx_allowed = 1;         // conv_hx64 / conv_hxg / conv_hxi may claim convs
  int hxg_mask = 3;           // PC_CONV_HXG: bit 0 the one-block-per-CU form, bit 1 the small-batch form
  int hxi_mask = 123;         // PC_CONV_HXI (plan_hxi below)
  int small_tiles = 1;        // PC_SMALL_TILES=0: no conv_fast small-batch tiles (15-19)
  int small_splitk = 0;       // PC_SMALL_SPLITK: split-K in the small-batch plans
  int small_plans = 1;        // PC_NO_SMALL_PLANS: the max-batch plans only
  int c8_rowb = 64;           // PC_C8_ROWB=128
  int sx_wg = 1;              // PC_SX_WG=0: staged weights on the fused tiles
  int stem_direct = 0;        // PC_STEM_DIRECT: the direct stem kernel
  // --- chains ---
  int chain = 1;              // PC_CHAIN=0: no resident chains
  int chain_min_batch = 32;   // PC_CHAIN_MIN
  int chain_wl = 0;           // PC_CHAIN_WL=2: fragment-major weights
  int chain_mode = 1;         // PC_CHAIN_MODE: 1 LDS-DMA weight ring, 0 register stream
  // layers per chained conv_hxi launch, 0: no cap (PC_HXI_CHAIN_MAX). A chained launch holds every CU at one
  // workgroup for its whole length, and the detection stream's kernels wait behind it: C3 interleaved on one
  // box, frames/s (4 runs each): per-layer 1032, cap 2 1040, 4 1047, 8 1049, 16 1048, none 1037
  // (profiles/r07a_hxi_chain_cap_sweep.txt)
  int hxi_chain_max = 8;
  int hxi28_occ1 = 0;         // PC_HXI28_OCC=1: the 28x28 split form at one workgroup per CU
  // PC_HXI_DENSE: the split 14x14 / 28x28 forms' fragments without padding columns (kHxiDense14 | kHxiDense28;
  // 0: the halo's pitch for both, 1 or not given: both dense, 2 / 4: one of them)
  int hxi_dense = 6;
  // --- launch-time forms ---
  int conv_dbg_set = 0;       // PC_CONV_DBG given (phase splits: no chained conv_hxi launches)
  int conv_dbg = 0;           // its value (ConvParams::dbg)
  int attn_stream = 0;        // PERSON_CAPTURE_AMD_ATTN=stream: pc_attn.hip for every attention shape
  int stem_unfused = 0;       // PC_STEM_UNFUSED: im2col + 1x1 conv instead of the fused stem
  int stem_generic = 0;       // PC_STEM_GENERIC: that conv on the generic kernel
  int hx64_wlds = 1;          // PC_HX64_WLDS=0: conv_hx64 without the LDS weight stage
  int wg_layout = 1;          // PC_WG_LAYOUT=0: the cfg table's wave layouts on the WG tiles
};
Tuning tuning_from_env();

// PC_CONV_HXI's default: every conv_hxi shape but plain f16 14x14x256 (bit 2, which the resident chain
// beats), and the chained launches of the one-image split forms (bit 6, plan_hxi_runs)
static const int kHxiDefaultMask = 123;

// sx: fused f16x3 split tiles on conv_fast (pc_conv_fast.hip SX); c8: its f16c8 form (C8);
// wg: the fused f16x3 tile takes its weight fragments from the fragment-ordered copy (pc_net::wfrag)
// hx: 1 conv_hx64, 2 / 5 conv_hxg and its small-batch form, 3 / 4 / 6 conv_hxi 14x14 / 28x28 / 7x7, 7-9 their
// small-batch forms
struct ConvPlan {
  int rowb = 0, cfg = 0, splitk = 1, halo = -1, fast = -1, t2d = -1, sx = 0, hx = 0, c8 = 0, wg = 0;
  long long M_per_image = 0;
  double flops_per_image = 0.0;
};
// A stem (tiny Cin) runs as im2col + a 1x1 MFMA conv over 32-element K rows.
struct StemPlan {
  int use_mfma = 0, npad = 0, cfg = 0, rowb = 0, cin_true = 0;
  int split = 0;            // f16x3 output: w is [npad][64] = W_hi | W_lo (fused stem only)
  void* w = nullptr;        // [npad][32] act dtype (device, uploaded by pc_net_create)
  float* bias = nullptr;    // [npad]
  float* slope = nullptr;   // [npad] or null
};
// Everything pc_net_create decides before it touches the device
struct NetPlan {
  std::vector<ConvPlan> plans;   // per op, for max_batch images
  // small-batch plan classes: plans_cls[c] holds the tiles chosen for cls_batch[c] images
  // (ascending); a run of N images takes the first class with N <= cls_batch[c], else `plans`
  std::vector<std::vector<ConvPlan>> plans_cls;
  std::vector<int> cls_batch;
  std::vector<StemPlan> stems;
  size_t stem_col_bytes = 0;     // im2col scratch shared by the stems
  size_t partial_bytes = 0;      // split-K workspace
  double flops_per_image = 0.0;
  int launches = 0;
};
int plan_net(const NetDesc& d, const Tuning& tu, NetPlan& out, std::string& err);

// What pc_net_profile_ops reports in [4] / [5] for a per-layer launch of a conv under plan pl:
// the kernel (100+k conv_fast tile k, 600+k its f16c8 form, 200+v t2d variant v, 500 conv_hx64, 501 conv_hxg,
// 502 / 503 / 505 conv_hxi 14x14 / 28x28 / 7x7, 504 / 506-508 the small-batch forms, k halo tile k, -1 igemm)
// and the generic kernel's tile cfg or, for conv_fast launches, their form: bit 0 fused split (SX),
// bit 1 register weight fragments (WG), bit 2 128-byte K rows
int plan_kernel_code(const ConvPlan& pl);
int plan_kernel_form(const ConvPlan& pl);

// the (first op, layers) launches of the chained conv_hxi form (pc_plan_hxi_runs)
void find_hxi_runs(const int32_t* ops, int nops, const int32_t* elig, const int32_t* outs, int nouts, int cap,
                   std::vector<std::pair<int, int>>& launches);

// host-side queries of the kernels' tables (pc_conv_*.hip, pc_ops.hip, pc_stem.hip)
static const int kNumConvCfgs = 14;   // pc_conv.hip launch_rowb
constexpr int kFastSmallCfg0 = 15, kFastSmallCfg1 = 19;   // conv_fast tiles 15..19: small-batch plans only
int conv_fast_num_cfgs();
int conv_fast_tile(int cfg, int* bc, int* bp);
int conv_fast_valid(int cfg, int rowb);
int conv_fast_valid_sx(int cfg, int rowb);
int conv_fast_valid_c8(int cfg, int rowb);
int conv_fast_valid_wg(int cfg);
int conv_halo_num_cfgs();
int conv_halo_tile(int cfg, int* bc, int* bp);
int conv_halo_fits(int cfg, int KH, int KW, int W);
int conv_t2d_select(int cin, int npad, int KH, int KW, int stride, int pad, int act, int out_f32, int ycs,
                    int ycoff, int split, int t2d_flags);
int conv_t2d_rows(int variant);
int conv_chain_fits(int H, int W, int C, int npad, long long ktot);
bool attention_head_dim_ok(int head_dim);

}  // namespace pc
