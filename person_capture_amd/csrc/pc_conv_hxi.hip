// Image-resident f16x3 3x3 convolutions for IResNet's 28x28x128 and 14x14x256 stages (gfx950): the
// ArcFace-x3 layers that run on conv_fast's fused WG tiles.
//
// conv_fast stages, per 32-channel K tile, the split pixel rows of one tap: every input pixel moves
// L2 -> LDS nine times (the tile's pixels re-read for each tap), through 4 LDS-DMA pieces per wave
// and a barrier per K tile. Its 128x256 tile on 28x28x128 issues only 48 MFMAs per wave between two
// barriers and ran at 36 % of the matrix pipe (r05/r06 per-layer probes). Here one workgroup owns
// ROWS full output rows of one image - every output channel - and stages the rows' padded halo once
// per group of 64 input channels (hi and lo: 256-byte slots), in a 2-stage ring: group g + 1 lands
// while group g's 18 k-steps (9 taps x two 32-channel blocks) run; one barrier per group, none inside.
//  * output pixels are enumerated as ROWS x PITCH slots (the halo's pitch: the map width + 2 padding
//    columns, rounded up to 16), so a tap is one slot offset for every 16-slot pixel fragment; the
//    PITCH - HW columns past the map are computed and discarded: 12.5 % at pitch 16 / 32, 14 fragments
//    for 196 pixels. The split 14x14x256 and 28x28x128 forms issue 13 (PC_HXI_DENSE, the default): the
//    first on a dense enumeration of its own (HxiGeom DENSE), the second at pitch 29 (PC_HXI_28D below);
//    the plain-f16, 7x7, one-workgroup-per-CU 28x28 and small-batch forms stay as described here;
//  * 8 waves = WCH channel groups x WPX fragment groups; a wave's weight fragments come from the
//    fragment-ordered copy (pc_net.cpp pack_wfrag) into registers a k-step ahead (double-buffered),
//    its pixel fragments from the halo in groups of at most 7;
//  * K order and MFMA order are conv_fast SX / WG's exactly - channel groups of 64 (every tap of a
//    group, the two 32-channel blocks per tap), per k-step W_lo*x_hi, W_hi*x_hi, W_hi*x_lo - and the
//    epilogue arithmetic is conv_epilogue_lds<SPLIT>'s, so the outputs are bit-identical to the fused
//    tiles every other plan class of the net runs (tests/test_gpu_arcface.py);
//  * LDS chunk swizzle: chunk q of slot h holds source chunk q ^ ((h & 7) << 1) - conflict-free
//    ds_read_b128 for 16 consecutive slots at any alignment, hi or lo, either block (checked
//    exhaustively over the instruction's lane groups, MI355X_MICROARCH.md §LDS);
//  * epilogue: a thread keeps one 8-channel group for all its pixels, so the channel bias and slopes
//    are loaded once, and the per-pixel term of each of its pixels (the residual's hi + lo, or a folded
//    pre-BN's border-class bias) is requested before the accumulators go to the LDS image, so the loads
//    overlap the transposition (the first form loaded both per item: its epilogue took 53 of 184 us on
//    28x28x128, profiles/r06f_hxi28_phase_split.txt).
#include "pc_conv_common.h"

namespace pc {

// SPLIT (f16x3): a halo slot holds one 64-channel group's hi and lo halves (256 bytes), staged group by
// group in a 2-stage ring; K = (group, tap, 32-channel block), 3 MFMA passes per k-step (the fused
// tiles' order). Plain f16 (the BASELINE C2 fp16 net): a slot holds every input channel (CIN * 2 bytes),
// staged once; K = (tap, 32-channel block), tap-major like conv_fast's plain tiles and the resident
// chain, one MFMA per fragment pair - so it is bit-identical to them as well.
// DENSE (the 14x14 map at pitch 16): the fragments enumerate the image's 196 pixels, not the halo's 224
// slots - 13 fragments (hxi_dense_pixel below).
template <int HW, int PITCH, int ROWS, int CIN, int COUT, int WCH, int WPX, bool SPLIT, int OCC, bool DENSE = false>
struct HxiGeom {
  static constexpr int NW = WCH * WPX, NT = 64 * NW;
  static constexpr int NPIX = ROWS * HW;
  // pixel fragments per workgroup (16 slots, or 16 pixels, each)
  static constexpr int NF = ((DENSE ? NPIX : ROWS * PITCH) + 15) / 16;
  // (NF not a multiple of WPX: the last fragment group is one short, its waves skip their last fragment)
  static constexpr int TP = (NF + WPX - 1) / WPX, TC = COUT / WCH / 16;
  static constexpr int CB = CIN / COUT;                      // channel blocks: workgroups per row block
  static constexpr int WPS = (NW * OCC + 3) / 4;             // waves per SIMD
  // fragments per read group (4 waves per SIMD - two 8-wave workgroups per CU: one at a time, the other
  // waves hide the reads)
  static constexpr int TPG = WPS > 2 ? 1 : (TP > 7 ? (TP + 1) / 2 : TP);
  static constexpr int NGRP = (TP + TPG - 1) / TPG;          // read groups (the last one short if TP is odd)
  // one wave per SIMD (the small-batch forms): no other wave hides a latency - the weights come 5 k-steps
  // ahead (not 1), and the pixel fragments of k-step k + 1 are read under k-step k's MFMAs (PF): 14x14 at
  // 12 images 34.9 -> 29.9 us. (Loader waves of their own for the halo pieces, 1-4 per workgroup, did not
  // beat the compute waves issuing them: 28.5-30.0 / 20.9-21.0 / 37-45 us, profiles/r06bh_hxs_phase.txt)
  static constexpr int WD = WPS == 1 ? 6 : 2;                // weight register buffers
  static constexpr bool PF = WPS == 1 && SPLIT && TPG == TP;
  static constexpr int SB = SPLIT ? 256 : CIN * 2;           // halo slot bytes
  static constexpr int NB = SPLIT ? 2 : CIN / 32;            // 32-channel blocks per staged group
  static constexpr int NG = SPLIT ? CIN / 64 : 1, KPG = 9 * NB, NKS = NG * KPG;
  // halo slots: the padded rows, + what the taps of the last fragment's discarded slots reach; dense: up to
  // the last pixel's last tap
  static constexpr int SLOTS = DENSE ? (ROWS - 1) * PITCH + (HW - 1) + 2 * PITCH + 2 + 1
                                     : (NF * 16 > ROWS * PITCH ? NF * 16 - ROWS * PITCH : 0) + (ROWS + 2) * PITCH + 2;
  static constexpr int PIECES = (SLOTS * SB + 1023) / 1024;
  static constexpr int STAGE = PIECES * 1024;
  // a 2-stage ring where the groups are several and two stages fit the workgroup's LDS share; else one
  // stage (at two workgroups per CU the other workgroup's MFMAs cover the exposed staging)
  static constexpr int NSTAGE = NG > 1 && 2 * STAGE * OCC <= 163840 ? 2 : 1;
  static constexpr int PC = COUT * NPIX * 4 <= 131072 / OCC ? COUT : COUT / 2;   // channels per epilogue pass
  static constexpr int NPASS = COUT / PC;
  static constexpr int RS = PC + 4;
  static constexpr int EPI = NPIX * RS * 4;
  static constexpr int SMEM = NSTAGE * STAGE > EPI ? NSTAGE * STAGE : EPI;
  static constexpr int WTILE = SPLIT ? 2048 : 1024;          // packed weight bytes per K tile and 16-row block
  static constexpr int CGN = PC / 8;                         // 8-channel items per pixel and pass
  static constexpr int IT = (NPIX + NT / CGN - 1) / (NT / CGN);   // items (pixels) per thread and pass
  // (a pitch of HW + 1: the right padding column of a row is the left one of the next)
  static_assert(PITCH >= HW + 1 && (NF % WPX == 0 || TPG == 1) && !(PF && (DENSE || NF % WPX != 0)), "pixel fragments");
  static_assert(DENSE ? WPX == 1 && SPLIT && HW == 14 && PITCH == 16 && ROWS == 14 && TPG == 7 : TP % TPG == 0,
                "dense enumeration");
  static_assert(COUT % (16 * WCH) == 0 && CIN % 64 == 0 && HW % ROWS == 0 && SB % 256 == 0, "tiling");
  static_assert(SMEM <= 163840, "LDS");
  static_assert(NPASS == 1 || WCH % 2 == 0, "epilogue passes split the channel waves");
};

// The dense enumeration of a 14x14 image in 13 fragments: output pixel (row, col) of fragment f's lane slot fr
// (col = 14: a discarded lane). The halo slot of a pixel at tap (0, 0) is 16 row + col.
//  * fragments 0-6: columns 0-7 of rows 2 f (lanes 0-7) and 2 f + 1 (lanes 8-15): slot 32 f + fr + (fr & 8).
//    The 8 slots that a ds_read_b128 lane group reads at one chunk parity (lane slots 0-3 and 12-15, or
//    4-11) have 8 different keys: conflict-free, as 16 consecutive slots are;
//  * fragments 7-12, j = f - 7: columns 8-13 of rows 2 j (lanes 0-5) and 2 j + 1 (lanes 8-13): slot
//    32 j + 8 + fr + (fr & 8), the same lane offset; lanes 6 and 7 take a pair of the 12 pixels left in
//    columns 8-13 of rows 12 and 13 - row 12 + j / 3, columns 8 + 2 (j % 3) and the next; lanes 14 and 15
//    are discarded and read the row's padding columns 14 and 15. The pair's keys are those of two other
//    lanes of its group: a 2-way conflict in every group of these 6 fragments' reads. Columns 8-13 share
//    their keys with columns 0-5, so 13 fragments cannot hold 196 pixels without a conflict
//    (tests/test_hxi_dense_cpu.py); the plain enumeration q = 16 f + fr has it in 12 fragments and needs
//    per-fragment lane offsets: 142.5 us per layer at 256 images for the pitch enumeration's 134.8
//    (profiles/r08_hxi_dense_layers_ab.txt).
__device__ __forceinline__ void hxi_dense_pixel(int f, int fr, int& row, int& col) {
  if (f < 7) {
    row = 2 * f + (fr >> 3), col = fr & 7;
  } else {
    const int j = f - 7, c = fr & 7;
    if (c < 6) row = 2 * j + (fr >> 3), col = 8 + c;
    else if (fr < 8) row = 12 + j / 3, col = 8 + 2 * (j % 3) + (fr & 1);
    else row = 0, col = 14;
  }
}

// One layer for this workgroup's rows: `p` is the launch's kernel argument (conv_hxi) or one entry of a
// chained launch's layer array (conv_hxi_chain, read through the constant address space - the array is
// uploaded once at plan time and never written while a kernel runs); N is the batch (the grid).
template <int HW, int PITCH, int ROWS, int CIN, int COUT, int WCH, int WPX, bool SPLIT, int OCC, bool DENSE, class P>
__device__ __forceinline__ void conv_hxi_layer(P& p, const int N, const int tid, char* smem) {
  using G = HxiGeom<HW, PITCH, ROWS, CIN, COUT, WCH, WPX, SPLIT, OCC, DENSE>;
  constexpr int NW = G::NW, NT = G::NT, TC = G::TC, TP = G::TP, TPG = G::TPG, NG = G::NG, NKS = G::NKS;
  constexpr int STAGE = G::STAGE, PIECES = G::PIECES, SB = G::SB, NB = G::NB, KPG = G::KPG;
  static_assert(G::SMEM * OCC <= 163840, "LDS for OCC workgroups per CU");
  static_assert(NW <= 16, "waves");
  auto& S = p.seg[0];
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wch = wave % WCH, wpx = wave / WCH;
  constexpr int RB = HW / ROWS, CB = G::CB;      // row blocks per image, channel blocks per row block
  // (a row block's CB workgroups are consecutive: on one XCD after the remap, sharing its halo in the L2)
  const int b = xcd_remap(blockIdx.x, N * RB * CB);
  const int cb = b % CB, nb = b / CB;
  const int n = nb / RB, r0 = (nb - n * RB) * ROWS;
  const int fr = lane & 15, kg = lane >> 4;

  auto rsrc = [](const void* base) __attribute__((always_inline)) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)0xffffffff, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t xrs = rsrc(S.x);
  const __amdgpu_buffer_rsrc_t wrs = rsrc(p.wfrag);

  // this wave's halo pieces i = wave + 8 j: LDS byte i * 1024 + lane * 16 = slot h, chunk position q,
  // holding source chunk c = q ^ ((h & 7) << 1) (the XOR touches the low 4 bits only): split: channels
  // 8 (c & 7) .. of the group's hi (c < 8) or lo half; plain: channels 8 c .. - of input pixel
  // (r0 - 1 + h / PITCH, h % PITCH - 1); zeros outside
  constexpr int PPW = (PIECES + NW - 1) / NW;
  // (offsets computed at each issue: kept in registers for all pieces they spilled the 256-register
  // plain 14x14 form, 17 pieces per wave)
  auto stage = [&](int g, int st) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      if (wave + NW * j < PIECES) {   // (wave-uniform)
        const int byte = (wave + NW * j) * 1024 + lane * 16;
        const int h = byte / SB, q = (byte % SB) >> 4;
        const int c = q ^ ((h & 7) << 1);
        const int iy = r0 - 1 + h / PITCH, ix = h % PITCH - 1;
        const bool ok = h < (ROWS + 2) * PITCH && (unsigned)iy < (unsigned)HW && (unsigned)ix < (unsigned)HW;
        const int cb = SPLIT ? ((c & 7) * 8 + (c >> 3) * CIN) * 2 : c * 16;
        unsigned off = ok ? (unsigned)((n * HW + iy) * HW + ix) * (unsigned)(S.cs * 2) + (unsigned)cb
                          : S.zero_off + (unsigned)((q & 15) << 4);
        asm volatile("" : "+v"(off));
        // split: the group's 64 channels ride in the scalar offset (128 bytes per group of each half)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_ptr_t)(smem + st * STAGE + (wave + NW * j) * 1024), 16, off,
                                                 g * 128, 0, 0);
      }
    }
  };
  // weight fragments of k-step s (packed K tile s; split: group s / 18, tap (s % 18) / 2, block s % 2,
  // plain: tap s / NB, block s % NB): row blocks TC wch .. TC wch + TC - 1 of npad / 16, each
  // [W_hi, W_lo] (split) or W (plain) x 1 KiB
  const int tile = (p.npad / 16) * G::WTILE;
  auto wload = [&](f16x8* wh, f16x8* wl, int s) __attribute__((always_inline)) {
#pragma unroll
    for (int a = 0; a < TC; ++a) {
      const int o = (cb * (COUT / 16) + TC * wch + a) * G::WTILE + lane * 16;
      wh[a] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, o, s * tile, 0));
      if constexpr (SPLIT) wl[a] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, o + 1024, s * tile, 0));
    }
  };
  constexpr int WD = G::WD;
  f16x8 wbh[WD][TC], wbl[WD][TC];
  stage(0, 0);
  static_for<WD - 1>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j < NKS) wload(wbh[j], wbl[j], j);
  });
  f16x8 bhp[2][G::PF ? TP : 1];   // (PF: this and the next k-step's hi pixel fragments)

  f32x4 acc[TC][TP];
#pragma unroll
  for (int a = 0; a < TC; ++a)
#pragma unroll
    for (int t = 0; t < TP; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.dbg & 8) return;   // tuning only (PC_CONV_DBG): prologue only

  // per-lane LDS byte of (tap, chunk kind) for slot fr + sh, sh = dy PITCH + dx the tap's slot shift (the
  // swizzle key is the slot's low bits: at a pitch that is not a multiple of 8 the row shift changes them)
  // (recomputed at each k-step - the asm keeps the compiler from hoisting all (tap, block) offsets of
  // the unrolled loop into registers at once: 24 of them in the plain 256-channel form)
  auto boff = [&](int sh, int chunk) __attribute__((always_inline)) {
    int h = fr;
    // (a pitch that puts the row shift into sh has 9 shifts x 4 chunks of these: at 128 registers the lane
    // slot is made opaque as well, or the compiler computes them once for all channel groups and spills the
    // 28x28 form at pitch 29: 76 bytes of scratch)
    if constexpr (PITCH % 8 != 0 && G::WPS > 2) asm volatile("" : "+v"(h));
    h += sh;
    unsigned v = (unsigned)(h * SB + ((chunk ^ ((h & 7) << 1)) << 4));
    asm volatile("" : "+v"(v));
    return v;
  };
  // halo slot of fragment t's first slot at tap (0, 0): fragment f = wpx * TP + t covers output slots
  // 16 f .. 16 f + 15 (slot o = output row o / PITCH, column o % PITCH; columns >= HW and rows >= ROWS are
  // discarded - a pitch that is not a multiple of 16 lets a fragment span two rows: the 7x7 form's 9)
  auto fslot = [&](int t) __attribute__((always_inline)) { return (wpx * TP + t) * 16; };
  // dense: the byte of slot h's chunk in the stage, ck = (blk * 4 + kg) << 4 the chunk's byte in an unswizzled
  // slot (the key touches bits 5-7 only; the lo chunk is 128 bytes from the hi one)
  auto dswz = [](int h, unsigned ck) __attribute__((always_inline)) {
    return ((unsigned)h << 8) | ((((unsigned)h << 5) & 0xe0u) ^ ck);
  };
  static_for<NG>([&](auto gc) __attribute__((always_inline)) {
    constexpr int g = decltype(gc)::value, st = G::NSTAGE == 2 ? (g & 1) : 0;
    if constexpr (G::NSTAGE == 1 && g > 0) {   // one stage: group g replaces g - 1 once every wave is done
      __syncthreads();
      stage(g, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      // group g's halo: every VMEM op but the youngest (the next WD - 1 k-steps' weights) has landed
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((WD - 1) * (SPLIT ? 2 * TC : TC)) : "memory");
    }
    __syncthreads();   // every wave's pieces of group g; every wave done reading group g - 1's stage
    if constexpr (G::NSTAGE == 2 && g + 1 < NG) stage(g + 1, st ^ 1);
    const char* base = smem + st * STAGE;
    static_for<KPG>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value, tap = k / NB, blk = k % NB, s = g * KPG + k, q = s % WD;
      constexpr int dy = tap / 3, dx = tap % 3;
      if constexpr (s + WD - 1 < NKS) wload(wbh[(s + WD - 1) % WD], wbl[(s + WD - 1) % WD], s + WD - 1);
      // (pitches that are multiples of 8 keep the row shift out of the swizzled offset: fewer live offsets -
      // folding it in spilled the two-workgroup 28x28 form)
      constexpr int sh = PITCH % 8 == 0 ? dx : dy * PITCH + dx, rsh = PITCH % 8 == 0 ? dy * PITCH : 0;
      const unsigned oh = DENSE ? 0u : boff(sh, blk * 4 + kg), ol = SPLIT && !DENSE ? boff(sh, 8 + blk * 4 + kg) : 0u;
      if (p.dbg & 2) return;   // tuning only: no MFMAs
      if constexpr (G::PF) {
        // the hi fragments were read at the previous k-step (the group's first: here), the lo ones at the top
        // of this one; the next k-step's hi fragments are requested before the last MFMA pass (same passes,
        // same order per accumulator)
        constexpr int cur = k & 1;
        if constexpr (k == 0) {
#pragma unroll
          for (int t = 0; t < TP; ++t) bhp[cur][t] = *reinterpret_cast<const f16x8*>(base + oh + (fslot(t) + rsh) * SB);
        }
        f16x8 bl[TP];
#pragma unroll
        for (int t = 0; t < TP; ++t) bl[t] = *reinterpret_cast<const f16x8*>(base + ol + (fslot(t) + rsh) * SB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TP; ++t)
            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbl[q][a], bhp[cur][t], acc[a][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TP; ++t)
            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bhp[cur][t], acc[a][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (k + 1 < KPG) {
          constexpr int tap1 = (k + 1) / NB, blk1 = (k + 1) % NB, dy1 = tap1 / 3, dx1 = tap1 % 3;
          constexpr int sh1 = PITCH % 8 == 0 ? dx1 : dy1 * PITCH + dx1, rsh1 = PITCH % 8 == 0 ? dy1 * PITCH : 0;
          const unsigned oh1 = boff(sh1, blk1 * 4 + kg);
#pragma unroll
          for (int t = 0; t < TP; ++t)
            bhp[cur ^ 1][t] = *reinterpret_cast<const f16x8*>(base + oh1 + (fslot(t) + rsh1) * SB);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TP; ++t)
            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bl[t], acc[a][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        return;
      }
      unsigned odn[DENSE ? TPG : 1];   // (dense: the second read group's lane offsets, computed under the first's MFMAs)
      static_for<G::NGRP>([&](auto pc) __attribute__((always_inline)) {
        constexpr int t0 = decltype(pc)::value * TPG, CNT = TP - t0 < TPG ? TP - t0 : TPG;
        if constexpr (G::NF % WPX != 0) {   // (wave-uniform: the short fragment group's last fragment)
          if (wpx * TP + t0 >= G::NF) return;
        }
        f16x8 bh[TPG], bl[SPLIT ? TPG : 1];
        if constexpr (DENSE) {
          // the lane slot's halo slot less the fragment's first (hxi_dense_pixel): fr + (fr & 8) for the lanes of
          // the two row runs - one offset for every fragment, as at the pitch enumeration; lanes 6 and 7 of the
          // fragments 7-12 have a slot of their own. Recomputed from an opaque lane slot at each k-step (hoisted
          // over the unrolled K loop the offsets do not fit the registers); those of fragments 7-12 in the
          // first read group, spread over its last MFMA pass (after it they held the wave's MFMAs back)
          unsigned od[TPG];
          int e = fr;
          asm volatile("" : "+v"(e));
          const unsigned ck = (unsigned)(blk * 4 + kg) << 4;
          const unsigned om = dswz(e + (e & 8) + dx, ck);
          auto imm = [](int f) __attribute__((always_inline)) { return f < 7 ? 32 * f : 32 * (f - 7) + 8; };
          static_for<CNT>([&](auto tc) __attribute__((always_inline)) {
            constexpr int t = decltype(tc)::value, f = t0 + t;
            od[t] = f < 7 ? om : odn[t];
            bh[t] = *reinterpret_cast<const f16x8*>(base + od[t] + (imm(f) + dy * PITCH) * SB);
          });
#pragma unroll
          for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int t = 0; t < CNT; ++t)
              acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbl[q][a], bh[t], acc[a][t0 + t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          static_for<CNT>([&](auto tc) __attribute__((always_inline)) {
            constexpr int t = decltype(tc)::value, f = t0 + t;
            constexpr int im = f < 7 ? 32 * f : 32 * (f - 7) + 8;
            bl[t] = *reinterpret_cast<const f16x8*>(base + (od[t] ^ 128u) + (im + dy * PITCH) * SB);
          });
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int t = 0; t < CNT; ++t)
              acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bh[t], acc[a][t0 + t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (t0 == 0) {
            static_for<TP - TPG>([&](auto tc) __attribute__((always_inline)) {
              constexpr int t = decltype(tc)::value, j = t, f = 7 + j;
              constexpr int X = (12 + j / 3) * PITCH + 8 + 2 * (j % 3);   // the pair's first slot
              odn[t] = (e & 14) == 6 ? dswz((e & 1) + (X - imm(f)) + dx, ck) : om;
            });
          }
#pragma unroll
          for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int t = 0; t < CNT; ++t)
              acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bl[t], acc[a][t0 + t], 0, 0, 0);
          if constexpr (t0 == 0) {   // (one MFMA, then 4 of the offsets' VALU operations)
#pragma unroll
            for (int i = 0; i < TC * CNT; ++i) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          return;
        }
#pragma unroll
        for (int t = 0; t < TPG; ++t)
          bh[t] = *reinterpret_cast<const f16x8*>(base + oh + (fslot(t0 + t) + rsh) * SB);
        if constexpr (!SPLIT) {   // plain f16: one MFMA per fragment pair
#pragma unroll
          for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int t = 0; t < TPG; ++t)
              acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bh[t], acc[a][t0 + t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          return;
        }
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TPG; ++t)
            acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbl[q][a], bh[t], acc[a][t0 + t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < TPG; ++t)
          bl[t] = *reinterpret_cast<const f16x8*>(base + ol + (fslot(t0 + t) + rsh) * SB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TPG; ++t)
            acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bh[t], acc[a][t0 + t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int t = 0; t < TPG; ++t)
            acc[a][t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wbh[q][a], bl[t], acc[a][t0 + t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      });
    });
  });
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (p.dbg & 4) return;   // tuning only: no epilogue

  // ---- epilogue in NPASS passes of PC channels: the waves of a pass's channels write their
  // accumulators into an f32 [pixel][channel] image over the LDS; then every thread finishes 8 channels
  // of one pixel per item with conv_epilogue_lds<SPLIT>'s arithmetic: bias (per channel, then the border
  // class), residual hi + lo before or after the activation select, channel keep mask, hi / lo stores ----
  constexpr int NPIX = G::NPIX, RS = G::RS, PC = G::PC, NPASS = G::NPASS, CGN = G::CGN, IT = G::IT;
  static_assert(NT % CGN == 0, "a thread keeps one 8-channel group");
  constexpr int PSTEP = NT / CGN;                     // pixel stride between a thread's items
  float* im = reinterpret_cast<float*>(smem);
  const bool smooth = p.act == ACT_SILU || p.act == ACT_GELU;
  const bool has_res = p.res_mode != RES_NONE;
  const bool pre_act = !p.act_after_res;
  const bool border = p.bias_mode == BIAS_BORDER9;
  const long long pix0 = (long long)n * HW * HW + r0 * HW;   // the workgroup's first output pixel
  const int cg = tid % CGN, pl0 = tid / CGN;
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int ch = cb * COUT + pass * PC + cg * 8;
    // per-thread channel terms (one 8-channel group for all of the thread's pixels): channel bias (0
    // otherwise, as conv_epilogue_lds adds it), negative-side slope (PReLU / 0 for ReLU / 1)
    float bc[8], sl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bc[j] = p.bias_mode == BIAS_CHANNEL ? p.bias[ch + j] : 0.f;
      sl[j] = p.act == ACT_PRELU ? p.slope[ch + j] : (p.act == ACT_RELU ? 0.f : 1.f);
    }
    // the per-pixel term of each of the thread's items, requested before anything waits on it: the
    // residual hi + lo (its f32 value), or the border-class bias of a folded pre-BN conv
    // (four waves per SIMD - two 8-wave workgroups per CU: loaded at the item instead - the other workgroup covers the latency, and
    // the registers are not there)
    constexpr bool PREF = G::WPS <= 2;
    float pre[PREF ? IT : 1][8];
    auto load_pre = [&](int k, float* dst) __attribute__((always_inline)) {
      const int pl = pl0 + PSTEP * k;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = 0.f;
      if (pl >= NPIX) return;
      if (has_res) {
        const f16* rp = reinterpret_cast<const f16*>(p.res) + (pix0 + pl) * p.rcs + ch;
        const f16x8 rh = *reinterpret_cast<const f16x8*>(rp);
        if constexpr (SPLIT) {
          const f16x8 rl = *reinterpret_cast<const f16x8*>(rp + p.rsplit);
#pragma unroll
          for (int j = 0; j < 8; ++j) dst[j] = (float)rh[j] + (float)rl[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dst[j] = (float)rh[j];
        }
      } else if (border) {
        const int oy = r0 + pl / HW, ox = pl % HW;
        const int rc = oy - 1 < 0 ? 0 : (oy + 1 >= HW ? 2 : 1);
        const int cc = ox - 1 < 0 ? 0 : (ox + 1 >= HW ? 2 : 1);
        const f32x4* bp = reinterpret_cast<const f32x4*>(p.bias + (rc * 3 + cc) * p.npad + ch);
        const f32x4 b0 = bp[0], b1 = bp[1];
        dst[0] = b0[0]; dst[1] = b0[1]; dst[2] = b0[2]; dst[3] = b0[3];
        dst[4] = b1[0]; dst[5] = b1[1]; dst[6] = b1[2]; dst[7] = b1[3];
      }
    };
    if constexpr (PREF) {
#pragma unroll
      for (int k = 0; k < IT; ++k) load_pre(k, pre[k]);
    }
    __syncthreads();   // the stages (pass 0) / the previous pass's image are no longer read
    if (NPASS == 1 || wch / (WCH / 2) == pass) {
#pragma unroll
      for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int t = 0; t < TP; ++t) {
          int orow, ocol;
          if constexpr (DENSE) {
            hxi_dense_pixel(t, fr, orow, ocol);
          } else {
            const int o = (wpx * TP + t) * 16 + fr;
            orow = o / PITCH, ocol = o % PITCH;
          }
          if (ocol < HW && orow < ROWS) {
            const int pl = orow * HW + ocol;
            const int cl = (NPASS == 1 ? wch : wch % (WCH / 2)) * TC * 16 + a * 16 + kg * 4;
            *reinterpret_cast<f32x4*>(im + pl * RS + cl) = acc[a][t];
          }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int pl = pl0 + PSTEP * k;
      if (pl >= NPIX) continue;
      float pk[8];
      if constexpr (PREF) {
#pragma unroll
        for (int j = 0; j < 8; ++j) pk[j] = pre[k][j];
      } else {
        load_pre(k, pk);
      }
      const long long pix = pix0 + pl;
      const f32x4 lo4 = *reinterpret_cast<const f32x4*>(im + pl * RS + cg * 8);
      const f32x4 hi4 = *reinterpret_cast<const f32x4*>(im + pl * RS + cg * 8 + 4);
      float v[8] = {lo4[0] + bc[0], lo4[1] + bc[1], lo4[2] + bc[2], lo4[3] + bc[3],
                    hi4[0] + bc[4], hi4[1] + bc[5], hi4[2] + bc[6], hi4[3] + bc[7]};
      if (border) {
        if (has_res) {   // (both: not produced by the programs that run here; loaded in place)
          const int oy = r0 + pl / HW, ox = pl % HW;
          const int rc = oy - 1 < 0 ? 0 : (oy + 1 >= HW ? 2 : 1);
          const int cc = ox - 1 < 0 ? 0 : (ox + 1 >= HW ? 2 : 1);
          const float* bp = p.bias + (rc * 3 + cc) * p.npad + ch;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += bp[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += pk[j];
        }
      }
      if (has_res && !pre_act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += pk[j];
      }
      if (smooth) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act_apply(v[j], p.act, 0.f);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * sl[j];
      }
      if (has_res && pre_act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += pk[j];
      }
      f16x8 yh, yl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = ch + j < p.cout ? v[j] : 0.f;
        yh[j] = (f16)x;
        yl[j] = (f16)(x - (float)yh[j]);
      }
      if (p.dbg & 16) continue;   // tuning only: no stores
      f16* yp = reinterpret_cast<f16*>(p.y) + pix * p.ycs + ch;
      *reinterpret_cast<f16x8*>(yp) = yh;
      if constexpr (SPLIT) *reinterpret_cast<f16x8*>(yp + p.ysplit) = yl;
    }
  }
}

template <int HW, int PITCH, int ROWS, int CIN, int COUT, int WCH, int WPX, bool SPLIT = true, int OCC = 1, bool DENSE = false>
__global__ __launch_bounds__(64 * WCH * WPX, (WCH * WPX * OCC + 3) / 4) void conv_hxi(ConvParams p) {
  __shared__ __attribute__((aligned(16))) char smem[HxiGeom<HW, PITCH, ROWS, CIN, COUT, WCH, WPX, SPLIT, OCC, DENSE>::SMEM];
  conv_hxi_layer<HW, PITCH, ROWS, CIN, COUT, WCH, WPX, SPLIT, OCC, DENSE>(p, p.N, (int)threadIdx.x, smem);
}

// A run of consecutive layers of the one-image-per-workgroup split forms (14x14x256, 7x7x512) as one
// launch, grid = N: workgroup n walks image n through layers lp[0 .. nl - 1] (pc_net.cpp plan_hxi_runs:
// each layer reads the previous one's output, a residual is a tensor written earlier in the run or
// before the launch - always by this workgroup, as it owns every row and channel of its image). The
// activations still go out to memory and come back as the next layer's halo; what goes is the kernel
// boundary: the end-of-kernel drain with nothing computing, the launch gap, the per-layer tail sync -
// the workgroups drift apart, so one's stores drain under the others' MFMAs. Per-layer code is
// conv_hxi's, so the bits are the per-layer launches' (tests/test_gpu_hxi_chain.py).
// Between two layers the workgroup's stores must be visible to its own halo DMA and residual loads:
// every wave waits for its stores (vmcnt(0)), workgroup-scope release, barrier, workgroup-scope acquire.
// The waves of a workgroup run on one CU and share its vector L1 (the kernels are not built in
// threadgroup-split mode), which the stores write through - so workgroup scope needs no L1 invalidate
// or L2 write-back, and no device-scope flush is needed (LLVM AMDGPUUsage, "Memory Model gfx942":
// workgroup-scope release / acquire fences in non-tgsplit mode are s_waitcnt only).
// The barrier also keeps the next layer's first halo stage off the LDS image a slower wave still reads.
template <int HW, int PITCH, int ROWS, int CIN, int COUT, int WCH, int WPX, bool DENSE = false>
__global__ __launch_bounds__(64 * WCH * WPX, (WCH * WPX + 3) / 4) void conv_hxi_chain(const ConvParams* lp, int nl) {
  __shared__ __attribute__((aligned(16))) char smem[HxiGeom<HW, PITCH, ROWS, CIN, COUT, WCH, WPX, true, 1, DENSE>::SMEM];
  typedef const __attribute__((address_space(4))) ConvParams CP;
  CP* cp = (CP*)lp;
  for (int l = 0; l < nl; ++l) {
    if (l) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    // (the thread index made opaque per layer: hoisted out of the layer loop, the per-thread offsets
    // derived from it stay live through the K loop and spill the 14x14 form, 233 registers as it is)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    conv_hxi_layer<HW, PITCH, ROWS, CIN, COUT, WCH, WPX, true, 1, DENSE>(cp[l], (int)gridDim.x, tid, smem);
  }
}

// the instantiated shapes: IResNet's 14x14x256 (one image per workgroup, 8 x 1 waves of 32 channels x
// 14 rows) and 28x28x128 (7 rows per workgroup, 4 x 2 waves of 32 channels x 7 fragments); plain f16
// 28x28x128 at two workgroups per CU (its halo stage is 73 KB)
#define PC_HXI_14 14, 16, 14, 256, 256, 8, 1
#define PC_HXI_28 28, 32, 7, 128, 128, 4, 2
// the split forms without padding columns in the fragments (PC_HXI_DENSE, the default):
// 196 pixels per workgroup in 13 fragments for the pitch enumeration's 14.
//  * 14x14x256: the dense enumeration over the same halo (HxiGeom DENSE, hxi_dense_pixel);
//  * 28x28x128: pitch 29 - the right padding column of row y is the left one of row y + 1, the 7 rows are
//    203 consecutive slots, a fragment spans two rows as in the 7x7 form; 16 consecutive slots stay
//    conflict-free. The two fragment groups take 7 and 6 fragments.
#define PC_HXI_28D 28, 29, 7, 128, 128, 4, 2
// 7x7x512 (the last stage, split only): one image per workgroup at pitch 9 - 63 slots in 4 fragments
// (77 % kept; a pitch of 16 would keep 44 %), 8 x 1 waves of 64 channels x 4 fragments
#define PC_HXI_7 7, 9, 7, 512, 512, 8, 1
// small-batch forms (a per-frame extract()'s ~12 ArcFace rows: 12 one-image workgroups would idle 244
// CUs, and conv_fast's 64x64 tile re-stages every pixel per tap and is bound by the LDS port): 32 output
// channels of 7 rows per workgroup - 16 workgroups per image (2 or 4 waves of 16 or 32 channels x 7
// fragments, or 4 at the 7x7 map), the rows' halo staged per 64-channel group as above. Same K order,
// MFMA order and epilogue: the same bits as every other form (tests/test_gpu_arcface.py)
#define PC_HXI_14S 14, 16, 7, 256, 32, 2, 1
#define PC_HXI_28S 28, 32, 7, 128, 32, 2, 2
#define PC_HXI_7S 7, 9, 7, 512, 32, 2, 1

// can a conv run here: one segment of C channels (split: X.C 2 C = [hi | lo]; plain f16: X.C C), dense,
// on an HW x HW map of an instantiated shape, C output channels written in the same form (dense), 3x3
// stride 1 pad 1, plain or same-size residual in the same form
int conv_hxi_ok(const ConvParams& p) {
  const ConvSeg& S = p.seg[0];
  const bool split = p.ysplit != 0;
  const int C = split ? S.C / 2 : S.C, w = split ? 2 : 1;
  const bool shape = (S.H == 14 && C == 256) || (S.H == 28 && C == 128) || (split && S.H == 7 && C == 512);
  return shape && p.nseg == 1 && S.cs == w * C && S.W == S.H && S.KH == 3 && S.KW == 3 && S.stride == 1 &&
         S.pad == 1 && p.OH == S.H && p.OW == S.H && p.npad == C && p.ycs == w * C && p.splitk == 1 && !p.out_f32 &&
         !p.yc8 && !p.rc8 && p.ktot == 9 * (split ? 3 : 1) * C && p.res_mode != RES_UP2 &&
         (p.res_mode == RES_NONE || (p.rsplit == (split ? C : 0) && p.rcs % 8 == 0)) && p.cwrite == C &&
         p.wfrag != nullptr && (!split || p.ysplit == C);
}

// (dense: Tuning::hxi_dense, read when the net is built)
hipError_t conv_hxi_launch(const ConvParams& p, int small, int occ1_28, int dense, hipStream_t s) {
  if (!conv_hxi_ok(p)) return hipErrorInvalidValue;
  const bool split = p.ysplit != 0;
  if (small) {   // (16 workgroups per image; split only)
    if (!split) return hipErrorInvalidValue;
    const dim3 grid(p.N * 16);
    if (p.OH == 7) hipLaunchKernelGGL((conv_hxi<PC_HXI_7S, true, 2>), grid, dim3(128), 0, s, p);
    else if (p.OH == 14) hipLaunchKernelGGL((conv_hxi<PC_HXI_14S, true, 2>), grid, dim3(128), 0, s, p);
    else hipLaunchKernelGGL((conv_hxi<PC_HXI_28S, true, 1>), grid, dim3(256), 0, s, p);
  } else if (p.OH == 7) {
    hipLaunchKernelGGL((conv_hxi<PC_HXI_7, true, 1>), dim3(p.N), dim3(512), 0, s, p);
  } else if (p.OH == 14) {
    // (half an image per workgroup at two per CU, 7 rows: 147.7 vs 145.3 us, profiles/r06t_hxi14_half_ab.txt)
    if (split && (dense & kHxiDense14)) hipLaunchKernelGGL((conv_hxi<PC_HXI_14, true, 1, true>), dim3(p.N), dim3(512), 0, s, p);
    else if (split) hipLaunchKernelGGL((conv_hxi<PC_HXI_14, true, 1>), dim3(p.N), dim3(512), 0, s, p);
    else hipLaunchKernelGGL((conv_hxi<PC_HXI_14, false, 1>), dim3(p.N), dim3(512), 0, s, p);
  } else {
    // (split: two workgroups per CU, one halo stage each, so one's epilogue runs under the other's MFMAs;
    // PC_HXI28_OCC=1 the 2-stage form, read when the net is built: pc_plan.cpp)
    if (split && occ1_28) hipLaunchKernelGGL((conv_hxi<PC_HXI_28, true, 1>), dim3(p.N * 4), dim3(512), 0, s, p);
    else if (split && (dense & kHxiDense28)) hipLaunchKernelGGL((conv_hxi<PC_HXI_28D, true, 2>), dim3(p.N * 4), dim3(512), 0, s, p);
    else if (split) hipLaunchKernelGGL((conv_hxi<PC_HXI_28, true, 2>), dim3(p.N * 4), dim3(512), 0, s, p);
    else hipLaunchKernelGGL((conv_hxi<PC_HXI_28, false, 2>), dim3(p.N * 4), dim3(512), 0, s, p);
  }
  return hipGetLastError();
}

// can a conv be a layer of a chained launch: the split one-image-per-workgroup shapes
int conv_hxi_chain_ok(const ConvParams& p) {
  return conv_hxi_ok(p) && p.ysplit != 0 && (p.OH == 14 || p.OH == 7) && p.dbg == 0;
}

// nl layers (d_layers: ConvParams[nl] on the device, each conv_hxi_chain_ok, all of one map size HW) for
// N images as one launch
hipError_t conv_hxi_chain_launch(const void* d_layers, int nl, int HW, int N, int dense, hipStream_t s) {
  if (!d_layers || nl < 1 || N < 1) return hipErrorInvalidValue;
  const ConvParams* lp = static_cast<const ConvParams*>(d_layers);
  if (HW == 14 && (dense & kHxiDense14)) hipLaunchKernelGGL((conv_hxi_chain<PC_HXI_14, true>), dim3(N), dim3(512), 0, s, lp, nl);
  else if (HW == 14) hipLaunchKernelGGL((conv_hxi_chain<PC_HXI_14>), dim3(N), dim3(512), 0, s, lp, nl);
  else if (HW == 7) hipLaunchKernelGGL((conv_hxi_chain<PC_HXI_7>), dim3(N), dim3(512), 0, s, lp, nl);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace pc
