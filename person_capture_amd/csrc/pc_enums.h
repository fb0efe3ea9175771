// Small integer codes shared by the kernels (pc_common.h) and the host-only planner (pc_net.h).
#pragma once

namespace pc {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2, ACT_SILU = 3, ACT_GELU = 4 };
enum BiasMode { BIAS_NONE = 0, BIAS_CHANNEL = 1, BIAS_BORDER9 = 2 };
enum ResMode { RES_NONE = 0, RES_SAME = 1, RES_UP2 = 2 };

// conv_t2d_select's tuning word (Tuning::t2d_flags): one bit per PC_T2D_* switch
enum T2dFlags {
  kT2dSplitOff = 1,   // PC_T2D_SPLIT=0
  kT2dSplit64 = 2,    // PC_T2D_SPLIT64
  kT2dNarrow = 4,     // PC_T2D_NARROW
  kT2dNbuf3 = 8,      // PC_T2D_NBUF3
  kT2d128 = 16,       // PC_T2D_128
  kT2d128x8 = 32,     // PC_T2D_128=8
};

// conv_hxi's split forms without padding columns in their pixel fragments (Tuning::hxi_dense, PC_HXI_DENSE)
enum HxiDense { kHxiDense14 = 2, kHxiDense28 = 4 };

}  // namespace pc
