// Device-side job descriptors of the curator kernels (pc_curate.hip), filled by pc_crop_metrics.
#pragma once
#include <stdint.h>

namespace pc {

// One resize target of an image: kind 0 = the gray plane itself (nothing to do), 1 = integer
// ratio (isx, isy), 2 = generic tables (xs / ys: where the target's start arrays begin in the
// shared start array; the starts index the shared coefficient array).
struct CurateTarget {
  uint8_t* dst;
  int pitch, ow, oh, kind, isx, isy, xs, ys;
};

struct CurateImg {
  const uint8_t* src;   // BGR u8
  int row_stride, w, h;
  int gpitch;           // gray plane pitch (a multiple of 16; the plane is 16-byte aligned)
  uint8_t* gray;
  CurateTarget t[2];    // [0] the <= 256 plane of the sharpness, [1] the 32x32 plane of the pHash
  unsigned* hist;       // [256]
  unsigned* row_sum;    // [h]
  unsigned* col_sum;    // [w]
  unsigned long long* sums;   // sum g2, sum L (two's complement), sum L^2
  int* wh;              // w2, h2 of the record
  float* coef;          // [64]
};

constexpr int CURATE_BAND = 32;   // rows per workgroup of curate_gray

}  // namespace pc
