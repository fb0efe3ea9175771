// cv2.resize INTER_AREA arithmetic for one output pixel of CN interleaved u8 channels, shared by the
// three-channel kernels of pc_image.hip and the one-channel (gray plane) kernel of pc_curate.hip:
// the same products in the same order whatever the channel count. Include after
// `#pragma clang fp contract(off)`: a fused multiply-add would change the float sums.
#pragma once
#include "pc_common.h"

namespace pc {

struct AreaTab { int si; int di; float alpha; };

// OpenCV's generic (non-integer scale) area path: float weights, accumulated per output pixel in
// source order (x-window of every source row, then the rows), saturate_cast<uchar> (round half to
// even) at the end. Window [i0, i1) of xtab, [j0, j1) of ytab.
template <int CN>
__device__ __forceinline__ void area_pixel(const uint8_t* __restrict__ src, long long row_stride,
                                           const AreaTab* __restrict__ xtab, int i0, int i1,
                                           const AreaTab* __restrict__ ytab, int j0, int j1, uint8_t* o) {
  float acc[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) acc[c] = 0.f;
  for (int j = j0; j < j1; ++j) {
    const AreaTab ty = ytab[j];
    const uint8_t* row = src + (long long)ty.si * row_stride;
    float rs[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) rs[c] = 0.f;
    for (int i = i0; i < i1; ++i) {
      const AreaTab tx = xtab[i];
#pragma unroll
      for (int c = 0; c < CN; ++c) rs[c] += (float)row[tx.si * CN + c] * tx.alpha;
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) acc[c] += rs[c] * ty.alpha;
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    int v = __float2int_rn(acc[c]);
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// An exact integer ratio isx x isy (hal::resize "is_area_fast", resizeAreaFast_Invoker): 2x2 takes
// ResizeAreaFastVec ((sum + 2) >> 2 for every byte); other ratios
// saturate_cast<uchar>(sum * (1.f / area)) (round half to even).
template <int CN>
__device__ __forceinline__ void area_fast_pixel(const uint8_t* __restrict__ src, long long row_stride, int isx,
                                                int isy, int dx, int dy, uint8_t* o) {
  const float scale = 1.f / (float)(isx * isy);
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    int sum = 0;
    for (int j = 0; j < isy; ++j) {
      const uint8_t* row = src + (long long)(dy * isy + j) * row_stride + (dx * isx) * CN + c;
      for (int i = 0; i < isx; ++i) sum += row[i * CN];
    }
    int v = (isx == 2 && isy == 2) ? ((sum + 2) >> 2) : __float2int_rn((float)sum * scale);
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

}  // namespace pc
