// cv2.resize INTER_AREA arithmetic for one output pixel of CN interleaved u8 channels, shared by the
// three-channel kernels of pc_image.hip and the one-channel (gray plane) kernel of pc_curate.hip:
// the same products in the same order whatever the channel count. Include after
// `#pragma clang fp contract(off)`: a fused multiply-add would change the float sums.
#pragma once
#include "pc_common.h"

namespace pc {

struct AreaTab { int si; int di; float alpha; };

// A pixel accessor px(sy, sx, v) puts the CN u8 channel values of source pixel (row sy, column sx) into
// v[CN]: interleaved memory (AreaMemPx), or NV12 planes converted in registers (pc_nv12.hip).
template <int CN>
struct AreaMemPx {
  const uint8_t* __restrict__ src;
  long long row_stride;
  __device__ __forceinline__ void operator()(int sy, int sx, int v[CN]) const {
    const uint8_t* p = src + (long long)sy * row_stride + sx * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) v[c] = p[c];
  }
};

// OpenCV's generic (non-integer scale) area path: float weights, accumulated per output pixel in
// source order (x-window of every source row, then the rows), saturate_cast<uchar> (round half to
// even) at the end. Window [i0, i1) of the x coefficients, [j0, j1) of the y coefficients; xt(i) /
// yt(j) return coefficient i / j as an AreaTab (a table in memory, or area_span_tap below).
template <int CN, typename PX, typename XT, typename YT>
__device__ __forceinline__ void area_pixel_taps_px(PX px, XT xt, int i0, int i1, YT yt, int j0, int j1, uint8_t* o) {
  float acc[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) acc[c] = 0.f;
  for (int j = j0; j < j1; ++j) {
    const AreaTab ty = yt(j);
    float rs[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) rs[c] = 0.f;
    for (int i = i0; i < i1; ++i) {
      const AreaTab tx = xt(i);
      int v[CN];
      px(ty.si, tx.si, v);
#pragma unroll
      for (int c = 0; c < CN; ++c) rs[c] += (float)v[c] * tx.alpha;
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

// The same over interleaved u8 memory.
template <int CN, typename XT, typename YT>
__device__ __forceinline__ void area_pixel_taps(const uint8_t* __restrict__ src, long long row_stride, XT xt, int i0,
                                                int i1, YT yt, int j0, int j1, uint8_t* o) {
  area_pixel_taps_px<CN>(AreaMemPx<CN>{src, row_stride}, xt, i0, i1, yt, j0, j1, o);
}

// The same with the coefficients in tables built on the host (imageops.area_tables).
template <int CN>
__device__ __forceinline__ void area_pixel(const uint8_t* __restrict__ src, long long row_stride,
                                           const AreaTab* __restrict__ xtab, int i0, int i1,
                                           const AreaTab* __restrict__ ytab, int j0, int j1, uint8_t* o) {
  area_pixel_taps<CN>(src, row_stride, [=](int i) { return xtab[i]; }, i0, i1, [=](int j) { return ytab[j]; }, j0, j1, o);
}

// cv::computeResizeAreaTab (cn = 1) for one destination index d of an ssize -> dsize axis at
// `scale`, in closed form: the coefficients of d are n consecutive source indices from s0; the first
// weighs w_first when `lead` (a partial leading cell), the last w_last when `trail`, every other one
// w_mid = 1 / cell. The same f64 operations in the same order as the host table
// (imageops._area_tables), each rounded once (no contraction), so the f32 weights are its bits.
struct AreaSpan { int s0, n; float w_first, w_mid, w_last; int lead, trail; };

__device__ __forceinline__ AreaSpan area_span(int d, int ssize, double scale) {
#pragma clang fp contract(off)
  const double fsx1 = d * scale;
  const double fsx2 = fsx1 + scale;
  const double cell = fmin(scale, ssize - fsx1);
  int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
  sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
  sx1 = sx1 < sx2 ? sx1 : sx2;
  AreaSpan s;
  s.lead = sx1 - fsx1 > 1e-3;
  s.trail = fsx2 - sx2 > 1e-3;
  s.s0 = sx1 - s.lead;
  s.n = s.lead + (sx2 - sx1) + s.trail;
  // (0 <= s0 and s0 + n <= ssize follow from the above for scale >= 1; the clamps keep every load
  // inside the axis whatever the caller passed)
  s.s0 = s.s0 < 0 ? 0 : (s.s0 > ssize - 1 ? ssize - 1 : s.s0);
  s.n = s.n < 0 ? 0 : (s.n > ssize - s.s0 ? ssize - s.s0 : s.n);
  s.w_first = (float)((sx1 - fsx1) / cell);
  s.w_mid = (float)(1.0 / cell);
  s.w_last = (float)(fmin(fmin(fsx2 - sx2, 1.0), cell) / cell);
  return s;
}

// coefficient t (0 <= t < s.n) of destination d
__device__ __forceinline__ AreaTab area_span_tap(const AreaSpan& s, int d, int t) {
  const float a = (t == 0 && s.lead) ? s.w_first : ((t == s.n - 1 && s.trail) ? s.w_last : s.w_mid);
  return AreaTab{s.s0 + t, d, a};
}

// An exact integer ratio isx x isy (hal::resize "is_area_fast", resizeAreaFast_Invoker): 2x2 takes
// ResizeAreaFastVec ((sum + 2) >> 2 for every byte); other ratios
// saturate_cast<uchar>(sum * (1.f / area)) (round half to even).
// (the sums are integers, so the channels of a pixel are summed together: one accessor call per tap)
template <int CN, typename PX>
__device__ __forceinline__ void area_fast_pixel_px(PX px, int isx, int isy, int dx, int dy, uint8_t* o) {
  const float scale = 1.f / (float)(isx * isy);
  int sum[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) sum[c] = 0;
  for (int j = 0; j < isy; ++j) {
    for (int i = 0; i < isx; ++i) {
      int v[CN];
      px(dy * isy + j, dx * isx + i, v);
#pragma unroll
      for (int c = 0; c < CN; ++c) sum[c] += v[c];
    }
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    int v = (isx == 2 && isy == 2) ? ((sum[c] + 2) >> 2) : __float2int_rn((float)sum[c] * scale);
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

template <int CN>
__device__ __forceinline__ void area_fast_pixel(const uint8_t* __restrict__ src, long long row_stride, int isx,
                                                int isy, int dx, int dy, uint8_t* o) {
  area_fast_pixel_px<CN>(AreaMemPx<CN>{src, row_stride}, isx, isy, dx, dy, o);
}

}  // namespace pc
