// Device-side job descriptors of the frame-gauge kernels (pc_gauge.hip), filled by pc_frame_gray,
// pc_gray_region_hist and pc_gray_motion.
#pragma once
#include <stdint.h>

namespace pc {

struct GaugeImg {
  const uint8_t* src;   // BGR u8
  long long row_stride;
  int w, h;
  int gpitch;           // gray plane pitch (a multiple of 16; the plane is 16-byte aligned)
  int pad_;
  uint8_t* gray;
  unsigned* row_sum;    // [h]
  unsigned* col_sum;    // [w], zero before the launch
};

// A rectangle of a gray plane: `base` is its top-left byte, rows `pitch` apart.
struct GaugeRegion {
  const uint8_t* base;
  long long pitch;
  int w, h;
  unsigned* hist;       // [256], zero before the launch
};

struct GaugeBox {
  const uint8_t* cur;   // top-left byte of the box in the current plane
  const uint8_t* prev;  // and in the previous one
  long long pitch;
  int w, h;
  unsigned* count;      // zero before the launch
};

// One workgroup of gauge_region_hist / gauge_motion: rows [y0, y0 + rows) of item `item`.
struct GaugeJob { int item, y0, rows, pad_; };

constexpr int GAUGE_BAND = 32;       // most rows per workgroup of frame_gray
constexpr int GAUGE_MIN_WG = 1024;   // workgroups a frame_gray launch tries to reach with shorter bands
constexpr int GAUGE_JOB_UNITS = 512; // 16-byte units a region / motion workgroup aims at

}  // namespace pc
