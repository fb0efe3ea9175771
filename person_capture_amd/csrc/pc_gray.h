// cv2.cvtColor(BGR2GRAY) for u8, stated once: OpenCV's 14-bit fixed-point coefficients
// (B 1868, G 9617, R 4899, rounding term 2^13). face_quality (pc_image.hip), curate_gray
// (pc_curate.hip) and frame_gray (pc_gauge.hip) all take their gray value from here.
#pragma once

namespace pc {

__device__ __forceinline__ int gray14(int b, int g, int r) {
  return (b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14;
}

}  // namespace pc
