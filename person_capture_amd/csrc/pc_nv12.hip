// NV12 frames on the device (gfx950): the colour conversion of the reference's frame source and the
// pre-scan's downscale fused with it.
//
// The reference's FfmpegPipeReader receives NV12 from the decoder when PC_PIPE_PIXFMT=nv12 (or after a
// pipe ENOMEM) and converts every frame on the CPU with float32 NumPy (FfmpegPipeReader._nv12_to_bgr,
// video_io.py:2888-2912). The operation, restated (person_capture_amd/frames.py holds the same in NumPy):
//   Y plane H x W u8, UV plane (H/2) x W u8 interleaved U, V; a chroma sample serves its 2 x 2 pixels;
//   C = y - 16, D = u - 128, E = v - 128 in f32, constants rounded to f32, every operation rounded once:
//     r = k0 C + k1 E        g = (k0 C - k2 D) - k3 E        b = k0 C + k4 D
//   clamp to [0, 255], truncate to u8, store B, G, R.
// A fused multiply-add changes 22 of the 2^24 (Y, U, V) triples, hence the pragma below.
//
// All of it is bandwidth-bound: 1.5 bytes read and 3 written per pixel.
#include "pc_common.h"

#pragma clang fp contract(off)

#include "pc_area.h"

namespace pc {

__device__ __forceinline__ unsigned nv12_u8(float x) {
  x = fminf(fmaxf(x, 0.f), 255.f);
  return (unsigned)(int)x;   // truncation, as ndarray.astype(uint8) of a clipped f32
}

// the chroma terms of one (U, V) sample, shared by its 2 x 2 pixels
struct Nv12Chroma { float rE, gD, gE, bD; };

__device__ __forceinline__ Nv12Chroma nv12_chroma(int u, int v) {
  const float D = (float)u - 128.0f, E = (float)v - 128.0f;
  Nv12Chroma c;
  c.rE = 1.79274107f * E;
  c.gD = 0.21324861f * D;
  c.gE = 0.53290933f * E;
  c.bD = 2.11240179f * D;
  return c;
}

// one pixel: bgr[0..2] as u8 values
__device__ __forceinline__ void nv12_pixel(int y, const Nv12Chroma& c, unsigned bgr[3]) {
  const float yc = 1.16438356f * ((float)y - 16.0f);
  bgr[0] = nv12_u8(yc + c.bD);
  bgr[1] = nv12_u8((yc - c.gD) - c.gE);
  bgr[2] = nv12_u8(yc + c.rE);
}

// ---------------------------------------------------------------------------
// pc_nv12_to_bgr: n frames of any sizes in one launch. A thread's unit is 16 pixels of two rows (one
// chroma row): two 16-byte Y loads, one 16-byte UV load, 3 x 16-byte stores per row. A frame whose
// plane pointers, strides or destination are not 16-byte aligned takes byte loads and stores for every
// unit, an aligned frame only for the last unit of a row when W % 16 != 0. No load leaves [row, row + W)
// of a source row, no store [row, row + 3 W) of a destination row.
// ---------------------------------------------------------------------------
struct Nv12Job {
  const uint8_t* y;
  const uint8_t* uv;
  uint8_t* dst;
  int H, W, y_stride, uv_stride, dst_stride;
  int aligned;      // every pointer and stride a multiple of 16
  int ux;           // units per row pair: ceil(W / 16)
  int wg0;          // the frame's first workgroup (a workgroup is 256 units of one frame)
};

__global__ __launch_bounds__(256) void nv12_to_bgr_u8(const Nv12Job* __restrict__ jobs, int n) {
  // the frame of this workgroup: the last job with wg0 <= blockIdx.x (uniform: scalar loads)
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const Nv12Job j = jobs[lo];
  const long long unit = (long long)((int)blockIdx.x - j.wg0) * 256 + threadIdx.x;
  const int rp = (int)(unit / j.ux);
  if (rp >= (j.H >> 1)) return;
  const int x0 = ((int)(unit - (long long)rp * j.ux)) * 16;
  const uint8_t* y0 = j.y + (long long)(2 * rp) * j.y_stride + x0;
  const uint8_t* y1 = y0 + j.y_stride;
  const uint8_t* uv = j.uv + (long long)rp * j.uv_stride + x0;
  uint8_t* d0 = j.dst + (long long)(2 * rp) * j.dst_stride + 3 * x0;
  uint8_t* d1 = d0 + j.dst_stride;
  if (j.aligned && x0 + 16 <= j.W) {
    // (the pointers come out of the job record as generic ones: say that they are global memory)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) const u32x4* gload_t;
    typedef __attribute__((address_space(1))) u32x4* gstore_t;
    const u32x4 a0 = *(gload_t)y0;
    const u32x4 a1 = *(gload_t)y1;
    const u32x4 c4 = *(gload_t)uv;
    const unsigned yw[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
    const unsigned cw[4] = {c4.x, c4.y, c4.z, c4.w};
    unsigned o[2][12];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 12; ++k) o[r][k] = 0u;
#pragma unroll
    for (int p = 0; p < 8; ++p) {   // chroma sample p: pixels 2 p, 2 p + 1 of both rows
      const unsigned w = cw[p >> 1] >> (16 * (p & 1));
      const Nv12Chroma c = nv12_chroma((int)(w & 0xffu), (int)((w >> 8) & 0xffu));
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int px = 2 * p + q;
          unsigned bgr[3];
          nv12_pixel((int)((yw[r][px >> 2] >> (8 * (px & 3))) & 0xffu), c, bgr);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const int b = 3 * px + ch;
            o[r][b >> 2] |= bgr[ch] << (8 * (b & 3));
          }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ((gstore_t)d0)[k] = u32x4{o[0][4 * k], o[0][4 * k + 1], o[0][4 * k + 2], o[0][4 * k + 3]};
      ((gstore_t)d1)[k] = u32x4{o[1][4 * k], o[1][4 * k + 1], o[1][4 * k + 2], o[1][4 * k + 3]};
    }
    return;
  }
  // byte-granular: W is even, so the unit is whole chroma samples
  const int np = (j.W - x0 < 16 ? j.W - x0 : 16) >> 1;
  for (int p = 0; p < np; ++p) {
    const Nv12Chroma c = nv12_chroma(uv[2 * p], uv[2 * p + 1]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int px = 2 * p + q;
      unsigned t[3], b[3];
      nv12_pixel(y0[px], c, t);
      nv12_pixel(y1[px], c, b);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        d0[3 * px + ch] = (uint8_t)t[ch];
        d1[3 * px + ch] = (uint8_t)b[ch];
      }
    }
  }
}

hipError_t nv12_to_bgr_launch(const void* d_jobs, int n, long long nwg, hipStream_t s) {
  if (n <= 0 || nwg <= 0 || nwg >= (1LL << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nv12_to_bgr_u8, dim3((unsigned)nwg), dim3(256), 0, s, (const Nv12Job*)d_jobs, n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Conversion fused into cv2.resize INTER_AREA (the pre-scan's downscale, gui_app.py:1505-1507) for n
// equally sized NV12 frames: the pc_area.h arithmetic over source pixels converted in registers, so no
// full-size BGR frame is written. One thread per output pixel; the bytes are those of nv12_to_bgr_u8
// followed by resize_area_u8 / resize_area_fast_u8 (the same functions on the same values).
// ---------------------------------------------------------------------------
struct Nv12Px {
  const uint8_t* __restrict__ y;
  const uint8_t* __restrict__ uv;
  long long y_stride, uv_stride;
  __device__ __forceinline__ void operator()(int sy, int sx, int v[3]) const {
    const uint8_t* c = uv + (long long)(sy >> 1) * uv_stride + (sx & ~1);
    unsigned bgr[3];
    nv12_pixel(y[(long long)sy * y_stride + sx], nv12_chroma(c[0], c[1]), bgr);
    v[0] = (int)bgr[0]; v[1] = (int)bgr[1]; v[2] = (int)bgr[2];
  }
};

struct Nv12AreaJob { const uint8_t* y; const uint8_t* uv; uint8_t* dst; };

__global__ __launch_bounds__(256) void nv12_resize_area_u8(const Nv12AreaJob* __restrict__ jobs, int y_stride,
                                                           int uv_stride, const AreaTab* __restrict__ xtab,
                                                           const int* __restrict__ xtab_start,
                                                           const AreaTab* __restrict__ ytab,
                                                           const int* __restrict__ ytab_start, int OH, int OW) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= OH * OW) return;
  const Nv12AreaJob job = jobs[blockIdx.y];
  const int dy = pix / OW, dx = pix - (pix / OW) * OW;
  area_pixel_taps_px<3>(Nv12Px{job.y, job.uv, y_stride, uv_stride}, [=](int i) { return xtab[i]; }, xtab_start[dx],
                        xtab_start[dx + 1], [=](int k) { return ytab[k]; }, ytab_start[dy], ytab_start[dy + 1],
                        job.dst + (long long)pix * 3);
}

__global__ __launch_bounds__(256) void nv12_resize_area_fast_u8(const Nv12AreaJob* __restrict__ jobs, int y_stride,
                                                                int uv_stride, int isx, int isy, int OH, int OW) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= OH * OW) return;
  const Nv12AreaJob job = jobs[blockIdx.y];
  const int dy = pix / OW, dx = pix - (pix / OW) * OW;
  area_fast_pixel_px<3>(Nv12Px{job.y, job.uv, y_stride, uv_stride}, isx, isy, dx, dy, job.dst + (long long)pix * 3);
}

hipError_t nv12_resize_area_launch(const void* d_jobs, int n, int y_stride, int uv_stride, const AreaTab* xtab,
                                   const int* xstart, const AreaTab* ytab, const int* ystart, int OH, int OW,
                                   hipStream_t s) {
  if (n <= 0 || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nv12_resize_area_u8, dim3((OH * OW + 255) / 256, n), dim3(256), 0, s, (const Nv12AreaJob*)d_jobs,
                     y_stride, uv_stride, xtab, xstart, ytab, ystart, OH, OW);
  return hipGetLastError();
}

hipError_t nv12_resize_area_fast_launch(const void* d_jobs, int n, int y_stride, int uv_stride, int isx, int isy,
                                        int OH, int OW, hipStream_t s) {
  if (n <= 0 || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nv12_resize_area_fast_u8, dim3((OH * OW + 255) / 256, n), dim3(256), 0, s,
                     (const Nv12AreaJob*)d_jobs, y_stride, uv_stride, isx, isy, OH, OW);
  return hipGetLastError();
}

}  // namespace pc
