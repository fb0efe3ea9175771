// HDR linear-light frames on the device (gfx950): EOTF, Hable tone map, BT.709 OETF and u8 store of the
// reference's frame source.
//
// An HDR source on an ffmpeg without libplacebo or zscale + tonemap makes the reference's FfmpegPipeReader
// read gbrpf32le (planar float32 G, B, R of the PQ or HLG signal, video_io.py:2513-2520) and convert every
// frame on the CPU with float32 NumPy: restack (video_io.py:3005-3014), _eotf_pq / _eotf_hlg (:3015-3018,
// :3239-3258), _python_tonemap_to_bgr8 (:3183-3192, :3276-3291). The operation is stated in full in
// person_capture_amd/frames_hdr.py, which holds the same in NumPy; in short, per pixel, every operation in
// f32 rounded once in the order written here, no fused multiply-add (the pragma below), IEEE division,
// subnormals kept, the two transcendentals defined as the f64 value rounded to f32:
//     P(x, e) = (float)pow((double)x, (double)e)   (e already an f32)      X(x) = (float)exp((double)x)
//
// The kernel is bound by f64 VALU work (nine P per PQ pixel), not by its 15 bytes per pixel.
#include "pc_common.h"
#include "../../include/pcgpu.h"

#pragma clang fp contract(off)

namespace pc {

// (the pixel arithmetic is plain C++ and also compiles for the host, where a stand-alone program can run it
// against the NumPy backend without a GPU)
__host__ __device__ __forceinline__ float hdr_P(float x, float e) { return (float)pow((double)x, (double)e); }
__host__ __device__ __forceinline__ float hdr_X(float x) { return (float)exp((double)x); }
__host__ __device__ __forceinline__ float hdr_clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// _eotf_pq (video_io.py:3239-3251); the exponents are f32(1 / m2), f32(1 / m1)
__host__ __device__ __forceinline__ float hdr_eotf_pq(float x) {
  const float v = hdr_clip01(x);
  const float p = hdr_P(v, 0x1.9f9b58p-7f);             // 32 / 2523
  const float vp = fmaxf(p - 0.8359375f, 0.f);          // c1 = 3424 / 4096
  float den = 18.8515625f - 18.6875f * p;               // c2 = 2413 / 128, c3 = 2392 / 128
  den = fabsf(den) < 1e-6f ? 1e-6f : den;
  return hdr_clip01(hdr_P(vp / den, 0x1.91c0d6p+2f));   // 16384 / 2610
}

// _eotf_hlg (video_io.py:3254-3258); the exp of the branch np.where discards is not taken
__host__ __device__ __forceinline__ float hdr_eotf_hlg(float x) {
  const float v = hdr_clip01(x);
  if (v <= 0.5f) return (v * v) / 3.0f;
  return (hdr_X((v - 0.55991073f) / 0.17883277f) + 0.28466892f) / 12.0f;
}

// _hable_filmic's h (video_io.py:3268-3271): C*B, D*E, D*F and E/F are f64 products rounded to f32
__host__ __device__ __forceinline__ float hdr_hable(float y) {
  const float A = 0.15f, B = 0.5f, CB = 0x1.99999ap-5f, DE = 0x1.0624dep-8f, DF = 0x1.eb851ep-5f,
              EF = 0x1.111112p-4f;
  return ((y * (A * y + CB) + DE) / (y * (A * y + B) + DF)) - EF;
}

// _oetf_bt709 (video_io.py:3261-3265) and the u8 store of _python_tonemap_to_bgr8 (:3290)
__host__ __device__ __forceinline__ unsigned hdr_oetf_u8(float N) {
  float o = N < 0.018f ? 4.5f * N : 1.099f * hdr_P(N, 0.45f) - 0.099f;
  o = hdr_clip01(o);
  return (unsigned)(int)(o * 255.0f + 0.5f);   // o in [0, 1]: truncation, as astype(uint8)
}

struct HdrJob {
  const float* r;
  const float* g;
  const float* b;
  uint8_t* dst;
  int H, W, pix_stride, row_stride, dst_stride, transfer;
  float t32, peak;   // f32(target_nits), f32(max(peak_nits, 1e-3))
  int wide;          // sample pointers and row strides multiples of 16 bytes, destination of 4
  int ux;            // units per row: ceil(W / 4)
  int wg0;           // the frame's first workgroup (a workgroup is 256 units of one frame)
  int pad_;
};

// one pixel: B | G << 8 | R << 16
__host__ __device__ __forceinline__ unsigned hdr_pixel(float r, float g, float b, int transfer, float t32, float peak) {
  float lr, lg, lb;
  if (transfer == PC_HDR_PQ) {
    lr = hdr_eotf_pq(r); lg = hdr_eotf_pq(g); lb = hdr_eotf_pq(b);
  } else if (transfer == PC_HDR_HLG) {
    lr = hdr_eotf_hlg(r); lg = hdr_eotf_hlg(g); lb = hdr_eotf_hlg(b);
  } else {
    lr = r; lg = g; lb = b;
  }
  const float Lr = hdr_clip01(lr) * 10000.0f, Lg = hdr_clip01(lg) * 10000.0f, Lb = hdr_clip01(lb) * 10000.0f;
  const float Y = (0.2627f * Lr + 0.6780f * Lg) + 0.0593f * Lb;
  const float white = 0x1.734428p-1f;   // f32 of h(11.2) evaluated in f64
  const float Yt = hdr_clip01(hdr_hable(Y / peak) / white) * t32;
  const float s = Yt / fmaxf(Y, 1e-6f);
  const float Nr = hdr_clip01(fminf(fmaxf(Lr * s, 0.f), t32) / 100.0f);
  const float Ng = hdr_clip01(fminf(fmaxf(Lg * s, 0.f), t32) / 100.0f);
  const float Nb = hdr_clip01(fminf(fmaxf(Lb * s, 0.f), t32) / 100.0f);
  return hdr_oetf_u8(Nb) | (hdr_oetf_u8(Ng) << 8) | (hdr_oetf_u8(Nr) << 16);
}

// ---------------------------------------------------------------------------
// pc_hdr_to_bgr: n frames of any sizes in one launch. A thread's unit is 4 consecutive pixels of a row,
// one after the other (one copy of the nine inlined f64 pow bodies, few live registers: the occupancy
// hides the f64 latency; the kernel's time is the f64 work, a tenth of the frame's upload). A whole unit of
// a `wide` frame takes three 16-byte loads (a float4 per plane, or the 12 interleaved floats) and one
// 12-byte store; any other unit float loads and byte stores. No load leaves the W pixels of a source
// row, no store [row, row + 3 W) of a destination row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hdr_to_bgr_u8(const HdrJob* __restrict__ jobs, int n) {
  // the frame of this workgroup: the last job with wg0 <= blockIdx.x (uniform: scalar loads)
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const HdrJob j = jobs[lo];
  const long long unit = (long long)((int)blockIdx.x - j.wg0) * 256 + threadIdx.x;
  const int row = (int)(unit / j.ux);
  if (row >= j.H) return;
  const int x0 = ((int)(unit - (long long)row * j.ux)) * 4;
  const long long so = (long long)row * j.row_stride + (long long)x0 * j.pix_stride;
  const float* pr = j.r + so;
  const float* pg = j.g + so;
  const float* pb = j.b + so;
  uint8_t* d = j.dst + (long long)row * j.dst_stride + 3 * x0;
  const int np = j.W - x0 < 4 ? j.W - x0 : 4;
  const bool wide = j.wide && np == 4;
  typedef __attribute__((address_space(1))) const f32x4* gload_t;
  f32x4 R = {0.f, 0.f, 0.f, 0.f}, G = R, B = R;
  if (wide) {
    if (j.pix_stride == 1) {
      R = *(gload_t)pr; G = *(gload_t)pg; B = *(gload_t)pb;
    } else {   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (pr is the frame's R pointer: the triple's start)
      const f32x4 a = ((gload_t)pr)[0], b = ((gload_t)pr)[1], c = ((gload_t)pr)[2];
      R = f32x4{a.x, a.w, b.z, c.y};
      G = f32x4{a.y, b.x, b.w, c.z};
      B = f32x4{a.z, b.y, c.x, c.w};
    }
  }
  unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int k = 0; k < np; ++k) {
    float r, g, b;
    if (wide) {
      r = k == 0 ? R.x : k == 1 ? R.y : k == 2 ? R.z : R.w;
      g = k == 0 ? G.x : k == 1 ? G.y : k == 2 ? G.z : G.w;
      b = k == 0 ? B.x : k == 1 ? B.y : k == 2 ? B.z : B.w;
    } else {
      r = pr[k * j.pix_stride]; g = pg[k * j.pix_stride]; b = pb[k * j.pix_stride];
    }
    const unsigned v = hdr_pixel(r, g, b, j.transfer, j.t32, j.peak);
    if (wide) {
      px[0] = k == 0 ? v : px[0]; px[1] = k == 1 ? v : px[1];
      px[2] = k == 2 ? v : px[2]; px[3] = k == 3 ? v : px[3];
    } else {
      d[3 * k] = (uint8_t)v; d[3 * k + 1] = (uint8_t)(v >> 8); d[3 * k + 2] = (uint8_t)(v >> 16);
    }
  }
  if (wide) {
    typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
    typedef __attribute__((address_space(1))) unsigned* gstore_t;
    const u32x3 o = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
    gstore_t q = (gstore_t)d;
    q[0] = o.x; q[1] = o.y; q[2] = o.z;
  }
}

hipError_t hdr_to_bgr_launch(const void* d_jobs, int n, long long nwg, hipStream_t s) {
  if (n <= 0 || nwg <= 0 || nwg >= (1LL << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hdr_to_bgr_u8, dim3((unsigned)nwg), dim3(256), 0, s, (const HdrJob*)d_jobs, n);
  return hipGetLastError();
}

}  // namespace pc
