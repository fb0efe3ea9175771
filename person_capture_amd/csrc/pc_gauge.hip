// Main-pass frame gauges (gfx950): the gray-plane measurements the reference's Processor.run takes on
// the CPU for every processed frame (gui_app.py:5740-8002).
//
//   frame_gray         BGR u8 -> gray plane, row sums, column sums (gui_app.py:5754 BGR2GRAY; the sums
//                      are what detect_black_borders, utils.py:152-196, reads through _autocrop_borders,
//                      gui_app.py:3360-3384). curate_gray's band scheme without the histogram.
//   gauge_region_hist  exact 256-bin histograms of rectangles of gray planes: the border strips of
//                      _is_real_letterbox_crop (gui_app.py:3386-3448), whose p95 / p99 / std the host
//                      derives from the counts
//   gauge_motion       pixels of a box with |cur - prev| > thresh: absdiff + threshold + countNonZero
//                      of _faceless_validate (gui_app.py:4275-4285)
//   gauge_resize       gray plane -> the <= 384 wide plane of _smart_crop_box's gradient saliency
//                      (gui_app.py:8295-8301), cv2.resize INTER_AREA (pc_area.h at one channel, the
//                      code curate_resize calls)
//
// Everything that leaves the device is an exact integer; every decision is taken on the host
// (frame_gauges.py).
#include "pc_common.h"

#pragma clang fp contract(off)

#include "pc_area.h"
#include "pc_gauge.h"
#include "pc_gray.h"

namespace pc {

__device__ __forceinline__ unsigned gauge_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// curate_gray's scheme (pc_curate.hip) without the histogram: a workgroup is `band` rows of one frame, a
// thread owns a 16-pixel column chunk (three 16-byte loads where the source row segment is aligned, byte
// loads otherwise and in the row's tail; one 16-byte store, the plane's pitch being a multiple of 16) and
// walks it down the band with the chunk's 16 column sums in registers. A row takes CW lanes (its chunks
// rounded up to whole waves, at most 256); frames narrower than 2048 pixels put R = 256 / CW rows side
// by side, wider ones loop over groups of 256 chunks. A wave holds one row, so its row sum is a wave
// reduction; the band owns its rows, so row sums are plain stores. Column sums always pass through the
// LDS (added there when R > 1, stored when a column has one owner), so that they leave as integer
// atomics on consecutive addresses, one per column and band: issued from the registers, lane l of a
// wave would add 64 bytes from lane l + 1, the shape global atomics are slowest at. Nothing is read
// outside [row, row + 3 w) of a source row.
union GrayRow { uint4 v[3]; uint8_t b[48]; };

__global__ __launch_bounds__(256) void frame_gray(const GaugeImg* __restrict__ imgs, const int2* __restrict__ bands,
                                                  int band) {
  __shared__ unsigned rowacc[GAUGE_BAND];
  __shared__ __attribute__((aligned(16))) unsigned colacc[256 * 16];
  const int2 bd = bands[blockIdx.x];
  const GaugeImg* d = imgs + bd.x;
  const uint8_t* src = d->src;
  const int w = d->w, h = d->h, gpitch = d->gpitch;
  const long long row_stride = d->row_stride;
  uint8_t* gray = d->gray;
  const int y0 = bd.y, y1 = min(y0 + band, h);
  const int tid = threadIdx.x;
  const int nchunk = (w + 15) >> 4;
  const int CW = min(256, (nchunk + 63) & ~63);
  const int R = 256 / CW;                     // 4, 2 or 1 (CW = 192: one row, the last wave idles)
  const int cx = tid % CW, ry = tid / CW;     // (wave-uniform ry: CW is whole waves)
  if (tid < GAUGE_BAND) rowacc[tid] = 0u;
  if (R > 1)
    for (int i = tid; i < 128 * 16; i += 256) colacc[i] = 0u;
  __syncthreads();
  for (int base = 0; base < nchunk; base += CW) {   // (one pass when R > 1)
    const int ch = base + cx;
    const bool live = ch < nchunk && ry < R;   // (CW = 192: the lanes of the last wave own nothing)
    const int x0 = ch << 4;
    const int nv = live ? min(16, w - x0) : 0;
    unsigned col[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) col[i] = 0u;
    auto load = [&](GrayRow& in, int y) {
      const uint8_t* p = src + (long long)y * row_stride + (long long)x0 * 3;
      if (nv == 16 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) in.v[k] = reinterpret_cast<const uint4*>(p)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 48; ++k) in.b[k] = k < nv * 3 ? p[k] : (uint8_t)0;
      }
    };
    auto convert = [&](const GrayRow& in, int y) {   // (every lane of the wave: the row sum shuffles)
      unsigned rs = 0u;
      if (live) {
        union { uint4 v; uint8_t b[16]; } out;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int g = gray14(in.b[i * 3], in.b[i * 3 + 1], in.b[i * 3 + 2]);
          out.b[i] = (uint8_t)g;   // (padding bytes of the tail: gray14(0, 0, 0) = 0)
          if (i < nv) {
            col[i] += (unsigned)g;
            rs += (unsigned)g;
          }
        }
        *reinterpret_cast<uint4*>(gray + (long long)y * gpitch + x0) = out.v;
      }
      rs = gauge_wave_sum(rs);
      if ((tid & 63) == 0 && rs) atomicAdd(&rowacc[y - y0], rs);
    };
    for (int y = ry < R ? y0 + ry : y1; y < y1; y += R) {   // (wave-uniform trip count)
      GrayRow ra;
      if (live) load(ra, y);
      convert(ra, y);
    }
    if (R > 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < nv && col[i]) atomicAdd(&colacc[cx * 16 + i], col[i]);   // (base = 0: cx * 16 + i is the column)
    } else {
      if (base) __syncthreads();   // the flush of the pass before has read colacc
      if (live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          reinterpret_cast<uint4*>(colacc + cx * 16)[j] = make_uint4(col[4 * j], col[4 * j + 1], col[4 * j + 2], col[4 * j + 3]);
      }
      __syncthreads();
      const int c0 = base << 4, nc = min(256 * 16, w - c0);
      for (int i = tid; i < nc; i += 256)
        if (colacc[i]) atomicAdd(d->col_sum + c0 + i, colacc[i]);
    }
  }
  __syncthreads();
  if (tid < y1 - y0) d->row_sum[y0 + tid] = rowacc[tid];
  if (R > 1)
    for (int i = tid; i < w; i += 256)
      if (colacc[i]) atomicAdd(d->col_sum + i, colacc[i]);
}

// A row segment [0, w) of a rectangle is cut into units: unit 0 the `lead` bytes before the first
// 16-byte boundary of the row's address, unit u >= 1 the 16 bytes from lead + 16 (u - 1) (fewer at the
// row's end). A whole unit is one aligned 16-byte load; a head, a tail or a strip narrower than its
// alignment gap goes byte by byte. U = (w + 15) / 16 + 1 units cover any row; no byte outside
// [0, w) is touched.
__device__ __forceinline__ void gauge_unit(int u, int lead, int w, int& a, int& nv) {
  a = u == 0 ? 0 : lead + ((u - 1) << 4);
  const int b = u == 0 ? lead : min(a + 16, w);
  nv = max(0, b - a);
}

// One workgroup per job: some rows of one region. Per-wave LDS histograms flushed with integer
// atomics (they commute: the counts do not depend on the order). A black bar is nearly one value,
// which would serialise 16 LDS atomics of every lane on one address; a thread therefore merges the
// runs of equal bytes of its unit and adds each run once.
__global__ __launch_bounds__(256) void gauge_region_hist(const GaugeRegion* __restrict__ regs,
                                                         const GaugeJob* __restrict__ jobs) {
  __shared__ unsigned hist[4][256];
  const GaugeJob jb = jobs[blockIdx.x];
  const GaugeRegion r = regs[jb.item];
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int i = tid; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const int U = ((r.w + 15) >> 4) + 1;
  const int total = jb.rows * U;   // (rows <= 16384, U <= 1025)
  for (int i = tid; i < total; i += 256) {
    const int ry = i / U, u = i - ry * U;
    const uint8_t* row = r.base + (long long)(jb.y0 + ry) * r.pitch;
    const int lead = min(r.w, (int)((16u - (unsigned)((uintptr_t)row & 15)) & 15u));
    int a, nv;
    gauge_unit(u, lead, r.w, a, nv);
    if (nv == 0) continue;
    union { uint4 v; uint8_t b[16]; } in;
    if (nv == 16) {
      in.v = *reinterpret_cast<const uint4*>(row + a);   // (u >= 1: row + lead is a 16-byte boundary)
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) in.b[k] = k < nv ? row[a + k] : (uint8_t)0;
    }
    int cur = in.b[0];
    unsigned cnt = 1u;
#pragma unroll
    for (int k = 1; k < 16; ++k) {
      if (k < nv) {
        const int v = in.b[k];
        if (v == cur) {
          ++cnt;
        } else {
          atomicAdd(&hist[wave][cur], cnt);
          cur = v;
          cnt = 1u;
        }
      }
    }
    atomicAdd(&hist[wave][cur], cnt);
  }
  __syncthreads();
  const unsigned hv = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
  if (hv) atomicAdd(r.hist + tid, hv);
}

// One workgroup per job: some rows of one box. Both planes share the pitch; where the two row
// addresses also share their offset from a 16-byte boundary, whole units are 16-byte loads of both,
// otherwise the row goes byte by byte. Every lane runs the same number of rounds, so each of the 16
// byte positions of a round is one wave ballot whose popcount is the wave's count for it; a wave's
// total goes to the LDS and the workgroup adds once to the box's counter.
__global__ __launch_bounds__(256) void gauge_motion(const GaugeBox* __restrict__ boxes, const GaugeJob* __restrict__ jobs,
                                                    int thresh) {
  __shared__ unsigned wcnt[4];
  const GaugeJob jb = jobs[blockIdx.x];
  const GaugeBox bx = boxes[jb.item];
  const int tid = threadIdx.x;
  const int U = ((bx.w + 15) >> 4) + 1;
  const int total = jb.rows * U;
  unsigned cnt = 0u;   // wave-uniform
  for (int i0 = 0; i0 < total; i0 += 256) {
    const int i = i0 + tid;
    int nv = 0;
    union { uint4 v; uint8_t b[16]; } c, p;
    c.v = make_uint4(0u, 0u, 0u, 0u);
    p.v = make_uint4(0u, 0u, 0u, 0u);
    if (i < total) {
      const int ry = i / U, u = i - ry * U;
      const long long off = (long long)(jb.y0 + ry) * bx.pitch;
      const uint8_t* crow = bx.cur + off;
      const uint8_t* prow = bx.prev + off;
      const bool same = (((uintptr_t)crow ^ (uintptr_t)prow) & 15) == 0;
      const int lead = same ? min(bx.w, (int)((16u - (unsigned)((uintptr_t)crow & 15)) & 15u)) : 0;
      int a;
      gauge_unit(u, lead, bx.w, a, nv);
      if (nv == 16 && same) {
        c.v = *reinterpret_cast<const uint4*>(crow + a);
        p.v = *reinterpret_cast<const uint4*>(prow + a);
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          c.b[k] = k < nv ? crow[a + k] : (uint8_t)0;
          p.b[k] = k < nv ? prow[a + k] : (uint8_t)0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int dlt = (int)c.b[k] - (int)p.b[k];
      const bool moved = k < nv && (dlt < 0 ? -dlt : dlt) > thresh;
      cnt += (unsigned)__popcll(__ballot(moved));
    }
  }
  if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    const unsigned t = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (t) atomicAdd(bx.count, t);
  }
}

// One thread per output pixel: kind 1 integer ratios, kind 2 generic tables (curate_resize's two calls).
__global__ __launch_bounds__(256) void gauge_resize(const uint8_t* __restrict__ gray, long long gpitch, int kind, int isx,
                                                    int isy, const AreaTab* __restrict__ xt, const int* __restrict__ xs,
                                                    const AreaTab* __restrict__ yt, const int* __restrict__ ys,
                                                    uint8_t* __restrict__ dst, long long dpitch, int ow, int oh) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= ow * oh) return;
  const int dy = pix / ow, dx = pix - dy * ow;
  uint8_t* o = dst + (long long)dy * dpitch + dx;
  if (kind == 1)
    area_fast_pixel<1>(gray, gpitch, isx, isy, dx, dy, o);
  else
    area_pixel<1>(gray, gpitch, xt, xs[dx], xs[dx + 1], yt, ys[dy], ys[dy + 1], o);
}

// ---------------------------------------------------------------------------
hipError_t frame_gray_launch(const void* d_imgs, const void* d_bands, int nbands, int band, hipStream_t s) {
  if (band < 1 || band > GAUGE_BAND) return hipErrorInvalidValue;
  hipLaunchKernelGGL(frame_gray, dim3(nbands), dim3(256), 0, s, (const GaugeImg*)d_imgs, (const int2*)d_bands, band);
  return hipGetLastError();
}

hipError_t gauge_region_hist_launch(const void* d_regs, const void* d_jobs, int njobs, hipStream_t s) {
  hipLaunchKernelGGL(gauge_region_hist, dim3(njobs), dim3(256), 0, s, (const GaugeRegion*)d_regs,
                     (const GaugeJob*)d_jobs);
  return hipGetLastError();
}

hipError_t gauge_motion_launch(const void* d_boxes, const void* d_jobs, int njobs, int thresh, hipStream_t s) {
  hipLaunchKernelGGL(gauge_motion, dim3(njobs), dim3(256), 0, s, (const GaugeBox*)d_boxes, (const GaugeJob*)d_jobs,
                     thresh);
  return hipGetLastError();
}

hipError_t gauge_resize_launch(const uint8_t* gray, long long gpitch, int kind, int isx, int isy, const void* xt,
                               const int* xs, const void* yt, const int* ys, uint8_t* dst, long long dpitch, int ow,
                               int oh, hipStream_t s) {
  hipLaunchKernelGGL(gauge_resize, dim3((ow * oh + 255) / 256), dim3(256), 0, s, gray, gpitch, kind, isx, isy,
                     (const AreaTab*)xt, xs, (const AreaTab*)yt, ys, dst, dpitch, ow, oh);
  return hipGetLastError();
}

}  // namespace pc
