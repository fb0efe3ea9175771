// Dataset-curator kernels (gfx950): per-crop image metrics and the MMR diversity ranking.
//
// The reference scores every candidate crop on the CPU through OpenCV, one image at a time
// (dataset_curator.py:55-113 phash64 / sharpness_norm / exposure_score, utils.py:152-196
// detect_black_borders), and ranks every scene with a pure-Python greedy loop
// (dataset_curator.py:211-238 mmr_select_with_q over the Fs @ Fs.T of :961-977). Here the device
// produces exact integers (histogram, row / column sums, Laplacian sums, the resized planes) and
// two quantities with a derived bound (the 8x8 DCT block, F F^T); everything that decides
// something is computed from them on the host with the reference's expressions (curate.py,
// DESIGN.md §10).
//
//   curate_gray      BGR u8 -> 14-bit-coefficient gray plane (pc_image.hip face_quality's
//                    arithmetic), histogram, row sums, column sums; one workgroup per band of rows
//   curate_resize    gray plane -> the <= 256 plane and the 32x32 plane, cv2.resize INTER_AREA
//                    (pc_area.h: the three-channel kernels' arithmetic at one channel)
//   curate_laplace   ksize-1 Laplacian (BORDER_REFLECT_101) of the <= 256 plane: sum g, sum L,
//                    sum L^2 as integers
//   curate_dct       8x8 low-frequency block of the orthonormal 32x32 DCT-II, f64 accumulation
//                    from a host-supplied cosine table
//   sim_matrix       S = F F^T, f32, fixed summation order
//   mmr_order        the greedy loop, one workgroup
#include "pc_common.h"

#pragma clang fp contract(off)

#include "pc_area.h"
#include "pc_curate.h"
#include "pc_gray.h"

namespace pc {

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A workgroup is CURATE_BAND rows of one image. A thread owns a 16-pixel column chunk (48 source
// bytes: three 16-byte loads where the row is 16-byte aligned, byte loads otherwise and in the
// row's tail) and walks it down the band with the chunk's 16 column sums in registers. A row takes
// CW lanes (its chunks rounded up to whole waves, at most 256); a crop narrower than 2048 pixels
// leaves room for R = 256 / CW rows side by side (a 768-wide crop has 48 chunks: one row per wave,
// four rows in flight; with one row at a time 208 of the 256 threads idled and the pass ran at
// 0.11 of HBM), wider ones loop over groups of 256 chunks. A wave always holds one row, so its
// row sum is a wave reduction. The gray plane's pitch is a multiple of 16, so every chunk is one
// 16-byte store (the tail's padding bytes are written as 0). Histogram: one LDS copy per wave,
// flushed with integer atomics; the band owns its rows, so row sums are plain stores; column sums
// meet in the LDS when R > 1 and leave as one integer atomic per column and band. Integer atomics
// commute: the outputs do not depend on the order.
__global__ __launch_bounds__(256) void curate_gray(const CurateImg* __restrict__ imgs, const int2* __restrict__ bands) {
  __shared__ unsigned hist[4][256];
  __shared__ unsigned rowacc[CURATE_BAND];
  __shared__ unsigned colacc[128 * 16];   // R > 1 only: at most 128 chunks
  const int2 bd = bands[blockIdx.x];
  const CurateImg* d = imgs + bd.x;
  const uint8_t* src = d->src;
  const int w = d->w, h = d->h, gpitch = d->gpitch;
  const long long row_stride = d->row_stride;
  uint8_t* gray = d->gray;
  const int y0 = bd.y, y1 = min(y0 + CURATE_BAND, h);
  const int tid = threadIdx.x, wave = tid >> 6;
  const int nchunk = (w + 15) >> 4;
  const int CW = min(256, (nchunk + 63) & ~63);
  const int R = 256 / CW;                     // 4, 2 or 1 (CW = 192: one row, the last wave idles)
  const int cx = tid % CW, ry = tid / CW;     // (wave-uniform ry: CW is whole waves)
  for (int i = tid; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0u;
  if (tid < CURATE_BAND) rowacc[tid] = 0u;
  if (R > 1)
    for (int i = tid; i < 128 * 16; i += 256) colacc[i] = 0u;
  __syncthreads();
  for (int base = 0; base < nchunk; base += CW) {   // (one pass when R > 1)
    const int ch = base + cx;
    const bool live = ch < nchunk;
    const int x0 = ch << 4;
    const int nv = live ? min(16, w - x0) : 0;
    unsigned col[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) col[i] = 0u;
    for (int y = ry < R ? y0 + ry : y1; y < y1; y += R) {   // (wave-uniform trip count: the row sum shuffles)
      unsigned rs = 0u;
      if (live) {
        const uint8_t* p = src + (long long)y * row_stride + (long long)x0 * 3;
        union { uint4 v[3]; uint8_t b[48]; } in;
        if (nv == 16 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
          for (int k = 0; k < 3; ++k) in.v[k] = reinterpret_cast<const uint4*>(p)[k];
        } else {
#pragma unroll
          for (int k = 0; k < 48; ++k) in.b[k] = k < nv * 3 ? p[k] : (uint8_t)0;
        }
        union { uint4 v; uint8_t b[16]; } out;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int g = gray14(in.b[i * 3], in.b[i * 3 + 1], in.b[i * 3 + 2]);
          out.b[i] = (uint8_t)g;
          if (i < nv) {
            col[i] += (unsigned)g;
            rs += (unsigned)g;
            atomicAdd(&hist[wave][g], 1u);
          }
        }
        *reinterpret_cast<uint4*>(gray + (long long)y * gpitch + x0) = out.v;
      }
      rs = wave_sum_u32(rs);
      if ((tid & 63) == 0 && rs) atomicAdd(&rowacc[y - y0], rs);
    }
    if (R > 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < nv && col[i]) atomicAdd(&colacc[cx * 16 + i], col[i]);   // (base = 0: cx * 16 + i is the column)
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < nv) atomicAdd(d->col_sum + x0 + i, col[i]);
    }
  }
  __syncthreads();
  const unsigned hv = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
  if (hv) atomicAdd(d->hist + tid, hv);
  if (tid < y1 - y0) d->row_sum[y0 + tid] = rowacc[tid];
  if (R > 1)
    for (int i = tid; i < w; i += 256)
      if (colacc[i]) atomicAdd(d->col_sum + i, colacc[i]);
}

// One thread per output pixel of one target of one image (grid.y = 2 images).
__global__ __launch_bounds__(256) void curate_resize(const CurateImg* __restrict__ imgs, const AreaTab* __restrict__ tabs,
                                                     const int* __restrict__ starts) {
  const CurateImg* d = imgs + (blockIdx.y >> 1);
  const CurateTarget t = d->t[blockIdx.y & 1];
  if (t.kind == 0) return;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= t.ow * t.oh) return;
  const int dy = pix / t.ow, dx = pix - (pix / t.ow) * t.ow;
  uint8_t* o = t.dst + (long long)dy * t.pitch + dx;
  if (t.kind == 1) {
    area_fast_pixel<1>(d->gray, d->gpitch, t.isx, t.isy, dx, dy, o);
  } else {
    const int* xs = starts + t.xs;
    const int* ys = starts + t.ys;
    area_pixel<1>(d->gray, d->gpitch, tabs, xs[dx], xs[dx + 1], tabs, ys[dy], ys[dy + 1], o);
  }
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101) for p in [-1, len]; an axis of length 1 maps to 0
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  return p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p);
}

// One 1024-thread workgroup per image over its <= 256 x 256 plane (face_quality's reduction with
// integer results: |L| <= 1020, so sum L^2 < 2^36 and everything is exact in 64 bits).
__global__ __launch_bounds__(1024) void curate_laplace(const CurateImg* __restrict__ imgs) {
  __shared__ long long red[3][16];
  const CurateImg* d = imgs + blockIdx.x;
  const CurateTarget t = d->t[0];
  const uint8_t* g = t.dst;
  const int w = t.ow, h = t.oh, n = w * h;
  const long long pitch = t.pitch;
  long long s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int y = i / w, x = i - (i / w) * w;
    const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h);
    const int c = g[y * pitch + x];
    const int l = (int)g[y * pitch + xm] + (int)g[y * pitch + xp] + (int)g[ym * pitch + x] + (int)g[yp * pitch + x] - 4 * c;
    s0 += c;
    s1 += l;
    s2 += (long long)l * l;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wv] = s0; red[1][wv] = s1; red[2][wv] = s2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    long long tsum = 0;
    for (int k = 0; k < 16; ++k) tsum += red[threadIdx.x][k];
    d->sums[threadIdx.x] = (unsigned long long)tsum;
  } else if (threadIdx.x == 64) {
    d->wh[0] = w;
    d->wh[1] = h;
  }
}

// block = C X C^T for the 8 lowest frequencies: dct[u][x] = c_u cos(pi (2 x + 1) u / 64) comes from
// the host in f64 (the device's cos is not used). tmp[u][x] = sum_y dct[u][y] X[y][x], y ascending;
// out[u][v] = sum_x tmp[u][x] dct[v][x], x ascending; all in f64, unfused, rounded once to f32.
__global__ __launch_bounds__(256) void curate_dct(const CurateImg* __restrict__ imgs, const double* __restrict__ dct) {
  __shared__ double C[8][32];
  __shared__ double tmp[8][32];
  __shared__ uint8_t X[32][32];
  const CurateImg* d = imgs + blockIdx.x;
  const CurateTarget t = d->t[1];
  const int tid = threadIdx.x;
  C[tid >> 5][tid & 31] = dct[tid];
  for (int i = tid; i < 1024; i += 256) X[i >> 5][i & 31] = t.dst[(long long)(i >> 5) * t.pitch + (i & 31)];
  __syncthreads();
  {
    const int u = tid >> 5, x = tid & 31;
    double a = 0.0;
    for (int y = 0; y < 32; ++y) a += C[u][y] * (double)X[y][x];
    tmp[u][x] = a;
  }
  __syncthreads();
  if (tid < 64) {
    const int u = tid >> 3, v = tid & 7;
    double a = 0.0;
    for (int x = 0; x < 32; ++x) a += tmp[u][x] * C[v][x];
    d->coef[tid] = (float)a;
  }
}

// ---------------------------------------------------------------------------
// S = F F^T (dataset_curator.py:971-973), f32. A workgroup is a 64 x 64 tile of S, a thread a
// 4 x 4 block of it; K goes through the LDS 16 columns at a time. Every element is one fmaf chain
// from +0 over k = 0 .. dim - 1 ascending (then the zero padding of the last K tile, which adds
// +0): acc = fmaf(F[i][k], F[j][k], acc). The product commutes, so S[i][j] and S[j][i] are the
// same chain and come out bit-equal; nothing depends on the schedule, so two runs give the same
// bytes. (No MFMA: the f32 MFMA sums four-wide partial products in an order of its own.)
// ---------------------------------------------------------------------------
constexpr int SIM_T = 64, SIM_K = 16;

__global__ __launch_bounds__(256) void sim_matrix(const float* __restrict__ F, int n, int dim, float* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) float As[SIM_K][SIM_T + 4];
  __shared__ __attribute__((aligned(16))) float Bs[SIM_K][SIM_T + 4];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * SIM_T, j0 = blockIdx.x * SIM_T;
  const int lr = tid >> 2, lk = (tid & 3) * 4;   // staging: row lr of the tile, 4 consecutive k
  const int ty = tid >> 4, tx = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < dim; k0 += SIM_K) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + lk + q;
      const bool kin = k < dim;
      As[lk + q][lr] = (kin && i0 + lr < n) ? F[(long long)(i0 + lr) * dim + k] : 0.f;
      Bs[lk + q][lr] = (kin && j0 + lr < n) ? F[(long long)(j0 + lr) * dim + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SIM_K; ++k) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[k][ty * 4]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[k][tx * 4]);
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(a[p], b[q], acc[p][q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + ty * 4 + p;
    if (i >= n) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx * 4 + q;
      if (j < n) S[(long long)i * n + j] = acc[p][q];
    }
  }
}

// ---------------------------------------------------------------------------
// Greedy MMR (dataset_curator.py:211-238). One workgroup of 1024 threads; thread t owns the items
// t, t + 1024, ... (n <= 8192: at most 8), their q, their running redundancy
// red_i = max(0, max over picked j of S[i][j]) and whether they are picked. A step scores the
// unpicked items, score_i = alpha (double)q_i - (1 - alpha) (double)red_i (unfused f64, the
// reference's Python arithmetic), takes the greatest score with the lowest index on ties (wave
// shuffles, then 16 LDS slots that every thread scans), and folds row `winner` of S into red:
// a coalesced row read, equal to the column by symmetry. One barrier per step (the LDS slots
// alternate); no grid-wide synchronisation anywhere.
// ---------------------------------------------------------------------------
constexpr int MMR_T = 1024, MMR_E = 8;

__global__ __launch_bounds__(MMR_T) void mmr_order(const float* __restrict__ S, const float* __restrict__ q, int n, int k,
                                                   double alpha, int* __restrict__ order) {
  __shared__ double sbest[2][16];
  __shared__ int sidx[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double qa[MMR_E];
  float red[MMR_E];
  bool open[MMR_E];
#pragma unroll
  for (int e = 0; e < MMR_E; ++e) {
    const int i = tid + e * MMR_T;
    open[e] = i < n;
    qa[e] = open[e] ? alpha * (double)q[i] : 0.0;
    red[e] = 0.f;
  }
  const double beta = 1.0 - alpha;
  const double NEG = -__builtin_huge_val();
  for (int step = 0; step < k; ++step) {
    double best = NEG;
    int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < MMR_E; ++e) {
      if (open[e]) {
        const double s = qa[e] - beta * (double)red[e];
        if (s > best || bi == 0x7fffffff) { best = s; bi = tid + e * MMR_T; }   // (e ascending: a tie keeps the lower index)
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    const int buf = step & 1;
    if (lane == 0) { sbest[buf][wave] = best; sidx[buf][wave] = bi; }
    __syncthreads();
    best = sbest[buf][0];
    bi = sidx[buf][0];
#pragma unroll
    for (int v = 1; v < 16; ++v) {
      const double ob = sbest[buf][v];
      const int oi = sidx[buf][v];
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) break;   // (k <= n: never; uniform over the workgroup)
    if (tid == 0) order[step] = bi;
    const float* row = S + (long long)bi * n;
#pragma unroll
    for (int e = 0; e < MMR_E; ++e) {
      const int i = tid + e * MMR_T;
      if (i == bi) open[e] = false;
      if (open[e]) red[e] = fmaxf(red[e], row[i]);
    }
  }
}

// ---------------------------------------------------------------------------
hipError_t curate_metrics_launch(const void* d_imgs, int n, const void* d_bands, int nbands, const void* d_tabs,
                                 const int* d_starts, const double* d_dct, int max_pixels, hipStream_t s) {
  const CurateImg* imgs = (const CurateImg*)d_imgs;
  hipLaunchKernelGGL(curate_gray, dim3(nbands), dim3(256), 0, s, imgs, (const int2*)d_bands);
  hipLaunchKernelGGL(curate_resize, dim3((max_pixels + 255) / 256, 2 * n), dim3(256), 0, s, imgs, (const AreaTab*)d_tabs,
                     d_starts);
  hipLaunchKernelGGL(curate_laplace, dim3(n), dim3(1024), 0, s, imgs);
  hipLaunchKernelGGL(curate_dct, dim3(n), dim3(256), 0, s, imgs, d_dct);
  return hipGetLastError();
}

hipError_t sim_matrix_launch(const float* F, int n, int dim, float* S, hipStream_t s) {
  const int g = (n + SIM_T - 1) / SIM_T;
  hipLaunchKernelGGL(sim_matrix, dim3(g, g), dim3(256), 0, s, F, n, dim, S);
  return hipGetLastError();
}

hipError_t mmr_order_launch(const float* S, const float* q, int n, int k, double alpha, int* order, hipStream_t s) {
  if (n > MMR_T * MMR_E || k > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mmr_order, dim3(1), dim3(MMR_T), 0, s, S, q, n, k, alpha, order);
  return hipGetLastError();
}

}  // namespace pc
