// OpenCLIP image preprocessing for ReIDEmbedder (gfx950).
//
// Restates the transform the reference applies per crop (reid_embedder.py:46-50:
// cv2.cvtColor(BGR2RGB) -> PIL.Image -> open_clip preprocess), i.e. [ext]
// open_clip_torch==3.2.0 image_transform(224, resize_mode='shortest', bicubic):
//   torchvision Resize(224) on a PIL image = Pillow Image.resize(BICUBIC): separable
//     two-pass resample, 22-bit fixed-point coefficients, u8 intermediate;
//   CenterCrop(224); ToTensor (/255); Normalize(OPENAI mean/std);
// and writes the ViT patch matrix directly: token 1 + (y/14)*16 + x/14, column
// ((y%14)*14 + x%14)*3 + c (the conv1 weight's [kh][kw][c] order), token 0 (class
// token slot) and the K padding 588..607 zero (ViT-L/14 at 224; side and patch are launch
// parameters, so the same kernels serve B/32, B/16, L/14-336 and H/14: ClipGeom).
// Coefficient tables are computed on the host exactly as Pillow's precompute_coeffs /
// normalize_coeffs_8bpc do (pc_host.cpp); both passes here are integer-exact, so the
// pixels equal Pillow's. Parity: tests/test_gpu_reid.py against PIL itself.
#include "pc_common.h"

#pragma clang fp contract(off)

namespace pc {

struct ClipPrepDesc {
  const uint8_t* src;     // BGR u8 crop (top-left), row_stride bytes per row
  int H, W, row_stride;
  int kh, kv;             // horizontal / vertical coefficient counts per output
  const int* hb;          // [side][2] (xmin, xcount) of the cropped output columns
  const int* hk;          // [side][kh] int32 Q22 weights
  const int* vb;          // [side][2] (ymin, ycount) of the cropped output rows, ymin relative to row0
  const int* vk;          // [side][kv]
  int row0, nrows;        // source rows the vertical pass reads: [row0, row0 + nrows)
  uint8_t* tmp;           // [nrows][side][3] horizontal-pass output
};

// Tower geometry: the square input side, the patch, grid = side / patch, tok = grid^2 + 1,
// K = 3 patch^2 and K padded to the conv K tile (224 / 14: 16, 257, 588, 608)
struct ClipGeom { int side, patch, grid, tok, K, kpad; };

__device__ __forceinline__ int clip8(int v) {
  v >>= 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// pass 1: rows [row0, row0+nrows) x the `side` cropped output columns
__global__ void clip_hpass(const ClipPrepDesc* __restrict__ descs, int side) {
  const ClipPrepDesc d = descs[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.nrows * side) return;
  const int r = i / side, x = i - (i / side) * side;
  const int xmin = d.hb[2 * x], xn = d.hb[2 * x + 1];
  const int* k = d.hk + x * d.kh;
  const uint8_t* row = d.src + (long long)(d.row0 + r) * d.row_stride;
  int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
  for (int j = 0; j < xn; ++j) {
    const uint8_t* px = row + (xmin + j) * 3;
    s0 += (int)px[0] * k[j];
    s1 += (int)px[1] * k[j];
    s2 += (int)px[2] * k[j];
  }
  uint8_t* o = d.tmp + (long long)i * 3;
  o[0] = (uint8_t)clip8(s0);
  o[1] = (uint8_t)clip8(s1);
  o[2] = (uint8_t)clip8(s2);
}

// pass 2: vertical resample + ToTensor + Normalize, scattered into the patch matrix.
// CENTRED (f16x3 tower, T = f16): rows of 2 x kpad, both halves the resampled u8 pixel minus 127.5
// (exact in f16); the normalisation is folded into the program (models_clip.compile_clip_vit).
template <typename T, bool CENTRED = false>
__global__ void clip_vpass_patch(const ClipPrepDesc* __restrict__ descs, T* __restrict__ out, ClipGeom g) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.tok * g.kpad) return;
  const int tok = i / g.kpad, kc = i - (i / g.kpad) * g.kpad;
  const int ROW = CENTRED ? 2 * g.kpad : g.kpad;
  T* o = out + ((long long)n * g.tok + tok) * ROW + kc;
  if (tok == 0 || kc >= g.K) {
    *o = (T)0.f;
    if constexpr (CENTRED) o[g.kpad] = (T)0.f;
    return;
  }
  const int pt = tok - 1, py = pt / g.grid, pxx = pt - (pt / g.grid) * g.grid;
  const int tap = kc / 3, c = kc - (kc / 3) * 3;   // c: RGB channel
  const int y = py * g.patch + tap / g.patch, x = pxx * g.patch + tap % g.patch;
  const ClipPrepDesc d = descs[n];
  const int ymin = d.vb[2 * y], yn = d.vb[2 * y + 1];
  const int* k = d.vk + y * d.kv;
  const int bc = 2 - c;   // BGR source channel
  int s = 1 << 21;
  for (int j = 0; j < yn; ++j) s += (int)d.tmp[((long long)(ymin + j) * g.side + x) * 3 + bc] * k[j];
  if constexpr (CENTRED) {
    o[0] = o[g.kpad] = (T)((float)clip8(s) - 127.5f);
    return;
  }
  const float v = (float)clip8(s) / 255.f;
  const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
  const float stdv = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
  *o = (T)((v - mean) / stdv);
}

// mode: 0 f16, 1 f32 (normalised [tok][kpad]), 2 centred f16 [tok][2 kpad]
hipError_t clip_prep_launch(int mode, const ClipPrepDesc* d_descs, int N, int max_rows, int side, int patch, void* out,
                            hipStream_t s) {
  if (side <= 0 || patch <= 0 || side % patch || N <= 0 || max_rows <= 0) return hipErrorInvalidValue;
  ClipGeom g;
  g.side = side; g.patch = patch; g.grid = side / patch; g.tok = g.grid * g.grid + 1;
  g.K = 3 * patch * patch; g.kpad = (g.K + 31) / 32 * 32;
  dim3 g1((max_rows * side + 255) / 256, N);
  hipLaunchKernelGGL(clip_hpass, g1, dim3(256), 0, s, d_descs, side);
  dim3 g2((g.tok * g.kpad + 255) / 256, N);
  if (mode == 2) hipLaunchKernelGGL((clip_vpass_patch<f16, true>), g2, dim3(256), 0, s, d_descs, (f16*)out, g);
  else if (mode == 1) hipLaunchKernelGGL(clip_vpass_patch<float>, g2, dim3(256), 0, s, d_descs, (float*)out, g);
  else hipLaunchKernelGGL(clip_vpass_patch<f16>, g2, dim3(256), 0, s, d_descs, (f16*)out, g);
  return hipGetLastError();
}

}  // namespace pc
