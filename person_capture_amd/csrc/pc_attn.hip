// Streaming attention for the OpenCLIP ViT family (gfx950): softmax(q k^T / sqrt(d)) v for every
// (image, head), open_clip ResidualAttentionBlock.attention, with the keys and values of a head
// passing through LDS in tiles of 64 keys, so the token count is bounded by the grid alone
// (pc_ops.hip mha_tokens keeps all keys of a head resident: head dim 64, T <= 272).
// Head dims 64 and 80 (ViT-H/14). Two forms, DESIGN.md §3.10:
//  * mha_stream   f32-class: f32 nets and the f16x3 split rows of an f16 net. The arithmetic
//                 contract of mha_tokens<float> / <float, SP>: q.k in f32, online softmax in
//                 f32, split rows read as hi + lo and written hi = f16(v), lo = f16(v - hi).
//                 One query per lane, the four waves share each tile's keys (16 each).
//  * mha_mfma     plain f16 nets: S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16 with
//                 f32 accumulation, f32 softmax statistics, P rounded to f16 once before PV.
//                 16 queries per wave; the query sits on the lane (lane & 15) in both products,
//                 so the softmax state needs no LDS and P goes from the accumulator of the first
//                 product into the operand of the second in registers.
#include "pc_common.h"

#include <type_traits>

namespace pc {

struct AttnParams {   // (pc_ops.hip)
  const void* qkv; int qcs;   // [N][T][qcs]: q at 0, k at E, v at 2E (E = heads*head_dim)
  void* out; int ocs;         // [N][T][ocs]
  int N, T, heads;
  float scale;                // 1/sqrt(head_dim)
  int qlo, olo;               // f16x3 split rows (both or neither): the lo halves at +qlo / +olo elements (0: plain)
};

constexpr int SA_Q = 64;        // queries per workgroup
constexpr int SA_WAVES = 4;
constexpr int SA_KT = 64;       // keys per LDS tile
constexpr int SA_WKEYS = SA_KT / SA_WAVES;   // keys of a tile per wave (mha_stream)
constexpr int SA_CHUNK = 8;     // keys scored per online-softmax update (mha_stream)

// ---------------------------------------------------------------------------
// f32-class form. LDS: the K and V tile as f32 (2 x 64 x D x 4 B), reused for the final combine
// of the four waves' partial states in two rounds of two slots (2 x 64 x (D + 2) x 4 B):
// 33,792 B at D = 64 and 41,984 B at D = 80, so three workgroups fit a CU's 160 KB at D = 80.
// ---------------------------------------------------------------------------
template <bool SP, int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void mha_stream(AttnParams p) {
  using S = typename std::conditional<SP, f16, float>::type;   // storage type of qkv / out
  constexpr int KV_BYTES = 2 * SA_KT * D * 4;
  constexpr int CMB_BYTES = 2 * SA_Q * (D + 2) * 4;
  constexpr int SMEM = KV_BYTES > CMB_BYTES ? KV_BYTES : CMB_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  float* Ks = reinterpret_cast<float*>(smem);
  float* Vs = Ks + SA_KT * D;
  const int nqb = (p.T + SA_Q - 1) / SA_Q;
  const int qb = blockIdx.x % nqb;
  const int h = (blockIdx.x / nqb) % p.heads;
  const int n = blockIdx.x / (nqb * p.heads);
  const int E = p.heads * D;
  const S* base = reinterpret_cast<const S*>(p.qkv) + (long long)n * p.T * p.qcs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = qb * SA_Q + lane;
  const bool qok = qi < p.T;
  float q[D];
  {
    const S* qr = base + (long long)(qok ? qi : 0) * p.qcs + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      if constexpr (SP) q[c] = ((float)qr[c] + (float)qr[p.qlo + c]) * p.scale;
      else q[c] = (float)qr[c] * p.scale;
    }
  }
  float m = -INFINITY, l = 0.f;
  float acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
  constexpr int VE = 16 / sizeof(S);
  for (int k0 = 0; k0 < p.T; k0 += SA_KT) {
    const int kn = min(SA_KT, p.T - k0);
    __syncthreads();   // the previous tile is no longer read
    for (int i = threadIdx.x; i < kn * (D / VE); i += blockDim.x) {
      const int t = i / (D / VE), c = (i % (D / VE)) * VE;
      const S* row = base + (long long)(k0 + t) * p.qcs + h * D + c;
      if constexpr (SP) {
        const f16x8 kh = *reinterpret_cast<const f16x8*>(row + E), kl = *reinterpret_cast<const f16x8*>(row + E + p.qlo);
        const f16x8 vh = *reinterpret_cast<const f16x8*>(row + 2 * E), vl = *reinterpret_cast<const f16x8*>(row + 2 * E + p.qlo);
#pragma unroll
        for (int j = 0; j < 8; j += 4) {
          f32x4 kf, vf;
#pragma unroll
          for (int u = 0; u < 4; ++u) { kf[u] = (float)kh[j + u] + (float)kl[j + u]; vf[u] = (float)vh[j + u] + (float)vl[j + u]; }
          *reinterpret_cast<f32x4*>(Ks + t * D + c + j) = kf;
          *reinterpret_cast<f32x4*>(Vs + t * D + c + j) = vf;
        }
      } else {
        *reinterpret_cast<f32x4*>(Ks + t * D + c) = *reinterpret_cast<const f32x4*>(row + E);
        *reinterpret_cast<f32x4*>(Vs + t * D + c) = *reinterpret_cast<const f32x4*>(row + 2 * E);
      }
    }
    __syncthreads();
    // this wave's keys of the tile (every lane reads the same K / V row: LDS broadcast)
    const int t1 = min(kn, (wave + 1) * SA_WKEYS);
    for (int t0 = wave * SA_WKEYS; t0 < t1; t0 += SA_CHUNK) {
      float sc[SA_CHUNK];
      float cm = -INFINITY;
#pragma unroll
      for (int j = 0; j < SA_CHUNK; ++j) {
        const int t = t0 + j;
        float sdot = -INFINITY;
        if (t < t1) {
          const float* kr = Ks + t * D;
          sdot = 0.f;
#pragma unroll
          for (int c = 0; c < D; ++c) sdot += q[c] * kr[c];
        }
        sc[j] = sdot;
        cm = fmaxf(cm, sdot);
      }
      const float mn = fmaxf(m, cm);
      const float corr = __expf(m - mn);   // m = -inf on the first chunk: corr = 0
      l *= corr;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] *= corr;
#pragma unroll
      for (int j = 0; j < SA_CHUNK; ++j) {
        const int t = t0 + j;
        if (t < t1) {
          const float e = __expf(sc[j] - mn);
          l += e;
          const float* vr = Vs + t * D;
#pragma unroll
          for (int c = 0; c < D; ++c) acc[c] += e * vr[c];
        }
      }
      m = mn;
    }
  }
  __syncthreads();   // K/V no longer read: reuse the LDS for the combine
  float* cmb = reinterpret_cast<float*>(smem);   // [slot][query][D + 2]
  // round 1: waves 2 and 3 hand their state to waves 0 and 1
  if (wave >= 2) {
    float* r = cmb + ((wave - 2) * SA_Q + lane) * (D + 2);
    r[0] = m;
    r[1] = l;
#pragma unroll
    for (int c = 0; c < D; ++c) r[2 + c] = acc[c];
  }
  __syncthreads();
  if (wave < 2) {   // merge, and leave the merged state in the same slot (this lane's own row)
    float* r = cmb + (wave * SA_Q + lane) * (D + 2);
    const float m2 = r[0];
    const float M = fmaxf(m, m2);
    const float f1 = m == -INFINITY ? 0.f : __expf(m - M);
    const float f2 = m2 == -INFINITY ? 0.f : __expf(m2 - M);
    r[0] = M;
    r[1] = l * f1 + r[1] * f2;
#pragma unroll
    for (int c = 0; c < D; ++c) r[2 + c] = acc[c] * f1 + r[2 + c] * f2;
  }
  __syncthreads();
  if (!qok) return;
  // round 2: wave w finishes dims [w D/4, (w + 1) D/4) of every query of the block from the two slots
  float mw[2], M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    mw[w] = cmb[(w * SA_Q + lane) * (D + 2)];
    M = fmaxf(M, mw[w]);
  }
  float L = 0.f, f[2];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    f[w] = mw[w] == -INFINITY ? 0.f : __expf(mw[w] - M);
    L += cmb[(w * SA_Q + lane) * (D + 2) + 1] * f[w];
  }
  const float inv = 1.0f / L;
  S* orow = reinterpret_cast<S*>(p.out) + ((long long)n * p.T + qi) * p.ocs + h * D;
  constexpr int DW = D / SA_WAVES;   // 16 / 20
  f16x4 oh[DW / 4], ol[DW / 4];
#pragma unroll
  for (int c = 0; c < DW; ++c) {
    const int d = wave * DW + c;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 2; ++w) v += cmb[(w * SA_Q + lane) * (D + 2) + 2 + d] * f[w];
    if constexpr (SP) {
      const float r = v * inv;
      const f16 hi = (f16)r;
      oh[c / 4][c % 4] = hi;
      ol[c / 4][c % 4] = (f16)(r - (float)hi);
    } else {
      orow[d] = v * inv;
    }
  }
  if constexpr (SP) {
#pragma unroll
    for (int g = 0; g < DW / 4; ++g) {
      *reinterpret_cast<f16x4*>(orow + wave * DW + g * 4) = oh[g];
      *reinterpret_cast<f16x4*>(orow + p.olo + wave * DW + g * 4) = ol[g];
    }
  }
}

// ---------------------------------------------------------------------------
// f16 matrix-core form. Per wave 16 queries, per workgroup 64; a tile is 64 keys.
//   S^T[key][query] = K Q^T: A = K rows (lane l: key l & 15, dims 8 (l >> 4) .. +8 of the k-step's 32),
//     B = Q (the same lane map on the query), accumulator: query l & 15, keys 4 (l >> 4) + reg of the
//     16-key block. Head dim 80 runs three k-steps over dims padded to 96 with zeros in LDS and in Q.
//   O^T[dim][query] = V^T P^T: the sum runs over the 32 keys of a k-step in the order the lane holds
//     them after the first product, key(l, j) = 16 (j >> 2) + 4 (l >> 4) + (j & 3): B = the lane's own P of
//     two 16-key blocks, rounded to f16; A = two 8-byte reads of the transposed V tile at that key order.
//     Accumulator: query l & 15, dims 16 nb + 4 (l >> 4) + reg: the row statistics and the rescale of O
//     stay on the lane (two xor shuffles over l >> 4 per tile for the row maximum).
// LDS: K [64][D' + 8] f16 (144- / 208-byte rows: the 16 rows of a 16-byte fragment read start 36 / 52
// banks apart), V^T [D][64 + 8] f16 (36-dword rows: the 8-byte reads of 16 rows x 2 key groups of a
// 32-lane half cover 32 distinct even banks; the dword writes of a half walk consecutive banks).
// 18,432 B at D = 64, 24,832 B at D = 80.
// ---------------------------------------------------------------------------
typedef f16 f16x2 __attribute__((ext_vector_type(2)));

template <int D>
__global__ __launch_bounds__(256) void mha_mfma(AttnParams p) {
  constexpr int DP = (D + 31) / 32 * 32;   // 64 / 96
  constexpr int KS = DP / 32;              // k-steps of K Q^T
  constexpr int NB = D / 16;               // 16-dim blocks of O^T
  constexpr int KROW = DP + 8;
  constexpr int VROW = SA_KT + 8;
  __shared__ __attribute__((aligned(16))) f16 Ks[SA_KT * KROW];
  __shared__ __attribute__((aligned(16))) f16 Vt[D * VROW];
  const int nqb = (p.T + SA_Q - 1) / SA_Q;
  const int qb = blockIdx.x % nqb;
  const int h = (blockIdx.x / nqb) % p.heads;
  const int n = blockIdx.x / (nqb * p.heads);
  const int E = p.heads * D;
  const f16* base = reinterpret_cast<const f16*>(p.qkv) + (long long)n * p.T * p.qcs + h * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int qi = qb * SA_Q + wave * 16 + r;
  const bool qok = qi < p.T;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (DP > D)   // the dims D .. DP of every K row stay zero
    for (int i = threadIdx.x; i < SA_KT * (DP - D); i += blockDim.x) Ks[(i / (DP - D)) * KROW + D + i % (DP - D)] = (f16)0.f;
  f16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = 32 * ks + 8 * g;
    qf[ks] = (qok && d0 < D) ? *reinterpret_cast<const f16x8*>(base + (long long)qi * p.qcs + d0) : zero8;
  }
  float m = -INFINITY, l = 0.f;   // l: this lane's keys only, summed over the four key groups at the end
  f32x4 o[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.T; k0 += SA_KT) {
    const int kn = min(SA_KT, p.T - k0);
    __syncthreads();   // the previous tile is no longer read
    for (int i = threadIdx.x; i < SA_KT * (D / 8); i += blockDim.x) {
      const int t = i / (D / 8), c = (i % (D / 8)) * 8;
      f16x8 v = zero8;   // keys past T: zero rows (their scores are masked below)
      if (t < kn) v = *reinterpret_cast<const f16x8*>(base + (long long)(k0 + t) * p.qcs + E + c);
      *reinterpret_cast<f16x8*>(Ks + t * KROW + c) = v;
    }
    // V transposed: one item = two keys x 8 dims, written as 8 dwords [dim][key pair]
    for (int i = threadIdx.x; i < (SA_KT / 2) * (D / 8); i += blockDim.x) {
      const int t = (i & (SA_KT / 2 - 1)) * 2, c = (i / (SA_KT / 2)) * 8;
      f16x8 a = zero8, b = zero8;
      if (t < kn) a = *reinterpret_cast<const f16x8*>(base + (long long)(k0 + t) * p.qcs + 2 * E + c);
      if (t + 1 < kn) b = *reinterpret_cast<const f16x8*>(base + (long long)(k0 + t + 1) * p.qcs + 2 * E + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) *reinterpret_cast<f16x2*>(Vt + (c + u) * VROW + t) = f16x2{a[u], b[u]};
    }
    __syncthreads();
    f32x4 s[SA_KT / 16];
#pragma unroll
    for (int b = 0; b < SA_KT / 16; ++b) {
      s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(Ks + (16 * b + r) * KROW + 32 * ks + 8 * g);
        s[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[b], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int b = 0; b < SA_KT / 16; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = (16 * b + 4 * g + j < kn) ? s[b][j] * p.scale : -INFINITY;
        s[b][j] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);       // finite: every tile holds at least one key
    const float corr = __expf(m - mn);   // m = -inf on the first tile: corr = 0
    l *= corr;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o[nb] *= corr;
    f16x8 pf[SA_KT / 32];
#pragma unroll
    for (int b = 0; b < SA_KT / 16; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __expf(s[b][j] - mn);
        l += e;
        pf[b >> 1][(b & 1) * 4 + j] = (f16)e;
      }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int ks = 0; ks < SA_KT / 32; ++ks) {
        const f16* vr = Vt + (16 * nb + r) * VROW + 32 * ks + 4 * g;
        const f16x4 v0 = *reinterpret_cast<const f16x4*>(vr), v1 = *reinterpret_cast<const f16x4*>(vr + 16);
        const f16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        o[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[ks], o[nb], 0, 0, 0);
      }
    m = mn;
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!qok) return;
  const float inv = 1.0f / l;
  f16* orow = reinterpret_cast<f16*>(p.out) + ((long long)n * p.T + qi) * p.ocs + h * D + 4 * g;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const f16x4 w = {(f16)(o[nb][0] * inv), (f16)(o[nb][1] * inv), (f16)(o[nb][2] * inv), (f16)(o[nb][3] * inv)};
    *reinterpret_cast<f16x4*>(orow + 16 * nb) = w;
  }
}

template <int D>
static void stream_launch_d(int f32, bool sp, const AttnParams& p, dim3 grid, hipStream_t s) {
  if (sp) hipLaunchKernelGGL((mha_stream<true, D>), grid, dim3(64 * SA_WAVES), 0, s, p);
  else if (f32) hipLaunchKernelGGL((mha_stream<false, D>), grid, dim3(64 * SA_WAVES), 0, s, p);
  else hipLaunchKernelGGL(mha_mfma<D>, grid, dim3(64 * SA_WAVES), 0, s, p);
}

hipError_t attention_stream_launch(int f32, const AttnParams& p, int head_dim, hipStream_t s) {
  if ((head_dim != 64 && head_dim != 80) || p.T <= 0 || p.N <= 0 || p.qcs % 8 || p.ocs % 4 || p.heads <= 0)
    return hipErrorInvalidValue;
  const long long nqb = (p.T + SA_Q - 1) / SA_Q;
  if (nqb * p.N * p.heads > 0x7fffffffLL) return hipErrorInvalidValue;
  dim3 grid((unsigned)(p.N * p.heads * nqb));
  const bool sp = p.qlo != 0;
  const int E = p.heads * head_dim;
  if (3 * E > p.qcs || E > p.ocs) return hipErrorInvalidValue;
  if (sp != (p.olo != 0) || (sp && (f32 || p.qlo % 8 || p.olo % 8 || p.ocs % 8 || p.qlo < 3 * E || p.qlo + 3 * E > p.qcs ||
                                    p.olo < E || p.olo + E > p.ocs)))
    return hipErrorInvalidValue;
  if (head_dim == 64) stream_launch_d<64>(f32, sp, p, grid, s);
  else stream_launch_d<80>(f32, sp, p, grid, s);
  return hipGetLastError();
}

}  // namespace pc
