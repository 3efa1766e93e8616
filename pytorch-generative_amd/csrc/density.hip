// density.hip — KDE and the Gaussian / Bernoulli mixture models (reference models/kde.py, models/mixture_models.py) on
// streaming log-density kernels.
//
// All three are a pairwise log-density matrix c[n][k] = sum_d f(x[n][d], theta[k][d]) reduced by logsumexp over k.
// Expanded, c is one or two GEMMs plus a per-column constant (X: (N, F), parameters (K, F)):
//   Bernoulli mixture  c = X L^T + colc,                         colc[k] = log pi_k - sum_d softplus(L[k][d])
//   Gaussian mixture   c = X B1^T + X^2 B2^T + colc,             B1 = mu / sigma^2, B2 = -1 / (2 sigma^2),
//                                                                colc[k] = log pi_k - sum_d (log sigma + mu^2 / (2 sigma^2)) - F/2 log 2 pi
//   Gaussian KDE       c = alpha X Y^T + colc (+ rowc[n] at the end), alpha = 1 / h^2, colc[k] = -alpha/2 |y_k|^2 - Z,
//                                                                rowc[n] = -alpha/2 |x_n|^2
// Nothing of size N x K leaves the chip: a workgroup owns 64 rows, walks 32-column tiles (the GEMM tile of
// masked_linear.hip: 4 waves, v_mfma_f32_16x16x4_f32, k in chunks of 64 through LDS with the next chunk prefetched into
// registers) and every lane keeps a running (max, sum) for the 4 rows x 2 columns it holds of each tile; the 16 lanes
// of a row merge once at the end. When there are few row tiles (KDE: small N, large K) the column tiles are split across
// workgroups; each writes its (max, sum) pair per row to a workspace and dn_merge_kernel merges them in split order.
//
// Accuracy: each k chunk is accumulated from zero and added to a running total (the two GEMMs of the Gaussian mixture
// separately), so the rounding error of a sum of F terms of size |c| / F grows with the number of chunks, not of terms.
// The mixtures' operands are centred on component 0 (B - B_0, colc - colc_0): the kernels see c' = c - log p_0(x_n),
// whose size is the DIFFERENCE between components, and log p_0(x_n) is added to the result from its direct form. The
// responsibilities exp(c' - lse') then carry the rounding of |c'|, not of |c| (hundreds at F = 784), and the forward
// keeps the pair (m, s) of lse' = m + log s so that the backward forms exp(c' - m) / s without the rounding of lse'.
//
// Mixture backward: from X, the saved (m, s) and the upstream g, w[n][k] = g[n] exp(c'[n][k] - m[n]) / s[n] is
// recomputed per 64 x 32 tile into LDS, and a workgroup (32 components x 256 features x a range of rows) accumulates on the VALU
//   Bernoulli  P1[k][d] = sum_n w x                      Gaussian  P1 = sum_n w (x - mu),  P2 = sum_n w (x - mu)^2
// (the centred forms: the expanded sum w x^2 - 2 mu sum w x + mu^2 sum w cancels), plus S[k] = sum_n w. Row ranges
// write partial sums to the workspace; dn_finish_kernel adds them in range order and applies
//   dL = P1 - sigmoid(L) S;   dmu = P1 / sigma^2;   dlog_std = P2 / sigma^2 - S;   dlogits = S - pi sum_k S.
// No atomics anywhere: bit-reproducible. Ragged edges are zero-filled on load and guarded on store.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int DN_BM = 64;            // rows per workgroup
constexpr int DN_BN = 32;            // columns per tile
constexpr int DN_KC = 64;            // features per LDS chunk
constexpr int DN_LD = DN_KC + 4;     // LDS row stride (floats): conflict-free MFMA operand reads
constexpr int DN_THREADS = 256;
constexpr int DN_A_PER = DN_BM * DN_KC / DN_THREADS;  // 16
constexpr int DN_B_PER = DN_BN * DN_KC / DN_THREADS;  // 8
constexpr int DN_DT = 256;           // backward: features per workgroup (one per thread)
constexpr int DN_WLD = DN_BN + 4;    // backward: LDS row stride of the w tile (float4 reads along k)
constexpr int DN_MAX_SPLITS = 64;    // forward column splits
constexpr int DN_MAX_NSPLITS = 16;   // backward row ranges
constexpr int DN_MAX_TILES = 65535;  // gridDim.y / .z

using pg_tile::f32x4;

enum { DN_BERNOULLI = PG_MIXTURE_BERNOULLI, DN_GAUSSIAN = PG_MIXTURE_GAUSSIAN };

struct DnOps {
  const float* x;     // (N, F)
  const float* b1;    // (K, F)
  const float* b2;    // (K, F) or NULL: multiplies x^2
  const float* colc;  // (K)
  float alpha;        // scales the b1 product
  int N, K, F;
};

// tot[t][q] = alpha sum_d x[r][d] b1[c][d] + sum_d x[r][d]^2 b2[c][d] for r = r0 + 16 wave + 4 (lane >> 4) + q,
// c = c0 + 16 t + (lane & 15); rows >= N and columns >= K read zeros. All 256 threads must call it.
template <bool TWO>
__device__ __forceinline__ void dn_tile(const DnOps& p, int r0, int c0, float* s_a, float* s_b1, float* s_b2,
                                        f32x4 (&tot)[2]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  float ra[DN_A_PER], rb1[DN_B_PER], rb2[TWO ? DN_B_PER : 1];
  auto load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < DN_A_PER; ++j) {
      const int e = tid + j * DN_THREADS, r = e / DN_KC, k = e % DN_KC;
      const int gr = r0 + r, gk = k0 + k;
      ra[j] = (gr < p.N && gk < p.F) ? p.x[(size_t)gr * p.F + gk] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < DN_B_PER; ++j) {
      const int e = tid + j * DN_THREADS, c = e / DN_KC, k = e % DN_KC;
      const int gc = c0 + c, gk = k0 + k;
      const bool ok = gc < p.K && gk < p.F;
      rb1[j] = ok ? p.b1[(size_t)gc * p.F + gk] : 0.f;
      if (TWO) rb2[j] = ok ? p.b2[(size_t)gc * p.F + gk] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < DN_A_PER; ++j) {
      const int e = tid + j * DN_THREADS;
      s_a[(e / DN_KC) * DN_LD + e % DN_KC] = ra[j];
    }
#pragma unroll
    for (int j = 0; j < DN_B_PER; ++j) {
      const int e = tid + j * DN_THREADS;
      s_b1[(e / DN_KC) * DN_LD + e % DN_KC] = rb1[j];
      if (TWO) s_b2[(e / DN_KC) * DN_LD + e % DN_KC] = rb2[j];
    }
  };
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 t1[2] = {zero, zero}, t2[2] = {zero, zero};
  const int nch = (p.F + DN_KC - 1) / DN_KC;
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
    store();
    __syncthreads();
    if (ch + 1 < nch) load((ch + 1) * DN_KC);  // in flight while this chunk is multiplied
    const float* ap = s_a + (wave * 16 + lr) * DN_LD + lk;
    const int b0 = lr * DN_LD + lk, b1o = (16 + lr) * DN_LD + lk;
    f32x4 a0 = zero, a1 = zero, q0 = zero, q1 = zero;  // this chunk alone: summed from zero
#pragma unroll
    for (int kk = 0; kk < DN_KC; kk += 4) {
      const float av = ap[kk];
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_b1[b0 + kk], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_b1[b1o + kk], a1, 0, 0, 0);
      if (TWO) {
        const float av2 = av * av;
        q0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av2, s_b2[b0 + kk], q0, 0, 0, 0);
        q1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av2, s_b2[b1o + kk], q1, 0, 0, 0);
      }
    }
    t1[0] += a0;
    t1[1] += a1;
    if (TWO) {
      t2[0] += q0;
      t2[1] += q1;
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) tot[t][q] = TWO ? fmaf(p.alpha, t1[t][q], t2[t][q]) : p.alpha * t1[t][q];
}

// online logsumexp state: (m, s) stands for m + log s; (-inf, 0) is the empty sum
__device__ __forceinline__ void dn_lse_push(float& m, float& s, float v) {
  const float mn = fmaxf(m, v);
  if (mn > -INFINITY) {  // v = m = -inf: nothing to add (and no exp(-inf + inf))
    s = s * expf(m - mn) + expf(v - mn);
    m = mn;
  }
}
__device__ __forceinline__ void dn_lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn > -INFINITY) {
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
  }
}
__device__ __forceinline__ float dn_lse_value(float m, float s) { return s > 0.f ? m + logf(s) : -INFINITY; }

// Forward: out[n] (+)= logsumexp_k c[n][k]. grid (splits, row tiles); split z walks column tiles [z * tper, (z + 1) * tper).
// part != NULL: the (m, s) pair of (split, row) goes to part[(z * N + n) * 2] instead.
// stats != NULL: the merged pair of row n is also kept at stats[2 n] (the mixtures' backward reads it).
template <bool TWO>
__global__ void __launch_bounds__(DN_THREADS) dn_lse_kernel(const DnOps p, float* __restrict__ out, int add_out,
                                                            float* __restrict__ part, float* __restrict__ stats,
                                                            int tper) {
  __shared__ float s_a[DN_BM * DN_LD];
  __shared__ float s_b1[DN_BN * DN_LD];
  __shared__ float s_b2[TWO ? DN_BN * DN_LD : 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int r0 = blockIdx.y * DN_BM;
  const int ntiles = (p.K + DN_BN - 1) / DN_BN;
  const int tbeg = blockIdx.x * tper, tend = min(ntiles, tbeg + tper);
  float m[4], s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] = -INFINITY, s[q] = 0.f;
  for (int tile = tbeg; tile < tend; ++tile) {
    const int c0 = tile * DN_BN;
    f32x4 tot[2];
    dn_tile<TWO>(p, r0, c0, s_a, s_b1, s_b2, tot);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int gc = c0 + t * 16 + lr;
      if (gc >= p.K) continue;
      const float cc = p.colc[gc];
#pragma unroll
      for (int q = 0; q < 4; ++q) dn_lse_push(m[q], s[q], tot[t][q] + cc);
    }
  }
  // the 16 lanes of a row (same lane >> 4) merge
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float m2 = __shfl_xor(m[q], off, 64), s2 = __shfl_xor(s[q], off, 64);
      dn_lse_merge(m[q], s[q], m2, s2);
    }
  }
  if (lr == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gr = r0 + wave * 16 + lk * 4 + q;
      if (gr >= p.N) continue;
      if (part) {
        part[((size_t)blockIdx.x * p.N + gr) * 2] = m[q];
        part[((size_t)blockIdx.x * p.N + gr) * 2 + 1] = s[q];
      } else {
        const float v = dn_lse_value(m[q], s[q]);
        out[gr] = add_out ? out[gr] + v : v;
        if (stats) stats[(size_t)gr * 2] = m[q], stats[(size_t)gr * 2 + 1] = s[q];
      }
    }
  }
}

__global__ void __launch_bounds__(256) dn_merge_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                       int add_out, float* __restrict__ stats, int N, int splits) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float m = -INFINITY, s = 0.f;
  for (int z = 0; z < splits; ++z) dn_lse_merge(m, s, part[((size_t)z * N + n) * 2], part[((size_t)z * N + n) * 2 + 1]);
  const float v = dn_lse_value(m, s);
  out[n] = add_out ? out[n] + v : v;
  if (stats) stats[(size_t)n * 2] = m, stats[(size_t)n * 2 + 1] = s;
}

// 256-thread block reductions (fixed tree: deterministic)
__device__ __forceinline__ float dn_block_sum(float v, float* s_red) {
  v = pg_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
__device__ __forceinline__ float dn_block_max(float v, float* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// logpi = log_softmax(logits) (one workgroup). All logits -inf: every logpi is -inf (torch gives NaN).
__global__ void __launch_bounds__(256) dn_log_softmax_kernel(const float* __restrict__ logits, float* __restrict__ logpi,
                                                             int K) {
  __shared__ float s_red[4];
  float mx = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) mx = fmaxf(mx, logits[k]);
  mx = dn_block_max(mx, s_red);
  float sum = 0.f;
  if (mx > -INFINITY)
    for (int k = threadIdx.x; k < K; k += 256) sum += expf(logits[k] - mx);
  sum = dn_block_sum(sum, s_red);
  const float lz = mx > -INFINITY ? mx + logf(sum) : 0.f;
  for (int k = threadIdx.x; k < K; k += 256) logpi[k] = logits[k] - lz;
}

__device__ __forceinline__ float dn_softplus(float l) { return fmaxf(l, 0.f) + log1pf(expf(-fabsf(l))); }

// One wave per component: the operand transforms of the mixtures (see the file header), CENTRED on component 0:
// b1, b2 and colc hold the difference to component 0's, so that c'[n][k] = c[n][k] - log p_0(x_n) is accumulated at the
// size of the differences between components, not of the log-densities themselves.
template <int KIND>
__global__ void __launch_bounds__(256) dn_mixture_prep_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                              const float* __restrict__ logpi, float* __restrict__ b1,
                                                              float* __restrict__ b2, float* __restrict__ colc, int K,
                                                              int F) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  float sum = 0.f;
  for (int d = lane; d < F; d += 64) {
    const size_t e = (size_t)k * F + d;
    if (KIND == DN_BERNOULLI) {
      const float l = p1[e], l0 = p1[d];
      b1[e] = l - l0;
      sum += dn_softplus(l) - dn_softplus(l0);
    } else {
      const float mu = p1[e], ls = p2[e], iv = expf(-2.f * ls);
      const float mu0 = p1[d], ls0 = p2[d], iv0 = expf(-2.f * ls0);
      b1[e] = mu * iv - mu0 * iv0;
      b2[e] = -0.5f * (iv - iv0);
      sum += (ls - ls0) + 0.5f * (mu * mu * iv - mu0 * mu0 * iv0);
    }
  }
  sum = pg_wave_sum(sum);
  if (lane == 0) colc[k] = logpi[k] - sum;
}

// out[n] = log p_0(x_n), the log-density of component 0 in its direct (not expanded) form (one wave per row)
template <int KIND>
__global__ void __launch_bounds__(256) dn_row_ref_kernel(const float* __restrict__ x, const float* __restrict__ p1,
                                                         const float* __restrict__ p2, float* __restrict__ out, int N,
                                                         int F) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float sum = 0.f;
  for (int d = lane; d < F; d += 64) {
    const float xv = x[(size_t)n * F + d];
    if (KIND == DN_BERNOULLI) {
      const float l = p1[d];
      sum += xv * l - dn_softplus(l);
    } else {
      const float ls = p2[d], z = (xv - p1[d]) * expf(-ls);
      sum += -ls - 0.5f * 1.8378770664093453f - 0.5f * z * z;
    }
  }
  sum = pg_wave_sum(sum);
  if (lane == 0) out[n] = sum;
}

// dst[r] = scale |src[r]|^2 + shift (one wave per row): KDE's per-column and per-row terms
__global__ void __launch_bounds__(256) dn_sqnorm_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                        float scale, float shift, int R, int F) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  float sum = 0.f;
  for (int d = lane; d < F; d += 64) {
    const float v = src[(size_t)r * F + d];
    sum = fmaf(v, v, sum);
  }
  sum = pg_wave_sum(sum);
  if (lane == 0) dst[r] = fmaf(scale, sum, shift);
}

// Backward partial sums. grid (feature tiles of 256, component tiles of 32, row ranges of `rper` rows).
template <int KIND>
__global__ void __launch_bounds__(DN_THREADS) dn_bwd_kernel(const DnOps p, const float* __restrict__ mean,
                                                            const float* __restrict__ stats, const float* __restrict__ g,
                                                            float* __restrict__ part1, float* __restrict__ part2,
                                                            float* __restrict__ part_s, int rper) {
  constexpr bool TWO = KIND == DN_GAUSSIAN;
  __shared__ float s_a[DN_BM * DN_LD];
  __shared__ float s_b1[DN_BN * DN_LD];
  __shared__ float s_b2[TWO ? DN_BN * DN_LD : 1];
  __shared__ __attribute__((aligned(16))) float s_w[DN_BM * DN_WLD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int d = blockIdx.x * DN_DT + tid;
  const bool dok = d < p.F;
  const int c0 = blockIdx.y * DN_BN;
  const int nbeg = blockIdx.z * rper, nend = min(p.N, nbeg + rper);
  float acc1[DN_BN], acc2[TWO ? DN_BN : 1], mu[TWO ? DN_BN : 1];
#pragma unroll
  for (int k = 0; k < DN_BN; ++k) {
    acc1[k] = 0.f;
    if (TWO) {
      acc2[k] = 0.f;
      mu[k] = (dok && c0 + k < p.K) ? mean[(size_t)(c0 + k) * p.F + d] : 0.f;
    }
  }
  float ssum = 0.f;  // S[c0 + tid] of this row range (tid < 32, feature tile 0)
  for (int r0 = nbeg; r0 < nend; r0 += DN_BM) {
    f32x4 tot[2];
    dn_tile<TWO>(p, r0, c0, s_a, s_b1, s_b2, tot);  // ends with a barrier: s_w of the previous chunk is no longer read
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int gc = c0 + t * 16 + lr;
      const float cc = gc < p.K ? p.colc[gc] : -INFINITY;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = wave * 16 + lk * 4 + q, gr = r0 + row;
        float w = 0.f;
        if (gr < nend && gc < p.K) {
          const float v = tot[t][q] + cc;
          const float sm = stats[(size_t)gr * 2 + 1];
          if (v > -INFINITY && sm > 0.f) w = g[gr] * expf(v - stats[(size_t)gr * 2]) / sm;
        }
        s_w[row * DN_WLD + t * 16 + lr] = w;
      }
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < DN_BN) {
      float v = 0.f;
      for (int n = 0; n < DN_BM; ++n) v += s_w[n * DN_WLD + tid];
      ssum += v;
    }
    if (dok) {
      const int rows = min(DN_BM, nend - r0);
      for (int n = 0; n < rows; ++n) {
        const float xv = p.x[(size_t)(r0 + n) * p.F + d];
        const float4* wrow = reinterpret_cast<const float4*>(s_w + n * DN_WLD);
#pragma unroll
        for (int k4 = 0; k4 < DN_BN / 4; ++k4) {
          const float4 w4 = wrow[k4];
          const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = k4 * 4 + j;
            if (TWO) {
              const float df = xv - mu[k], wd = wv[j] * df;
              acc1[k] += wd;
              acc2[k] = fmaf(wd, df, acc2[k]);
            } else {
              acc1[k] = fmaf(wv[j], xv, acc1[k]);
            }
          }
        }
      }
    }
    // the next dn_tile's first barrier comes after its stores to s_a / s_b only: s_w is rewritten after its last one
  }
  if (dok) {
#pragma unroll
    for (int k = 0; k < DN_BN; ++k) {
      if (c0 + k >= p.K) continue;
      const size_t e = ((size_t)blockIdx.z * p.K + c0 + k) * p.F + d;
      part1[e] = acc1[k];
      if (TWO) part2[e] = acc2[k];
    }
  }
  if (blockIdx.x == 0 && tid < DN_BN && c0 + tid < p.K) part_s[(size_t)blockIdx.z * p.K + c0 + tid] = ssum;
}

// Adds the row ranges in order and applies the parameter transforms; results are ADDED to the gradients.
template <int KIND>
__global__ void __launch_bounds__(256) dn_finish_kernel(const float* __restrict__ part1, const float* __restrict__ part2,
                                                        const float* __restrict__ part_s, const float* __restrict__ p1,
                                                        const float* __restrict__ p2, float* __restrict__ d1,
                                                        float* __restrict__ d2, int K, int F, int ns) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)K * F;
  if (e >= total) return;
  const int k = (int)(e / F);
  float a1 = 0.f, a2 = 0.f, sk = 0.f;
  for (int z = 0; z < ns; ++z) {
    a1 += part1[(size_t)z * total + e];
    if (KIND == DN_GAUSSIAN) a2 += part2[(size_t)z * total + e];
    sk += part_s[(size_t)z * K + k];
  }
  if (KIND == DN_BERNOULLI) {
    const float l = p1[e];
    const float sg = l >= 0.f ? 1.f / (1.f + expf(-l)) : expf(l) / (1.f + expf(l));
    if (d1) d1[e] += a1 - sg * sk;
  } else {
    const float iv = expf(-2.f * p2[e]);
    if (d1) d1[e] += a1 * iv;
    if (d2) d2[e] += a2 * iv - sk;
  }
}

// dlogits[k] += S[k] - pi_k sum_j S[j] (the gradient through log_softmax), one workgroup
__global__ void __launch_bounds__(256) dn_finish_logits_kernel(const float* __restrict__ part_s,
                                                               const float* __restrict__ logpi, float* __restrict__ dl,
                                                               int K, int ns) {
  __shared__ float s_red[4];
  float tot = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) {
    float sk = 0.f;
    for (int z = 0; z < ns; ++z) sk += part_s[(size_t)z * K + k];
    tot += sk;
  }
  tot = dn_block_sum(tot, s_red);
  for (int k = threadIdx.x; k < K; k += 256) {
    float sk = 0.f;
    for (int z = 0; z < ns; ++z) sk += part_s[(size_t)z * K + k];
    dl[k] += sk - expf(logpi[k]) * tot;
  }
}

// Parzen window: out[n] = log(coef count / K), count = #{k : |x[n][d] - y[k][d]| / h <= 0.5 for every d} in the
// reference's fp32 order (subtract, abs, divide, compare), early exit per pair. One workgroup per test row.
__global__ void __launch_bounds__(256) dn_parzen_kernel(const float* __restrict__ x, const float* __restrict__ y, float h,
                                                        float coef, float* __restrict__ out, int K, int F) {
  __shared__ int s_cnt[4];
  const float* xr = x + (size_t)blockIdx.x * F;
  int cnt = 0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float* yr = y + (size_t)k * F;
    int dd = 0;
    while (dd < F && __fdiv_rn(fabsf(xr[dd] - yr[dd]), h) <= 0.5f) ++dd;
    cnt += dd == F;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    float v;
    if (isinf(coef))  // the reference's mean of inf * {0, 1}: NaN as soon as one window misses
      v = c == K ? INFINITY : NAN;
    else
      v = logf(coef * (float)c / (float)K);
    out[blockIdx.x] = v;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------

int dn_check(const char* name, int N, int K, int F) {
  PG_REQUIRE(N >= 1 && K >= 1 && F >= 1, PG_ESHAPE, "%s: N = %d, K = %d, F = %d must all be >= 1", name, N, K, F);
  PG_REQUIRE(pg_cdiv(N, DN_BM) <= DN_MAX_TILES && pg_cdiv(K, DN_BN) <= DN_MAX_TILES, PG_ESHAPE,
             "%s: N = %d above %d or K = %d above %d", name, N, DN_MAX_TILES * DN_BM, K, DN_MAX_TILES * DN_BN);
  PG_REQUIRE((long)N * F < (1L << 40) && (long)K * F < (1L << 40), PG_ESHAPE, "%s: N * F or K * F too large", name);
  return 0;
}

// Column splits of the forward: with fewer than 256 row tiles the column tiles are spread until about 512 workgroups run.
int dn_splits(int N, int K, int& tper) {
  const int rows = pg_cdiv(N, DN_BM), tiles = pg_cdiv(K, DN_BN);
  int sp = 1;
  if (rows < 256 && tiles >= 4) sp = std::min(std::min(pg_cdiv(512, rows), tiles), DN_MAX_SPLITS);
  tper = pg_cdiv(tiles, sp);
  return pg_cdiv(tiles, tper);
}

size_t dn_lse_ws(int N, int K) {
  int tper;
  const int sp = dn_splits(N, K, tper);
  return sp > 1 ? (size_t)sp * N * 2 : 0;
}

// Row ranges of the backward: whole 64-row chunks, until about 512 workgroups run.
int dn_nsplits(int N, int K, int F, int& rper) {
  const long wgs = (long)pg_cdiv(F, DN_DT) * pg_cdiv(K, DN_BN);
  const int chunks = pg_cdiv(N, DN_BM);
  const int ns = (int)std::min<long>(std::min<long>((512 + wgs - 1) / wgs, chunks), DN_MAX_NSPLITS);
  rper = pg_cdiv(chunks, ns) * DN_BM;
  return pg_cdiv(N, rper);
}

size_t dn_align(size_t n) { return (n + 3) & ~(size_t)3; }  // workspace sections stay 16-byte aligned

// workspace layout of the mixtures: logpi (K) | colc (K) | b1 (K F) [| b2 (K F)] | forward partials or backward partials
size_t dn_mixture_head(int kind, int K, int F) {
  return 2 * dn_align(K) + (kind == DN_GAUSSIAN ? 2 : 1) * dn_align((size_t)K * F);
}

int dn_lse_launch(const DnOps& p, float* out, int add_out, float* stats, float* ws, size_t ws_floats, hipStream_t st,
                  const char* name) {
  int tper;
  const int sp = dn_splits(p.N, p.K, tper);
  float* part = nullptr;
  if (sp > 1) {
    PG_REQUIRE(ws != nullptr && ws_floats >= (size_t)sp * p.N * 2, PG_EINVAL,
               "%s: workspace of %zu floats too small (_workspace_floats)", name, ws_floats);
    part = ws;
  }
  dim3 grid((unsigned)sp, (unsigned)pg_cdiv(p.N, DN_BM));
  if (p.b2)
    hipLaunchKernelGGL(dn_lse_kernel<true>, grid, dim3(DN_THREADS), 0, st, p, out, add_out, part, stats, tper);
  else
    hipLaunchKernelGGL(dn_lse_kernel<false>, grid, dim3(DN_THREADS), 0, st, p, out, add_out, part, stats, tper);
  PG_LAUNCH_CHECK(name);
  if (sp > 1) {
    hipLaunchKernelGGL(dn_merge_kernel, dim3((unsigned)pg_cdiv(p.N, 256)), dim3(256), 0, st, part, out, add_out,
                       stats, p.N, sp);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

// log_softmax + operand transforms into the head of the workspace; fills the operands of the tile kernels
int dn_mixture_prepare(int kind, const float* x, const float* logits, const float* p1, const float* p2, float* ws, int N,
                       int K, int F, hipStream_t st, const char* name, DnOps& p, float*& logpi, float*& rest) {
  logpi = ws;
  float* colc = ws + dn_align(K);
  float* b1 = colc + dn_align(K);
  float* b2 = b1 + dn_align((size_t)K * F);
  hipLaunchKernelGGL(dn_log_softmax_kernel, dim3(1), dim3(256), 0, st, logits, logpi, K);
  PG_LAUNCH_CHECK(name);
  if (kind == DN_GAUSSIAN)
    hipLaunchKernelGGL(dn_mixture_prep_kernel<DN_GAUSSIAN>, dim3((unsigned)pg_cdiv(K, 4)), dim3(256), 0, st, p1, p2, logpi,
                       b1, b2, colc, K, F);
  else
    hipLaunchKernelGGL(dn_mixture_prep_kernel<DN_BERNOULLI>, dim3((unsigned)pg_cdiv(K, 4)), dim3(256), 0, st, p1, p2,
                       logpi, b1, (float*)nullptr, colc, K, F);
  PG_LAUNCH_CHECK(name);
  p.x = x;
  p.b1 = b1;
  p.b2 = kind == DN_GAUSSIAN ? b2 : nullptr;
  p.colc = colc;
  p.alpha = 1.f;
  p.N = N;
  p.K = K;
  p.F = F;
  rest = ws + dn_mixture_head(kind, K, F);
  return 0;
}

int dn_mixture_check(const char* name, int kind, int N, int K, int F) {
  PG_REQUIRE(kind == DN_BERNOULLI || kind == DN_GAUSSIAN, PG_EINVAL, "%s: unknown mixture kind %d", name, kind);
  return dn_check(name, N, K, F);
}

}  // namespace

PG_EXPORT size_t pg_mixture_workspace_floats(int kind, int N, int K, int F, int backward) {
  if (N < 1 || K < 1 || F < 1 || (kind != DN_BERNOULLI && kind != DN_GAUSSIAN)) return 0;
  const size_t head = dn_mixture_head(kind, K, F);
  if (!backward) return head + dn_lse_ws(N, K);
  int rper;
  const size_t ns = (size_t)dn_nsplits(N, K, F, rper);
  return head + ns * dn_align((size_t)K * F) * (kind == DN_GAUSSIAN ? 2 : 1) + ns * dn_align(K);
}

PG_EXPORT int pg_mixture_fwd(int kind, const float* x, const float* mixture_logits, const float* p1, const float* p2,
                             float* lse, float* stats, int N, int K, int F, float* ws, size_t ws_floats, void* stream) {
  const char* name = "pg_mixture_fwd";
  const int rc = dn_mixture_check(name, kind, N, K, F);
  if (rc) return rc;
  PG_REQUIRE(x && mixture_logits && p1 && lse && stats && (kind != DN_GAUSSIAN || p2), PG_EINVAL, "%s: null pointer", name);
  const size_t need = pg_mixture_workspace_floats(kind, N, K, F, 0);
  PG_REQUIRE(ws != nullptr && ws_floats >= need, PG_EINVAL, "%s: workspace of %zu floats < %zu (pg_mixture_workspace_floats)",
             name, ws_floats, need);
  DnOps p;
  float *logpi, *rest;
  const int rp = dn_mixture_prepare(kind, x, mixture_logits, p1, p2, ws, N, K, F, (hipStream_t)stream, name, p, logpi, rest);
  if (rp) return rp;
  // lse = log p_0(x) + logsumexp_k c'
  if (kind == DN_GAUSSIAN)
    hipLaunchKernelGGL(dn_row_ref_kernel<DN_GAUSSIAN>, dim3((unsigned)pg_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, x, p1,
                       p2, lse, N, F);
  else
    hipLaunchKernelGGL(dn_row_ref_kernel<DN_BERNOULLI>, dim3((unsigned)pg_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, x,
                       p1, p2, lse, N, F);
  PG_LAUNCH_CHECK(name);
  return dn_lse_launch(p, lse, 1, stats, rest, ws_floats - dn_mixture_head(kind, K, F), (hipStream_t)stream, name);
}

PG_EXPORT int pg_mixture_bwd(int kind, const float* x, const float* mixture_logits, const float* p1, const float* p2,
                             const float* stats, const float* g, float* d_logits, float* d1, float* d2, int N, int K, int F,
                             float* ws, size_t ws_floats, void* stream) {
  const char* name = "pg_mixture_bwd";
  const int rc = dn_mixture_check(name, kind, N, K, F);
  if (rc) return rc;
  PG_REQUIRE(x && mixture_logits && p1 && stats && g && (kind != DN_GAUSSIAN || p2), PG_EINVAL, "%s: null pointer", name);
  const size_t need = pg_mixture_workspace_floats(kind, N, K, F, 1);
  PG_REQUIRE(ws != nullptr && ws_floats >= need, PG_EINVAL, "%s: workspace of %zu floats < %zu (pg_mixture_workspace_floats)",
             name, ws_floats, need);
  hipStream_t st = (hipStream_t)stream;
  DnOps p;
  float *logpi, *rest;
  const int rp = dn_mixture_prepare(kind, x, mixture_logits, p1, p2, ws, N, K, F, st, name, p, logpi, rest);
  if (rp) return rp;
  int rper;
  const int ns = dn_nsplits(N, K, F, rper);
  const size_t kf = dn_align((size_t)K * F);
  float* part1 = rest;
  float* part2 = kind == DN_GAUSSIAN ? part1 + ns * kf : nullptr;
  float* part_s = part1 + (kind == DN_GAUSSIAN ? 2 : 1) * ns * kf;
  dim3 grid((unsigned)pg_cdiv(F, DN_DT), (unsigned)pg_cdiv(K, DN_BN), (unsigned)ns);
  const long total = (long)K * F;
  if (kind == DN_GAUSSIAN) {
    hipLaunchKernelGGL(dn_bwd_kernel<DN_GAUSSIAN>, grid, dim3(DN_THREADS), 0, st, p, p1, stats, g, part1, part2, part_s,
                       rper);
    PG_LAUNCH_CHECK(name);
    if (d1 || d2) {
      hipLaunchKernelGGL(dn_finish_kernel<DN_GAUSSIAN>, dim3((unsigned)pg_cdiv(total, 256)), dim3(256), 0, st, part1, part2,
                         part_s, p1, p2, d1, d2, K, F, ns);
      PG_LAUNCH_CHECK(name);
    }
  } else {
    hipLaunchKernelGGL(dn_bwd_kernel<DN_BERNOULLI>, grid, dim3(DN_THREADS), 0, st, p, p1, stats, g, part1, part2, part_s,
                       rper);
    PG_LAUNCH_CHECK(name);
    if (d1) {
      hipLaunchKernelGGL(dn_finish_kernel<DN_BERNOULLI>, dim3((unsigned)pg_cdiv(total, 256)), dim3(256), 0, st, part1, part2,
                         part_s, p1, p2, d1, d2, K, F, ns);
      PG_LAUNCH_CHECK(name);
    }
  }
  if (d_logits) {
    hipLaunchKernelGGL(dn_finish_logits_kernel, dim3(1), dim3(256), 0, st, part_s, logpi, d_logits, K, ns);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

PG_EXPORT size_t pg_kde_workspace_floats(int N, int K, int F) {
  if (N < 1 || K < 1 || F < 1) return 0;
  return dn_align(K) + dn_lse_ws(N, K);
}

PG_EXPORT int pg_kde_gaussian(const float* test, const float* train, float bandwidth, float* out, int N, int K, int F,
                              float* ws, size_t ws_floats, void* stream) {
  const char* name = "pg_kde_gaussian";
  const int rc = dn_check(name, N, K, F);
  if (rc) return rc;
  PG_REQUIRE(test && train && out, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(bandwidth > 0.f && std::isfinite(bandwidth), PG_EINVAL, "%s: bandwidth %g must be positive and finite", name,
             (double)bandwidth);
  const size_t need = pg_kde_workspace_floats(N, K, F);
  PG_REQUIRE(ws != nullptr && ws_floats >= need, PG_EINVAL, "%s: workspace of %zu floats < %zu (pg_kde_workspace_floats)", name,
             ws_floats, need);
  hipStream_t st = (hipStream_t)stream;
  const double h = bandwidth;
  const float alpha = (float)(1.0 / (h * h));
  const float z = (float)(0.5 * F * log(2.0 * M_PI) + F * log(h) + log((double)K));
  float* colc = ws;
  hipLaunchKernelGGL(dn_sqnorm_kernel, dim3((unsigned)pg_cdiv(K, 4)), dim3(256), 0, st, train, colc, -0.5f * alpha, -z, K, F);
  PG_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(dn_sqnorm_kernel, dim3((unsigned)pg_cdiv(N, 4)), dim3(256), 0, st, test, out, -0.5f * alpha, 0.f, N, F);
  PG_LAUNCH_CHECK(name);
  DnOps p;
  p.x = test;
  p.b1 = train;
  p.b2 = nullptr;
  p.colc = colc;
  p.alpha = alpha;
  p.N = N;
  p.K = K;
  p.F = F;
  return dn_lse_launch(p, out, 1, nullptr, ws + dn_align(K), ws_floats - dn_align(K), st, name);
}

PG_EXPORT int pg_kde_parzen(const float* test, const float* train, float bandwidth, float coef, float* out, int N, int K,
                            int F, void* stream) {
  const char* name = "pg_kde_parzen";
  PG_REQUIRE(N >= 1 && K >= 1 && F >= 1, PG_ESHAPE, "%s: N = %d, K = %d, F = %d must all be >= 1", name, N, K, F);
  PG_REQUIRE(test && train && out, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(bandwidth > 0.f && std::isfinite(bandwidth), PG_EINVAL, "%s: bandwidth %g must be positive and finite", name,
             (double)bandwidth);
  hipLaunchKernelGGL(dn_parzen_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, test, train, bandwidth, coef,
                     out, K, F);
  PG_LAUNCH_CHECK(name);
  return 0;
}
