// categorical.hip — the K-way softmax pixel likelihood of the autoregressive image models (PixelCNN, GatedPixelCNN,
// PixelSNAIL, ImageGPT as published): negative log-likelihood forward / backward and the per-position draw.
//
// Logits are (N, K C, H, W), read as (N, K, C, H W): class-major, so every class k of image n is one dense row of
// M = C * H W sub-pixels and a sub-pixel's K logits lie M floats apart. Targets are images (N, C, H, W) at the levels
// j / (K - 1); the class is t = clamp(rint(x (K - 1)), 0, K - 1).
//
// Both loss kernels are pure streams (forward 4 K bytes per sub-pixel, backward 8 K) over the same geometry, which
// pg_categorical_plan chooses from K and H W % 4 alone (N and C are validated, they do not change it):
//   unit    `vec` consecutive sub-pixels of one image (4 = one 16-byte load per class, when H W % 4 == 0 and the operands are
//           16-byte aligned; else 1)
//   group   `lanes_per_pixel` = S lanes (a power of two <= 64) share one unit: lane s of the group walks the classes
//           s, s + S, s + 2 S, ... with several independent loads in flight
//   wave    64 / S units side by side: lane = s * (64 / S) + j, so that the lanes of one class row read consecutive
//           addresses and the S partial (max, sum) pairs of a unit meet by __shfl_xor over the lane bits above log2(64 / S).
// At batch 64, 28 x 28 there are only 50 k sub-pixels: one lane per sub-pixel would leave most of the chip idle behind 256
// dependent loads. S is the largest power of two that leaves a lane 64 classes, and at most 8 (K = 256: S = 4; K >= 512:
// S = 8). A sweep of the classes kept per lane on an MI355X (tools/exp/categorical_split_sweep.py ->
// profiles/categorical_split_sweep.txt; three shapes at K = 256, one at K = 1024, S = 1..64 each) has forward + backward
// within 5 % of the best split at S = 4 for K = 256 and best at S = 8 for K = 1024 (where K / 64 = 16 is 21 % slower), and
// S >= 16 slower everywhere: more lanes per sub-pixel shorten a wave's contiguous piece of a class row (64 / S units of
// 4 or 16 bytes: 128 bytes at S = 8 on the 4-wide path) faster than they add loads in flight. The kernels themselves take
// any power of two up to 64.
//
// The forward keeps a running (max, sum) per sub-pixel — the online logsumexp of density.hip, pushed a batch of loads at
// a time so that a batch costs one rescale — writes lse = max + log(sum) and adds (1 / N) sum (lse - z_t) into the
// scalar loss: one fp32 atomic per workgroup, as pg_bce_logits_fwd (the scalar feeds no gradient). The per-sample sums,
// asked for by evaluation only, come from a second kernel with one workgroup per image and a fixed-order reduction.
// The backward writes dlogits = g / N (exp(z - lse) - [k == t]): no reduction, bit-reproducible. Nothing of size
// (N, K, ...) exists besides the logits and their gradient.
//
// Accuracy: with logits of size 400 the fp32 value of lse is only good to 1.5e-5, and every probability of the sub-pixel
// would carry that as a common relative error — three times the element-wise gradient gate where p_t - 1 is small. So the
// forward keeps the rounding residual of max + log(sum) (an exact two-sum) in a second plane behind lse, and the backward
// forms exp((z - lse) - residual): z - lse is exact where it matters (z within a factor two of lse), as in torch's
// (z - max) - log(sum).
//
// The draw is one wave per (n, c): lane l owns the classes [l ceil(K / 64), (l + 1) ceil(K / 64)). With
// e_k = exp((z_k - max) / T), the lane sums are added in lane order, so that the running sum of class k is
// (sum of the lanes before) + (the lane's own running sum): it never decreases, and it ends exactly at the total the
// threshold u * total is formed from. The class is the first whose running sum exceeds the threshold strictly.
#include <math.h>
#include <stdlib.h>

#include "categorical.h"  // cat_class, cat_merge
#include "common.h"

namespace {

constexpr int CAT_THREADS = 256;
constexpr int CAT_MAX_K = 4096;
constexpr int CAT_CLASSES_PER_LANE = 64;  // the split leaves a lane at least this many classes (see the file header)
constexpr int CAT_MAX_SPLIT = 8;          // and goes no further than this

template <int VEC>
struct CatVec;
template <>
struct CatVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <>
struct CatVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// where a lane's unit lies; lanes past the last unit are parked on it (they take part in the shuffles, store nothing)
struct CatPos {
  size_t z0;   // logits offset of class 0
  size_t x0;   // offset into the images / lse
  int s;       // first class of this lane
  bool live;
};

template <int VEC>
__device__ __forceinline__ CatPos cat_pos(long units, long units_per_image, int K, long M, int S) {
  const int lane = threadIdx.x & 63;
  const int per_wave = 64 / S;
  const long wave = (long)blockIdx.x * (CAT_THREADS / 64) + (threadIdx.x >> 6);
  long unit = wave * per_wave + (lane & (per_wave - 1));
  CatPos p;
  p.live = unit < units;
  if (!p.live) unit = units - 1;
  const long n = unit / units_per_image, mu = unit - n * units_per_image;
  p.z0 = (size_t)n * K * M + (size_t)mu * VEC;
  p.x0 = (size_t)n * M + (size_t)mu * VEC;
  p.s = lane / per_wave;
  return p;
}

template <int VEC, int UN>
__global__ void __launch_bounds__(CAT_THREADS) cat_nll_fwd_kernel(const float* __restrict__ z, const float* __restrict__ x,
                                                                  float* __restrict__ lse, float* __restrict__ loss,
                                                                  long units, long units_per_image, int K, long M, int S,
                                                                  float invN) {
  const size_t plane = (size_t)units * VEC;  // lse | residual
  const CatPos p = cat_pos<VEC>(units, units_per_image, K, M, S);
  CatVec<VEC> zt;  // the target's logit: lane 0 of a group alone needs it
#pragma unroll
  for (int c = 0; c < VEC; ++c) zt.v[c] = 0.f;
  if (p.live && p.s == 0) {
    CatVec<VEC> xv;
    xv.load(x + p.x0);
#pragma unroll
    for (int c = 0; c < VEC; ++c) zt.v[c] = z[p.z0 + (size_t)cat_class(xv.v[c], K) * M + c];  // issued ahead of the stream
  }
  float m[VEC], sum[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) m[c] = -INFINITY, sum[c] = 0.f;
  const float* zp = z + p.z0;
  int k = p.s;
  for (; k + (UN - 1) * S < K; k += UN * S) {
    CatVec<VEC> v[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) v[i].load(zp + (size_t)(k + i * S) * M);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      float mn = m[c];
#pragma unroll
      for (int i = 0; i < UN; ++i) mn = fmaxf(mn, v[i].v[c]);
      const float ref = mn > -INFINITY ? mn : 0.f;
      float acc = sum[c] * __expf(m[c] - ref);
#pragma unroll
      for (int i = 0; i < UN; ++i) acc += __expf(v[i].v[c] - ref);
      sum[c] = acc, m[c] = mn;
    }
  }
  for (; k < K; k += S) {
    CatVec<VEC> v;
    v.load(zp + (size_t)k * M);
#pragma unroll
    for (int c = 0; c < VEC; ++c) cat_merge(m[c], sum[c], v.v[c], 1.f);
  }
  for (int off = 64 / S; off < 64; off <<= 1) {
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const float m2 = __shfl_xor(m[c], off, 64), s2 = __shfl_xor(sum[c], off, 64);
      cat_merge(m[c], sum[c], m2, s2);
    }
  }
  float nll = 0.f;
  if (p.live && p.s == 0) {
    CatVec<VEC> out, res;
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const float lg = logf(sum[c]), hi = m[c] + lg, bb = hi - m[c];
      out.v[c] = hi;
      res.v[c] = (m[c] - (hi - bb)) + (lg - bb);  // max + log(sum) = hi + res exactly
      nll += (hi - zt.v[c]) + res.v[c];
    }
    out.store(lse + p.x0);
    res.store(lse + plane + p.x0);
  }
  nll = pg_wave_sum(nll);
  __shared__ float part[CAT_THREADS / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = nll;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, ((part[0] + part[1]) + (part[2] + part[3])) * invN);
}

// per_sample[n] = sum over the image's sub-pixels of lse - z_t: one workgroup per image, fixed-order sums
__global__ void __launch_bounds__(CAT_THREADS) cat_per_sample_kernel(const float* __restrict__ z, const float* __restrict__ x,
                                                                     const float* __restrict__ lse,
                                                                     float* __restrict__ per_sample, int K, long M) {
  const size_t n = blockIdx.x, plane = (size_t)gridDim.x * M;
  float acc = 0.f;
  for (long i = threadIdx.x; i < M; i += CAT_THREADS) {
    const int t = cat_class(x[n * M + i], K);
    acc += (lse[n * M + i] - z[(n * K + t) * M + i]) + lse[plane + n * M + i];
  }
  acc = pg_wave_sum(acc);
  __shared__ float part[CAT_THREADS / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) per_sample[n] = (part[0] + part[1]) + (part[2] + part[3]);
}

template <int VEC, int UN>
__global__ void __launch_bounds__(CAT_THREADS) cat_nll_bwd_kernel(const float* __restrict__ z, const float* __restrict__ x,
                                                                  const float* __restrict__ lse, const float* __restrict__ g,
                                                                  float* __restrict__ dz, long units, long units_per_image,
                                                                  int K, long M, int S, float invN) {
  const CatPos p = cat_pos<VEC>(units, units_per_image, K, M, S);
  if (!p.live) return;  // no shuffles here
  const float gs = g[0] * invN;
  CatVec<VEC> xv, l, lo;
  xv.load(x + p.x0);
  l.load(lse + p.x0);
  lo.load(lse + (size_t)units * VEC + p.x0);
  int t[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) t[c] = cat_class(xv.v[c], K);
  const float* zp = z + p.z0;
  float* dp = dz + p.z0;
  int k = p.s;
  for (; k + (UN - 1) * S < K; k += UN * S) {
    CatVec<VEC> v[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) v[i].load(zp + (size_t)(k + i * S) * M);
#pragma unroll
    for (int i = 0; i < UN; ++i) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) v[i].v[c] = gs * (__expf((v[i].v[c] - l.v[c]) - lo.v[c]) - (k + i * S == t[c] ? 1.f : 0.f));
      v[i].store(dp + (size_t)(k + i * S) * M);
    }
  }
  for (; k < K; k += S) {
    CatVec<VEC> v;
    v.load(zp + (size_t)k * M);
#pragma unroll
    for (int c = 0; c < VEC; ++c) v.v[c] = gs * (__expf((v.v[c] - l.v[c]) - lo.v[c]) - (k == t[c] ? 1.f : 0.f));
    v.store(dp + (size_t)k * M);
  }
}

// One wave per draw d = n * C + c; the logit of class k is z[n * sn + (k * C + c) * sk].
__global__ void __launch_bounds__(CAT_THREADS) cat_sample_kernel(const float* __restrict__ z, long sn, long sk,
                                                                 const float* __restrict__ uniforms, float* __restrict__ out,
                                                                 int draws, int C, int K, float inv_t) {
  const int d = blockIdx.x * (CAT_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= draws) return;  // the whole wave leaves
  const int n = d / C, c = d - n * C;
  const float* zp = z + (size_t)n * sn + (size_t)c * sk;
  const size_t kstep = (size_t)C * sk;
  const int chunk = (K + 63) / 64;
  const int k0 = min(lane * chunk, K), k1 = min(k0 + chunk, K);
  float mx = -INFINITY;
  for (int k = k0; k < k1; ++k) mx = fmaxf(mx, zp[k * kstep]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float mine = 0.f;
  for (int k = k0; k < k1; ++k) mine += expf((zp[k * kstep] - mx) * inv_t);
  float before = 0.f, total = 0.f;  // the lane sums in lane order: total is the running sum after the last class
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const float v = __shfl(mine, j, 64);
    if (j < lane) before += v;
    total += v;
  }
  const float thresh = uniforms[d] * total;
  int pick = K;  // "none"
  float run = 0.f;
  for (int k = k0; k < k1; ++k) {
    run += expf((zp[k * kstep] - mx) * inv_t);  // the same values in the same order as `mine`
    if (pick == K && before + run > thresh) pick = k;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pick = min(pick, __shfl_xor(pick, off, 64));
  if (pick >= K) pick = K - 1;  // rounding (or a NaN) left none: the last class
  if (lane == 0) out[d] = __fdiv_rn((float)pick, (float)(K - 1));
}

// The geometry of the loss launches. vec_ok = 0 forces the scalar path (operands that are not 16-byte aligned).
int cat_plan(int K, int HW, int vec_ok, int& S, int& vec) {
  vec = (vec_ok && HW % 4 == 0) ? 4 : 1;
  // A/B (PG_VARIANT=ab builds only): classes a lane keeps at least
  static const int per_lane = PG_AB_INT("PG_CAT_CLASSES_PER_LANE", 0);
  const int keep = per_lane >= 4 ? per_lane : CAT_CLASSES_PER_LANE;
  const int cap = per_lane >= 4 ? 64 : CAT_MAX_SPLIT;  // a sweep goes all the way
  S = 1;
  while (S < cap && 2 * S * keep <= K) S <<= 1;
  return 0;
}

int cat_check(const char* name, int N, int C, int K, int HW) {
  PG_REQUIRE(N >= 1 && C >= 1 && HW >= 1, PG_ESHAPE, "%s: N = %d, C = %d, HW = %d must all be >= 1", name, N, C, HW);
  PG_REQUIRE(K >= 2 && K <= CAT_MAX_K, PG_ESHAPE, "%s: %d classes outside 2..%d", name, K, CAT_MAX_K);
  PG_REQUIRE((long)C * HW < (1L << 31) && (long)N * C * HW < (1L << 31) && (long)N * C * HW * (long)K < (1L << 40), PG_ESHAPE,
             "%s: N * C * HW = %ld sub-pixels of %d classes are too many", name, (long)N * C * HW, K);
  return 0;
}

inline bool cat_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct CatLaunch {
  long units, units_per_image, M;
  int S, vec;
  unsigned blocks;
};

CatLaunch cat_launch(int N, int C, int K, int HW, bool aligned) {
  CatLaunch a;
  cat_plan(K, HW, aligned ? 1 : 0, a.S, a.vec);
  a.M = (long)C * HW;
  a.units_per_image = a.M / a.vec;
  a.units = (long)N * a.units_per_image;
  const long waves = pg_cdiv(a.units, 64 / a.S);
  a.blocks = (unsigned)pg_cdiv(waves, CAT_THREADS / 64);
  return a;
}

}  // namespace

PG_EXPORT int pg_categorical_plan(int N, int C, int K, int HW, int* lanes_per_pixel, int* vec) {
  const int rc = cat_check("pg_categorical_plan", N, C, K, HW);
  if (rc) return rc;
  PG_REQUIRE(lanes_per_pixel && vec, PG_EINVAL, "pg_categorical_plan: null pointer");
  return cat_plan(K, HW, 1, *lanes_per_pixel, *vec);
}

PG_EXPORT int pg_categorical_nll_fwd(const float* logits, const float* x, float* lse, float* per_sample, float* loss, int N,
                                     int C, int K, int HW, void* stream) {
  const char* name = "pg_categorical_nll_fwd";
  const int rc = cat_check(name, N, C, K, HW);
  if (rc) return rc;
  PG_REQUIRE(logits && x && lse && loss, PG_EINVAL, "%s: null pointer", name);
  const CatLaunch a = cat_launch(N, C, K, HW, cat_aligned(logits) && cat_aligned(x) && cat_aligned(lse));
  hipStream_t st = (hipStream_t)stream;
  const float invN = 1.f / (float)N;
  if (a.vec == 4)
    hipLaunchKernelGGL((cat_nll_fwd_kernel<4, 4>), dim3(a.blocks), dim3(CAT_THREADS), 0, st, logits, x, lse, loss, a.units,
                       a.units_per_image, K, a.M, a.S, invN);
  else
    hipLaunchKernelGGL((cat_nll_fwd_kernel<1, 8>), dim3(a.blocks), dim3(CAT_THREADS), 0, st, logits, x, lse, loss, a.units,
                       a.units_per_image, K, a.M, a.S, invN);
  PG_LAUNCH_CHECK(name);
  if (per_sample) {
    hipLaunchKernelGGL(cat_per_sample_kernel, dim3((unsigned)N), dim3(CAT_THREADS), 0, st, logits, x, lse, per_sample, K, a.M);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

PG_EXPORT int pg_categorical_nll_bwd(const float* logits, const float* x, const float* lse, const float* g, float* dlogits,
                                     int N, int C, int K, int HW, void* stream) {
  const char* name = "pg_categorical_nll_bwd";
  const int rc = cat_check(name, N, C, K, HW);
  if (rc) return rc;
  PG_REQUIRE(logits && x && lse && g && dlogits, PG_EINVAL, "%s: null pointer", name);
  const CatLaunch a =
      cat_launch(N, C, K, HW, cat_aligned(logits) && cat_aligned(x) && cat_aligned(lse) && cat_aligned(dlogits));
  hipStream_t st = (hipStream_t)stream;
  const float invN = 1.f / (float)N;
  if (a.vec == 4)
    hipLaunchKernelGGL((cat_nll_bwd_kernel<4, 4>), dim3(a.blocks), dim3(CAT_THREADS), 0, st, logits, x, lse, g, dlogits,
                       a.units, a.units_per_image, K, a.M, a.S, invN);
  else
    hipLaunchKernelGGL((cat_nll_bwd_kernel<1, 8>), dim3(a.blocks), dim3(CAT_THREADS), 0, st, logits, x, lse, g, dlogits,
                       a.units, a.units_per_image, K, a.M, a.S, invN);
  PG_LAUNCH_CHECK(name);
  return 0;
}

PG_EXPORT int pg_categorical_sample(const float* logits, long sn, long sk, const float* uniforms, float* out, int N, int C,
                                    int K, float inv_temperature, void* stream) {
  const char* name = "pg_categorical_sample";
  const int rc = cat_check(name, N, C, K, 1);
  if (rc) return rc;
  PG_REQUIRE(logits && uniforms && out, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(sn > 0 && sk > 0, PG_EINVAL, "%s: strides (%ld, %ld) must be positive", name, sn, sk);
  PG_REQUIRE(inv_temperature > 0.f && std::isfinite(inv_temperature), PG_EINVAL,
             "%s: inverse temperature %g must be positive and finite", name, (double)inv_temperature);
  const int draws = N * C;
  hipLaunchKernelGGL(cat_sample_kernel, dim3((unsigned)pg_cdiv(draws, CAT_THREADS / 64)), dim3(CAT_THREADS), 0,
                     (hipStream_t)stream, logits, sn, sk, uniforms, out, draws, C, K, inv_temperature);
  PG_LAUNCH_CHECK(name);
  return 0;
}
