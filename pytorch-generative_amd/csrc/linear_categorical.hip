// linear_categorical.hip — the model's last 1x1 convolution fused into the K-way softmax likelihood of categorical.hip:
// loss = categorical_nll(conv1x1(transform(h))) without the (N, K C, H, W) logits or their gradient ever being written.
//
// h (N, Cin, HW) are the head's input features, w (K C, Cin) its weight, class-major (output channel o = k C + c),
// b (K C) an optional bias, x (N, C, HW) the images at the levels j / (K - 1) (cat_class). `transform` is applied to
// the features while a tile is staged: none, relu, or LayerNorm over the Cin channels (biased variance, eps inside
// the root, one Newton step on v_rsq_f32, as gpt_ends.hip).
//
// Geometry (pg_linear_categorical_plan). The N HW pixels are one sequence p = n HW + hw, cut into tiles of 16
// consecutive pixels (a tile may span images). A workgroup is ONE wave; workgroup r owns the consecutive tiles
// [r tpr, min((r + 1) tpr, tiles)) with tpr = ceil(tiles / rows). Lane l of the wave is (j, g) = (l & 15, l >> 4).
//   staging  lane (j, g) loads the channel quads g, g + 4, ... of pixel j, transforms them and keeps the tile in LDS as
//            float4 hs4[quad][pixel]. LayerNorm's sums meet over the four lanes of a pixel by __shfl_xor 16 / 32.
//   logits   z[16 classes x 16 pixels] = W h + b on v_mfma_f32_16x16x4_f32, 16 channels per step: lane (i, g) holds
//            the float4 w[class i][16 s + 4 g ..] as A, lane (j, g) the float4 hs4[4 s + g][pixel j] as B, and
//            component e of both is one MFMA (the contraction order is a permutation both operands share). The
//            accumulator starts at the bias. Lane (j, g) then holds the classes k0 + 4 g + r, r = 0..3, of pixel j.
//   forward  a running (max, sum) per lane (cat_merge rules, four classes per rescale), merged over g once per
//            sub-pixel; lse and the rounding residual of max + log(sum) are the two planes of the dense path.
//   backward recomputes z with the same device function (the same MFMA chain: the same bits), forms
//            d = g / N (exp((z - lse) - residual) - [k == t]) in the accumulator layout and uses it three times:
//              dh += W^T d    d is already a valid B operand (k = g <-> class 4 g + r); A = w[class 4 g + r][ci]
//              dW += d h^T    d goes through a 16 x 16 LDS transpose to become A; B = the staged tile
//              db += sum d    over the 16 lanes of a group
//            dh passes through the transform's derivative (relu mask / LayerNorm backward from the statistics
//            recomputed while staging) and is written once.
// dW, db, d ln_w, d ln_b accumulate over all tiles of the workgroup in ONE partial row
//   [ dW (K C x Cin) | db (K C) | d ln_w (Cin) | d ln_b (Cin) ]
// kept in LDS when it fits (copied to the workspace at the end), else in the workspace row itself (zeroed by the
// launch; every word has one owner lane, so the read-modify-writes are ordered). pg_linear_categorical_reduce adds the
// rows to their destinations in row order: no float atomics on a gradient, bit-reproducible. The weights (and bias)
// are staged in LDS when they fit next to that, else streamed from memory one class tile at a time. LDS per workgroup
// stays within 64 KB. Sub-pixels with large logits are refined in float64 (lc_refine_from below): the two lse planes hold the
// normaliser of the EXACT logits to the same 4e-6 as on the dense path. The scalar loss takes one fp32 atomic per workgroup, as pg_categorical_nll_fwd; per-sample
// sums come from a third plane of lse (the sub-pixel's lse - z_t) summed in a fixed order by one workgroup per image.
#include <math.h>

#include "categorical.h"
#include "common.h"
#include "mfma_tile.h"

namespace {

using pg_tile::f32x4;
using pg_tile::mfma16;

constexpr int LC_PX = 16;             // pixels per tile
constexpr int LC_MAX_ROWS = 1024;     // workgroups (= partial rows) at most: four waves per CU
constexpr int LC_LDS_BYTES = 65536;   // LDS a workgroup may take
constexpr int LC_DT = 17;             // row pitch of the d^T transpose tile
constexpr int LC_MAX_K = 4096;
constexpr int LC_RED_THREADS = 256;

struct LcArgs {
  const float* h; const float* w; const float* b; const float* lnw; const float* lnb; const float* x;
  float* lse;        // forward: written; backward: read
  float* loss;       // forward
  const float* g;    // backward
  float* dh;         // backward
  float* ws;         // backward
  float eps, invN;
  int N, C, K, Cin, HW, transform;
  long P;            // N * HW
  int tiles, w_lds, acc_lds, nll_plane;
};

struct LcPlan {
  int tiles, rows, tpr;
  long row_len, weight_floats;
  int w_lds_fwd, w_lds_bwd, acc_lds;
  int lds_fwd, lds_bwd;  // bytes
};

// Stages the transformed features of the lane's pixel (feature offset `hoff` = n Cin HW + hw) into hs4[quad][pixel];
// LayerNorm also leaves xhat in hx4 when it is given. Returns LayerNorm's reciprocal standard deviation.
__device__ __forceinline__ float lc_stage(const LcArgs& a, float4* hs4, float4* hx4, size_t hoff, int j, int g) {
  const int q = a.Cin >> 2;
  const size_t HW = (size_t)a.HW;
  float s = 0.f;
  for (int c4 = g; c4 < q; c4 += 4) {
    const float* p = a.h + hoff + (size_t)(4 * c4) * HW;
    float4 v = make_float4(p[0], p[HW], p[2 * HW], p[3 * HW]);
    if (a.transform == PG_LC_RELU) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    s += (v.x + v.y) + (v.z + v.w);
    hs4[c4 * LC_PX + j] = v;
  }
  if (a.transform != PG_LC_LN) return 0.f;
  const float invC = 1.f / (float)a.Cin;
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const float mu = s * invC;
  float qq = 0.f;
  for (int c4 = g; c4 < q; c4 += 4) {  // the lane re-reads its own stores
    const float4 v = hs4[c4 * LC_PX + j];
    const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
    qq = fmaf(d0, d0, qq), qq = fmaf(d1, d1, qq), qq = fmaf(d2, d2, qq), qq = fmaf(d3, d3, qq);
  }
  qq += __shfl_xor(qq, 16, 64);
  qq += __shfl_xor(qq, 32, 64);
  const float var = qq * invC + a.eps;
  float rs = rsqrtf(var);
  rs = rs * (1.5f - 0.5f * var * rs * rs);
  for (int c4 = g; c4 < q; c4 += 4) {
    float4 v = hs4[c4 * LC_PX + j];
    v = make_float4((v.x - mu) * rs, (v.y - mu) * rs, (v.z - mu) * rs, (v.w - mu) * rs);
    if (hx4) hx4[c4 * LC_PX + j] = v;
    const float4 lw = *reinterpret_cast<const float4*>(a.lnw + 4 * c4), lb = *reinterpret_cast<const float4*>(a.lnb + 4 * c4);
    hs4[c4 * LC_PX + j] = make_float4(fmaf(v.x, lw.x, lb.x), fmaf(v.y, lw.y, lb.y), fmaf(v.z, lw.z, lb.z), fmaf(v.w, lw.w, lb.w));
  }
  return rs;
}

// z of the classes k0 + 4 g + r (r = 0..3) of channel c at the lane's pixel. wp / bp: weights and bias, in LDS or in memory.
// Rows past K - 1 are clamped (the caller masks them).
__device__ __forceinline__ f32x4 lc_z(const float* wp, const float* bp, const float4* hs4, int K, int C, int Cin, int c, int k0,
                                      int j, int g) {
  f32x4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = min(k0 + 4 * g + r, K - 1);
    acc[r] = bp ? bp[(size_t)k * C + c] : 0.f;
  }
  const float* wr = wp + ((size_t)min(k0 + j, K - 1) * C + c) * Cin;
  const int q = Cin >> 2;
  for (int c40 = 0; c40 < q; c40 += 4) {
    const int c4 = c40 + g;
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    if (c4 < q) {
      av = *reinterpret_cast<const float4*>(wr + 4 * c4);
      bv = hs4[c4 * LC_PX + j];
    }
    acc = mfma16(av.x, bv.x, acc);
    acc = mfma16(av.y, bv.y, acc);
    acc = mfma16(av.z, bv.z, acc);
    acc = mfma16(av.w, bv.w, acc);
  }
  return acc;
}

// Where the logits are large their own fp32 rounding is what limits the normaliser: a logit of size 100 carries 1e-5, more
// than the 4e-6 the two lse planes are held to. A sub-pixel whose |lse| reaches lc_refine_from(Cin) therefore has the
// classes that carry its probability mass (z >= lse - LC_REFINE_WINDOW; the rest weigh less than e^-18) evaluated once more
// in float64 from the raw features (lc_z64), by the lane that holds them: the forward adds sum p_k (z64_k - z_k) — the
// first-order change of the logsumexp, the second order is below 1e-9 — to the residual plane, and the backward forms the
// same classes' exp((z64 - lse) - residual) in float64 before rounding. The threshold keeps the random walk of the fp32
// chain, 0.3 ulp(|z|) sqrt(Cin), near 2e-6 where nothing is refined; ordinary logits (|lse| below it) never take this path.
constexpr float LC_REFINE_WINDOW = 18.f;
__device__ __forceinline__ float lc_refine_from(int Cin) { return Cin > 64 ? 8.f : 16.f; }

// LayerNorm statistics of the pixel in float64
__device__ __forceinline__ void lc_stats64(const LcArgs& a, size_t hoff, double& mu, double& rs) {
  const size_t HW = (size_t)a.HW;
  double s = 0.0;
  for (int ci = 0; ci < a.Cin; ++ci) s += (double)a.h[hoff + ci * HW];
  mu = s / (double)a.Cin;
  double q = 0.0;
  for (int ci = 0; ci < a.Cin; ++ci) {
    const double d = (double)a.h[hoff + ci * HW] - mu;
    q = fma(d, d, q);
  }
  rs = 1.0 / sqrt(q / (double)a.Cin + (double)a.eps);
}

// the logit of class k, channel c at the pixel, in float64 (mu, rs: lc_stats64, LayerNorm only)
__device__ __forceinline__ double lc_z64(const LcArgs& a, size_t hoff, int c, int k, double mu, double rs) {
  const size_t HW = (size_t)a.HW, o = (size_t)k * a.C + c;
  const float* wr = a.w + o * a.Cin;
  double acc = a.b ? (double)a.b[o] : 0.0;
  for (int ci = 0; ci < a.Cin; ++ci) {
    double y = (double)a.h[hoff + ci * HW];
    if (a.transform == PG_LC_RELU) y = y > 0.0 ? y : 0.0;
    else if (a.transform == PG_LC_LN) y = fma((y - mu) * rs, (double)a.lnw[ci], (double)a.lnb[ci]);
    acc = fma((double)wr[ci], y, acc);
  }
  return acc;
}

// copies the weights (and the bias, zeros without one) into LDS: wl = [ w (K C x Cin) | b (K C) ]
__device__ __forceinline__ void lc_stage_weights(const LcArgs& a, float* wl) {
  const long nw = (long)a.K * a.C * a.Cin, nb = (long)a.K * a.C;
  for (long i = threadIdx.x; i < nw; i += 64) wl[i] = a.w[i];
  for (long i = threadIdx.x; i < nb; i += 64) wl[nw + i] = a.b ? a.b[i] : 0.f;
}

struct LcPixel {
  bool live;
  size_t hoff;  // n Cin HW + hw
  size_t xoff;  // n C HW + hw
};

__device__ __forceinline__ LcPixel lc_pixel(const LcArgs& a, int tile, int j) {
  const long p = (long)tile * LC_PX + j;
  LcPixel px;
  px.live = p < a.P;
  const long pc = px.live ? p : a.P - 1;  // parked on the last pixel: takes part in every shuffle, stores nothing
  const long n = pc / a.HW, hw = pc - n * a.HW;
  px.hoff = (size_t)n * a.Cin * a.HW + (size_t)hw;
  px.xoff = (size_t)n * a.C * a.HW + (size_t)hw;
  return px;
}

__global__ void __launch_bounds__(64) lc_fwd_kernel(LcArgs a) {
  extern __shared__ float4 lc_smem4[];
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int K = a.K, C = a.C, Cin = a.Cin;
  float4* hs4 = lc_smem4;
  float* wl = reinterpret_cast<float*>(hs4 + (Cin >> 2) * LC_PX);
  if (a.w_lds) lc_stage_weights(a, wl);
  const float* wp = a.w_lds ? wl : a.w;
  const float* bp = a.w_lds ? wl + (size_t)K * C * Cin : a.b;
  const size_t plane = (size_t)a.N * C * a.HW;
  const bool ln = a.transform == PG_LC_LN;
  const int tpr = (a.tiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = blockIdx.x * tpr, t1 = min(t0 + tpr, a.tiles);
  float nll = 0.f;
  for (int tile = t0; tile < t1; ++tile) {
    const LcPixel px = lc_pixel(a, tile, j);
    __syncthreads();  // the previous tile's reads (and the weight staging) are done
    lc_stage(a, hs4, nullptr, px.hoff, j, g);
    __syncthreads();
    double mu64 = 0.0, rs64 = 0.0;  // the pixel's float64 LayerNorm statistics, made when first needed
    bool have64 = false;
    for (int c = 0; c < C; ++c) {
      const size_t xo = px.xoff + (size_t)c * a.HW;
      const int t = cat_class(a.x[xo], K);
      float m = -INFINITY, sum = 0.f, zt = 0.f;
      for (int k0 = 0; k0 < K; k0 += 16) {
        f32x4 z = lc_z(wp, bp, hs4, K, C, Cin, c, k0, j, g);
        float mn = m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = k0 + 4 * g + r;
          if (k >= K) z[r] = -INFINITY;
          if (k == t) zt = z[r];
          mn = fmaxf(mn, z[r]);
        }
        const float ref = mn > -INFINITY ? mn : 0.f;
        float acc = sum * __expf(m - ref);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc += __expf(z[r] - ref);
        sum = acc, m = mn;
      }
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(sum, off, 64);
        cat_merge(m, sum, m2, s2);
        zt += __shfl_xor(zt, off, 64);  // one lane of the four holds it, the others 0
      }
      const float lg = logf(sum), hi = m + lg, bb = hi - m;
      float res = (m - (hi - bb)) + (lg - bb);  // max + log(sum) = hi + res exactly
      const bool refine = px.live && fabsf(hi) >= lc_refine_from(Cin);
      if (__ballot(refine) != 0) {  // wave-uniform: large logits somewhere in the tile (see lc_refine_from)
        float corr = 0.f;
        for (int k0 = 0; k0 < K; k0 += 16) {
          const f32x4 z = lc_z(wp, bp, hs4, K, C, Cin, c, k0, j, g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = k0 + 4 * g + r;
            if (refine && k < K && z[r] - hi >= -LC_REFINE_WINDOW) {
              if (ln && !have64) lc_stats64(a, px.hoff, mu64, rs64), have64 = true;
              corr += __expf(z[r] - hi) * (float)(lc_z64(a, px.hoff, c, k, mu64, rs64) - (double)z[r]);
            }
          }
        }
        corr += __shfl_xor(corr, 16, 64);
        corr += __shfl_xor(corr, 32, 64);
        res += corr;
      }
      if (px.live && g == 0) {
        const float v = (hi - zt) + res;
        a.lse[xo] = hi;
        a.lse[plane + xo] = res;
        if (a.nll_plane) a.lse[2 * plane + xo] = v;
        nll += v;
      }
    }
  }
  nll = pg_wave_sum(nll);
  if (lane == 0) atomicAdd(a.loss, nll * a.invN);
}

// per_sample[n] = sum of the image's sub-pixel terms: one workgroup per image, fixed-order sums
__global__ void __launch_bounds__(LC_RED_THREADS) lc_per_sample_kernel(const float* __restrict__ nll, float* __restrict__ per_sample,
                                                                      long M) {
  const size_t n = blockIdx.x;
  float acc = 0.f;
  for (long i = threadIdx.x; i < M; i += LC_RED_THREADS) acc += nll[n * M + i];
  acc = pg_wave_sum(acc);
  __shared__ float part[LC_RED_THREADS / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) per_sample[n] = (part[0] + part[1]) + (part[2] + part[3]);
}

// sum over the 16 lanes of a group (all of them get it)
__device__ __forceinline__ float lc_group_sum(float v) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// CT: 16-channel tiles of the features the kernel is instantiated for (>= ceil(Cin / 16))
template <int CT>
__global__ void __launch_bounds__(64) lc_bwd_kernel(LcArgs a) {
  extern __shared__ float4 lc_smem4[];
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int K = a.K, C = a.C, Cin = a.Cin, q = Cin >> 2;
  const size_t KC = (size_t)K * C;
  float4* hs4 = lc_smem4;
  float4* hx4 = hs4 + q * LC_PX;
  float* dT = reinterpret_cast<float*>(hx4 + q * LC_PX);
  float* wl = dT + 16 * LC_DT;
  float* accl = wl + (a.w_lds ? KC * Cin + KC : 0);
  const size_t row_len = KC * Cin + KC + 2 * (size_t)Cin;
  float* row = a.ws + (size_t)blockIdx.x * row_len;
  float* acc = a.acc_lds ? accl : row;  // LDS, or the workspace row (zeroed by the launch)
  if (a.w_lds) lc_stage_weights(a, wl);
  if (a.acc_lds)
    for (size_t i = lane; i < row_len; i += 64) accl[i] = 0.f;
  const float* wp = a.w_lds ? wl : a.w;
  const float* bp = a.w_lds ? wl + KC * Cin : a.b;
  float* accW = acc;
  float* accB = accW + KC * Cin;
  float* accLw = accB + KC;
  float* accLb = accLw + Cin;
  const float* hs = reinterpret_cast<const float*>(hs4);
  const size_t plane = (size_t)a.N * C * a.HW;
  const float gs = a.g[0] * a.invN;
  const float invC = 1.f / (float)Cin;
  const bool ln = a.transform == PG_LC_LN;
  const int tpr = (a.tiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = blockIdx.x * tpr, t1 = min(t0 + tpr, a.tiles);
  for (int tile = t0; tile < t1; ++tile) {
    const LcPixel px = lc_pixel(a, tile, j);
    __syncthreads();
    const float rs = lc_stage(a, hs4, ln ? hx4 : nullptr, px.hoff, j, g);
    __syncthreads();
    f32x4 dha[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dha[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    double mu64 = 0.0, rs64 = 0.0;
    bool have64 = false;
    for (int c = 0; c < C; ++c) {
      const size_t xo = px.xoff + (size_t)c * a.HW;
      const int t = cat_class(a.x[xo], K);
      const float l = a.lse[xo], lo = a.lse[plane + xo];
      const bool refine = px.live && fabsf(l) >= lc_refine_from(Cin);  // the forward's rule, from the saved plane
      for (int k0 = 0; k0 < K; k0 += 16) {
        const f32x4 z = lc_z(wp, bp, hs4, K, C, Cin, c, k0, j, g);
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = k0 + 4 * g + r;
          float e = (z[r] - l) - lo;
          if (refine && k < K && z[r] - l >= -LC_REFINE_WINDOW) {
            if (ln && !have64) lc_stats64(a, px.hoff, mu64, rs64), have64 = true;
            e = (float)((lc_z64(a, px.hoff, c, k, mu64, rs64) - (double)l) - (double)lo);
          }
          const float v = gs * (__expf(e) - (k == t ? 1.f : 0.f));
          d[r] = (px.live && k < K) ? v : 0.f;
        }
        // db: the group's 16 pixels
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = k0 + 4 * g + r;
          const float v = lc_group_sum(d[r]);
          if (j == 0 && k < K && a.b) accB[(size_t)k * C + c] += v;
        }
        // dh += W^T d: A = w[class k0 + 4 g + r][channel 16 ct + j], B = d[r]
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (ct * 16 < Cin) {
            const int ci = min(ct * 16 + j, Cin - 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = min(k0 + 4 * g + r, K - 1);
              dha[ct] = mfma16(wp[((size_t)k * C + c) * Cin + ci], d[r], dha[ct]);
            }
          }
        }
        // dW += d h^T: d^T through LDS (class-local row, pixel column), then A = d^T[class j][pixel 4 g + e],
        // B = hs[channel 16 ct + j][pixel 4 g + e]
        __syncthreads();  // the previous class tile's reads of dT
#pragma unroll
        for (int r = 0; r < 4; ++r) dT[(4 * g + r) * LC_DT + j] = d[r];
        __syncthreads();
        float ta[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ta[e] = dT[j * LC_DT + 4 * g + e];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (ct * 16 < Cin) {
            const int ci = ct * 16 + j, cic = min(ci, Cin - 1);
            f32x4 cw;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = k0 + 4 * g + r;
              cw[r] = (k < K && ci < Cin) ? accW[((size_t)k * C + c) * Cin + ci] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) cw = mfma16(ta[e], hs[((cic >> 2) * LC_PX + 4 * g + e) * 4 + (cic & 3)], cw);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = k0 + 4 * g + r;
              if (k < K && ci < Cin) accW[((size_t)k * C + c) * Cin + ci] = cw[r];
            }
          }
        }
      }
    }
    // dha[ct][r] = d loss / d transform(h)[channel 16 ct + 4 g + r][pixel j]: through the transform's derivative
    float s1 = 0.f, s2 = 0.f;
    if (ln) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (ct * 16 < Cin) {  // uniform: the shuffles below are taken by the whole wave
          const int c4 = ct * 4 + g;
          const bool ok = c4 < q;
          const int c4c = ok ? c4 : q - 1;
          const float4 xh = hx4[c4c * LC_PX + j];
          const float4 lw = *reinterpret_cast<const float4*>(a.lnw + 4 * c4c);
          const float xe[4] = {xh.x, xh.y, xh.z, xh.w}, we[4] = {lw.x, lw.y, lw.z, lw.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float dy = ok ? dha[ct][r] : 0.f;
            const float vw = lc_group_sum(dy * xe[r]), vb = lc_group_sum(dy);  // masked pixels carry d = 0
            if (j == 0 && ok) {
              accLw[4 * c4 + r] += vw;
              accLb[4 * c4 + r] += vb;
            }
            const float dxh = dy * we[r];
            dha[ct][r] = dxh;
            s1 += dxh;
            s2 = fmaf(dxh, xe[r], s2);
          }
        }
      }
      s1 += __shfl_xor(s1, 16, 64), s2 += __shfl_xor(s2, 16, 64);
      s1 += __shfl_xor(s1, 32, 64), s2 += __shfl_xor(s2, 32, 64);
      s1 *= invC, s2 *= invC;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c4 = ct * 4 + g;
      if (c4 < q) {
        const float4 y = ln ? hx4[c4 * LC_PX + j] : hs4[c4 * LC_PX + j];
        const float ye[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = dha[ct][r];
          if (ln) v = rs * (v - s1 - ye[r] * s2);
          else if (a.transform == PG_LC_RELU) v = ye[r] > 0.f ? v : 0.f;
          if (px.live) a.dh[px.hoff + (size_t)(4 * c4 + r) * a.HW] = v;
        }
      }
    }
  }
  if (a.acc_lds) {
    __syncthreads();
    for (size_t i = lane; i < row_len; i += 64) row[i] = accl[i];
  }
}

// dest[i] += sum over the rows, in row order: 64 consecutive words per workgroup, four interleaved row sequences merged in a
// fixed order
__global__ void __launch_bounds__(LC_RED_THREADS) lc_reduce_kernel(const float* __restrict__ ws, int rows, long row_len, long nW,
                                                                  long nB, int Cin, float* __restrict__ dW, float* __restrict__ db,
                                                                  float* __restrict__ dlw, float* __restrict__ dlb) {
  const int e = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + e;
  __shared__ float part[LC_RED_THREADS];
  float s = 0.f;
  if (i < row_len) {
    const float* p = ws + i;
    int r = rg;
    for (; r + 28 < rows; r += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + 4 * u) * row_len];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < rows; r += 4) s += p[(size_t)r * row_len];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (rg == 0 && i < row_len) {
    const float tot = (part[e] + part[64 + e]) + (part[128 + e] + part[192 + e]);
    float* dst = nullptr;
    if (i < nW) dst = dW ? dW + i : nullptr;
    else if (i < nW + nB) dst = db ? db + (i - nW) : nullptr;
    else if (i < nW + nB + Cin) dst = dlw ? dlw + (i - nW - nB) : nullptr;
    else dst = dlb ? dlb + (i - nW - nB - Cin) : nullptr;
    if (dst) *dst += tot;
  }
}

int lc_check(const char* name, int N, int C, int K, int Cin, int HW, int transform) {
  PG_REQUIRE(N >= 1 && C >= 1 && HW >= 1, PG_ESHAPE, "%s: N = %d, C = %d, HW = %d must all be >= 1", name, N, C, HW);
  PG_REQUIRE(K >= 2 && K <= LC_MAX_K, PG_ESHAPE, "%s: %d classes outside 2..%d", name, K, LC_MAX_K);
  PG_REQUIRE(Cin >= 4 && Cin <= 256 && Cin % 4 == 0, PG_ESHAPE, "%s: %d input channels (a multiple of 4 in 4..256)", name, Cin);
  PG_REQUIRE(transform == PG_LC_NONE || transform == PG_LC_RELU || transform == PG_LC_LN, PG_ESHAPE,
             "%s: unknown input transform %d", name, transform);
  PG_REQUIRE((long)C * HW < (1L << 31) && (long)N * C * HW < (1L << 31) && (long)N * C * HW * (long)K < (1L << 40), PG_ESHAPE,
             "%s: N * C * HW = %ld sub-pixels of %d classes are too many", name, (long)N * C * HW, K);
  PG_REQUIRE((long)N * HW + LC_PX < (1L << 31) && (long)K * C * (Cin + 1) + 2 * Cin < (1L << 31), PG_ESHAPE,
             "%s: N * HW = %ld pixels or K * C * Cin = %ld weights are too many", name, (long)N * HW, (long)K * C * Cin);
  return 0;
}

LcPlan lc_plan(int N, int C, int K, int Cin, int HW) {
  LcPlan p;
  const long P = (long)N * HW, KC = (long)K * C;
  p.tiles = (int)((P + LC_PX - 1) / LC_PX);
  p.row_len = KC * Cin + KC + 2 * Cin;
  p.weight_floats = KC * Cin + KC;
  const long cap = (long)N * C * HW * (long)K / 4;  // a quarter of the logits
  long rows = cap / p.row_len;
  if (rows > LC_MAX_ROWS) rows = LC_MAX_ROWS;
  if (rows > p.tiles) rows = p.tiles;
  if (rows < 1) rows = 1;
  p.tpr = (int)((p.tiles + rows - 1) / rows);
  p.rows = (p.tiles + p.tpr - 1) / p.tpr;
  const long tile_f = (long)Cin * LC_PX, lim = LC_LDS_BYTES / 4;
  long f = tile_f;
  p.w_lds_fwd = f + p.weight_floats <= lim;
  if (p.w_lds_fwd) f += p.weight_floats;
  p.lds_fwd = (int)(4 * f);
  long bb = 2 * tile_f + 16 * LC_DT;
  p.acc_lds = bb + p.row_len <= lim;
  if (p.acc_lds) bb += p.row_len;
  p.w_lds_bwd = bb + p.weight_floats <= lim;
  if (p.w_lds_bwd) bb += p.weight_floats;
  p.lds_bwd = (int)(4 * bb);
  return p;
}

inline bool lc_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

LcArgs lc_args(const float* h, const float* w, const float* b, const float* ln_w, const float* ln_b, float eps, const float* x,
               int N, int C, int K, int Cin, int HW, int transform, const LcPlan& p) {
  LcArgs a = {};
  a.h = h, a.w = w, a.b = b, a.lnw = ln_w, a.lnb = ln_b, a.x = x;
  a.eps = eps, a.invN = 1.f / (float)N;
  a.N = N, a.C = C, a.K = K, a.Cin = Cin, a.HW = HW, a.transform = transform;
  a.P = (long)N * HW;
  a.tiles = p.tiles;
  return a;
}

}  // namespace

PG_EXPORT int pg_linear_categorical_plan(int N, int C, int K, int Cin, int HW, int transform, int* pixels_per_tile, int* rows,
                                         int* lds_bytes, size_t* workspace_floats) {
  const int rc = lc_check("pg_linear_categorical_plan", N, C, K, Cin, HW, transform);
  if (rc) return rc;
  PG_REQUIRE(pixels_per_tile && rows && lds_bytes && workspace_floats, PG_EINVAL, "pg_linear_categorical_plan: null pointer");
  const LcPlan p = lc_plan(N, C, K, Cin, HW);
  *pixels_per_tile = LC_PX;
  *rows = p.rows;
  *lds_bytes = p.lds_bwd > p.lds_fwd ? p.lds_bwd : p.lds_fwd;
  *workspace_floats = (size_t)p.rows * (size_t)p.row_len;
  return 0;
}

PG_EXPORT int pg_linear_categorical_nll_fwd(const float* h, const float* w, const float* b, const float* ln_w, const float* ln_b,
                                            float eps, const float* x, float* lse, float* per_sample, float* loss, int N, int C,
                                            int K, int Cin, int HW, int transform, void* stream) {
  const char* name = "pg_linear_categorical_nll_fwd";
  const int rc = lc_check(name, N, C, K, Cin, HW, transform);
  if (rc) return rc;
  PG_REQUIRE(h && w && x && lse && loss, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(transform != PG_LC_LN || (ln_w && ln_b), PG_EINVAL, "%s: LayerNorm without its weight and bias", name);
  PG_REQUIRE(lc_aligned(w) && (transform != PG_LC_LN || (lc_aligned(ln_w) && lc_aligned(ln_b))), PG_EINVAL,
             "%s: the weights must be 16-byte aligned", name);
  const LcPlan p = lc_plan(N, C, K, Cin, HW);
  LcArgs a = lc_args(h, w, b, ln_w, ln_b, eps, x, N, C, K, Cin, HW, transform, p);
  a.lse = lse, a.loss = loss;
  a.w_lds = p.w_lds_fwd;
  a.nll_plane = per_sample != nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lc_fwd_kernel, dim3((unsigned)p.rows), dim3(64), (size_t)p.lds_fwd, st, a);
  PG_LAUNCH_CHECK(name);
  if (per_sample) {
    hipLaunchKernelGGL(lc_per_sample_kernel, dim3((unsigned)N), dim3(LC_RED_THREADS), 0, st, lse + 2 * (size_t)N * C * HW,
                       per_sample, (long)C * HW);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

PG_EXPORT int pg_linear_categorical_nll_bwd(const float* h, const float* w, const float* b, const float* ln_w, const float* ln_b,
                                            float eps, const float* x, const float* lse, const float* g, float* dh, int N, int C,
                                            int K, int Cin, int HW, int transform, float* workspace, size_t workspace_floats,
                                            void* stream) {
  const char* name = "pg_linear_categorical_nll_bwd";
  const int rc = lc_check(name, N, C, K, Cin, HW, transform);
  if (rc) return rc;
  PG_REQUIRE(h && w && x && lse && g && dh && workspace, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(transform != PG_LC_LN || (ln_w && ln_b), PG_EINVAL, "%s: LayerNorm without its weight and bias", name);
  PG_REQUIRE(lc_aligned(w) && (transform != PG_LC_LN || (lc_aligned(ln_w) && lc_aligned(ln_b))), PG_EINVAL,
             "%s: the weights must be 16-byte aligned", name);
  const LcPlan p = lc_plan(N, C, K, Cin, HW);
  const size_t need = (size_t)p.rows * (size_t)p.row_len;
  PG_REQUIRE(workspace_floats >= need, PG_EINVAL, "%s: workspace of %zu floats, %zu needed", name, workspace_floats, need);
  LcArgs a = lc_args(h, w, b, ln_w, ln_b, eps, x, N, C, K, Cin, HW, transform, p);
  a.lse = const_cast<float*>(lse), a.g = g, a.dh = dh, a.ws = workspace;
  a.w_lds = p.w_lds_bwd, a.acc_lds = p.acc_lds;
  hipStream_t st = (hipStream_t)stream;
  if (!p.acc_lds) {  // the rows accumulate in place
    const hipError_t e = hipMemsetAsync(workspace, 0, need * sizeof(float), st);
    PG_REQUIRE(e == hipSuccess, (int)e, "%s: clearing the workspace failed: %s", name, hipGetErrorString(e));
  }
  const int cts = (Cin + 15) / 16;
  const dim3 grid((unsigned)p.rows), block(64);
  if (cts <= 1) hipLaunchKernelGGL(lc_bwd_kernel<1>, grid, block, (size_t)p.lds_bwd, st, a);
  else if (cts <= 2) hipLaunchKernelGGL(lc_bwd_kernel<2>, grid, block, (size_t)p.lds_bwd, st, a);
  else if (cts <= 4) hipLaunchKernelGGL(lc_bwd_kernel<4>, grid, block, (size_t)p.lds_bwd, st, a);
  else if (cts <= 8) hipLaunchKernelGGL(lc_bwd_kernel<8>, grid, block, (size_t)p.lds_bwd, st, a);
  else hipLaunchKernelGGL(lc_bwd_kernel<16>, grid, block, (size_t)p.lds_bwd, st, a);
  PG_LAUNCH_CHECK(name);
  return 0;
}

PG_EXPORT int pg_linear_categorical_reduce(const float* workspace, int rows, int KC, int Cin, int transform, float* dW, float* db,
                                           float* dln_w, float* dln_b, void* stream) {
  const char* name = "pg_linear_categorical_reduce";
  PG_REQUIRE(rows >= 1 && KC >= 2 && Cin >= 4 && Cin <= 256 && Cin % 4 == 0 && (long)KC * (Cin + 1) + 2 * Cin < (1L << 31), PG_ESHAPE,
             "%s: rows = %d, K * C = %d, Cin = %d", name, rows, KC, Cin);
  PG_REQUIRE(transform == PG_LC_NONE || transform == PG_LC_RELU || transform == PG_LC_LN, PG_ESHAPE,
             "%s: unknown input transform %d", name, transform);
  PG_REQUIRE(workspace && dW, PG_EINVAL, "%s: null pointer", name);
  const long nW = (long)KC * Cin, nB = KC;
  const bool ln = transform == PG_LC_LN;
  const long row_len = nW + nB + 2 * Cin;
  hipLaunchKernelGGL(lc_reduce_kernel, dim3((unsigned)pg_cdiv(row_len, 64)), dim3(LC_RED_THREADS), 0, (hipStream_t)stream,
                     workspace, rows, row_len, nW, nB, Cin, dW, db, ln ? dln_w : nullptr, ln ? dln_b : nullptr);
  PG_LAUNCH_CHECK(name);
  return 0;
}
