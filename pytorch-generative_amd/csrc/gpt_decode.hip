// gpt_decode.hip — one raster position of ALL transformer blocks of ImageGPT for all samples, in one launch.
//
// In decode, sample n at position p depends only on sample n's own earlier positions (its K / V caches): nothing crosses
// samples anywhere in the model. One workgroup therefore carries one sample through every block of the position with no
// grid-wide synchronisation; the activations of the sample (one column of the (C, ld) plane pg_sample_embed writes) live
// in LDS from the first LayerNorm to the last residual add. Per block (reference image_gpt.py:50-52 with :107-108):
//   a = LN1(h); [q | k | v] = Wqkv a + b; caches[:, p] = k, v; o = softmax_{j <= p - strict}(q . k_j / sqrt(dk)) v_j;
//   b = h + Wproj o + bproj; m = W2 gelu(W1 LN2(b) + b1) + b2; h = h + (b + m)
// Any C % 4 == 0 in 4..256 and any head split: the step is latency-bound (about 12 C^2 MACs per block and sample), so the
// matrix-vector products run on the VALU with lanes over OUTPUT rows against weights packed (in, out) — a wave reads 64
// consecutive floats per input element, the input element itself is an LDS broadcast.
// No float atomics; every reduction has a fixed order, and a workgroup sees nothing but its own column: column n of the
// output is bit-identical from run to run and whatever N and ld are.
#include "common.h"

namespace {

constexpr int GD_THREADS = 256;
constexpr int GD_WAVES = GD_THREADS / 64;
constexpr int GD_MAX_C = 256, GD_MAX_BLOCKS = 64, GD_MAX_L = 4096;
constexpr int GD_LDS_LIMIT = 64 * 1024;
constexpr int GD_JU = 4, GD_DU = 8, GD_CU = 4;  // attention: keys x head channels / channels x key strides loaded per batch

// The one function that decides the domain and the layouts: pg_gpt_decode_plan reports it, pg_gpt_decode_step launches by it.
struct GdPlan {
  int off[PG_GPT_DECODE_FIELDS];  // float offsets of a block's parameters inside its slice of the pack
  int block_floats;               // floats per block
  long pack_floats;               // blocks * block_floats
  int part_floats;                // LDS: partial sums of a split matrix-vector product
  int lds_bytes;
  char msg[160];
};

#define GD_REQUIRE(cond, code, ...)                \
  do {                                             \
    if (!(cond)) {                                 \
      snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__); \
      return (code);                               \
    }                                              \
  } while (0)

int gd_plan(int C, int heads, int blocks, int L, GdPlan& pl) {
  pl.msg[0] = 0;
  GD_REQUIRE(C > 0 && heads > 0 && blocks > 0 && L > 0, PG_EINVAL, "pg_gpt_decode: non-positive dimension");
  GD_REQUIRE(C % 4 == 0 && C >= 4 && C <= GD_MAX_C, PG_ESHAPE,
             "pg_gpt_decode: %d channels unsupported (a multiple of 4 in 4..%d)", C, GD_MAX_C);
  GD_REQUIRE(C % heads == 0, PG_ESHAPE, "pg_gpt_decode: %d heads do not divide %d channels", heads, C);
  GD_REQUIRE(blocks <= GD_MAX_BLOCKS, PG_ESHAPE, "pg_gpt_decode: %d blocks unsupported (at most %d)", blocks, GD_MAX_BLOCKS);
  GD_REQUIRE(L <= GD_MAX_L, PG_ESHAPE, "pg_gpt_decode: sequence length %d unsupported (at most %d)", L, GD_MAX_L);
  const int sizes[PG_GPT_DECODE_FIELDS] = {C, C, 3 * C * C, 3 * C, C * C, C, C, C, 4 * C * C, 4 * C, 4 * C * C, C};
  int at = 0;
  for (int f = 0; f < PG_GPT_DECODE_FIELDS; ++f) {
    pl.off[f] = at;
    at += sizes[f];
  }
  pl.block_floats = at;
  pl.pack_floats = (long)at * blocks;
  // a product with fewer than 4 x 64 output rows splits its input over the waves: at most 4 x 64 or 2 x 128 partial sums
  pl.part_floats = 4 * C > 256 ? 4 * C : 256;
  // h, a, [q | k | v], b, hidden, partial sums, scores, 2 x 4 wave results
  pl.lds_bytes = (C + C + 3 * C + C + 4 * C + pl.part_floats + L + 2 * GD_WAVES) * (int)sizeof(float);
  GD_REQUIRE(pl.lds_bytes <= GD_LDS_LIMIT, PG_ESHAPE, "pg_gpt_decode: %d bytes of LDS exceed %d", pl.lds_bytes, GD_LDS_LIMIT);
  return 0;
}

struct GdArgs {
  const float* x;
  float* out;
  const float* pack;
  float* kc;
  float* vc;
  const int* pos_dev;
  int N, C, heads, blocks, L, ld, p, strict;
  int block_floats, part_floats;
  int off[PG_GPT_DECODE_FIELDS];
  float eps, scale2;
};

__device__ __forceinline__ float gd_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// out[t] = LN(x)[t] for t < C. Every wave reduces the whole vector by itself (C <= 256: four elements per lane, then the
// xor butterfly, whose result is the same in every lane and every wave): no barrier inside. out must not alias x.
__device__ __forceinline__ void gd_layernorm(const float* x, const float* __restrict__ g, const float* __restrict__ b,
                                             float* out, int C, float eps, int tid, int lane) {
  float v[4], s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = lane + 64 * i;
    v[i] = idx < C ? x[idx] : 0.f;
    s += v[i];
  }
  const float inv_c = 1.f / (float)C;
  const float mean = pg_wave_sum(s) * inv_c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float d = lane + 64 * i < C ? v[i] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.f / sqrtf(pg_wave_sum(q) * inv_c + eps);
  if (tid < C) out[tid] = fmaf((x[tid] - mean) * rstd, g[tid], b[tid]);
}

// part[s * R + r] = sum over the s-th slice of k of w[k * R + r] * x[k]: lanes over 64 consecutive rows r, the input split
// in S = 4 / ceil(R / 64) slices (1 from three chunks of rows on) so that all four waves work when the output is short.
// Returns S; the caller adds part[0 .. S) of a row in that order after a barrier.
__device__ __forceinline__ int gd_matvec(const float* __restrict__ w, int K, int R, const float* x, float* part, int wave,
                                         int lane) {
  const int nchunks = (R + 63) >> 6;
  const int S = nchunks >= 3 ? 1 : GD_WAVES / nchunks;  // K % 4 == 0 and S in {1, 2, 4}: the slices are equal
  const int kper = K / S;
  for (int item = wave; item < nchunks * S; item += GD_WAVES) {
    const int chunk = item % nchunks, slice = item / nchunks;
    const int r = chunk * 64 + lane;
    const float* wr = w + (r < R ? r : R - 1);
    const int k0 = slice * kper, k1 = k0 + kper;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int k = k0;
    // the step is a chain of dependent memory latencies: 32 weight loads are in flight before the first multiply-add.
    // Four accumulators over k % 4, whatever the batch size: the summation order does not depend on it.
    for (; k + 32 <= k1; k += 32) {
      float wv[32];
#pragma unroll
      for (int i = 0; i < 32; ++i) wv[i] = wr[(size_t)(k + i) * R];
#pragma unroll
      for (int i = 0; i < 32; i += 4) {
        a0 = fmaf(wv[i], x[k + i], a0);
        a1 = fmaf(wv[i + 1], x[k + i + 1], a1);
        a2 = fmaf(wv[i + 2], x[k + i + 2], a2);
        a3 = fmaf(wv[i + 3], x[k + i + 3], a3);
      }
    }
#pragma unroll 4
    for (; k + 4 <= k1; k += 4) {
      a0 = fmaf(wr[(size_t)k * R], x[k], a0);
      a1 = fmaf(wr[(size_t)(k + 1) * R], x[k + 1], a1);
      a2 = fmaf(wr[(size_t)(k + 2) * R], x[k + 2], a2);
      a3 = fmaf(wr[(size_t)(k + 3) * R], x[k + 3], a3);
    }
    for (; k < k1; ++k) a0 = fmaf(wr[(size_t)k * R], x[k], a0);
    if (r < R) part[slice * R + r] = (a0 + a1) + (a2 + a3);
  }
  return S;
}

__device__ __forceinline__ float gd_combine(const float* part, int S, int R, int r, float bias) {
  float s = part[r];
  for (int i = 1; i < S; ++i) s += part[i * R + r];
  return s + bias;
}

__global__ void __launch_bounds__(GD_THREADS) gpt_decode_step_kernel(const GdArgs A) {
  extern __shared__ float gd_lds[];
  const int C = A.C, L = A.L, n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* h = gd_lds;            // the residual stream of this sample
  float* a = h + C;             // LN1(h), then o, then LN2(b)
  float* qkv = a + C;           // [q | k | v]
  float* bres = qkv + 3 * C;    // b = h + proj(o)
  float* hid = bres + C;        // gelu(fc1)
  float* part = hid + 4 * C;    // partial sums of a split product
  float* sc = part + A.part_floats;  // scores / probabilities of one head
  float* red = sc + L;          // per-wave maxima [0, 4) and sums [4, 8)

  int p = A.p;
  if (A.pos_dev) p = *A.pos_dev;
  p = min(max(p, 0), L - 1);  // a stale device position can never index outside the caches
  const int dk = C / A.heads;
  const bool self = A.strict == 0;  // the position's own key is admitted; the p cached keys j < p always are

  if (tid < C) h[tid] = A.x[(size_t)tid * A.ld + n];
  __syncthreads();

  for (int blk = 0; blk < A.blocks; ++blk) {
    const float* P = A.pack + (size_t)blk * A.block_floats;
    float* kcn = A.kc + ((size_t)blk * A.N + n) * C * L;
    float* vcn = A.vc + ((size_t)blk * A.N + n) * C * L;

    gd_layernorm(h, P + A.off[PG_GD_LN1_W], P + A.off[PG_GD_LN1_B], a, C, A.eps, tid, lane);
    __syncthreads();
    int S = gd_matvec(P + A.off[PG_GD_WQKV], C, 3 * C, a, part, wave, lane);
    __syncthreads();
    for (int r = tid; r < 3 * C; r += GD_THREADS) {
      const float v = gd_combine(part, S, 3 * C, r, P[A.off[PG_GD_BQKV] + r]);
      qkv[r] = v;
      if (r >= 2 * C) vcn[(size_t)(r - 2 * C) * L + p] = v;  // the only cache entries this launch writes: column p
      else if (r >= C) kcn[(size_t)(r - C) * L + p] = v;
    }
    __syncthreads();

    // attention, one head at a time over the whole workgroup; the position's own k / v come from LDS, never from the cache
    if (p == 0 && !self) {
      if (tid < C) a[tid] = 0.f;  // no key admitted
    } else {
      for (int hd = 0; hd < A.heads; ++hd) {
        const float* qh = qkv + hd * dk;
        const float* kh = qkv + C + hd * dk;
        const float* vh = qkv + 2 * C + hd * dk;
        const float* kp = kcn + (size_t)hd * dk * L;
        const float* vp = vcn + (size_t)hd * dk * L;
        const bool mine = self && tid == (p & (GD_THREADS - 1));  // owner of key p: after its cached keys, in ascending j
        float lmax = -1.0e30f;
        // scores of the cached keys, lanes over j: 4 keys x 8 head channels = 32 cache loads in flight per thread (the
        // loop is a chain of memory latencies); lanes past p and channels past dk re-read a valid entry with weight 0.
        // A key's score is one chain over d in ascending order.
        for (int j0 = tid; j0 < p; j0 += GD_JU * GD_THREADS) {
          int jj[GD_JU];
          float s[GD_JU];
#pragma unroll
          for (int u = 0; u < GD_JU; ++u) {
            jj[u] = min(j0 + u * GD_THREADS, p - 1);
            s[u] = 0.f;
          }
          for (int d0 = 0; d0 < dk; d0 += GD_DU) {
            float kv[GD_JU][GD_DU];
#pragma unroll
            for (int e = 0; e < GD_DU; ++e) {
              const float* kd = kp + (size_t)min(d0 + e, dk - 1) * L;
#pragma unroll
              for (int u = 0; u < GD_JU; ++u) kv[u][e] = kd[jj[u]];
            }
#pragma unroll
            for (int e = 0; e < GD_DU; ++e) {
              const float qv = d0 + e < dk ? qh[min(d0 + e, dk - 1)] : 0.f;
#pragma unroll
              for (int u = 0; u < GD_JU; ++u) s[u] = fmaf(qv, kv[u][e], s[u]);
            }
          }
#pragma unroll
          for (int u = 0; u < GD_JU; ++u) {
            const int j = j0 + u * GD_THREADS;
            if (j < p) {
              const float sv = s[u] * A.scale2;
              sc[j] = sv;
              lmax = fmaxf(lmax, sv);
            }
          }
        }
        if (mine) {
          float s = 0.f;
          for (int d = 0; d < dk; ++d) s = fmaf(qh[d], kh[d], s);
          s *= A.scale2;
          sc[p] = s;
          lmax = fmaxf(lmax, s);
        }
        lmax = gd_wave_max(lmax);
        if (lane == 0) red[wave] = lmax;
        __syncthreads();
        const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float lsum = 0.f;
        for (int j = tid; j < p; j += GD_THREADS) {  // each thread revisits the scores it wrote itself
          const float e = __builtin_amdgcn_exp2f(sc[j] - m);
          sc[j] = e;
          lsum += e;
        }
        if (mine) {
          const float e = __builtin_amdgcn_exp2f(sc[p] - m);
          sc[p] = e;
          lsum += e;
        }
        lsum = pg_wave_sum(lsum);
        if (lane == 0) red[GD_WAVES + wave] = lsum;
        __syncthreads();
        const float inv = 1.f / (((red[4] + red[5]) + red[6]) + red[7]);  // >= 1 term equal to 1: never 0
        // o[c] = sum_j P_j v[c][j], lanes over j, a wave reduction per channel: wave w takes channels w, w + 4, w + 8, ...,
        // four of them x 8 strides of j = 32 cache loads in flight per lane; each (channel, lane) sum is one chain in
        // ascending j, the position's own value (from LDS) last.
        for (int c0 = wave; c0 < dk; c0 += GD_CU * GD_WAVES) {
          float acc[GD_CU];
#pragma unroll
          for (int u = 0; u < GD_CU; ++u) acc[u] = 0.f;
          for (int j0 = lane; j0 < p; j0 += GD_DU * 64) {
            float vv[GD_CU][GD_DU], pv[GD_DU];
#pragma unroll
            for (int e = 0; e < GD_DU; ++e) {
              const int j = j0 + e * 64;
              const int jc = min(j, p - 1);
              pv[e] = j < p ? sc[jc] : 0.f;
#pragma unroll
              for (int u = 0; u < GD_CU; ++u) vv[u][e] = vp[(size_t)min(c0 + u * GD_WAVES, dk - 1) * L + jc];
            }
#pragma unroll
            for (int e = 0; e < GD_DU; ++e)
#pragma unroll
              for (int u = 0; u < GD_CU; ++u) acc[u] = fmaf(pv[e], vv[u][e], acc[u]);
          }
#pragma unroll
          for (int u = 0; u < GD_CU; ++u) {
            const int c = c0 + u * GD_WAVES;  // wave-uniform
            if (c < dk) {
              float t = acc[u];
              if (self && lane == (p & 63)) t = fmaf(sc[p], vh[c], t);
              t = pg_wave_sum(t);
              if (lane == 0) a[hd * dk + c] = t * inv;
            }
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();

    S = gd_matvec(P + A.off[PG_GD_WPROJ], C, C, a, part, wave, lane);
    __syncthreads();
    if (tid < C) bres[tid] = h[tid] + gd_combine(part, S, C, tid, P[A.off[PG_GD_BPROJ] + tid]);
    __syncthreads();
    gd_layernorm(bres, P + A.off[PG_GD_LN2_W], P + A.off[PG_GD_LN2_B], a, C, A.eps, tid, lane);
    __syncthreads();
    S = gd_matvec(P + A.off[PG_GD_W1], C, 4 * C, a, part, wave, lane);
    __syncthreads();
    for (int r = tid; r < 4 * C; r += GD_THREADS) hid[r] = pg_gelu(gd_combine(part, S, 4 * C, r, P[A.off[PG_GD_B1] + r]));
    __syncthreads();
    S = gd_matvec(P + A.off[PG_GD_W2], 4 * C, C, hid, part, wave, lane);
    __syncthreads();
    if (tid < C) h[tid] = h[tid] + (bres[tid] + gd_combine(part, S, C, tid, P[A.off[PG_GD_B2] + tid]));
    __syncthreads();
  }
  if (tid < C) A.out[(size_t)tid * A.ld + n] = h[tid];
}

}  // namespace

PG_EXPORT int pg_gpt_decode_plan(int C, int heads, int blocks, int L, int* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_GPT_DECODE_PLAN_INTS, PG_EINVAL, "pg_gpt_decode_plan: null pointer or short output array");
  GdPlan pl;
  const int rc = gd_plan(C, heads, blocks, L, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  PG_REQUIRE(pl.pack_floats < (1L << 31), PG_ESHAPE, "pg_gpt_decode_plan: pack too large");
  out[0] = (int)pl.pack_floats;
  out[1] = pl.block_floats;
  out[2] = pl.lds_bytes;
  out[3] = GD_THREADS;
  for (int f = 0; f < PG_GPT_DECODE_FIELDS; ++f) out[4 + f] = pl.off[f];
  return 0;
}

PG_EXPORT int pg_gpt_decode_step(const float* x, float* out, const float* pack, float* k_cache, float* v_cache, int N,
                                 int C, int heads, int blocks, int L, int ld, int p, int strict, float eps,
                                 const int* pos_dev, void* stream) {
  PG_REQUIRE(x && out && pack && k_cache && v_cache, PG_EINVAL, "pg_gpt_decode_step: null pointer");
  PG_REQUIRE(N > 0 && ld >= N, PG_EINVAL, "pg_gpt_decode_step: bad dims");
  PG_REQUIRE(strict == 0 || strict == 1, PG_EINVAL, "pg_gpt_decode_step: strict must be 0/1");
  PG_REQUIRE(eps > 0.f, PG_EINVAL, "pg_gpt_decode_step: eps must be positive");
  GdPlan pl;
  const int rc = gd_plan(C, heads, blocks, L, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  PG_REQUIRE(p >= 0 && p < L, PG_EINVAL, "pg_gpt_decode_step: position outside the sequence");
  GdArgs A;
  A.x = x; A.out = out; A.pack = pack; A.kc = k_cache; A.vc = v_cache; A.pos_dev = pos_dev;
  A.N = N; A.C = C; A.heads = heads; A.blocks = blocks; A.L = L; A.ld = ld; A.p = p; A.strict = strict;
  A.block_floats = pl.block_floats; A.part_floats = pl.part_floats;
  for (int f = 0; f < PG_GPT_DECODE_FIELDS; ++f) A.off[f] = pl.off[f];
  A.eps = eps;
  A.scale2 = 1.44269504088896340736f / sqrtf((float)(C / heads));
  hipLaunchKernelGGL(gpt_decode_step_kernel, dim3((unsigned)N), dim3(GD_THREADS), (size_t)pl.lds_bytes,
                     (hipStream_t)stream, A);
  PG_LAUNCH_CHECK("pg_gpt_decode_step");
  return 0;
}
