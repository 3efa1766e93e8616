// nade.hip — NADE (reference models/autoregressive/nade.py:42-68) as a chunked prefix scan, forward and backward, all fp32.
//
// Per sample n: a_0 = in_b; l_i = h_b[i] + relu(a_i) . h_W[i, :]; p_i = sigmoid(l_i); a_{i+1} = a_i + x_i in_W[:, i]. The ReLU sits
// between the prefix sum and the dot product, so this is no GEMM; the reference walks the D dimensions in a Python loop. Here the
// scan over D is cut into chunks of NA_T dimensions:
//   * nade_ckpt_kernel forms the pre-activations at the chunk starts, A_c = in_b + X[:, :cT] in_W[:, :cT]^T, by the recurrence's
//     own sequence of fused multiply-adds (one thread per (sample, unit), j ascending), and writes them as (chunks, N, Hp): the
//     CHECKPOINTS the backward starts from;
//   * nade_scan_fwd_kernel: one workgroup per (tile of 64 samples, chunk). Lanes run over samples, a wave keeps `a` of NA_U hidden
//     units in registers and walks the chunk: per step and unit one max, one fma into the logit, one fma into `a`, the two weight
//     values wave-uniform LDS broadcast reads. The four waves take interleaved slabs of NA_U units until H is covered; a logit is
//     the sum over a wave's units in ascending order, then over the four waves in order: fixed by H alone, so a sample's row is
//     bit-identical from run to run, for any N and any slot of its tile;
//   * the backward turns the arrangement round, because every gradient is a sum over samples: lanes run over hidden units, a
//     thread keeps the chunk's two weight rows and both gradient rows of its unit in registers and takes the samples of its
//     partial row one after the other (delta and x of a sample tile are wave-uniform LDS reads), so no sum crosses lanes.
//     nade_bwd_chunk_kernel recomputes a_i from the checkpoint by the forward's own fmaf sequence (the ReLU mask is the forward's
//     bit for bit; nothing is recovered by subtraction), keeps the chunk's mask bits in one register, accumulates d_h_W, walks the
//     chunk backwards for S_j and the in-chunk part of d_in_W, and writes the chunk total of e per (sample, unit);
//     nade_suffix_kernel turns the chunk totals into inclusive suffix sums over chunks (c descending); nade_bwd_cross_kernel adds
//     the cross-chunk term X_c^T E_{>c} of d_in_W and forms d_in_b from E_{>=0};
//   * sums over samples: a workgroup owns one of at most NA_MAX_ROWS partial rows and loops over the sample tiles r, r + R, ...
//     of its row; nade_merge_kernel adds the rows in order into the gradients. Every order depends on the shape alone: no float
//     atomics, gradients bit-identical from run to run. No host synchronisation, no allocation: the step captures into a hipGraph.
#include "common.h"

namespace {

constexpr int NA_T = 32;          // chunk length over D: the mask bits of a chunk are one 32-bit register per unit
constexpr int NA_U = 16;          // hidden units a forward thread keeps in registers
constexpr int NA_WAVES = 4;       // waves of a forward workgroup: interleaved slabs of NA_U units
constexpr int NA_SLAB = NA_U * NA_WAVES;  // hidden units a forward workgroup covers per pass; Hp is a multiple of it
constexpr int NA_TILE = 64;       // samples per forward workgroup (lanes)
constexpr int NA_CK_TILE = 16;    // samples per checkpoint workgroup
constexpr int NA_BT = 16;         // samples per backward tile
constexpr int NA_BH = 256;        // hidden units (threads) per backward workgroup
constexpr int NA_MAX_ROWS = 16;   // cap of the partial rows of the sums over samples
constexpr int NA_MAX_H = 8192;

// The one function that decides the domain and the geometry: pg_nade_plan reports it, every launch goes by it.
struct NaPlan {
  int chunks, hp, dp, tiles, btiles, rows, hblocks;
  long fwd_groups, ckpt_groups, bwd_groups, ckpt_floats, ws_floats;
  char msg[160];
};

#define NA_REQUIRE(cond, code, ...)                  \
  do {                                               \
    if (!(cond)) {                                   \
      snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__); \
      return (code);                                 \
    }                                                \
  } while (0)

int na_plan(int D, int H, int N, NaPlan& pl) {
  pl.msg[0] = 0;
  NA_REQUIRE(D > 0 && H > 0 && N > 0, PG_EINVAL, "pg_nade: non-positive dimension");
  NA_REQUIRE(H <= NA_MAX_H, PG_ESHAPE, "pg_nade: %d hidden units unsupported (at most %d)", H, NA_MAX_H);
  pl.chunks = pg_cdiv(D, NA_T);
  pl.dp = pl.chunks * NA_T;
  pl.hp = pg_cdiv(H, NA_SLAB) * NA_SLAB;
  pl.tiles = pg_cdiv(N, NA_TILE);
  pl.btiles = pg_cdiv(N, NA_BT);
  pl.rows = pl.btiles < NA_MAX_ROWS ? pl.btiles : NA_MAX_ROWS;
  pl.hblocks = pg_cdiv(pl.hp, NA_BH);
  pl.fwd_groups = (long)pl.tiles * pl.chunks;
  pl.ckpt_groups = (long)pg_cdiv(N, NA_CK_TILE) * (pl.hp / 64);
  pl.bwd_groups = (long)pl.hblocks * pl.chunks * pl.rows;
  const long lim = (1L << 31) - 1;
  NA_REQUIRE(pl.fwd_groups <= lim && pl.ckpt_groups <= lim && pl.bwd_groups <= lim && (long)N * pl.hp / 256 < lim &&
                 2L * D * H + D + H < (1L << 40),
             PG_ESHAPE, "pg_nade: N = %d, D = %d, H = %d is too large for one launch", N, D, H);
  pl.ckpt_floats = (long)pl.chunks * N * pl.hp;
  pl.ws_floats = (long)pl.rows * (2L * pl.dp * pl.hp + pl.dp + pl.hp);
  return 0;
}

// workspace: [rows][dp][hp] d_h_W | [rows][hp][dp] d_in_W | [rows][dp] d_h_b | [rows][hp] d_in_b
struct NaWs {
  float *w2, *w1, *b2, *b1;
};
NaWs na_ws(float* ws, const NaPlan& pl) {
  NaWs w;
  w.w2 = ws;
  w.w1 = w.w2 + (size_t)pl.rows * pl.dp * pl.hp;
  w.b2 = w.w1 + (size_t)pl.rows * pl.dp * pl.hp;
  w.b1 = w.b2 + (size_t)pl.rows * pl.dp;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Checkpoints: ckpt[c][n][h] = in_b[h] + sum_{j < c T} x[n][j] in_W[h][j], j ascending, one fmaf per term (the recurrence's own
// sequence). Lanes over 64 hidden units, a wave owns 4 of the tile's 16 samples; in_W and x tiles of a chunk go through LDS.
__global__ void __launch_bounds__(256) nade_ckpt_kernel(const float* __restrict__ x, const float* __restrict__ in_w,
                                                        const float* __restrict__ in_b, float* __restrict__ ckpt, int N, int D,
                                                        int H, int hp, int chunks) {
  __shared__ float ws[NA_T][65];
  __shared__ float xs[NA_CK_TILE][NA_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hblocks = hp / 64;
  const int h0 = (blockIdx.x % hblocks) * 64, n0 = (blockIdx.x / hblocks) * NA_CK_TILE;
  const int h = h0 + lane;
  float a[4];
  const float b = h < H ? in_b[h] : 0.f;  // padded units: a = 0 throughout
#pragma unroll
  for (int s = 0; s < 4; ++s) a[s] = b;
  for (int c = 0;; ++c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = n0 + wave * 4 + s;
      if (n < N) ckpt[((size_t)c * N + n) * hp + h] = a[s];
    }
    if (c == chunks - 1) break;  // the sum over the last chunk is never a chunk start
    const int j0 = c * NA_T;     // a full chunk: j0 + NA_T <= D
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 64 * NA_T / 256; ++k) {
      const int idx = k * 256 + tid, hh = idx / NA_T, j = idx % NA_T;
      ws[j][hh] = h0 + hh < H ? in_w[(size_t)(h0 + hh) * D + j0 + j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NA_CK_TILE * NA_T / 256; ++k) {
      const int idx = k * 256 + tid, s = idx / NA_T, j = idx % NA_T;
      xs[s][j] = n0 + s < N ? x[(size_t)(n0 + s) * D + j0 + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NA_T; ++j) {
      const float w = ws[j][lane];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = fmaf(xs[wave * 4 + s][j], w, a[s]);
    }
  }
}

// numerically safe sigmoid: e = exp(-|l|) <= 1
__device__ __forceinline__ float na_sigmoid(float l) {
  const float e = __expf(-fabsf(l));
  const float r = 1.f / (1.f + e);
  return l >= 0.f ? r : e * r;
}
// sigmoid'(l) = p (1 - p) without forming 1 - p
__device__ __forceinline__ float na_dsigmoid(float l) {
  const float e = __expf(-fabsf(l));
  const float r = 1.f / (1.f + e);
  return e * r * r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Forward scan of one chunk for one tile of 64 samples (lanes). blockIdx.x = tile * chunks + chunk.
__global__ void __launch_bounds__(64 * NA_WAVES) nade_scan_fwd_kernel(const float* __restrict__ x, const float* __restrict__ in_w,
                                                                      const float* __restrict__ h_w, const float* __restrict__ h_b,
                                                                      const float* __restrict__ ckpt, float* __restrict__ probs,
                                                                      float* __restrict__ logits, int N, int D, int H, int hp,
                                                                      int chunks) {
  __shared__ __attribute__((aligned(16))) float w2s[NA_WAVES][NA_T][NA_U];  // h_W[i0 + i][unit]
  __shared__ __attribute__((aligned(16))) float w1s[NA_WAVES][NA_T][NA_U];  // in_W[unit][i0 + i]
  __shared__ float red[NA_WAVES][NA_T][NA_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x % chunks, tile = blockIdx.x / chunks;
  const int i0 = c * NA_T;
  const int n = tile * NA_TILE + lane;
  const int nr = n < N ? n : N - 1;  // a lane past N recomputes the last sample and writes nothing
  float xr[NA_T], acc[NA_T];
#pragma unroll
  for (int i = 0; i < NA_T; ++i) {
    xr[i] = i0 + i < D ? x[(size_t)nr * D + i0 + i] : 0.f;
    acc[i] = 0.f;
  }
  const float* __restrict__ arow = ckpt + ((size_t)c * N + nr) * hp;
  for (int s0 = 0; s0 < hp; s0 += NA_SLAB) {
    __syncthreads();  // the previous pass's reads of the weight tiles
#pragma unroll
    for (int k = 0; k < NA_T * NA_SLAB / 256; ++k) {
      const int idx = k * 256 + tid;
      {  // h_W: consecutive threads along h
        const int i = idx / NA_SLAB, hh = idx % NA_SLAB, h = s0 + hh;
        w2s[hh / NA_U][i][hh % NA_U] = (h < H && i0 + i < D) ? h_w[(size_t)(i0 + i) * H + h] : 0.f;
      }
      {  // in_W: consecutive threads along i
        const int hh = idx / NA_T, i = idx % NA_T, h = s0 + hh;
        w1s[hh / NA_U][i][hh % NA_U] = (h < H && i0 + i < D) ? in_w[(size_t)h * D + i0 + i] : 0.f;
      }
    }
    __syncthreads();
    float a[NA_U];
    const float4* __restrict__ ap = reinterpret_cast<const float4*>(arow + s0 + wave * NA_U);
#pragma unroll
    for (int q = 0; q < NA_U / 4; ++q) {
      const float4 f = ap[q];
      a[4 * q] = f.x; a[4 * q + 1] = f.y; a[4 * q + 2] = f.z; a[4 * q + 3] = f.w;
    }
#pragma unroll
    for (int i = 0; i < NA_T; ++i) {
      float part = 0.f;
#pragma unroll
      for (int u = 0; u < NA_U; ++u) part = fmaf(fmaxf(a[u], 0.f), w2s[wave][i][u], part);
      acc[i] += part;
#pragma unroll
      for (int u = 0; u < NA_U; ++u) a[u] = fmaf(xr[i], w1s[wave][i][u], a[u]);
    }
  }
#pragma unroll
  for (int i = 0; i < NA_T; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
  if (n < N) {
    for (int i = wave; i < NA_T && i0 + i < D; i += NA_WAVES) {
      const float l = h_b[i0 + i] + (((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane]);
      const size_t o = (size_t)n * D + i0 + i;
      logits[o] = l;
      probs[o] = na_sigmoid(l);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Backward of one chunk for one partial row. blockIdx.x = (row * chunks + chunk) * hblocks + hblock; thread = hidden unit.
__global__ void __launch_bounds__(NA_BH) nade_bwd_chunk_kernel(const float* __restrict__ x, const float* __restrict__ in_w,
                                                               const float* __restrict__ h_w, const float* __restrict__ logits,
                                                               const float* __restrict__ g, const float* __restrict__ ckpt,
                                                               float* __restrict__ etot, float* __restrict__ pw2,
                                                               float* __restrict__ pw1, float* __restrict__ pb2, int N, int D,
                                                               int H, int hp, int dp, int chunks, int hblocks, int rows,
                                                               int btiles) {
  __shared__ __attribute__((aligned(16))) float dl[NA_BT][NA_T];  // delta[n][i0 + i] = G sigmoid'(l)
  __shared__ __attribute__((aligned(16))) float xs[NA_BT][NA_T];
  const int tid = threadIdx.x;
  const int hblock = blockIdx.x % hblocks, c = (blockIdx.x / hblocks) % chunks, row = blockIdx.x / (hblocks * chunks);
  const int i0 = c * NA_T;
  const int h = hblock * NA_BH + tid;
  const bool live = h < hp;
  const int hr = live ? h : hp - 1;
  float w2[NA_T], w1[NA_T], dw2[NA_T], dw1[NA_T];
#pragma unroll
  for (int i = 0; i < NA_T; ++i) {
    const bool ok = hr < H && i0 + i < D;
    w2[i] = ok ? h_w[(size_t)(i0 + i) * H + hr] : 0.f;
    w1[i] = ok ? in_w[(size_t)hr * D + i0 + i] : 0.f;
    dw2[i] = 0.f;
    dw1[i] = 0.f;
  }
  float db2 = 0.f;  // threads 0 .. NA_T - 1 of hblock 0: sum over the row's samples of delta[:, i0 + tid]
  for (int t = row; t < btiles; t += rows) {
    const int n0 = t * NA_BT;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NA_BT * NA_T / NA_BH; ++k) {
      const int idx = k * NA_BH + tid, s = idx / NA_T, i = idx % NA_T;
      const bool ok = n0 + s < N && i0 + i < D;
      const size_t o = ok ? (size_t)(n0 + s) * D + i0 + i : 0;
      dl[s][i] = ok ? g[o] * na_dsigmoid(logits[o]) : 0.f;
      xs[s][i] = ok ? x[o] : 0.f;
    }
    __syncthreads();
    if (hblock == 0 && tid < NA_T) {
#pragma unroll
      for (int s = 0; s < NA_BT; ++s) db2 += dl[s][tid];  // samples past N hold 0
    }
    const int ns = N - n0 < NA_BT ? N - n0 : NA_BT;
    for (int s = 0; s < ns; ++s) {
      const size_t ai = ((size_t)c * N + n0 + s) * hp + hr;
      float a = ckpt[ai];
      unsigned mask = 0;
#pragma unroll
      for (int i = 0; i < NA_T; ++i) {
        dw2[i] = fmaf(dl[s][i], fmaxf(a, 0.f), dw2[i]);
        mask |= a > 0.f ? 1u << i : 0u;
        a = fmaf(xs[s][i], w1[i], a);  // the forward's own step
      }
      float S = 0.f;
#pragma unroll
      for (int j = NA_T - 1; j >= 0; --j) {
        dw1[j] = fmaf(xs[s][j], S, dw1[j]);
        S += (mask >> j) & 1u ? dl[s][j] * w2[j] : 0.f;
      }
      if (live) etot[ai] = S;
    }
  }
  if (live) {
    float* __restrict__ o2 = pw2 + ((size_t)row * dp + i0) * hp + h;
    float* __restrict__ o1 = pw1 + ((size_t)row * hp + h) * dp + i0;
#pragma unroll
    for (int i = 0; i < NA_T; ++i) {
      o2[(size_t)i * hp] = dw2[i];
      o1[i] = dw1[i];
    }
  }
  if (hblock == 0 && tid < NA_T) pb2[(size_t)row * dp + i0 + tid] = db2;
}

// etot[c] <- sum_{c' >= c} etot[c'], c descending: one thread per (sample, unit).
__global__ void __launch_bounds__(256) nade_suffix_kernel(float* __restrict__ etot, size_t per_chunk, int chunks) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per_chunk) return;
  float run = 0.f;
  for (int c = chunks - 1; c >= 0; --c) {
    run += etot[(size_t)c * per_chunk + idx];
    etot[(size_t)c * per_chunk + idx] = run;
  }
}

// pw1[row][h][i0 + j] += sum_n x[n][i0 + j] E_{> c}[n][h] over the row's samples; chunk 0 also forms the row's part of d_in_b.
// Same (row, chunk, hblock) -> thread mapping as nade_bwd_chunk_kernel, launched after it on the same stream.
__global__ void __launch_bounds__(NA_BH) nade_bwd_cross_kernel(const float* __restrict__ x, const float* __restrict__ einc,
                                                               float* __restrict__ pw1, float* __restrict__ pb1, int N, int D,
                                                               int hp, int dp, int chunks, int hblocks, int rows, int btiles) {
  __shared__ __attribute__((aligned(16))) float xs[NA_BT][NA_T];
  const int tid = threadIdx.x;
  const int hblock = blockIdx.x % hblocks, c = (blockIdx.x / hblocks) % chunks, row = blockIdx.x / (hblocks * chunks);
  const bool cross = c + 1 < chunks;
  if (!cross && c != 0) return;  // the last chunk has no later one
  const int i0 = c * NA_T;
  const int h = hblock * NA_BH + tid;
  const bool live = h < hp;
  const int hr = live ? h : hp - 1;
  float acc[NA_T];
#pragma unroll
  for (int j = 0; j < NA_T; ++j) acc[j] = 0.f;
  float db1 = 0.f;
  for (int t = row; t < btiles; t += rows) {
    const int n0 = t * NA_BT;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NA_BT * NA_T / NA_BH; ++k) {
      const int idx = k * NA_BH + tid, s = idx / NA_T, j = idx % NA_T;
      xs[s][j] = (n0 + s < N && i0 + j < D) ? x[(size_t)(n0 + s) * D + i0 + j] : 0.f;
    }
    __syncthreads();
    const int ns = N - n0 < NA_BT ? N - n0 : NA_BT;
    for (int s = 0; s < ns; ++s) {
      const size_t at = (size_t)(n0 + s) * hp + hr;
      if (c == 0) db1 += einc[at];
      if (cross) {
        const float e = einc[(size_t)(c + 1) * N * hp + at];
#pragma unroll
        for (int j = 0; j < NA_T; ++j) acc[j] = fmaf(xs[s][j], e, acc[j]);
      }
    }
  }
  if (live) {
    if (cross) {
      float* __restrict__ o1 = pw1 + ((size_t)row * hp + h) * dp + i0;
#pragma unroll
      for (int j = 0; j < NA_T; ++j) o1[j] += acc[j];
    }
    if (c == 0) pb1[(size_t)row * hp + h] = db1;
  }
}

// out += sum over the partial rows, in order. One thread per gradient element: d_h_W (D, H) | d_in_W (H, D) | d_h_b | d_in_b.
__global__ void __launch_bounds__(256) nade_merge_kernel(const float* __restrict__ pw2, const float* __restrict__ pw1,
                                                         const float* __restrict__ pb2, const float* __restrict__ pb1,
                                                         float* __restrict__ d_h_w, float* __restrict__ d_in_w,
                                                         float* __restrict__ d_h_b, float* __restrict__ d_in_b, int D, int H,
                                                         int hp, int dp, int rows) {
  const size_t dh = (size_t)D * H;
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float* __restrict__ src;
  float* dst;
  size_t stride;
  if (idx < dh) {
    src = pw2 + (idx / H) * hp + idx % H; stride = (size_t)dp * hp; dst = d_h_w ? d_h_w + idx : nullptr;
  } else if ((idx -= dh) < dh) {
    src = pw1 + (idx / D) * dp + idx % D; stride = (size_t)hp * dp; dst = d_in_w ? d_in_w + idx : nullptr;
  } else if ((idx -= dh) < (size_t)D) {
    src = pb2 + idx; stride = dp; dst = d_h_b ? d_h_b + idx : nullptr;
  } else if ((idx -= D) < (size_t)H) {
    src = pb1 + idx; stride = hp; dst = d_in_b ? d_in_b + idx : nullptr;
  } else {
    return;
  }
  if (!dst) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += src[(size_t)r * stride];
  *dst += s;
}

}  // namespace

PG_EXPORT int pg_nade_plan(int D, int H, int N, long long* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_NADE_PLAN_INTS, PG_EINVAL, "pg_nade_plan: null pointer or short output array");
  NaPlan pl;
  const int rc = na_plan(D, H, N, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  const long lds_fwd = (long)sizeof(float) * (2 * NA_WAVES * NA_T * NA_U + NA_WAVES * NA_T * NA_TILE);
  out[0] = NA_T;
  out[1] = pl.chunks;
  out[2] = NA_U;
  out[3] = NA_TILE;
  out[4] = pl.hp;
  out[5] = pl.fwd_groups;
  out[6] = NA_BT;
  out[7] = pl.rows;
  out[8] = pg_cdiv(pl.btiles, pl.rows);  // sample tiles a backward workgroup loops over
  out[9] = pl.bwd_groups;
  out[10] = lds_fwd;  // the largest of the kernels
  out[11] = pl.ckpt_floats;
  out[12] = pl.ws_floats;
  out[13] = NA_MAX_ROWS;
  out[14] = NA_MAX_H;
  return 0;
}

PG_EXPORT int pg_nade_fwd(const float* x, const float* in_w, const float* in_b, const float* h_w, const float* h_b, float* ckpt,
                          float* probs, float* logits, int N, int D, int H, void* stream) {
  PG_REQUIRE(x && in_w && in_b && h_w && h_b && ckpt && probs && logits, PG_EINVAL, "pg_nade_fwd: null pointer");
  PG_REQUIRE((uintptr_t)ckpt % 16 == 0, PG_EINVAL, "pg_nade_fwd: the checkpoints must be 16-byte aligned");
  NaPlan pl;
  const int rc = na_plan(D, H, N, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nade_ckpt_kernel, dim3((unsigned)pl.ckpt_groups), dim3(256), 0, st, x, in_w, in_b, ckpt, N, D, H, pl.hp,
                     pl.chunks);
  PG_LAUNCH_CHECK("pg_nade_fwd");
  hipLaunchKernelGGL(nade_scan_fwd_kernel, dim3((unsigned)pl.fwd_groups), dim3(64 * NA_WAVES), 0, st, x, in_w, h_w, h_b, ckpt,
                     probs, logits, N, D, H, pl.hp, pl.chunks);
  PG_LAUNCH_CHECK("pg_nade_fwd");
  return 0;
}

PG_EXPORT int pg_nade_bwd(const float* x, const float* in_w, const float* h_w, const float* logits, const float* g,
                          const float* ckpt, float* etot, float* d_in_w, float* d_in_b, float* d_h_w, float* d_h_b, int N, int D,
                          int H, float* ws, size_t ws_floats, void* stream) {
  PG_REQUIRE(x && in_w && h_w && logits && g && ckpt && etot && ws, PG_EINVAL, "pg_nade_bwd: null pointer");
  NaPlan pl;
  const int rc = na_plan(D, H, N, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  PG_REQUIRE(ws_floats >= (size_t)pl.ws_floats, PG_EINVAL, "pg_nade_bwd: workspace of %zu floats, %ld needed", ws_floats,
             pl.ws_floats);
  const NaWs w = na_ws(ws, pl);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nade_bwd_chunk_kernel, dim3((unsigned)pl.bwd_groups), dim3(NA_BH), 0, st, x, in_w, h_w, logits, g, ckpt,
                     etot, w.w2, w.w1, w.b2, N, D, H, pl.hp, pl.dp, pl.chunks, pl.hblocks, pl.rows, pl.btiles);
  PG_LAUNCH_CHECK("pg_nade_bwd");
  const size_t per_chunk = (size_t)N * pl.hp;
  hipLaunchKernelGGL(nade_suffix_kernel, dim3((unsigned)((per_chunk + 255) / 256)), dim3(256), 0, st, etot, per_chunk,
                     pl.chunks);
  PG_LAUNCH_CHECK("pg_nade_bwd");
  hipLaunchKernelGGL(nade_bwd_cross_kernel, dim3((unsigned)pl.bwd_groups), dim3(NA_BH), 0, st, x, etot, w.w1, w.b1, N, D, pl.hp,
                     pl.dp, pl.chunks, pl.hblocks, pl.rows, pl.btiles);
  PG_LAUNCH_CHECK("pg_nade_bwd");
  const size_t total = 2 * (size_t)D * H + D + H;
  hipLaunchKernelGGL(nade_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w.w2, w.w1, w.b2, w.b1, d_h_w,
                     d_in_w, d_h_b, d_in_b, D, H, pl.hp, pl.dp, pl.rows);
  PG_LAUNCH_CHECK("pg_nade_bwd");
  return 0;
}
