// dense_linear.hip — dense linear layers on large-tile fp32-MFMA GEMMs, and the two streaming kernel pairs of NICE (reference
// models/flow/nice.py): the diagonal scaling layer and the logistic prior.
//
// One tiled kernel computes C[r][c] = sum_k A(r, k) B(c, k) for the three products of a linear layer
// (x: (N, in) with row stride ldx, w: (out, in) dense, y / dy: (N, out) with their row strides):
//   forward   y  = act(x w^T + b)  or  res + sign (x w^T + b)      rows n, cols o, k = i   (A = x, B = w: both k-contiguous)
//   data grad dx = sign (dy w) [* (relu_out > 0)] [+ addend]       rows n, cols i, k = o   (A = dy k-contiguous, B = w row-contiguous)
//   wgrad     dw += sign dy^T x, db += sign sum_n dy                rows o, cols i, k = n   (A = dy^T, B = x^T: both row-contiguous)
// Every activation operand takes a row stride in floats, so a coupling block reads one half of an (N, F) tensor and writes the
// other half of another with no copy.
//
// The tile, in its small (64 x 64) and large (128 x 128) variants, its LDS strides and the fmaf-chain order of every sum are
// mfma_tile.h's; this file adds the operand addressing, the bias row sum and the epilogue. Of the LDS accesses that are not
// conflict free there, the row-contiguous staging stores are the data gradient's weight and both operands of the weight
// gradient, the row walk is the bias sum. dl_plan is the one function that decides the domain, the variant and the k-split:
// the large tile where it alone fills three quarters of the 256 CUs, else the small one, split along k where even that leaves
// half the chip idle.
// A k-split writes raw partial sums to a caller-provided workspace; dl_reduce_kernel adds the slices in slice order and applies
// the epilogue. Each output element is owned by one lane; no float atomics; every order depends on the shape alone, so results
// are bit-identical from run to run. No host synchronisation, no allocation: capturable. Ragged edges are zero-filled on load
// and guarded on store.
#include <algorithm>

#include "common.h"
#include "mfma_tile.h"

namespace {

enum { DL_FWD = PG_DENSE_FWD, DL_DGRAD = PG_DENSE_DGRAD, DL_WGRAD = PG_DENSE_WGRAD };
enum { DL_SMALL = pg_tile::SMALL, DL_LARGE = pg_tile::LARGE };
template <int V>
using DlTile = pg_tile::Tile<V>;

constexpr int DL_THREADS = pg_tile::THREADS;
constexpr int DL_CUS = 256;           // workgroups that fill the chip
constexpr int DL_LARGE_MIN = 192;     // large tiles from which the large variant is taken
constexpr int DL_SPLIT_BELOW = 128;   // small tiles below which the k range is split
constexpr int DL_MAX_SLICES = 64;
constexpr int DL_MAX_DIM = 1 << 30;   // k offsets stay inside an int with a chunk to spare

struct DlArgs {
  const float* a;     // A(r, k) = a[r * a_rs + k * a_ks]
  const float* b;     // B(c, k) = b[c * b_rs + k * b_ks]
  const float* bias;  // + bias[c] (may be NULL)
  const float* gate;  // keep where gate[r * ldgate + c] > 0 (may be NULL)
  const float* add;   // + add[r * ldadd + c] behind the scale (may be NULL)
  float* c;           // C[r * ldc + c]
  float* db;          // weight gradient: db[r] += scale * sum_k A(r, k) (may be NULL)
  float* part;        // k-split: raw partial sums [slice][R][C], then the bias rows [slice][R]
  long a_rs, a_ks, b_rs, b_ks, ldgate, ldadd, ldc;
  int R, C, K, kper, slices, col_tiles, relu, accumulate;
  float scale;
};

// The epilogue of one finished sum: the same arithmetic whether the GEMM kernel or the k-split reduce applies it.
__device__ __forceinline__ void dl_finish(const DlArgs& p, int r, int c, float v) {
  if (p.bias) v += p.bias[c];
  if (p.relu) v = v > 0.f ? v : 0.f;
  if (p.gate && !(p.gate[(size_t)r * p.ldgate + c] > 0.f)) v = 0.f;
  v *= p.scale;  // +1 or -1: exact
  if (p.add) v += p.add[(size_t)r * p.ldadd + c];
  float* dst = p.c + (size_t)r * p.ldc + c;
  *dst = p.accumulate ? *dst + v : v;
}

template <int V, bool AK, bool BK>
__global__ void __launch_bounds__(DL_THREADS) dl_gemm_kernel(const DlArgs p) {
  using T = DlTile<V>;
  constexpr int BM = T::BM, BN = T::BN, KC = T::KC, LD = T::LD;
  __shared__ float s_a[BM * LD];
  __shared__ float s_b[BN * LD];
  const pg_tile::Lanes<V> ln;
  const int tid = ln.tid;
  const int r0 = (blockIdx.x / p.col_tiles) * BM, c0 = (blockIdx.x % p.col_tiles) * BN;
  const int kbeg = blockIdx.y * p.kper;
  const int kend = min(p.K, kbeg + p.kper);

  pg_tile::Regs<V> ra, rb;
  pg_tile::Acc<V> acc;
  pg_tile::zero<V>(acc);
  float dbsum = 0.f;  // weight gradient: thread tid < BM sums row tid of A in k order
  const bool do_db = p.db != nullptr && c0 == 0;
  auto load = [&](int ch) {
    pg_tile::load_operand<V, AK>(ra, p.a, p.a_rs, p.a_ks, r0, p.R, kbeg + ch * KC, kend, tid);
    pg_tile::load_operand<V, BK>(rb, p.b, p.b_rs, p.b_ks, c0, p.C, kbeg + ch * KC, kend, tid);
  };
  auto store = [&]() {
    pg_tile::store_operand<V, AK>(s_a, ra, tid);
    pg_tile::store_operand<V, BK>(s_b, rb, tid);
  };
  auto bias_sum = [&](int) {
    if (do_db && tid < BM) {
      const float* row = s_a + tid * LD;
#pragma unroll
      for (int k = 0; k < KC; ++k) dbsum += row[k];  // zero beyond the slice
    }
  };
  PG_TILE_PIPELINE(V, false, 0, (kend - kbeg + KC - 1) / KC, load, store, acc, s_a, s_b, ln, bias_sum);  // dl_plan: every slice holds a chunk
  if (do_db && tid < BM && r0 + tid < p.R) {
    if (p.part)
      p.part[(size_t)p.slices * p.R * p.C + (size_t)blockIdx.y * p.R + r0 + tid] = dbsum;
    else
      p.db[r0 + tid] += p.scale * dbsum;
  }

  PG_TILE_FOR_EACH_OUTPUT(V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (gc >= p.C || gr >= p.R) continue;
    if (p.part)
      p.part[((size_t)blockIdx.y * p.R + gr) * p.C + gc] = PG_TILE_OUTPUT(acc);
    else
      dl_finish(p, gr, gc, PG_TILE_OUTPUT(acc));
  }
}

// k-split epilogue: the slices' partial sums in slice order, then the epilogue; behind the R * C outputs, the R bias sums.
__global__ void __launch_bounds__(256) dl_reduce_kernel(const DlArgs p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.R * p.C;
  if (e < total) {
    float v = 0.f;
    for (int z = 0; z < p.slices; ++z) v += p.part[(size_t)z * total + e];
    dl_finish(p, (int)(e / p.C), (int)(e % p.C), v);
  } else if (p.db && e - total < (size_t)p.R) {
    const size_t r = e - total;
    float v = 0.f;
    for (int z = 0; z < p.slices; ++z) v += p.part[(size_t)p.slices * total + (size_t)z * p.R + r];
    p.db[r] += p.scale * v;
  }
}

// The one function that decides the domain, the tile variant, the k-split and the workspace: pg_dense_linear_plan reports it,
// every launch goes by it.
struct DlPlan {
  int R, C, K, variant, bm, bn, kc, row_tiles, col_tiles, slices, kper;
  long groups, reduce_groups, ws_floats;
  char msg[200];
};

#define DL_REQUIRE(cond, code, ...)                  \
  do {                                               \
    if (!(cond)) {                                   \
      snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__); \
      return (code);                                 \
    }                                                \
  } while (0)

int dl_plan(int N, int in, int out, int kind, DlPlan& pl) {
  pl.msg[0] = 0;
  DL_REQUIRE(kind == DL_FWD || kind == DL_DGRAD || kind == DL_WGRAD, PG_EINVAL, "pg_dense_linear: kind %d is none of forward, data gradient, weight gradient", kind);
  DL_REQUIRE(N >= 1 && in >= 1 && out >= 1, PG_ESHAPE, "pg_dense_linear: N = %d, in = %d, out = %d must all be >= 1", N, in, out);
  DL_REQUIRE(N <= DL_MAX_DIM && in <= DL_MAX_DIM && out <= DL_MAX_DIM, PG_ESHAPE,
             "pg_dense_linear: N = %d, in = %d, out = %d is too large for one launch (at most 2^30 each)", N, in, out);
  pl.R = kind == DL_WGRAD ? out : N;
  pl.C = kind == DL_FWD ? out : in;
  pl.K = kind == DL_FWD ? in : (kind == DL_DGRAD ? out : N);
  const long lim = (1L << 31) - 1;
  const long large = (long)pg_cdiv(pl.R, 128) * pg_cdiv(pl.C, 128);
  pl.variant = large >= DL_LARGE_MIN ? DL_LARGE : DL_SMALL;
  pl.bm = pl.bn = pl.variant == DL_LARGE ? 128 : 64;
  pl.kc = pl.variant == DL_LARGE ? DlTile<DL_LARGE>::KC : DlTile<DL_SMALL>::KC;
  pl.row_tiles = pg_cdiv(pl.R, pl.bm);
  pl.col_tiles = pg_cdiv(pl.C, pl.bn);
  const long tiles = (long)pl.row_tiles * pl.col_tiles;
  const int chunks = pg_cdiv(pl.K, pl.kc);
  int ks = 1;
  if (pl.variant == DL_SMALL && tiles < DL_SPLIT_BELOW && chunks >= 4)  // at least two chunks per slice
    ks = (int)std::min<long>(std::min<long>((DL_CUS + tiles - 1) / tiles, chunks / 2), DL_MAX_SLICES);
  pl.kper = pg_cdiv(chunks, ks) * pl.kc;
  pl.slices = pg_cdiv(pl.K, pl.kper);
  pl.groups = tiles * pl.slices;
  const long cells = (long)pl.R * pl.C + (kind == DL_WGRAD ? pl.R : 0);
  pl.ws_floats = pl.slices > 1 ? pl.slices * cells : 0;
  pl.reduce_groups = pl.slices > 1 ? (cells + 255) / 256 : 0;
  DL_REQUIRE(tiles <= lim && pl.reduce_groups <= lim, PG_ESHAPE, "pg_dense_linear: N = %d, in = %d, out = %d is too large for one launch", N, in,
             out);
  return 0;
}

DlArgs dl_args(const DlPlan& pl) {
  DlArgs p;
  p.a = p.b = p.bias = p.gate = p.add = nullptr;
  p.c = p.db = p.part = nullptr;
  p.a_rs = p.a_ks = p.b_rs = p.b_ks = p.ldgate = p.ldadd = p.ldc = 0;
  p.R = pl.R;
  p.C = pl.C;
  p.K = pl.K;
  p.kper = pl.kper;
  p.slices = pl.slices;
  p.col_tiles = pl.col_tiles;
  p.relu = p.accumulate = 0;
  p.scale = 1.f;
  return p;
}

template <bool AK, bool BK>
int dl_launch(const DlPlan& pl, DlArgs p, float* ws, size_t ws_floats, hipStream_t st, const char* name) {
  if (pl.slices > 1) {
    PG_REQUIRE(ws != nullptr && ws_floats >= (size_t)pl.ws_floats, PG_EINVAL, "%s: workspace of %zu floats, %ld needed (pg_dense_linear_plan)",
               name, ws_floats, pl.ws_floats);
    p.part = ws;
  }
  const dim3 grid((unsigned)((long)pl.row_tiles * pl.col_tiles), (unsigned)pl.slices);
  if (pl.variant == DL_LARGE)
    hipLaunchKernelGGL((dl_gemm_kernel<DL_LARGE, AK, BK>), grid, dim3(DL_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((dl_gemm_kernel<DL_SMALL, AK, BK>), grid, dim3(DL_THREADS), 0, st, p);
  PG_LAUNCH_CHECK(name);
  if (pl.slices > 1) {
    hipLaunchKernelGGL(dl_reduce_kernel, dim3((unsigned)pl.reduce_groups), dim3(256), 0, st, p);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

#define DL_PLAN_OR_RETURN(pl, N, in, out, kind) \
  DlPlan pl;                                    \
  {                                             \
    const int rc__ = dl_plan(N, in, out, kind, pl); \
    if (rc__) {                                 \
      pg_set_error("%s", pl.msg);               \
      return rc__;                              \
    }                                           \
  }

// ---------------------------------------------------------------------------------------------------------------------------
// NICE's scaling layer: z = y exp(sign s), s (F) broadcast over the N rows.
__global__ void __launch_bounds__(256) nice_scale_fwd_kernel(const float* __restrict__ y, const float* __restrict__ s,
                                                             float* __restrict__ z, size_t total, int F, float sign) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  z[e] = y[e] * expf(sign * s[e % F]);
}

constexpr int NS_ROW_SAMPLES = 16;  // samples of a partial row, before the cap
constexpr int NS_MAX_ROWS = 64;     // cap of the partial rows of the sum over samples

int ns_rows(int N) { return std::min(pg_cdiv(N, NS_ROW_SAMPLES), NS_MAX_ROWS); }

// dy = dz exp(sign s); part[row][j] = sum over the row's samples, n ascending, of dz[n][j] z[n][j]. blockIdx.y = partial row.
__global__ void __launch_bounds__(256) nice_scale_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ z,
                                                             const float* __restrict__ s, float* __restrict__ dy,
                                                             float* __restrict__ part, int N, int F, int per, float sign) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= F) return;
  const int nbeg = blockIdx.y * per, nend = min(N, nbeg + per);
  const float e = expf(sign * s[j]);
  float acc = 0.f;
  for (int n = nbeg; n < nend; ++n) {
    const size_t o = (size_t)n * F + j;
    const float g = dz[o];
    if (dy) dy[o] = g * e;
    acc = fmaf(g, z[o], acc);
  }
  part[(size_t)blockIdx.y * F + j] = acc;
}

// ds[j] += sign * (the partial rows in row order)
__global__ void __launch_bounds__(256) nice_scale_merge_kernel(const float* __restrict__ part, float* __restrict__ ds, int F, int rows,
                                                               float sign) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= F) return;
  float v = 0.f;
  for (int r = 0; r < rows; ++r) v += part[(size_t)r * F + j];
  ds[j] += sign * v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The logistic prior: log p(z) = -(softplus(z) + softplus(-z)) = -(|z| + 2 log1p(exp(-|z|))) per element, summed per sample.
// One workgroup per sample; a thread sums its features j = tid, tid + 256, ... in order, a wave by the butterfly, the four
// waves in wave order: fixed by F alone.
__global__ void __launch_bounds__(256) logistic_logprob_fwd_kernel(const float* __restrict__ z, float* __restrict__ lp, int F) {
  __shared__ float red[4];
  const float* __restrict__ row = z + (size_t)blockIdx.x * F;
  float acc = 0.f;
  for (int j = threadIdx.x; j < F; j += 256) {
    const float a = fabsf(row[j]);
    acc += a + 2.f * log1pf(expf(-a));
  }
  acc = pg_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) lp[blockIdx.x] = -(((red[0] + red[1]) + red[2]) + red[3]);
}

// dz = -g[n] tanh(z / 2), tanh(|z| / 2) = (1 - e) / (1 + e) with e = exp(-|z|) <= 1
__global__ void __launch_bounds__(256) logistic_logprob_bwd_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                                   float* __restrict__ dz, size_t total, int F) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const float v = z[e];
  const float ex = expf(-fabsf(v));
  const float t = (1.f - ex) / (1.f + ex);
  dz[e] = -g[e / F] * (v >= 0.f ? t : -t);
}

int nice_stream_check(const char* name, int N, int F) {
  PG_REQUIRE(N >= 1 && F >= 1, PG_ESHAPE, "%s: N = %d, F = %d must both be >= 1", name, N, F);
  PG_REQUIRE(((long)N * F + 255) / 256 <= (1L << 31) - 1, PG_ESHAPE, "%s: N = %d, F = %d is too large for one launch", name, N, F);
  return 0;
}

}  // namespace

PG_EXPORT int pg_dense_linear_plan(int N, int in, int out, int kind, long long* outv, int out_len) {
  PG_REQUIRE(outv && out_len >= PG_DENSE_PLAN_INTS, PG_EINVAL, "pg_dense_linear_plan: null pointer or short output array");
  DL_PLAN_OR_RETURN(pl, N, in, out, kind);
  outv[0] = pl.variant;
  outv[1] = pl.bm;
  outv[2] = pl.bn;
  outv[3] = pl.kc;
  outv[4] = pl.R;
  outv[5] = pl.C;
  outv[6] = pl.K;
  outv[7] = pl.row_tiles;
  outv[8] = pl.col_tiles;
  outv[9] = pl.slices;
  outv[10] = pl.kper;
  outv[11] = pl.groups;
  outv[12] = pl.reduce_groups;
  outv[13] = pl.ws_floats;
  return 0;
}

PG_EXPORT int pg_dense_linear_fwd(const float* x, long ldx, const float* w, const float* b, const float* res, long ldres, int sign,
                                  float* y, long ldy, int N, int in, int out, int relu, float* ws, size_t ws_floats, void* stream) {
  DL_PLAN_OR_RETURN(pl, N, in, out, DL_FWD);
  PG_REQUIRE(x && w && y, PG_EINVAL, "pg_dense_linear_fwd: null pointer");
  PG_REQUIRE(ldx >= in && ldy >= out && (!res || ldres >= out), PG_EINVAL, "pg_dense_linear_fwd: a row stride below its row length");
  PG_REQUIRE(!res || ((sign == 1 || sign == -1) && !relu), PG_EINVAL,
             "pg_dense_linear_fwd: the residual epilogue takes sign +1 or -1 and no ReLU");
  DlArgs p = dl_args(pl);
  p.a = x;
  p.a_rs = ldx;
  p.a_ks = 1;
  p.b = w;
  p.b_rs = in;
  p.b_ks = 1;
  p.bias = b;
  p.relu = relu != 0;
  p.add = res;
  p.ldadd = ldres;
  p.scale = res ? (float)sign : 1.f;
  p.c = y;
  p.ldc = ldy;
  return dl_launch<true, true>(pl, p, ws, ws_floats, (hipStream_t)stream, "pg_dense_linear_fwd");
}

PG_EXPORT int pg_dense_linear_dgrad(const float* dy, long lddy, const float* w, const float* relu_out, long ldrelu, const float* addend,
                                    long ldadd, int sign, float* dx, long lddx, int N, int in, int out, float* ws, size_t ws_floats,
                                    void* stream) {
  DL_PLAN_OR_RETURN(pl, N, in, out, DL_DGRAD);
  PG_REQUIRE(dy && w && dx, PG_EINVAL, "pg_dense_linear_dgrad: null pointer");
  PG_REQUIRE(lddy >= out && lddx >= in && (!relu_out || ldrelu >= in) && (!addend || ldadd >= in), PG_EINVAL,
             "pg_dense_linear_dgrad: a row stride below its row length");
  PG_REQUIRE(sign == 1 || sign == -1, PG_EINVAL, "pg_dense_linear_dgrad: sign must be +1 or -1");
  DlArgs p = dl_args(pl);
  p.a = dy;
  p.a_rs = lddy;
  p.a_ks = 1;
  p.b = w;  // B(c = i, k = o) = w[o * in + i]
  p.b_rs = 1;
  p.b_ks = in;
  p.gate = relu_out;
  p.ldgate = ldrelu;
  p.add = addend;
  p.ldadd = ldadd;
  p.scale = (float)sign;
  p.c = dx;
  p.ldc = lddx;
  return dl_launch<true, false>(pl, p, ws, ws_floats, (hipStream_t)stream, "pg_dense_linear_dgrad");
}

PG_EXPORT int pg_dense_linear_wgrad(const float* x, long ldx, const float* dy, long lddy, int sign, float* dw, float* db, int N, int in,
                                    int out, float* ws, size_t ws_floats, void* stream) {
  DL_PLAN_OR_RETURN(pl, N, in, out, DL_WGRAD);
  PG_REQUIRE(x && dy && dw, PG_EINVAL, "pg_dense_linear_wgrad: null pointer");
  PG_REQUIRE(ldx >= in && lddy >= out, PG_EINVAL, "pg_dense_linear_wgrad: a row stride below its row length");
  PG_REQUIRE(sign == 1 || sign == -1, PG_EINVAL, "pg_dense_linear_wgrad: sign must be +1 or -1");
  DlArgs p = dl_args(pl);
  p.a = dy;  // A(r = o, k = n) = dy[n * lddy + o]
  p.a_rs = 1;
  p.a_ks = lddy;
  p.b = x;  // B(c = i, k = n) = x[n * ldx + i]
  p.b_rs = 1;
  p.b_ks = ldx;
  p.scale = (float)sign;
  p.accumulate = 1;
  p.c = dw;
  p.ldc = in;
  p.db = db;
  return dl_launch<false, false>(pl, p, ws, ws_floats, (hipStream_t)stream, "pg_dense_linear_wgrad");
}

PG_EXPORT int pg_nice_scale_fwd(const float* y, const float* s, float* z, int N, int F, int sign, void* stream) {
  const int rc = nice_stream_check("pg_nice_scale_fwd", N, F);
  if (rc) return rc;
  PG_REQUIRE(y && s && z, PG_EINVAL, "pg_nice_scale_fwd: null pointer");
  PG_REQUIRE(sign == 1 || sign == -1, PG_EINVAL, "pg_nice_scale_fwd: sign must be +1 or -1");
  const size_t total = (size_t)N * F;
  hipLaunchKernelGGL(nice_scale_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, s, z, total, F,
                     (float)sign);
  PG_LAUNCH_CHECK("pg_nice_scale_fwd");
  return 0;
}

PG_EXPORT size_t pg_nice_scale_bwd_workspace_floats(int N, int F) {
  if (N < 1 || F < 1) return 0;
  return (size_t)ns_rows(N) * F;
}

PG_EXPORT int pg_nice_scale_bwd(const float* dz, const float* z, const float* s, float* dy, float* ds, int N, int F, int sign, float* ws,
                                size_t ws_floats, void* stream) {
  const int rc = nice_stream_check("pg_nice_scale_bwd", N, F);
  if (rc) return rc;
  PG_REQUIRE(dz && z && s && ws, PG_EINVAL, "pg_nice_scale_bwd: null pointer");
  PG_REQUIRE(sign == 1 || sign == -1, PG_EINVAL, "pg_nice_scale_bwd: sign must be +1 or -1");
  const int rows = ns_rows(N);
  PG_REQUIRE(ws_floats >= (size_t)rows * F, PG_EINVAL, "pg_nice_scale_bwd: workspace of %zu floats, %zu needed", ws_floats, (size_t)rows * F);
  const hipStream_t st = (hipStream_t)stream;
  const int per = pg_cdiv(N, rows);
  hipLaunchKernelGGL(nice_scale_bwd_kernel, dim3((unsigned)pg_cdiv(F, 256), (unsigned)rows), dim3(256), 0, st, dz, z, s, dy, ws, N, F, per,
                     (float)sign);
  PG_LAUNCH_CHECK("pg_nice_scale_bwd");
  if (ds) {
    hipLaunchKernelGGL(nice_scale_merge_kernel, dim3((unsigned)pg_cdiv(F, 256)), dim3(256), 0, st, ws, ds, F, rows, (float)sign);
    PG_LAUNCH_CHECK("pg_nice_scale_bwd");
  }
  return 0;
}

PG_EXPORT int pg_logistic_logprob_fwd(const float* z, float* lp, int N, int F, void* stream) {
  const int rc = nice_stream_check("pg_logistic_logprob_fwd", N, F);
  if (rc) return rc;
  PG_REQUIRE(z && lp, PG_EINVAL, "pg_logistic_logprob_fwd: null pointer");
  hipLaunchKernelGGL(logistic_logprob_fwd_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, z, lp, F);
  PG_LAUNCH_CHECK("pg_logistic_logprob_fwd");
  return 0;
}

PG_EXPORT int pg_logistic_logprob_bwd(const float* z, const float* g, float* dz, int N, int F, void* stream) {
  const int rc = nice_stream_check("pg_logistic_logprob_bwd", N, F);
  if (rc) return rc;
  PG_REQUIRE(z && g && dz, PG_EINVAL, "pg_logistic_logprob_bwd: null pointer");
  const size_t total = (size_t)N * F;
  hipLaunchKernelGGL(logistic_logprob_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, g, dz, total,
                     F);
  PG_LAUNCH_CHECK("pg_logistic_logprob_bwd");
  return 0;
}
