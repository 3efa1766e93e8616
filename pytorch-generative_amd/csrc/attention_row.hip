// attention_row.hip — the attention half of the row-cached sampler (PixelSNAIL): all W queries of image row r against
// K / V caches of the rows above plus the row's own keys, in one launch of a static shape.
//
//   o[x] = sum_j softmax_j(q[x] . k_j / sqrt(dk)) v_j   over   every cache key of rows y < r,  keys x' < x of row r,
//                                                             and x' == x unless mask_center
// The row's own k / v come from kv_row, never from the cache; with write_cache the launch also stores them into cache row r.
// No cache row >= r is read and no row but r is written, so a launch has no read / write overlap and the row index may come
// from a device int: the launch is the same for every row and can sit in one captured graph.
//
// VALU work (PixelSNAIL's dk is 4). A workgroup owns (sample, head, up to 32 queries of the row). The keys — the r W cached
// ones, then the row's own — pass through LDS in tiles of T keys that every query of the workgroup consumes:
//   score phase: a wave per query, lanes over the keys of the tile; tile maximum and sum by the xor butterfly, the running
//                (max, sum) of the query and the factor that rescales its accumulator are kept in LDS;
//   value phase: a thread per (query, 4 value channels), one chain over the keys of the tile in ascending order.
// The loads of tile t + 1 are issued into registers before the arithmetic of tile t and stored to LDS after it.
// No float atomics; every reduction has a fixed order and a workgroup sees one sample only: the output of sample n is
// bit-identical from run to run and whatever N is.
#include "common.h"

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_WAVES = AR_THREADS / 64;
constexpr int AR_MAX_DK = 64, AR_MAX_DV = 128, AR_MAX_W = 256, AR_MAX_HW = 4096, AR_MAX_GRID = 65535;
constexpr int AR_QB = 32;      // queries per workgroup
constexpr int AR_MAX_T = 128;  // keys per tile: at most two per lane in the score phase
constexpr int AR_PF = 32;      // tile elements a thread holds in registers while the previous tile is consumed
constexpr int AR_ITEMS = 4;    // (query, 4 value channels) accumulators per thread: AR_QB * (AR_MAX_DV / 4) / AR_THREADS
constexpr int AR_LDS_LIMIT = 64 * 1024;
constexpr float AR_NONE = -1.0e30f;  // running maximum of a query that has admitted no key yet

// The one function that decides the domain and the launch geometry: pg_attn_row_plan reports it, pg_attn_row launches by it.
struct ArPlan {
  int qb, chunks;       // queries per workgroup, workgroups per row
  int T, tshift;        // keys per tile (a power of two), its log2
  int dvp;              // floats per key of the V tile: a multiple of 4 (float4 reads), an odd number of quads
  int off_k, off_s, off_q, off_st;  // float offsets of the LDS regions behind the V tile
  int lds_bytes;
  char msg[160];
};

#define AR_REQUIRE(cond, code, ...)                  \
  do {                                               \
    if (!(cond)) {                                   \
      snprintf(pl.msg, sizeof(pl.msg), __VA_ARGS__); \
      return (code);                                 \
    }                                                \
  } while (0)

int ar_round4(int v) { return (v + 3) & ~3; }

int ar_plan(int heads, int dk, int dv, int H, int W, ArPlan& pl) {
  pl.msg[0] = 0;
  AR_REQUIRE(heads > 0 && dk > 0 && dv > 0 && H > 0 && W > 0, PG_EINVAL, "pg_attn_row: non-positive dimension");
  AR_REQUIRE(heads <= AR_MAX_GRID, PG_ESHAPE, "pg_attn_row: %d heads unsupported (at most %d)", heads, AR_MAX_GRID);
  AR_REQUIRE(dk <= AR_MAX_DK, PG_ESHAPE, "pg_attn_row: key width %d unsupported (1..%d per head)", dk, AR_MAX_DK);
  AR_REQUIRE(dv <= AR_MAX_DV, PG_ESHAPE, "pg_attn_row: value width %d unsupported (1..%d per head)", dv, AR_MAX_DV);
  AR_REQUIRE(W <= AR_MAX_W, PG_ESHAPE, "pg_attn_row: row length %d unsupported (1..%d)", W, AR_MAX_W);
  AR_REQUIRE((long)H * W <= AR_MAX_HW, PG_ESHAPE, "pg_attn_row: %d x %d pixels unsupported (at most %d)", H, W, AR_MAX_HW);
  pl.qb = W < AR_QB ? W : AR_QB;
  pl.chunks = (W + pl.qb - 1) / pl.qb;
  // the largest power of two with (dk + dv) T <= AR_THREADS * AR_PF: 128 up to 64 channels, 64 up to 128, 32 up to 192
  pl.T = AR_MAX_T;
  pl.tshift = 7;
  while ((dk + dv) * pl.T > AR_THREADS * AR_PF) {
    pl.T >>= 1;
    --pl.tshift;
  }
  const int dv4 = ar_round4(dv);
  pl.dvp = ((dv4 >> 2) & 1) ? dv4 : dv4 + 4;
  pl.off_k = pl.T * pl.dvp;
  pl.off_s = pl.off_k + dk * pl.T;
  pl.off_q = pl.off_s + ar_round4(pl.qb * (pl.T + 1));
  pl.off_st = pl.off_q + ar_round4(pl.qb * dk);
  pl.lds_bytes = (pl.off_st + 3 * pl.qb) * (int)sizeof(float);
  AR_REQUIRE(pl.lds_bytes <= AR_LDS_LIMIT, PG_ESHAPE, "pg_attn_row: %d bytes of LDS exceed %d", pl.lds_bytes, AR_LDS_LIMIT);
  return 0;
}

struct ArArgs {
  const float* q;
  const float* kv;
  float* kc;
  float* vc;
  float* o;
  const int* row_dev;
  int heads, dk, dv, H, W, r, mask_center, write_cache;
  int qb, T, tshift, dvp, off_k, off_s, off_q, off_st;
  float scale2;
};

__device__ __forceinline__ float ar_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// The keys of tile t: a run of the cache (channel stride H W) or of the row itself (channel stride W).
struct ArTile {
  const float* k;
  const float* v;
  int stride, j0, cnt, is_row;
};

// Element e = i * AR_THREADS + tid of a tile is (channel e >> tshift, key e & (T - 1)), K channels first: lanes over
// consecutive keys. Unconditional loads at clamped addresses (keys past cnt and elements past the tile re-read a valid
// entry, which is never used): 8 independent loads per group, all groups in flight before the first use.
__device__ __forceinline__ void ar_tile_load(float (&pf)[AR_PF], const ArTile& tl, int dk, int dv, int T, int tshift,
                                             int npf, int tid) {
#pragma unroll
  for (int i0 = 0; i0 < AR_PF; i0 += 8) {
    if (i0 < npf) {
#pragma unroll
      for (int i = i0; i < i0 + 8; ++i) {
        const int e = i * AR_THREADS + tid;
        const int ch = min(e >> tshift, dk + dv - 1);
        const int jc = tl.j0 + min(e & (T - 1), tl.cnt - 1);
        const float* src = ch < dk ? tl.k + (size_t)ch * tl.stride : tl.v + (size_t)(ch - dk) * tl.stride;
        pf[i] = src[jc];
      }
    }
  }
}

__device__ __forceinline__ void ar_tile_store(const float (&pf)[AR_PF], float* Ks, float* Vs, int dk, int dv, int T,
                                              int tshift, int dvp, int npf, int tid) {
  const int total = (dk + dv) << tshift;
#pragma unroll
  for (int i0 = 0; i0 < AR_PF; i0 += 8) {
    if (i0 < npf) {
#pragma unroll
      for (int i = i0; i < i0 + 8; ++i) {
        const int e = i * AR_THREADS + tid;
        const int ch = e >> tshift, jj = e & (T - 1);
        if (e < total) {
          if (ch < dk) Ks[ch * T + jj] = pf[i];
          else Vs[jj * dvp + (ch - dk)] = pf[i];
        }
      }
    }
  }
}

__global__ void __launch_bounds__(AR_THREADS) attn_row_kernel(const ArArgs A) {
  extern __shared__ __attribute__((aligned(16))) float ar_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.z, hd = blockIdx.y, x0 = blockIdx.x * A.qb;
  const int W = A.W, HW = A.H * A.W, dk = A.dk, dv = A.dv, heads = A.heads;
  const int T = A.T, tshift = A.tshift, dvp = A.dvp, TP = T + 1;
  const int nq = min(A.qb, W - x0);
  int r = A.r;
  if (A.row_dev) r = *A.row_dev;
  r = min(max(r, 0), A.H - 1);  // a stale device row can never index outside the caches

  float* Vs = ar_lds;             // [T][dvp]
  float* Ks = ar_lds + A.off_k;   // [dk][T]
  float* Ss = ar_lds + A.off_s;   // [qb][T + 1]: the probabilities of the tile
  float* Qs = ar_lds + A.off_q;   // [qb][dk]
  float* Ms = ar_lds + A.off_st;  // running maximum, running sum, rescale factor of the tile, per query
  float* Ls = Ms + A.qb;
  float* As = Ls + A.qb;

  float* kc = A.kc + ((size_t)n * heads + hd) * dk * HW;
  float* vc = A.vc + ((size_t)n * heads + hd) * dv * HW;
  const float* krow = A.kv + ((size_t)n * heads * (dk + dv) + (size_t)hd * dk) * W;
  const float* vrow = A.kv + ((size_t)n * heads * (dk + dv) + (size_t)heads * dk + (size_t)hd * dv) * W;
  const float* qrow = A.q + ((size_t)n * heads + hd) * dk * W;

  // the cached keys of rows < r, then the keys of the row up to the last query of this workgroup
  const int nkc = r * W;
  const int nkr = x0 + nq - (A.mask_center ? 1 : 0);
  const int nct = (nkc + T - 1) >> tshift, nrt = (nkr + T - 1) >> tshift;
  const int ntiles = nct + nrt;
  const int npf = (((dk + dv) << tshift) + AR_THREADS - 1) / AR_THREADS;

  auto tile = [&](int t) {
    ArTile tl;
    if (t < nct) {
      tl.k = kc; tl.v = vc; tl.stride = HW; tl.j0 = t << tshift; tl.cnt = min(T, nkc - tl.j0); tl.is_row = 0;
    } else {
      tl.k = krow; tl.v = vrow; tl.stride = W; tl.j0 = (t - nct) << tshift; tl.cnt = min(T, nkr - tl.j0); tl.is_row = 1;
    }
    return tl;
  };

  float pf[AR_PF];
  if (ntiles > 0) ar_tile_load(pf, tile(0), dk, dv, T, tshift, npf, tid);

  if (A.write_cache) {  // the only cache entries this launch writes: row r, the columns of this workgroup
    for (int e = tid; e < (dk + dv) * nq; e += AR_THREADS) {
      const int ch = e / nq, x = x0 + (e - ch * nq);
      if (ch < dk) kc[(size_t)ch * HW + (size_t)r * W + x] = krow[(size_t)ch * W + x];
      else vc[(size_t)(ch - dk) * HW + (size_t)r * W + x] = vrow[(size_t)(ch - dk) * W + x];
    }
  }
  for (int e = tid; e < nq * dk; e += AR_THREADS) {
    const int d = e / nq, xx = e - d * nq;
    Qs[xx * dk + d] = qrow[(size_t)d * W + x0 + xx];
  }
  if (tid < nq) {
    Ms[tid] = AR_NONE;
    Ls[tid] = 0.f;
  }

  // a thread's (query, 4 value channels) items
  const int nc4 = (dv + 3) >> 2, nitems = nq * nc4;
  int ixx[AR_ITEMS], ic4[AR_ITEMS];
  float4 acc[AR_ITEMS];
#pragma unroll
  for (int i = 0; i < AR_ITEMS; ++i) {
    const int item = min(i * AR_THREADS + tid, nitems - 1);
    ixx[i] = item / nc4;
    ic4[i] = item - ixx[i] * nc4;
    acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int own = A.mask_center ? 0 : 1;

  for (int t = 0; t < ntiles; ++t) {
    const ArTile tl = tile(t);
    ar_tile_store(pf, Ks, Vs, dk, dv, T, tshift, dvp, npf, tid);
    __syncthreads();
    if (t + 1 < ntiles) ar_tile_load(pf, tile(t + 1), dk, dv, T, tshift, npf, tid);  // in flight under the arithmetic below

    // score phase: a wave per query, lanes over the keys of the tile
    for (int xx = wave; xx < nq; xx += AR_WAVES) {
      const int lim = tl.is_row ? x0 + xx + own - tl.j0 : tl.cnt;  // keys [0, lim) of the tile are admitted
      const float* qx = Qs + xx * dk;
      float s[2];
      bool ok[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int jj = lane + 64 * u;
        const int jc = min(jj, T - 1);
        float d = 0.f;
        for (int c = 0; c < dk; ++c) d = fmaf(qx[c], Ks[c * T + jc], d);
        ok[u] = jj < tl.cnt && jj < lim;
        s[u] = ok[u] ? d * A.scale2 : AR_NONE;
      }
      const float m_old = Ms[xx];
      const float m_new = fmaxf(m_old, ar_wave_max(fmaxf(s[0], s[1])));
      float p[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        p[u] = ok[u] ? __builtin_amdgcn_exp2f(s[u] - m_new) : 0.f;
        const int jj = lane + 64 * u;
        if (jj < T) Ss[xx * TP + jj] = p[u];
      }
      const float sum = pg_wave_sum(p[0] + p[1]);
      if (lane == 0) {
        const float alpha = __builtin_amdgcn_exp2f(m_old - m_new);  // 1 while nothing is admitted, 0 at the first admitted key
        Ms[xx] = m_new;
        Ls[xx] = fmaf(Ls[xx], alpha, sum);
        As[xx] = alpha;
      }
    }
    __syncthreads();

    // value phase: one chain per (query, channel) over the keys of the tile in ascending order
#pragma unroll
    for (int i = 0; i < AR_ITEMS; ++i) {
      if (i * AR_THREADS < nitems) {
        const float alpha = As[ixx[i]];
        const float* prow = Ss + ixx[i] * TP;
        const float4* vcol = reinterpret_cast<const float4*>(Vs) + ic4[i];
        const int vstep = dvp >> 2;
        float4 a = acc[i];
        a.x *= alpha; a.y *= alpha; a.z *= alpha; a.w *= alpha;
        for (int jj = 0; jj < tl.cnt; ++jj) {
          const float pj = prow[jj];
          const float4 v = vcol[jj * vstep];
          a.x = fmaf(pj, v.x, a.x);
          a.y = fmaf(pj, v.y, a.y);
          a.z = fmaf(pj, v.z, a.z);
          a.w = fmaf(pj, v.w, a.w);
        }
        acc[i] = a;
      }
    }
    __syncthreads();
  }
  if (ntiles == 0) __syncthreads();  // Ls of the prologue

  float* orow = A.o + ((size_t)n * heads + hd) * dv * W;
#pragma unroll
  for (int i = 0; i < AR_ITEMS; ++i) {
    if (i * AR_THREADS + tid < nitems) {
      const float l = Ls[ixx[i]];
      const float inv = l > 0.f ? 1.f / l : 0.f;  // no key admitted: exactly 0
      const float e[4] = {acc[i].x, acc[i].y, acc[i].z, acc[i].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = ic4[i] * 4 + k;
        if (c < dv) orow[(size_t)c * W + x0 + ixx[i]] = e[k] * inv;
      }
    }
  }
}

__global__ void __launch_bounds__(AR_THREADS) row_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               long planes, int H, int W, int r, const int* row_dev) {
  if (row_dev) r = *row_dev;
  r = min(max(r, 0), H - 1);
  const long total = planes * W;
  for (long i = (long)blockIdx.x * AR_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * AR_THREADS) {
    const long pl = i / W;
    const int x = (int)(i - pl * W);
    dst[i] = src[(pl * H + r) * W + x];
  }
}

}  // namespace

PG_EXPORT int pg_attn_row_plan(int heads, int dk, int dv, int H, int W, int* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_ATTN_ROW_PLAN_INTS, PG_EINVAL, "pg_attn_row_plan: null pointer or short output array");
  ArPlan pl;
  const int rc = ar_plan(heads, dk, dv, H, W, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  out[0] = AR_THREADS;
  out[1] = pl.lds_bytes;
  out[2] = pl.T;
  out[3] = pl.chunks;  // grid: (row chunks, heads, N)
  out[4] = heads;
  out[5] = pl.qb;
  return 0;
}

PG_EXPORT int pg_attn_row(const float* q_row, const float* kv_row, float* k_cache, float* v_cache, float* o_row, int N,
                          int heads, int dk, int dv, int H, int W, int r, int mask_center, int write_cache,
                          const int* row_dev, void* stream) {
  PG_REQUIRE(q_row && kv_row && k_cache && v_cache && o_row, PG_EINVAL, "pg_attn_row: null pointer");
  PG_REQUIRE(N > 0, PG_EINVAL, "pg_attn_row: bad dims");
  PG_REQUIRE((mask_center == 0 || mask_center == 1) && (write_cache == 0 || write_cache == 1), PG_EINVAL,
             "pg_attn_row: mask_center and write_cache must be 0/1");
  ArPlan pl;
  const int rc = ar_plan(heads, dk, dv, H, W, pl);
  if (rc) {
    pg_set_error("%s", pl.msg);
    return rc;
  }
  PG_REQUIRE(r >= 0 && r < H, PG_EINVAL, "pg_attn_row: row outside the image");
  PG_REQUIRE(N <= AR_MAX_GRID, PG_ESHAPE, "pg_attn_row: batch %d unsupported (at most %d)", N, AR_MAX_GRID);
  ArArgs A;
  A.q = q_row; A.kv = kv_row; A.kc = k_cache; A.vc = v_cache; A.o = o_row; A.row_dev = row_dev;
  A.heads = heads; A.dk = dk; A.dv = dv; A.H = H; A.W = W; A.r = r; A.mask_center = mask_center; A.write_cache = write_cache;
  A.qb = pl.qb; A.T = pl.T; A.tshift = pl.tshift; A.dvp = pl.dvp;
  A.off_k = pl.off_k; A.off_s = pl.off_s; A.off_q = pl.off_q; A.off_st = pl.off_st;
  A.scale2 = 1.44269504088896340736f / sqrtf((float)dk);
  hipLaunchKernelGGL(attn_row_kernel, dim3((unsigned)pl.chunks, (unsigned)heads, (unsigned)N), dim3(AR_THREADS),
                     (size_t)pl.lds_bytes, (hipStream_t)stream, A);
  PG_LAUNCH_CHECK("pg_attn_row");
  return 0;
}

PG_EXPORT int pg_row_gather(const float* src, float* dst, int N, int C, int H, int W, int r, const int* row_dev,
                            void* stream) {
  PG_REQUIRE(src && dst, PG_EINVAL, "pg_row_gather: null pointer");
  PG_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, PG_EINVAL, "pg_row_gather: non-positive dimension");
  PG_REQUIRE(r >= 0 && r < H, PG_EINVAL, "pg_row_gather: row outside the image");
  const long planes = (long)N * C;
  PG_REQUIRE(planes * H * W < (1L << 31), PG_ESHAPE, "pg_row_gather: tensor too large");
  const long total = planes * W;
  const int blocks = (int)((total + AR_THREADS - 1) / AR_THREADS);
  hipLaunchKernelGGL(row_gather_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(AR_THREADS), 0,
                     (hipStream_t)stream, src, dst, planes, H, W, r, row_dev);
  PG_LAUNCH_CHECK("pg_row_gather");
  return 0;
}
