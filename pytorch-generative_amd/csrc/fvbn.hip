// fvbn.hip — the Fully Visible Belief Network (reference models/autoregressive/fvbn.py) on PACKED triangular storage:
// logits = x tril(W, -1)^T + b, its weight gradient, and a one-launch ancestral sampler.
//
// Packed layout (fv_off / fv_pad, the one definition; pg_fvbn_row_offset reports it): row i of the strictly lower triangle holds
// len(i) = max(1, i) values (row 0: the dummy weight the reference multiplies by a zero input) followed by zeros up to
// pad(i) = roundup(len(i), 4) floats; off(i) = sum_{k < i} pad(k), P(D) = off(D). Every row starts 16-byte aligned.
//
//   forward  rows n, cols i, k = j, on the small tile of mfma_tile.h (64 x 64, k chunks of 32; geometry, LDS stride and chain
//            order are stated there). Column tile c reads k only up to min(D, 64 c + 64) - 1: nothing above the diagonal is multiplied.
//            The weight operand is read with 16-byte loads inside row i's own storage (a chunk of 4 starting at j < i ends
//            before off(i) + pad(i)) and every element j >= i is replaced by zero by a predicate, so neither the next row's
//            storage nor row 0's dummy weight is ever read. Heavy column tiles are launched first. The sum over j has a
//            two-level order fixed by i alone: an fmaf chain inside every slice of 4 chunks, the slices added in ascending
//            order. Where there are fewer than 128 output tiles the slices become workgroups of their own, write raw
//            partial sums to a workspace and a second launch adds them in the same order: the same bits as without a split,
//            so a sample's row does not depend on N.
//   wgrad    rows i, cols j, k = n: the same tile, 64 x 64 tiles of dW with tile column <= tile row only (a triangular tile index), written
//            straight into the packed layout where j < i < D; pads and row 0 are never written. db from the tiles of tile
//            column 0. Where the triangle has fewer than 128 tiles the batch is cut into slices whose raw partial sums go to a
//            workspace and are merged in slice order by a second launch (as dense_linear.hip's k-split).
//   sampler  one wave carries up to 4 samples with x in LDS; per dimension i the lanes read row i with 16-byte loads (the
//            first 4 chunks per lane of row i + 1, and its canvas / uniform / bias entries, are requested before row i is
//            reduced), a lane sums its chunks in ascending order, the wave by the butterfly: an order fixed by i alone.
// Every output element is owned by one lane; no float atomics; no host synchronisation, no allocation: capturable. fv_plan is
// the one function that decides the domain and every geometry; pg_fvbn_plan reports it and every launch goes by it.
#include <algorithm>

#include "common.h"
#include "mfma_tile.h"

namespace {

using pg_tile::f32x4;
constexpr int FV_V = pg_tile::SMALL;  // forward and weight gradient run on the small tile of mfma_tile.h
using FvTile = pg_tile::Tile<FV_V>;
constexpr int FV_THREADS = pg_tile::THREADS;
constexpr int FV_T = FvTile::BM;     // edge of an output tile
constexpr int FV_KC = FvTile::KC;    // k per LDS chunk
constexpr int FV_LD = FvTile::LD;    // LDS row stride
constexpr int FV_SLICE = 4;          // forward: k chunks of a slice, the unit of its two-level sum and of its k-split
constexpr int FV_CUS = 256;          // workgroups that fill the chip
constexpr int FV_SPLIT_BELOW = 128;  // weight-gradient tiles below which the batch is split
constexpr int FV_MAX_SLICES = 64;
constexpr int FV_MAX_D = 8192;
constexpr int FV_MAX_N = 1 << 30;
constexpr int FV_S_MAX = 4;            // sampler: samples of a workgroup (one wave)
constexpr int FV_S_LDS_FLOATS = 12288; // sampler: floats of x a workgroup keeps in LDS
constexpr int FV_S_PF = 4;             // sampler: 16-byte chunks per lane requested one row ahead

__host__ __device__ inline long fv_off(int i) {
  if (i <= 0) return 0;
  const long m = i - 1, q = m >> 2, r = m & 3;  // 4 + sum_{k = 1}^{m} 4 ceil(k / 4)
  return 4 + 4 * (q + 1) * (2 * q + r);
}
__host__ __device__ inline int fv_len(int i) { return i < 1 ? 1 : i; }
__host__ __device__ inline int fv_pad(int i) { return (fv_len(i) + 3) & ~3; }

// Tile t of the lower triangle of tiles, row by row: (0, 0), (1, 0), (1, 1), (2, 0), ...
__host__ __device__ inline void fv_tri(int t, int& ti, int& tj) {
  int r = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  ti = r;
  tj = t - r * (r + 1) / 2;
}

// k range of forward column tile ct: j < i <= min(D, 64 ct + 64) - 1
__host__ __device__ inline int fv_fwd_kend(int D, int ct) { return (D < ct * FV_T + FV_T ? D : ct * FV_T + FV_T) - 1; }

// k slices of forward column tile ct: FV_SLICE chunks each
__host__ __device__ inline int fv_fwd_slices(int D, int ct) {
  return ((fv_fwd_kend(D, ct) + FV_KC - 1) / FV_KC + FV_SLICE - 1) / FV_SLICE;
}

struct FvFwdArgs {
  const float* x;
  const float* wp;
  const float* b;
  float* y;
  float* part;  // k-split: raw partial sums [slice][row tile][64 * 64], the slices of all column tiles numbered through
  int N, D, col_tiles, row_tiles, slices;
  int base[FV_MAX_D / FV_T + 1];  // base[ct]: the first slice of column tile ct; base[col_tiles] = slices
};

// The sum over j of one output has a two-level order fixed by i alone: an fmaf chain inside every slice of FV_SLICE chunks
// (each started from zero), the slices added in ascending order, then the bias. SPLIT = false: a workgroup walks all slices of
// its column tile and adds them in registers. SPLIT = true: one workgroup per (slice, row tile) writes its raw chain to the
// workspace and fv_fwd_reduce_kernel adds the slices in the same order: the same bits either way.
template <bool SPLIT>
__global__ void __launch_bounds__(FV_THREADS) fv_fwd_kernel(const FvFwdArgs p) {
  constexpr int A_PER = FV_T * FV_KC / FV_THREADS;      // 8 floats of x per thread and chunk
  constexpr int B_PER = FV_T * FV_KC / 4 / FV_THREADS;  // 2 chunks of 4 weights
  __shared__ float s_a[FV_T * FV_LD];
  __shared__ float s_b[FV_T * FV_LD];
  const pg_tile::Lanes<FV_V> ln;
  const int tid = ln.tid;
  int ct, rt, ch_beg, ch_end, s = 0;
  if (SPLIT) {
    s = (int)(blockIdx.x % p.slices);
    rt = (int)(blockIdx.x / p.slices);
    ct = 0;
    while (p.base[ct + 1] <= s) ++ct;  // s < base[col_tiles] = slices
    ch_beg = (s - p.base[ct]) * FV_SLICE;
    ch_end = ch_beg + FV_SLICE;
  } else {
    ct = p.col_tiles - 1 - (int)(blockIdx.x % p.col_tiles);  // the longest k ranges first
    rt = (int)(blockIdx.x / p.col_tiles);
    ch_beg = 0;
    ch_end = 1 << 30;
  }
  const int r0 = rt * FV_T, c0 = ct * FV_T;
  const int kend = fv_fwd_kend(p.D, ct);
  const int nch = min(ch_end, (kend + FV_KC - 1) / FV_KC);

  const float* brow[B_PER];  // row c0 + c of the packed weight
  int bcol[B_PER];
#pragma unroll
  for (int j = 0; j < B_PER; ++j) {
    bcol[j] = c0 + (tid + j * FV_THREADS) / (FV_KC / 4);
    brow[j] = p.wp + fv_off(bcol[j] < p.D ? bcol[j] : 0);
  }

  float ra[A_PER];
  f32x4 rb[B_PER];
  auto load = [&](int ch) {
    const int k0 = ch * FV_KC;
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int e = tid + j * FV_THREADS;
      const int gr = r0 + e / FV_KC, gk = k0 + e % FV_KC;
      ra[j] = (gr < p.N && gk < kend) ? p.x[(size_t)gr * p.D + gk] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int gc = bcol[j], gk = k0 + ((tid + j * FV_THREADS) % (FV_KC / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      // gk is a multiple of 4 below gc = len(gc): gk + 3 < pad(gc), inside row gc's own storage; row 0 is never read
      if (gc < p.D && gk < gc) v = *reinterpret_cast<const f32x4*>(brow[j] + gk);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (gk + t >= gc) v[t] = 0.f;  // on and above the diagonal: zero whatever the pads hold
      rb[j] = v;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int e = tid + j * FV_THREADS;
      s_a[(e / FV_KC) * FV_LD + e % FV_KC] = ra[j];
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int e = tid + j * FV_THREADS;
      float* dst = s_b + (e / (FV_KC / 4)) * FV_LD + (e % (FV_KC / 4)) * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) dst[t] = rb[j][t];
    }
  };

  pg_tile::Acc<FV_V> acc, tot;
  pg_tile::zero<FV_V>(acc);
  pg_tile::zero<FV_V>(tot);
  auto fold = [&](int ch) {
    if (!SPLIT && ((ch + 1) % FV_SLICE == 0 || ch + 1 == nch)) {  // a slice is complete: add it, start the next from zero
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
          acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  };
  PG_TILE_PIPELINE(FV_V, true, ch_beg, nch, load, store, acc, s_a, s_b, ln, fold);

  PG_TILE_FOR_EACH_OUTPUT(FV_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (SPLIT)
      p.part[((size_t)s * p.row_tiles + rt) * (FV_T * FV_T) + li * FV_T + lj] = PG_TILE_OUTPUT(acc);
    else if (gc < p.D && gr < p.N)
      p.y[(size_t)gr * p.D + gc] = PG_TILE_OUTPUT(tot) + p.b[gc];
  }
}

// k-split epilogue: y[n][i] = (the slices of i's column tile in ascending order) + b[i]
__global__ void __launch_bounds__(256) fv_fwd_reduce_kernel(const FvFwdArgs p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)p.N * p.D) return;
  const int n = (int)(e / p.D), i = (int)(e % p.D);
  const int ct = i / FV_T, rt = n / FV_T;
  const size_t cell = (size_t)(n % FV_T) * FV_T + i % FV_T;
  float v = 0.f;
  for (int s = p.base[ct]; s < p.base[ct + 1]; ++s) v += p.part[((size_t)s * p.row_tiles + rt) * (FV_T * FV_T) + cell];
  p.y[e] = v + p.b[i];
}

struct FvWgArgs {
  const float* x;
  const float* dy;
  float* dwp;   // packed, may be NULL
  float* db;    // may be NULL
  float* part;  // N-split: raw partial sums [slice][tile][64 * 64], then the bias rows [slice][64 col_tiles]
  int N, D, tiles, col_tiles, slices, nper;
};

__global__ void __launch_bounds__(FV_THREADS) fv_wgrad_kernel(const FvWgArgs p) {
  constexpr int PER = FV_T * FV_KC / FV_THREADS;  // 8 floats of each operand per thread and chunk
  __shared__ float s_a[FV_T * FV_LD];  // dy^T: rows i, k = n
  __shared__ float s_b[FV_T * FV_LD];  // x^T: rows j, k = n
  const pg_tile::Lanes<FV_V> ln;
  const int tid = ln.tid;
  int ti, tj;
  fv_tri((int)blockIdx.x, ti, tj);
  const int r0 = ti * FV_T, c0 = tj * FV_T;
  const int nbeg = (int)blockIdx.y * p.nper;
  const int nend = min(p.N, nbeg + p.nper);

  float ra[PER], rb[PER];
  auto load = [&](int ch) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + j * FV_THREADS;
      const int r = e % FV_T, gn = nbeg + ch * FV_KC + e / FV_T;
      const bool ok = gn < nend;
      ra[j] = (ok && r0 + r < p.D) ? p.dy[(size_t)gn * p.D + r0 + r] : 0.f;
      rb[j] = (ok && c0 + r < p.D) ? p.x[(size_t)gn * p.D + c0 + r] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + j * FV_THREADS;
      s_a[(e % FV_T) * FV_LD + e / FV_T] = ra[j];
      s_b[(e % FV_T) * FV_LD + e / FV_T] = rb[j];
    }
  };

  pg_tile::Acc<FV_V> acc;
  pg_tile::zero<FV_V>(acc);
  float dbsum = 0.f;  // thread tid < 64 sums row tid of dy^T in n order
  const bool do_db = p.db != nullptr && tj == 0;
  auto bias_sum = [&](int) {
    if (do_db && tid < FV_T) {
      const float* row = s_a + tid * FV_LD;
#pragma unroll
      for (int k = 0; k < FV_KC; ++k) dbsum += row[k];  // zero beyond the slice
    }
  };
  PG_TILE_PIPELINE(FV_V, true, 0, (nend - nbeg + FV_KC - 1) / FV_KC, load, store, acc, s_a, s_b, ln, bias_sum);
  if (do_db && tid < FV_T) {
    if (p.part)
      p.part[(size_t)p.slices * p.tiles * (FV_T * FV_T) + (size_t)blockIdx.y * (p.col_tiles * FV_T) + r0 + tid] = dbsum;
    else if (r0 + tid < p.D)
      p.db[r0 + tid] += dbsum;
  }
  if (!p.part && !p.dwp) return;

  PG_TILE_FOR_EACH_OUTPUT(FV_V, ln, li, lj) {
    const int gi = r0 + li, gj = c0 + lj;
    if (p.part)
      p.part[((size_t)blockIdx.y * p.tiles + blockIdx.x) * (FV_T * FV_T) + li * FV_T + lj] = PG_TILE_OUTPUT(acc);
    else if (gi < p.D && gj < gi)
      p.dwp[fv_off(gi) + gj] += PG_TILE_OUTPUT(acc);
  }
}

// N-split epilogue: the slices' partial sums in slice order, added into the packed layout; behind the tiles, the bias sums.
__global__ void __launch_bounds__(256) fv_wgrad_reduce_kernel(const FvWgArgs p) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.tiles * (FV_T * FV_T);
  if (e < total) {
    if (!p.dwp) return;
    int ti, tj;
    fv_tri((int)(e / (FV_T * FV_T)), ti, tj);
    const int gi = ti * FV_T + (int)(e % (FV_T * FV_T)) / FV_T, gj = tj * FV_T + (int)(e % FV_T);
    if (gi >= p.D || gj >= gi) return;
    float v = 0.f;
    for (int z = 0; z < p.slices; ++z) v += p.part[(size_t)z * total + e];
    p.dwp[fv_off(gi) + gj] += v;
  } else if (p.db && e - total < (size_t)p.D) {
    const size_t r = e - total;
    float v = 0.f;
    for (int z = 0; z < p.slices; ++z) v += p.part[(size_t)p.slices * total + (size_t)z * (p.col_tiles * FV_T) + r];
    p.db[r] += v;
  }
}

// The ancestral chain of S samples per one-wave workgroup. xs: S rows of Dp = roundup(D, 4) floats, zero until decided, so
// that the last chunk of a row meets zeros on both sides at j >= i.
template <int S>
__global__ void __launch_bounds__(64) fv_sample_kernel(const float* __restrict__ wp, const float* __restrict__ b, float* canvas,
                                                       const float* __restrict__ uniforms, float* logits_out, int N, int D, int Dp) {
  extern __shared__ __align__(16) float xs[];
  const int lane = threadIdx.x;
  for (int e = lane; e < S * Dp; e += 64) xs[e] = 0.f;
  __syncthreads();
  const int n = (int)blockIdx.x * S + lane;  // lane s < S decides sample s
  const bool own = lane < S && n < N;
  const size_t base = own ? (size_t)n * D : 0;
  float c_next = own ? canvas[base] : 0.f, u_next = own ? uniforms[base] : 0.f, b_next = b[0];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 nxt[FV_S_PF];
#pragma unroll
  for (int c = 0; c < FV_S_PF; ++c) nxt[c] = zero4;  // row 0 has no predecessors: its dummy weight is never read

  for (int i = 0; i < D; ++i) {
    f32x4 cur[FV_S_PF];
#pragma unroll
    for (int c = 0; c < FV_S_PF; ++c) cur[c] = nxt[c];
    const float c_i = c_next, u_i = u_next, b_i = b_next;
    const int nch = i >= 1 ? (i + 3) >> 2 : 0;  // 16-byte chunks of row i: pad(i) / 4
    const f32x4* row = reinterpret_cast<const f32x4*>(wp + fv_off(i));
    if (i + 1 < D) {  // row i + 1 is requested before row i is reduced
      const f32x4* row1 = reinterpret_cast<const f32x4*>(wp + fv_off(i + 1));
      const int nch1 = (i + 4) >> 2;
#pragma unroll
      for (int c = 0; c < FV_S_PF; ++c) {
        const int ch = c * 64 + lane;
        nxt[c] = ch < nch1 ? row1[ch] : zero4;
      }
      if (own) {
        c_next = canvas[base + i + 1];
        u_next = uniforms[base + i + 1];
      }
      b_next = b[i + 1];
    }
    float acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.f;
#pragma unroll
    for (int c = 0; c < FV_S_PF; ++c) {
      const int ch = c * 64 + lane;
      if (ch < nch) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + s * Dp + 4 * ch);
          acc[s] = fmaf(cur[c][3], xv[3], fmaf(cur[c][2], xv[2], fmaf(cur[c][1], xv[1], fmaf(cur[c][0], xv[0], acc[s]))));
        }
      }
    }
    for (int ch = FV_S_PF * 64 + lane; ch < nch; ch += 64) {
      const f32x4 w = row[ch];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + s * Dp + 4 * ch);
        acc[s] = fmaf(w[3], xv[3], fmaf(w[2], xv[2], fmaf(w[1], xv[1], fmaf(w[0], xv[0], acc[s]))));
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float v = pg_wave_sum(acc[s]);
      if (lane == s) mine = v;
    }
    if (own) {
      const float l = b_i + mine;
      const float xi = c_i >= 0.f ? c_i : (u_i < 1.f / (1.f + expf(-l)) ? 1.f : 0.f);
      xs[lane * Dp + i] = xi;
      canvas[base + i] = xi;
      if (logits_out) logits_out[base + i] = l;
    }
    __syncthreads();
  }
}

// dense (D, D) -> packed: the strict lower triangle, row 0's dummy value from [0][0], zeros in the pads. blockIdx.y = row.
__global__ void __launch_bounds__(256) fv_pack_kernel(const float* __restrict__ dense, float* __restrict__ wp, int D) {
  const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= fv_pad(i)) return;
  wp[fv_off(i) + c] = c < fv_len(i) ? dense[(size_t)i * D + c] : 0.f;
}

// packed -> dense (D, D): zeros on and above the diagonal, except row 0's dummy value at [0][0]
__global__ void __launch_bounds__(256) fv_unpack_kernel(const float* __restrict__ wp, float* __restrict__ dense, int D) {
  const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  dense[(size_t)i * D + c] = c < fv_len(i) ? wp[fv_off(i) + c] : 0.f;
}

struct FvPlan {
  long packed, fwd_groups, fwd_weight_tiles, fwd_slices, fwd_reduce_groups, fwd_ws_floats, wgrad_groups, reduce_groups, ws_floats, sample_groups;
  int col_tiles, row_tiles, tiles, slices, nper, sample_s, sample_lds, fwd_split;
};

int fv_plan(int D, int N, FvPlan& pl, const char* name) {
  PG_REQUIRE(D >= 1 && D <= FV_MAX_D, PG_ESHAPE, "%s: D = %d unsupported (1 .. %d)", name, D, FV_MAX_D);
  PG_REQUIRE(N >= 1 && N <= FV_MAX_N, PG_ESHAPE, "%s: N = %d unsupported (1 .. 2^30)", name, N);
  const long lim = (1L << 31) - 1;
  pl.packed = fv_off(D);
  pl.col_tiles = pg_cdiv(D, FV_T);
  pl.row_tiles = pg_cdiv(N, FV_T);
  pl.fwd_groups = (long)pl.col_tiles * pl.row_tiles;
  PG_REQUIRE(pl.fwd_groups <= lim, PG_ESHAPE, "%s: N = %d, D = %d is too large for one launch", name, N, D);
  pl.fwd_weight_tiles = pl.fwd_slices = 0;
  for (int ct = 0; ct < pl.col_tiles; ++ct) {
    pl.fwd_weight_tiles += pg_cdiv(fv_fwd_kend(D, ct), FV_KC);
    pl.fwd_slices += fv_fwd_slices(D, ct);
  }
  // the forward's k-split: where the output tiles leave half the chip idle and some column tile has more than one slice
  pl.fwd_split = pl.fwd_groups < FV_SPLIT_BELOW && pl.fwd_slices > pl.col_tiles;
  if (pl.fwd_split) pl.fwd_groups = pl.fwd_slices * pl.row_tiles;
  pl.fwd_ws_floats = pl.fwd_split ? pl.fwd_groups * (FV_T * FV_T) : 0;
  pl.fwd_reduce_groups = pl.fwd_split ? ((long)N * D + 255) / 256 : 0;
  pl.tiles = pl.col_tiles * (pl.col_tiles + 1) / 2;
  const int chunks = pg_cdiv(N, FV_KC);
  int ks = 1;
  if (pl.tiles < FV_SPLIT_BELOW && chunks >= 4)  // at least two chunks per slice
    ks = (int)std::min<long>(std::min<long>((FV_CUS + pl.tiles - 1) / pl.tiles, chunks / 2), FV_MAX_SLICES);
  pl.nper = pg_cdiv(chunks, ks) * FV_KC;
  pl.slices = pg_cdiv(N, pl.nper);
  pl.wgrad_groups = (long)pl.tiles * pl.slices;
  const long cells = (long)pl.tiles * (FV_T * FV_T) + (long)pl.col_tiles * FV_T;
  pl.ws_floats = pl.slices > 1 ? pl.slices * cells : 0;
  pl.reduce_groups = pl.slices > 1 ? (cells + 255) / 256 : 0;
  const int Dp = (D + 3) & ~3;
  int s = FV_S_MAX;
  while (s > 1 && (s * Dp > FV_S_LDS_FLOATS || s / 2 >= N)) s /= 2;
  pl.sample_s = s;
  pl.sample_groups = pg_cdiv(N, s);
  pl.sample_lds = s * Dp * (int)sizeof(float);
  return 0;
}

bool fv_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

PG_EXPORT long long pg_fvbn_row_offset(int i) { return i < 0 ? -1 : (long long)fv_off(i); }

PG_EXPORT int pg_fvbn_plan(int D, int N, long long* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_FVBN_PLAN_INTS, PG_EINVAL, "pg_fvbn_plan: null pointer or short output array");
  FvPlan pl;
  const int rc = fv_plan(D, N, pl, "pg_fvbn_plan");
  if (rc) return rc;
  out[0] = pl.packed;
  out[1] = FV_T;
  out[2] = FV_KC;
  out[3] = pl.col_tiles;
  out[4] = pl.row_tiles;
  out[5] = pl.fwd_groups;
  out[6] = pl.fwd_weight_tiles;
  out[7] = pl.tiles;
  out[8] = pl.slices;
  out[9] = pl.nper;
  out[10] = pl.wgrad_groups;
  out[11] = pl.reduce_groups;
  out[12] = pl.ws_floats;
  out[13] = pl.sample_s;
  out[14] = pl.sample_groups;
  out[15] = pl.sample_lds;
  out[16] = FV_MAX_D;
  out[17] = FV_SLICE;
  out[18] = pl.fwd_slices;
  out[19] = pl.fwd_split;
  out[20] = pl.fwd_reduce_groups;
  out[21] = pl.fwd_ws_floats;
  return 0;
}

PG_EXPORT int pg_fvbn_tiles(int D, int kind, long long* out, long long cap, long long* count) {
  PG_REQUIRE(count && (out || cap == 0), PG_EINVAL, "pg_fvbn_tiles: null pointer");
  PG_REQUIRE(kind == PG_FVBN_TILES_FWD || kind == PG_FVBN_TILES_WGRAD, PG_EINVAL, "pg_fvbn_tiles: kind %d is neither forward nor weight gradient",
             kind);
  FvPlan pl;
  const int rc = fv_plan(D, 1, pl, "pg_fvbn_tiles");
  if (rc) return rc;
  long long n = 0;
  auto emit = [&](int i0, int i1, int j0, int j1) {
    if (n < cap) {
      long long* o = out + 4 * n;
      o[0] = i0, o[1] = i1, o[2] = j0, o[3] = j1;
    }
    ++n;
  };
  if (kind == PG_FVBN_TILES_FWD) {
    for (int ct = 0; ct < pl.col_tiles; ++ct) {
      const int kend = fv_fwd_kend(D, ct);
      for (int k0 = 0; k0 < kend; k0 += FV_KC) emit(ct * FV_T, std::min(D, ct * FV_T + FV_T), k0, std::min(kend, k0 + FV_KC));
    }
  } else {
    for (int t = 0; t < pl.tiles; ++t) {
      int ti, tj;
      fv_tri(t, ti, tj);
      emit(ti * FV_T, std::min(D, ti * FV_T + FV_T), tj * FV_T, std::min(D, tj * FV_T + FV_T));
    }
  }
  *count = n;
  return 0;
}

PG_EXPORT int pg_fvbn_fwd(const float* x, const float* wp, const float* b, float* logits, int N, int D, float* ws, size_t ws_floats,
                          void* stream) {
  FvPlan pl;
  const int rc = fv_plan(D, N, pl, "pg_fvbn_fwd");
  if (rc) return rc;
  PG_REQUIRE(x && wp && b && logits, PG_EINVAL, "pg_fvbn_fwd: null pointer");
  PG_REQUIRE(fv_aligned16(wp), PG_EINVAL, "pg_fvbn_fwd: the packed weight is not 16-byte aligned");
  FvFwdArgs p;
  p.x = x;
  p.wp = wp;
  p.b = b;
  p.y = logits;
  p.part = nullptr;
  p.N = N;
  p.D = D;
  p.col_tiles = pl.col_tiles;
  p.row_tiles = pl.row_tiles;
  p.slices = (int)pl.fwd_slices;
  p.base[0] = 0;
  for (int ct = 0; ct < pl.col_tiles; ++ct) p.base[ct + 1] = p.base[ct] + fv_fwd_slices(D, ct);
  const hipStream_t st = (hipStream_t)stream;
  if (pl.fwd_split) {
    PG_REQUIRE(ws != nullptr && ws_floats >= (size_t)pl.fwd_ws_floats, PG_EINVAL, "pg_fvbn_fwd: workspace of %zu floats, %ld needed (pg_fvbn_plan)",
               ws_floats, pl.fwd_ws_floats);
    p.part = ws;
    hipLaunchKernelGGL(fv_fwd_kernel<true>, dim3((unsigned)pl.fwd_groups), dim3(FV_THREADS), 0, st, p);
    PG_LAUNCH_CHECK("pg_fvbn_fwd");
    hipLaunchKernelGGL(fv_fwd_reduce_kernel, dim3((unsigned)pl.fwd_reduce_groups), dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL(fv_fwd_kernel<false>, dim3((unsigned)pl.fwd_groups), dim3(FV_THREADS), 0, st, p);
  }
  PG_LAUNCH_CHECK("pg_fvbn_fwd");
  return 0;
}

PG_EXPORT int pg_fvbn_wgrad(const float* x, const float* dy, float* dwp, float* db, int N, int D, float* ws, size_t ws_floats,
                            void* stream) {
  FvPlan pl;
  const int rc = fv_plan(D, N, pl, "pg_fvbn_wgrad");
  if (rc) return rc;
  PG_REQUIRE(x && dy, PG_EINVAL, "pg_fvbn_wgrad: null pointer");
  if (!dwp && !db) return 0;
  FvWgArgs p;
  p.x = x;
  p.dy = dy;
  p.dwp = dwp;
  p.db = db;
  p.part = nullptr;
  p.N = N;
  p.D = D;
  p.tiles = pl.tiles;
  p.col_tiles = pl.col_tiles;
  p.slices = pl.slices;
  p.nper = pl.nper;
  if (pl.slices > 1) {
    PG_REQUIRE(ws != nullptr && ws_floats >= (size_t)pl.ws_floats, PG_EINVAL, "pg_fvbn_wgrad: workspace of %zu floats, %ld needed (pg_fvbn_plan)",
               ws_floats, pl.ws_floats);
    p.part = ws;
  }
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fv_wgrad_kernel, dim3((unsigned)pl.tiles, (unsigned)pl.slices), dim3(FV_THREADS), 0, st, p);
  PG_LAUNCH_CHECK("pg_fvbn_wgrad");
  if (pl.slices > 1) {
    hipLaunchKernelGGL(fv_wgrad_reduce_kernel, dim3((unsigned)pl.reduce_groups), dim3(256), 0, st, p);
    PG_LAUNCH_CHECK("pg_fvbn_wgrad");
  }
  return 0;
}

PG_EXPORT int pg_fvbn_sample(const float* wp, const float* b, float* canvas, const float* uniforms, float* logits_out, int N, int D,
                             void* stream) {
  FvPlan pl;
  const int rc = fv_plan(D, N, pl, "pg_fvbn_sample");
  if (rc) return rc;
  PG_REQUIRE(wp && b && canvas && uniforms, PG_EINVAL, "pg_fvbn_sample: null pointer");
  PG_REQUIRE(fv_aligned16(wp), PG_EINVAL, "pg_fvbn_sample: the packed weight is not 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)pl.sample_groups), block(64);
  const int Dp = (D + 3) & ~3;
  const size_t lds = (size_t)pl.sample_lds;
  if (pl.sample_s == 4)
    hipLaunchKernelGGL(fv_sample_kernel<4>, grid, block, lds, st, wp, b, canvas, uniforms, logits_out, N, D, Dp);
  else if (pl.sample_s == 2)
    hipLaunchKernelGGL(fv_sample_kernel<2>, grid, block, lds, st, wp, b, canvas, uniforms, logits_out, N, D, Dp);
  else
    hipLaunchKernelGGL(fv_sample_kernel<1>, grid, block, lds, st, wp, b, canvas, uniforms, logits_out, N, D, Dp);
  PG_LAUNCH_CHECK("pg_fvbn_sample");
  return 0;
}

PG_EXPORT int pg_fvbn_pack(const float* dense, float* wp, int D, void* stream) {
  FvPlan pl;
  const int rc = fv_plan(D, 1, pl, "pg_fvbn_pack");
  if (rc) return rc;
  PG_REQUIRE(dense && wp, PG_EINVAL, "pg_fvbn_pack: null pointer");
  hipLaunchKernelGGL(fv_pack_kernel, dim3((unsigned)pg_cdiv(fv_pad(D - 1), 256), (unsigned)D), dim3(256), 0, (hipStream_t)stream, dense, wp, D);
  PG_LAUNCH_CHECK("pg_fvbn_pack");
  return 0;
}

PG_EXPORT int pg_fvbn_unpack(const float* wp, float* dense, int D, void* stream) {
  FvPlan pl;
  const int rc = fv_plan(D, 1, pl, "pg_fvbn_unpack");
  if (rc) return rc;
  PG_REQUIRE(wp && dense, PG_EINVAL, "pg_fvbn_unpack: null pointer");
  hipLaunchKernelGGL(fv_unpack_kernel, dim3((unsigned)pg_cdiv(D, 256), (unsigned)D), dim3(256), 0, (hipStream_t)stream, wp, dense, D);
  PG_LAUNCH_CHECK("pg_fvbn_unpack");
  return 0;
}
