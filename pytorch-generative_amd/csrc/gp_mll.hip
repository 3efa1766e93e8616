// gp_mll.hip — the log marginal likelihood of a Gaussian process and its gradients with respect to the hyperparameters, from
// the factor K = K_f + noise_var I = L L^T that gp.hip caches (r = y - value, z = L^-1 r, alpha = L^-T z):
//     log p(y) = -1/2 sum z^2 - p sum_i log L_ii - (n p / 2) log 2 pi
//     G = alpha alpha^T - p K^-1,   d/d std = sum G K_f / std,   d/d l = sum G K_f D2 / (2 l^3),   d/d noise_var = tr G / 2.
//
// The triangular structure. K^-1 = X X^T with X = L^-T, which is UPPER triangular:
//   * pg_gp_trtri_t solves X L^T = I right-looking in panels of 64 columns at absolute multiples of 64. Row r of X is zero
//     left of column r, so panel k is solved for the rows above its end only: the diagonal block and the blocks above it by
//     the fmaf chain plus one division of gp_common.h's substitution on the VALU (gp_subst_diag_kernel<false, true>: the
//     diagonal block starts from the identity and keeps its upper triangle), then the (k + 1) x (P - 1 - k) tiles to the
//     right on the MFMA, seeded with x — with zero for the row tile k, which is touched for the first time. Element (r, c) is
//     one chain (delta_rc - sum_{k < c} x_rk l_ck) / l_cc in ascending k, as in gp.hip.
//   * pg_gp_gram_upper forms (X X^T)_ij = sum_{k >= max(i, j)} x_ik x_jk for the tiles on or below the diagonal; tile (I, J)
//     starts its k loop at 64 I. What lies below the diagonal of x is garbage and is masked to zero on the way into LDS: it adds
//     exact zeros to a chain in ascending k.
//   Both cost about n^3 / 3 flops, as the factorisation does.
//   * pg_gp_se_mll_sums contracts G with K_f and K_f D2 without writing either: one workgroup per tile on or below the diagonal
//     forms alpha_i . alpha_j on the MFMA, D2 by se_kernel's two routes (same bits), reads the tile of H = X X^T once, and reduces
//     three sums in a fixed order — lane (16 elements in the order of PG_TILE_FOR_EACH_OUTPUT), wave (shuffle tree), the four
//     waves in order — to one fp32 partial row per tile. gp_mll_finish_kernel adds the rows in double: thread t the tiles t,
//     t + 256, ... ascending, then a fixed tree over the 256 threads.
//   * pg_gp_stat_mll_sums is the same reduction for every stationary kind with one shared lengthscale (the kind is a
//     template parameter; pg_gp_se_mll_sums is pg_gp_stat_mll_sums with kind SE), and pg_gp_ard_mll_sums the one for per-dimension
//     lengthscales: d + 2 sums per tile, the per-dimension terms by exact differences on the VALU in two passes over the
//     column chunks of x (gp_ard_mll_sums_kernel); gp_ard_plan decides its domain (d <= 256).
// No float atomics, no host synchronisation, no allocation: capturable, bit-identical from run to run. gp_mll_plan is the one
// function that decides domain and geometry; every entry point calls it and reports a missing device only afterwards.
#include "gp_common.h"

namespace {

constexpr int MLL_DIRECT_LD = GP_SE_DIRECT_D + 1;  // LDS row stride of the rows of x on the exact-difference route
constexpr int MLL_SUMS = 3;                        // sum G K_f, sum G K_f D2, tr G

// Tile t of the triangular enumeration (0, 0), (1, 0), (1, 1), (2, 0), ...: I its row tile, J <= I its column tile.
__device__ __forceinline__ void mll_tri_tile(int t, int& I, int& J) {
  I = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  J = t - I * (I + 1) / 2;
}

// A thread's share of the chunk at absolute column k0 of rows row0 .. row0 + 63 of the upper triangular x: zero below the
// diagonal (k < row: not read), from row R and from column kend on; negated on the way in if NEG.
template <bool NEG>
__device__ __forceinline__ void mll_load_upper(pg_tile::Regs<GP_V>& reg, const float* __restrict__ x, long ldx, int row0, int R, int k0,
                                               int kend, int tid) {
#pragma unroll
  for (int j = 0; j < GP_T * GP_KC / GP_THREADS; ++j) {
    int r, k;
    pg_tile::coord<GP_T, GP_KC, true>(tid + j * GP_THREADS, r, k);
    const int gr = row0 + r, gk = k0 + k;
    const float v = (gr < R && gk < kend && gk >= gr) ? x[(size_t)gr * ldx + gk] : 0.f;
    reg[j] = NEG ? -v : v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The update after panel k (j0 = 64 k): x[r][c] -= sum_{k' < 64} x[r][j0 + k'] l[c][j0 + k'] for the rows r < j0 + 64 and the
// columns c >= j0 + 64, one 64 x 64 tile per workgroup. The row tile of the panel itself has not been written yet: it is
// seeded with zero and its operand is the upper triangle of the diagonal block.
__global__ void __launch_bounds__(GP_THREADS) gp_trtri_update_kernel(const float* __restrict__ l, long ld, float* __restrict__ x, long ldx,
                                                                     int n, int j0, int col_tiles) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  const int r0 = (blockIdx.x / col_tiles) * GP_T, c0 = j0 + GP_T + (blockIdx.x % col_tiles) * GP_T;
  const bool fresh = r0 == j0;
  const pg_tile::Lanes<GP_V> ln;
  const int tid = ln.tid;
  pg_tile::Acc<GP_V> acc;
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {  // the chain continues from x
    const int gr = r0 + li, gc = c0 + lj;
    PG_TILE_OUTPUT(acc) = (!fresh && gc < n) ? x[(size_t)gr * ldx + gc] : 0.f;
  }
  pg_tile::Regs<GP_V> ra, rb;
  auto load = [&](int ch) {
    mll_load_upper<true>(ra, x, ldx, r0, j0 + GP_T, j0 + ch * GP_KC, j0 + GP_T, tid);
    pg_tile::load_operand<GP_V, true>(rb, l + j0, ld, 1, c0, n, ch * GP_KC, GP_T, tid);
  };
  auto store = [&]() {
    pg_tile::store_operand<GP_V, true>(s_a, ra, tid);
    pg_tile::store_operand<GP_V, true>(s_b, rb, tid);
  };
  auto none = [](int) {};
  PG_TILE_PIPELINE(GP_V, false, 0, GP_T / GP_KC, load, store, acc, s_a, s_b, ln, none);
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (gc < n) x[(size_t)gr * ldx + gc] = PG_TILE_OUTPUT(acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// H = X X^T on the tiles on or below the diagonal: tile (I, J) sums k from 64 I on.
__global__ void __launch_bounds__(GP_THREADS) gp_gram_upper_kernel(const float* __restrict__ x, long ldx, int n, float* __restrict__ h,
                                                                   long ldh, int mirror) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  int I, J;
  mll_tri_tile(blockIdx.x, I, J);
  const int r0 = I * GP_T, c0 = J * GP_T;
  const pg_tile::Lanes<GP_V> ln;
  const int tid = ln.tid;
  pg_tile::Acc<GP_V> acc;
  pg_tile::zero<GP_V>(acc);
  pg_tile::Regs<GP_V> ra, rb;
  auto load = [&](int ch) {
    mll_load_upper<false>(ra, x, ldx, r0, n, ch * GP_KC, n, tid);
    mll_load_upper<false>(rb, x, ldx, c0, n, ch * GP_KC, n, tid);
  };
  auto store = [&]() {
    pg_tile::store_operand<GP_V, true>(s_a, ra, tid);
    pg_tile::store_operand<GP_V, true>(s_b, rb, tid);
  };
  auto none = [](int) {};
  PG_TILE_PIPELINE(GP_V, false, r0 / GP_KC, (n + GP_KC - 1) / GP_KC, load, store, acc, s_a, s_b, ln, none);  // r0 < n: a chunk at least
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (!(gr < n && gc <= gr)) continue;
    h[(size_t)gr * ldh + gc] = PG_TILE_OUTPUT(acc);
    if (mirror && gc != gr) h[(size_t)gc * ldh + gr] = PG_TILE_OUTPUT(acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The reduction. ROUTE 0: exact differences (d <= 16), ROUTE 1: |a|^2 + |b|^2 - 2 a.b on the MFMA, clamped at 0.
struct GpMllSumsArgs {
  const float* x;
  const float* h;
  const float* at;
  float* ws;
  long ldx, ldh, lda;
  int n, d, p;
  float std2, neg_inv, pf;
  float inv_l2;    // the shared-lengthscale kinds other than SE: r^2 = D2 inv_l2
  const float* w;  // the ARD reduction: 1 / l per column
};

// g = alpha_i . alpha_j over the p columns of y for the tile at (r0, c0), on the MFMA for every p.
__device__ __forceinline__ void mll_alpha_outer(const GpMllSumsArgs& p, int r0, int c0, float* s_a, float* s_b, const pg_tile::Lanes<GP_V>& ln,
                                                pg_tile::Acc<GP_V>& g) {
  const int tid = ln.tid;
  pg_tile::zero<GP_V>(g);
  pg_tile::Regs<GP_V> ra, rb;
  auto load = [&](int ch) {
    pg_tile::load_operand<GP_V, false>(ra, p.at, 1, p.lda, r0, p.n, ch * GP_KC, p.p, tid);
    pg_tile::load_operand<GP_V, false>(rb, p.at, 1, p.lda, c0, p.n, ch * GP_KC, p.p, tid);
  };
  auto store = [&]() {
    pg_tile::store_operand<GP_V, false>(s_a, ra, tid);
    pg_tile::store_operand<GP_V, false>(s_b, rb, tid);
  };
  auto none = [](int) {};
  PG_TILE_PIPELINE(GP_V, false, 0, (p.p + GP_KC - 1) / GP_KC, load, store, g, s_a, s_b, ln, none);
}

// KIND = PG_GP_KIND_SE is the reduction as it always was (sum G K_f, sum G K_f D2, tr G; the finish applies 1 / (2 l^3)). The
// Matern kinds take K_f = std^2 phi(r) and accumulate G std^2 omega(r) r^2 as the second sum (the finish applies 1 / (2 l)).
template <int ROUTE, int KIND>
__global__ void __launch_bounds__(GP_THREADS) gp_se_mll_sums_kernel(const GpMllSumsArgs p) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  __shared__ float s_n[2 * GP_T];
  __shared__ float s_red[4 * MLL_SUMS];
  int I, J;
  mll_tri_tile(blockIdx.x, I, J);
  const int r0 = I * GP_T, c0 = J * GP_T;
  const pg_tile::Lanes<GP_V> ln;
  const int tid = ln.tid;

  // alpha_i . alpha_j over the p columns of y: alpha^T is (p, n), so both operands are row-contiguous
  pg_tile::Acc<GP_V> g;
  mll_alpha_outer(p, r0, c0, s_a, s_b, ln, g);

  // the squared distances, with the bits of se_kernel's route
  pg_tile::Acc<GP_V> sq;
  pg_tile::zero<GP_V>(sq);
  if (ROUTE == 0) {
    GP_STAGE_ROWS(MLL_DIRECT_LD, s_a, s_b, p.x, p.ldx, r0, p.n, p.x, p.ldx, c0, p.n, 0, p.d, tid);
    __syncthreads();
    // Not an unscaled GpLaneDiffs, which is the same arithmetic: with it sums_ms of tools/gp_mll_bench.py at d = 1 read
    // 1.01 / 1.06 / 1.05 of the parent at n = 8192 in three visits, beside 1.00 / 1.01 / 1.02 for the untouched MFMA route at
    // d = 64 (profiles/gp_one_path.json). Written out, the kernel compiles to the parent's instructions.
    for (int k = 0; k < p.d; ++k) {
      float av[2][4], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) av[i][q] = s_a[pg_tile::out_row<GP_V>(ln, i, q) * MLL_DIRECT_LD + k];
        bv[i] = s_b[pg_tile::out_col<GP_V>(ln, i) * MLL_DIRECT_LD + k];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float df = av[i][q] - bv[j];
            sq[i][j][q] = fmaf(df, df, sq[i][j][q]);
          }
    }
  } else {
    GpMma m;
    m.a = p.x;
    m.b = p.x;
    m.a_rs = p.ldx;
    m.b_rs = p.ldx;
    m.b_ks = 1;
    m.R = p.n;
    m.C = p.n;
    m.K = p.d;
    float norm = 0.f;
    gp_mma_tile<true, false, true>(m, r0, c0, s_a, s_b, ln, sq, norm);
    if (tid < 2 * GP_T) s_n[tid] = norm;
    __syncthreads();
    PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, r, c) {
      PG_TILE_OUTPUT(sq) = fmaxf(fmaf(-2.f, PG_TILE_OUTPUT(sq), s_n[r] + s_n[GP_T + c]), 0.f);
    }
  }

  float sum[MLL_SUMS] = {0.f, 0.f, 0.f};
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (!(gr < p.n && gc <= gr)) continue;
    const float gv = fmaf(-p.pf, p.h[(size_t)gr * p.ldh + gc], PG_TILE_OUTPUT(g));
    if (gc == gr) {  // K_f = std^2 and D2 = 0 exactly
      sum[0] = fmaf(gv, p.std2, sum[0]);
      sum[2] += gv;
    } else {  // (i, j) and (j, i)
      const float d2 = PG_TILE_OUTPUT(sq);
      if (KIND == PG_GP_KIND_SE) {
        const float t = 2.f * gv * (p.std2 * expf(d2 * p.neg_inv));
        sum[0] += t;
        sum[1] = fmaf(t, d2, sum[1]);
      } else {
        const float r2 = d2 * p.inv_l2;
        float phi, omega;
        gp_stat_phi_omega<KIND>(r2, phi, omega);
        const float t = 2.f * gv * p.std2;
        sum[0] = fmaf(t, phi, sum[0]);
        sum[1] = fmaf(t * omega, r2, sum[1]);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < MLL_SUMS; ++s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum[s] += __shfl_down(sum[s], off);
    if ((tid & 63) == 0) s_red[(tid >> 6) * MLL_SUMS + s] = sum[s];
  }
  __syncthreads();
  if (tid < MLL_SUMS)
    p.ws[(size_t)blockIdx.x * MLL_SUMS + tid] =
        ((s_red[tid] + s_red[MLL_SUMS + tid]) + s_red[2 * MLL_SUMS + tid]) + s_red[3 * MLL_SUMS + tid];
}

// ---------------------------------------------------------------------------------------------------------------------------
// The ARD reduction: per tile on or below the diagonal, sum G K_f, tr G and, for every column c of x,
//     S_c = sum_ij G_ij std^2 omega(r_ij) ((x_ic - x_jc) w_c)^2          (off-diagonal elements twice, the diagonal adds 0).
// G as above (alpha_i . alpha_j on the MFMA, minus p h from the lower triangle). The per-dimension terms are exact differences
// on the VALU: the rows of x go through LDS in chunks of at most 64 columns, TWICE — pass 1 sums r^2 = sum_c ((x_ic - x_jc) w_c)^2
// in ascending c and turns it into the coefficient 2 G std^2 omega(r) of each of a thread's 16 elements (kept in the registers
// r^2 had), pass 2 forms the squares again and adds coefficient x square per column: 16 elements in the order of
// PG_TILE_FOR_EACH_OUTPUT, the wave by a shuffle tree, the four waves in order. With one chunk (d <= 64) the rows are staged once.
// One partial row of d + 2 floats per tile: [sum G K_f, tr G, S_0 .. S_{d-1}].
constexpr int ARD_LD = GP_ARD_CHUNK + 1;

template <int KIND>
__global__ void __launch_bounds__(GP_THREADS) gp_ard_mll_sums_kernel(const GpMllSumsArgs p) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  __shared__ float s_xa[GP_T * ARD_LD];
  __shared__ float s_xb[GP_T * ARD_LD];
  __shared__ float s_w[GP_ARD_CHUNK];
  __shared__ float s_col[4 * GP_ARD_MAX_D];
  __shared__ float s_red[4 * 2];
  int I, J;
  mll_tri_tile(blockIdx.x, I, J);
  const int r0 = I * GP_T, c0 = J * GP_T;
  const pg_tile::Lanes<GP_V> ln;
  const int tid = ln.tid;

  pg_tile::Acc<GP_V> g;
  mll_alpha_outer(p, r0, c0, s_a, s_b, ln, g);

  const int chunks = (p.d + GP_ARD_CHUNK - 1) / GP_ARD_CHUNK;
  auto stage = [&](int k0, int kc) {
    __syncthreads();  // the readers of the chunk before are done
    GP_STAGE_ROWS(ARD_LD, s_xa, s_xb, p.x, p.ldx, r0, p.n, p.x, p.ldx, c0, p.n, k0, kc, tid);
    if (tid < kc) s_w[tid] = p.w[k0 + tid];
    __syncthreads();
  };
  GpLaneDiffs<ARD_LD> df(ln);  // the rows of x behind a thread's elements

  // pass 1: r^2, then the coefficients
  pg_tile::Acc<GP_V> sq;
  pg_tile::zero<GP_V>(sq);
  for (int ch = 0; ch < chunks; ++ch) {
    const int k0 = ch * GP_ARD_CHUNK, kc = min(GP_ARD_CHUNK, p.d - k0);
    stage(k0, kc);
    for (int k = 0; k < kc; ++k) {
      df.fetch(s_xa, s_xb, k);
      df.add_squares(sq, s_w[k]);
    }
  }
  float sum[2] = {0.f, 0.f};  // sum G K_f, tr G
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    float coef = 0.f;
    if (gr < p.n && gc <= gr) {
      const float gv = fmaf(-p.pf, p.h[(size_t)gr * p.ldh + gc], PG_TILE_OUTPUT(g));
      if (gc == gr) {  // K_f = std^2 exactly, and every difference is 0
        sum[0] = fmaf(gv, p.std2, sum[0]);
        sum[1] += gv;
      } else {  // (i, j) and (j, i)
        float phi, omega;
        gp_stat_phi_omega<KIND>(PG_TILE_OUTPUT(sq), phi, omega);
        const float t = 2.f * gv * p.std2;
        sum[0] = fmaf(t, phi, sum[0]);
        coef = t * omega;
      }
    }
    PG_TILE_OUTPUT(sq) = coef;
  }

  // pass 2: per column, coefficient x ((x_ic - x_jc) w_c)^2
  for (int ch = 0; ch < chunks; ++ch) {
    const int k0 = ch * GP_ARD_CHUNK, kc = min(GP_ARD_CHUNK, p.d - k0);
    if (chunks > 1) stage(k0, kc);
    for (int k = 0; k < kc; ++k) {
      const float wk = s_w[k];
      df.fetch(s_xa, s_xb, k);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float dv = df.diff(i, j, q, wk);
            s = fmaf(sq[i][j][q], dv * dv, s);
          }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
      if ((tid & 63) == 0) s_col[(tid >> 6) * GP_ARD_MAX_D + k0 + k] = s;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum[k] += __shfl_down(sum[k], off);
    if ((tid & 63) == 0) s_red[(tid >> 6) * 2 + k] = sum[k];
  }
  __syncthreads();
  float* row = p.ws + (size_t)blockIdx.x * (p.d + 2);
  if (tid < 2) row[tid] = ((s_red[tid] + s_red[2 + tid]) + s_red[4 + tid]) + s_red[6 + tid];
  if (tid < p.d)  // d <= 256 = the threads of the workgroup
    row[2 + tid] = ((s_col[tid] + s_col[GP_ARD_MAX_D + tid]) + s_col[2 * GP_ARD_MAX_D + tid]) + s_col[3 * GP_ARD_MAX_D + tid];
}

// The sum of `len` doubles per thread slot, a fixed tree over the 256 threads; the total is in s[0 .. len) afterwards.
template <int LEN>
__device__ __forceinline__ void mll_tree(double* s, const double (&v)[LEN], int tid) {
#pragma unroll
  for (int k = 0; k < LEN; ++k) s[k * GP_THREADS + tid] = v[k];
  __syncthreads();
  for (int half = GP_THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int k = 0; k < LEN; ++k) s[k * GP_THREADS + tid] += s[k * GP_THREADS + tid + half];
    }
    __syncthreads();
  }
}

// inv_2l3: what the second sum is scaled by, 1 / (2 l^3) for the squared exponential and 1 / (2 l) for the other kinds
__global__ void __launch_bounds__(GP_THREADS) gp_mll_finish_kernel(const float* __restrict__ ws, int tiles, double inv_std, double inv_2l3,
                                                                   float* __restrict__ out) {
  __shared__ double s[MLL_SUMS * GP_THREADS];
  const int tid = threadIdx.x;
  double v[MLL_SUMS] = {0., 0., 0.};
  for (int t = tid; t < tiles; t += GP_THREADS) {
#pragma unroll
    for (int k = 0; k < MLL_SUMS; ++k) v[k] += (double)ws[(size_t)t * MLL_SUMS + k];
  }
  mll_tree<MLL_SUMS>(s, v, tid);
  if (tid == 0) {
    out[0] = (float)(s[0] * inv_std);
    out[1] = (float)(s[GP_THREADS] * inv_2l3);
    out[2] = (float)(0.5 * s[2 * GP_THREADS]);
  }
}

// The ARD finish: workgroup c adds column c of the partial rows in double — thread t the tiles t, t + 256, ... ascending, then
// the fixed tree — and applies 1 / std (c = 0), 1 / 2 (c = 1) or 1 / (2 l) = w / 2 of its column.
__global__ void __launch_bounds__(GP_THREADS) gp_ard_finish_kernel(const float* __restrict__ ws, int tiles, int row_floats, double inv_std,
                                                                   const float* __restrict__ w, float* __restrict__ out) {
  __shared__ double s[GP_THREADS];
  const int tid = threadIdx.x, c = blockIdx.x;
  double v[1] = {0.};
  for (int t = tid; t < tiles; t += GP_THREADS) v[0] += (double)ws[(size_t)t * row_floats + c];
  mll_tree<1>(s, v, tid);
  if (tid == 0) {
    const double scale = c == 0 ? inv_std : (c == 1 ? 0.5 : 0.5 * (double)w[c - 2]);
    out[c] = (float)(s[0] * scale);
  }
}

// log p(y) and sum alpha: one workgroup, thread t the elements t, t + 256, ... of every row ascending, then the fixed tree.
__global__ void __launch_bounds__(GP_THREADS) gp_mll_value_kernel(const float* __restrict__ l, long ld, int n, const float* __restrict__ zt,
                                                                  long ldz, const float* __restrict__ at, long lda, int p,
                                                                  float* __restrict__ out) {
  __shared__ double s[3 * GP_THREADS];
  const int tid = threadIdx.x;
  double v[3] = {0., 0., 0.};  // sum z^2, sum log L_ii, sum alpha
  for (int c = 0; c < p; ++c)
    for (int i = tid; i < n; i += GP_THREADS) {
      const double z = (double)zt[(size_t)c * ldz + i];
      v[0] = fma(z, z, v[0]);
      v[2] += (double)at[(size_t)c * lda + i];
    }
  for (int i = tid; i < n; i += GP_THREADS) v[1] += log((double)l[(size_t)i * ld + i]);
  mll_tree<3>(s, v, tid);
  if (tid == 0) {
    const double log_2pi = 1.8378770664093454835606594728112;
    out[0] = (float)(-0.5 * s[0] - (double)p * s[GP_THREADS] - 0.5 * (double)n * (double)p * log_2pi);
    out[1] = (float)s[2 * GP_THREADS];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The one function that decides the domain (gp_plan's) and the geometry of everything above.
struct GpMllPlan {
  int panels, se_route, p_chunks;
  long trtri_launches, trtri_products, tiles, gram_products, ws_floats;
};

int gp_mll_plan(int n, int d, int p, GpMllPlan& ml, const char* name) {
  GP_PLAN_OR_RETURN(pl, n, 1, d, p, name);
  const long P = pl.panels;
  ml.panels = pl.panels;
  ml.se_route = pl.se_route;
  ml.p_chunks = pg_cdiv(p, GP_KC);
  ml.trtri_launches = 2 * P - 1;                 // a substitution per panel, an update after every panel but the last
  ml.trtri_products = (P - 1) * P * (P + 1) / 6;  // sum_k (k + 1)(P - 1 - k)
  ml.tiles = P * (P + 1) / 2;
  ml.gram_products = P * (P + 1) * (P + 2) / 6;  // sum_I (I + 1)(P - I)
  ml.ws_floats = MLL_SUMS * ml.tiles;
  return 0;
}

// The domain and the geometry of the ARD reduction: gp_mll_plan's, and d <= 256.
struct GpArdPlan {
  long tiles, row_floats, ws_floats;
  int chunks;
};

int gp_ard_plan(int n, int d, int p, GpArdPlan& ap, const char* name) {
  GpMllPlan ml;
  const int rc = gp_mll_plan(n, d, p, ml, name);
  if (rc) return rc;
  PG_REQUIRE(d <= GP_ARD_MAX_D, PG_ESHAPE, "%s: d = %d: per-dimension lengthscale gradients are built for at most %d input columns", name, d,
             GP_ARD_MAX_D);
  ap.tiles = ml.tiles;
  ap.row_floats = d + 2;
  ap.ws_floats = ap.tiles * ap.row_floats;
  ap.chunks = pg_cdiv(d, GP_ARD_CHUNK);
  return 0;
}

#define GP_MLL_PLAN_OR_RETURN(ml, n, d, p, name)      \
  GpMllPlan ml;                                       \
  {                                                   \
    const int rc__ = gp_mll_plan(n, d, p, ml, name);  \
    if (rc__) return rc__;                            \
  }                                                   \
  (void)ml;

}  // namespace

PG_EXPORT int pg_gp_mll_plan(int n, int d, int p, long long* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_GP_MLL_PLAN_INTS, PG_EINVAL, "pg_gp_mll_plan: null pointer or short output array");
  GP_MLL_PLAN_OR_RETURN(ml, n, d, p, "pg_gp_mll_plan");
  out[0] = GP_T;
  out[1] = ml.panels;
  out[2] = ml.trtri_launches;
  out[3] = ml.trtri_products;
  out[4] = ml.tiles;
  out[5] = ml.gram_products;
  out[6] = ml.tiles;
  out[7] = ml.tiles;
  out[8] = ml.ws_floats;
  out[9] = ml.se_route;
  out[10] = GP_SE_DIRECT_D;
  out[11] = GP_MAX_N;
  out[12] = GP_MAX_D;
  out[13] = GP_MAX_P;
  out[14] = ml.p_chunks;
  out[15] = 2;
  return 0;
}

PG_EXPORT int pg_gp_trtri_t(const float* l, long ld, int n, float* x, long ldx, void* stream) {
  GP_MLL_PLAN_OR_RETURN(ml, n, 1, 1, "pg_gp_trtri_t");
  PG_REQUIRE(l && x && ld >= n && ldx >= n, PG_EINVAL, "pg_gp_trtri_t: null pointer or a row stride below the row length");
  PG_REQUIRE(l != x, PG_EINVAL, "pg_gp_trtri_t: x must not be l (they share the diagonal)");
  GP_TRY(gp_device("pg_gp_trtri_t"));
  const hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < ml.panels; ++k) {
    const int j0 = k * GP_T, jb = std::min(GP_T, n - j0), right = ml.panels - 1 - k;
    hipLaunchKernelGGL((gp_subst_diag_kernel<false, true>), dim3((unsigned)(k + 1)), dim3(GP_THREADS), 0, st, l + (size_t)j0 * ld + j0, ld,
                       x + j0, ldx, j0 + jb, jb, 0);
    PG_LAUNCH_CHECK("pg_gp_trtri_t");
    if (right > 0) {
      hipLaunchKernelGGL(gp_trtri_update_kernel, dim3((unsigned)((k + 1) * right)), dim3(GP_THREADS), 0, st, l, ld, x, ldx, n, j0, right);
      PG_LAUNCH_CHECK("pg_gp_trtri_t");
    }
  }
  return 0;
}

PG_EXPORT int pg_gp_gram_upper(const float* x, long ldx, int n, float* h, long ldh, int flags, void* stream) {
  GP_MLL_PLAN_OR_RETURN(ml, n, 1, 1, "pg_gp_gram_upper");
  PG_REQUIRE(x && h && ldx >= n && ldh >= n, PG_EINVAL, "pg_gp_gram_upper: null pointer or a row stride below the row length");
  PG_REQUIRE((flags & ~PG_GP_MIRROR) == 0, PG_EINVAL, "pg_gp_gram_upper: flags %d", flags);
  PG_REQUIRE(x != h, PG_EINVAL, "pg_gp_gram_upper: h must not be x (they share the diagonal)");
  GP_TRY(gp_device("pg_gp_gram_upper"));
  hipLaunchKernelGGL(gp_gram_upper_kernel, dim3((unsigned)ml.tiles), dim3(GP_THREADS), 0, (hipStream_t)stream, x, ldx, n, h, ldh,
                     (flags & PG_GP_MIRROR) != 0);
  PG_LAUNCH_CHECK("pg_gp_gram_upper");
  return 0;
}

namespace {

// What the two reductions check after their plan accepted the call, and the arguments of their kernels. inv_ls: the per-dimension
// reduction's 1 / l (`ard`; the scalar lengthscale is then 1 and not checked), else NULL. A missing device is reported last.
int gp_mll_sums_args(const char* name, int kind, const float* x, long ldx, int n, int d, float std, float lengthscale, bool ard,
                     const float* inv_ls, const float* h, long ldh, const float* alpha_t, long lda, int p, float* ws, size_t ws_floats,
                     long ws_needed, const float* out, GpMllSumsArgs& a) {
  PG_REQUIRE(gp_kind_known(kind), PG_EINVAL, "%s: kind %d is none of PG_GP_KIND_*", name, kind);
  PG_REQUIRE(x && (inv_ls || !ard) && h && alpha_t && ws && out, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(ldx >= d && ldh >= n && lda >= n, PG_EINVAL, "%s: a row stride below its row length", name);
  if (ard)
    PG_REQUIRE(std == std && std != 0.f, PG_EINVAL, "%s: std = %g no NaN and not 0", name, (double)std);
  else
    PG_REQUIRE(lengthscale > 0.f && std == std && std != 0.f, PG_EINVAL, "%s: lengthscale = %g must be > 0, std = %g no NaN and not 0", name,
               (double)lengthscale, (double)std);
  PG_REQUIRE(ws_floats >= (size_t)ws_needed, PG_EINVAL, "%s: the workspace holds %zu floats, %ld are needed", name, ws_floats, ws_needed);
  GP_TRY(gp_device(name));
  a.x = x;
  a.h = h;
  a.at = alpha_t;
  a.ws = ws;
  a.ldx = ldx;
  a.ldh = ldh;
  a.lda = lda;
  a.n = n;
  a.d = d;
  a.p = p;
  a.std2 = std * std;
  a.neg_inv = -0.5f / (lengthscale * lengthscale);
  a.pf = (float)p;
  a.inv_l2 = 1.f / (lengthscale * lengthscale);
  a.w = inv_ls;
  return 0;
}

// the one launch path of pg_gp_se_mll_sums (kind SE) and pg_gp_stat_mll_sums
int gp_stat_mll_sums(const char* name, int kind, const float* x, long ldx, int n, int d, float std, float lengthscale, const float* h, long ldh,
                     const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream) {
  GP_MLL_PLAN_OR_RETURN(ml, n, d, p, name);
  GpMllSumsArgs a;
  GP_TRY(gp_mll_sums_args(name, kind, x, ldx, n, d, std, lengthscale, false, nullptr, h, ldh, alpha_t, lda, p, ws, ws_floats, ml.ws_floats, out, a));
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ml.tiles), block(GP_THREADS);
  gp_with_kind(kind, [&](auto K) {
    if (ml.se_route == 0)
      hipLaunchKernelGGL((gp_se_mll_sums_kernel<0, decltype(K)::value>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((gp_se_mll_sums_kernel<1, decltype(K)::value>), grid, block, 0, st, a);
  });
  PG_LAUNCH_CHECK(name);
  const double l3 = (double)lengthscale * (double)lengthscale * (double)lengthscale;
  const double scale = kind == PG_GP_KIND_SE ? 0.5 / l3 : 0.5 / (double)lengthscale;
  hipLaunchKernelGGL(gp_mll_finish_kernel, dim3(1), dim3(GP_THREADS), 0, st, (const float*)ws, (int)ml.tiles, 1.0 / (double)std, scale, out);
  PG_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace

PG_EXPORT int pg_gp_se_mll_sums(const float* x, long ldx, int n, int d, float std, float lengthscale, const float* h, long ldh,
                                const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream) {
  return gp_stat_mll_sums("pg_gp_se_mll_sums", PG_GP_KIND_SE, x, ldx, n, d, std, lengthscale, h, ldh, alpha_t, lda, p, ws, ws_floats, out, stream);
}

PG_EXPORT int pg_gp_stat_mll_sums(int kind, const float* x, long ldx, int n, int d, float std, float lengthscale, const float* h, long ldh,
                                  const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream) {
  return gp_stat_mll_sums("pg_gp_stat_mll_sums", kind, x, ldx, n, d, std, lengthscale, h, ldh, alpha_t, lda, p, ws, ws_floats, out, stream);
}

PG_EXPORT int pg_gp_ard_plan(int n, int d, int p, long long* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_GP_ARD_PLAN_INTS, PG_EINVAL, "pg_gp_ard_plan: null pointer or short output array");
  GpArdPlan ap;
  GP_TRY(gp_ard_plan(n, d, p, ap, "pg_gp_ard_plan"));
  out[0] = GP_T;
  out[1] = ap.tiles;
  out[2] = ap.row_floats;
  out[3] = ap.ws_floats;
  out[4] = ap.chunks;
  out[5] = 2;
  out[6] = GP_ARD_MAX_D;
  out[7] = GP_ARD_CHUNK;
  return 0;
}

PG_EXPORT int pg_gp_ard_mll_sums(int kind, const float* x, long ldx, int n, int d, float std, const float* inv_ls, const float* h, long ldh,
                                 const float* alpha_t, long lda, int p, float* ws, size_t ws_floats, float* out, void* stream) {
  const char* name = "pg_gp_ard_mll_sums";
  GpArdPlan ap;
  GP_TRY(gp_ard_plan(n, d, p, ap, name));
  GpMllSumsArgs a;
  GP_TRY(gp_mll_sums_args(name, kind, x, ldx, n, d, std, 1.f, true, inv_ls, h, ldh, alpha_t, lda, p, ws, ws_floats, ap.ws_floats, out, a));
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ap.tiles), block(GP_THREADS);
  gp_with_kind(kind, [&](auto K) { hipLaunchKernelGGL(gp_ard_mll_sums_kernel<decltype(K)::value>, grid, block, 0, st, a); });
  PG_LAUNCH_CHECK(name);
  hipLaunchKernelGGL(gp_ard_finish_kernel, dim3((unsigned)ap.row_floats), block, 0, st, (const float*)ws, (int)ap.tiles, (int)ap.row_floats,
                     1.0 / (double)std, inv_ls, out);
  PG_LAUNCH_CHECK(name);
  return 0;
}

PG_EXPORT int pg_gp_mll_value(const float* l, long ld, int n, const float* zt, long ldz, const float* alpha_t, long lda, int p, float* out,
                              void* stream) {
  GP_MLL_PLAN_OR_RETURN(ml, n, 1, p, "pg_gp_mll_value");
  PG_REQUIRE(l && zt && alpha_t && out, PG_EINVAL, "pg_gp_mll_value: null pointer");
  PG_REQUIRE(ld >= n && ldz >= n && lda >= n, PG_EINVAL, "pg_gp_mll_value: a row stride below its row length");
  GP_TRY(gp_device("pg_gp_mll_value"));
  hipLaunchKernelGGL(gp_mll_value_kernel, dim3(1), dim3(GP_THREADS), 0, (hipStream_t)stream, l, ld, n, zt, ldz, alpha_t, lda, p, out);
  PG_LAUNCH_CHECK("pg_gp_mll_value");
  return 0;
}
