// gp.hip — the dense symmetric solve of a Gaussian process (reference models/gaussian_process.py): squared-exponential
// covariance, a blocked right-looking fp32 Cholesky factorisation that can be APPENDED to, the triangular solves X L^T = B and
// X L = B, and the strided GEMM update C = C -/+ A B^T they are built from. Everything is fp32 and every operand is a row-major
// matrix with a leading dimension in floats, so a factor lives in a buffer larger than itself.
//
// The chain-order property. Element (i, j) of the factor is
//     l_ij = (a_ij - sum_{k < j} l_ik l_jk) / l_jj          (a square root on the diagonal),
// and every kernel here forms that sum as ONE chain v = fmaf(-l_ik, l_jk, v) in ascending k that starts from a_ij:
//   * gp_gemm_kernel seeds its accumulators with the tile of C and multiplies -A on the tile of mfma_tile.h, whose sums are one
//     fmaf chain per output in k order from whatever the accumulator held: a trailing update applied panel after panel
//     continues the same chain, whatever the blocking;
//   * gp_potrf_diag_kernel and gp_subst_diag_kernel (gp_common.h) continue it on the VALU inside the panel of 64 columns that
//     holds j, then take one square root or one IEEE division (no explicit inverse of a diagonal block).
// The chain of an element therefore does not depend on how many rows the matrix had when its row was factored: completing rows
// n_done .. n of a factor (pg_gp_potrf with n_done > 0) gives the bits of the full factorisation. Panels sit at absolute
// multiples of 64; the MFMA only multiplies whole finished panels, the panel that contains n_done is finished on the VALU.
//
// No float atomics, each output element is owned by one lane, every order is fixed by the shape: bit-identical from run to
// run. No host synchronisation and no allocation: capturable. gp_plan is the one function that decides the domain and the
// geometry; every entry point calls it, and reports a missing device only after it accepted the problem.
//
// Stationary kernels. The covariance kernels are templated on the kind (squared exponential, Matern 3/2, Matern 5/2) and on
// per-dimension (ARD) lengthscales w_c = 1 / l_c; pg_gp_se_kernel is pg_gp_stat_kernel with kind SE and no inv_ls. With
// ARD the exact-difference route forms (a_c - b_c) w_c and the MFMA route SCALES THE ROWS WHILE STAGING them into LDS
// (gp_mma_tile's SCALE): one launch either way, no scaled copy of the rows, an element's bits depend on its two rows and w alone.
#include "gp_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// C = C -/+ A B^T. The accumulators are seeded with the tile of C. lower: only elements with c <= r + diag_off are read and
// written, tiles wholly above that line return at once; mirror (square, diag_off = 0): C[c][r] = C[r][c] too.
struct GpGemmArgs {
  GpMma m;
  float* c;
  long ldc;
  int diag_off, lower, mirror, col_tiles;
};

template <bool BK, bool NEG>
__global__ void __launch_bounds__(GP_THREADS) gp_gemm_kernel(const GpGemmArgs p) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  const int r0 = (blockIdx.x / p.col_tiles) * GP_T, c0 = (blockIdx.x % p.col_tiles) * GP_T;
  if (p.lower && c0 > r0 + (GP_T - 1) + p.diag_off) return;
  const pg_tile::Lanes<GP_V> ln;
  pg_tile::Acc<GP_V> acc;
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {  // the chain continues from C
    const int gr = r0 + li, gc = c0 + lj;
    const bool ok = gr < p.m.R && gc < p.m.C && (!p.lower || gc <= gr + p.diag_off);
    PG_TILE_OUTPUT(acc) = ok ? p.c[(size_t)gr * p.ldc + gc] : 0.f;
  }
  float unused = 0.f;
  gp_mma_tile<BK, NEG, false>(p.m, r0, c0, s_a, s_b, ln, acc, unused);
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, li, lj) {
    const int gr = r0 + li, gc = c0 + lj;
    if (!(gr < p.m.R && gc < p.m.C && (!p.lower || gc <= gr + p.diag_off))) continue;
    p.c[(size_t)gr * p.ldc + gc] = PG_TILE_OUTPUT(acc);
    if (p.mirror && gc != gr) p.c[(size_t)gc * p.ldc + gr] = PG_TILE_OUTPUT(acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Stationary covariance K[i][j] = std^2 phi(r) (gp_common.h), templated on the kind and on ARD. The squared-exponential kernel
// with one shared lengthscale, <PG_GP_KIND_SE, false>, is K[i][j] = std^2 exp(-|a_i - b_j|^2 / (2 l^2)) as it always was:
// neg_inv = -1 / (2 l^2) and std2 come from the host. The other shared-lengthscale kinds take r^2 = |a_i - b_j|^2 inv_l2; with
// ARD the distances arrive scaled by w = 1 / l per column (the exact-difference route forms (a_c - b_c) w_c, difference first;
// the MFMA route SCALES THE ROWS WHILE STAGING them into LDS: no extra launch, no scaled copy of the rows kept anywhere).
// lower / mirror as in the GEMM; diag: elements with j == i + diag_off are written as exactly diag_val.
struct GpSeArgs {
  const float* a;
  const float* b;
  float* k;
  long lda, ldb, ldk;
  int n, m, d, diag_off, lower, mirror, diag, col_tiles;
  float std2, neg_inv, diag_val;
  const float* w;
  float inv_l2;
};

template <int KIND, bool ARD>
__device__ __forceinline__ void gp_se_store(const GpSeArgs& p, int gr, int gc, float sq) {
  if (!(gr < p.n && gc < p.m && (!p.lower || gc <= gr + p.diag_off))) return;
  float v;
  if (KIND == PG_GP_KIND_SE && !ARD) {
    v = p.std2 * expf(sq * p.neg_inv);
  } else {
    float phi, omega;
    gp_stat_phi_omega<KIND>(ARD ? sq : sq * p.inv_l2, phi, omega);
    v = p.std2 * phi;
  }
  if (p.diag && gc == gr + p.diag_off) v = p.diag_val;
  p.k[(size_t)gr * p.ldk + gc] = v;
  if (p.mirror && gc != gr) p.k[(size_t)gc * p.ldk + gr] = v;
}

// exact differences sum_k (a_ik - b_jk)^2 on the VALU, k ascending; d <= 64. A thread owns 4 x 4 elements of the tile.
// ARD: sum_k ((a_ik - b_jk) w_k)^2.
template <int KIND, bool ARD>
__global__ void __launch_bounds__(GP_THREADS) gp_se_direct_kernel(const GpSeArgs p) {
  __shared__ float s_a[GP_T * GP_TRI_LD];
  __shared__ float s_b[GP_T * GP_TRI_LD];
  __shared__ float s_w[ARD ? GP_SE_DIRECT_MAX_D : 1];
  const int r0 = (blockIdx.x / p.col_tiles) * GP_T, c0 = (blockIdx.x % p.col_tiles) * GP_T;
  if (p.lower && c0 > r0 + (GP_T - 1) + p.diag_off) return;
  const int tid = threadIdx.x;
  GP_STAGE_ROWS(GP_TRI_LD, s_a, s_b, p.a, p.lda, r0, p.n, p.b, p.ldb, c0, p.m, 0, p.d, tid);
  if (ARD && tid < p.d) s_w[tid] = p.w[tid];
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  float sq[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) sq[i][j] = 0.f;
  for (int k = 0; k < p.d; ++k) {
    float av[4], bv[4];
    const float wk = ARD ? s_w[k] : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      av[i] = s_a[(ty + 16 * i) * GP_TRI_LD + k];
      bv[i] = s_b[(tx + 16 * i) * GP_TRI_LD + k];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float df = av[i] - bv[j];
        if (ARD) df *= wk;
        sq[i][j] = fmaf(df, df, sq[i][j]);
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) gp_se_store<KIND, ARD>(p, r0 + ty + 16 * i, c0 + tx + 16 * j, sq[i][j]);
}

// |a|^2 + |b|^2 - 2 a.b with the cross term on the MFMA, clamped at 0 before the exp (and the square root). ARD: of the rows
// scaled by w on their way into LDS.
template <int KIND, bool ARD>
__global__ void __launch_bounds__(GP_THREADS) gp_se_mfma_kernel(const GpSeArgs p) {
  __shared__ float s_a[GP_T * GP_LD];
  __shared__ float s_b[GP_T * GP_LD];
  __shared__ float s_n[2 * GP_T];
  const int r0 = (blockIdx.x / p.col_tiles) * GP_T, c0 = (blockIdx.x % p.col_tiles) * GP_T;
  if (p.lower && c0 > r0 + (GP_T - 1) + p.diag_off) return;
  const pg_tile::Lanes<GP_V> ln;
  GpMma m;
  m.a = p.a;
  m.b = p.b;
  m.a_rs = p.lda;
  m.b_rs = p.ldb;
  m.b_ks = 1;
  m.R = p.n;
  m.C = p.m;
  m.K = p.d;
  m.w = p.w;
  pg_tile::Acc<GP_V> acc;
  pg_tile::zero<GP_V>(acc);
  float norm = 0.f;
  gp_mma_tile<true, false, true, ARD>(m, r0, c0, s_a, s_b, ln, acc, norm);
  if (threadIdx.x < 2 * GP_T) s_n[threadIdx.x] = norm;
  __syncthreads();
  PG_TILE_FOR_EACH_OUTPUT(GP_V, ln, r, c) {
    const float sq = fmaf(-2.f, PG_TILE_OUTPUT(acc), s_n[r] + s_n[GP_T + c]);
    gp_se_store<KIND, ARD>(p, r0 + r, c0 + c, fmaxf(sq, 0.f));
  }
}

__global__ void __launch_bounds__(256) gp_add_diag_kernel(float* __restrict__ a, long ld, int n, float value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[(size_t)i * ld + i] += value;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The unblocked Cholesky of one diagonal block (jb <= 64 rows), right-looking inside the block, one workgroup. Rows < done
// are final and are not written; rows >= done continue their chains from the values the updates left. Per column j: phase A
// forms column j of the factor into col[] (a square root for the pivot if j >= done, an IEEE division below it for rows >=
// done); phase B writes it back and applies it to the columns c in (j, i] of the rows i >= done. A pivot that is not > 0
// (a NaN included) is recorded as base + j + 1 in *info, by one plain store and only while *info is 0; the kernel goes on.
__global__ void __launch_bounds__(GP_THREADS) gp_potrf_diag_kernel(float* __restrict__ a, long ld, int jb, int done, int base,
                                                                   int* __restrict__ info) {
  __shared__ float s[GP_T * GP_BLK_LD];
  __shared__ float col[GP_T];
  const int tid = threadIdx.x;
  for (int e = tid; e < GP_T * GP_T; e += GP_THREADS) {
    const int i = e >> 6, c = e & 63;
    s[i * GP_BLK_LD + c] = (i < jb && c <= i) ? a[(size_t)i * ld + c] : 0.f;
  }
  int bad = 0;
  const int ui = tid >> 2, uc = tid & 3;  // the row and the column residue this thread updates
  for (int j = 0; j < jb; ++j) {
    __syncthreads();
    if (tid < GP_T) {
      const float d = s[j * GP_BLK_LD + j];
      const bool pivot = j >= done;
      const float ljj = pivot ? sqrtf(d) : d;
      if (pivot && !(d > 0.f) && bad == 0) bad = base + j + 1;
      const float v = s[tid * GP_BLK_LD + j];
      col[tid] = tid == j ? ljj : ((tid > j && tid >= done) ? v / ljj : v);
    }
    __syncthreads();
    if (tid < GP_T && tid >= j) s[tid * GP_BLK_LD + j] = col[tid];
    if (ui >= done && ui > j) {
      const float li = col[ui];
      for (int q = (j + 1) >> 2; q <= ui >> 2; ++q) {
        const int c = 4 * q + uc;
        if (c > j && c <= ui) s[ui * GP_BLK_LD + c] = fmaf(-li, col[c], s[ui * GP_BLK_LD + c]);
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < GP_T * GP_T; e += GP_THREADS) {
    const int i = e >> 6, c = e & 63;
    if (i < jb && i >= done && c <= i) a[(size_t)i * ld + c] = s[i * GP_BLK_LD + c];
  }
  if (tid == 0 && bad != 0 && *info == 0) *info = bad;
}

// the launches; arguments are checked by the callers
int gp_gemm(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int R, int C, int K, int diag_off, int flags,
            hipStream_t st, const char* name) {
  GpGemmArgs p;
  p.m.a = a;
  p.m.a_rs = lda;
  p.m.b = b;
  const bool bt = (flags & PG_GP_B_TRANS) != 0;
  p.m.b_rs = bt ? 1 : ldb;
  p.m.b_ks = bt ? ldb : 1;
  p.m.R = R;
  p.m.C = C;
  p.m.K = K;
  p.c = c;
  p.ldc = ldc;
  p.diag_off = diag_off;
  p.lower = (flags & PG_GP_LOWER) != 0;
  p.mirror = (flags & PG_GP_MIRROR) != 0;
  p.col_tiles = pg_cdiv(C, GP_T);
  const dim3 grid((unsigned)((long)pg_cdiv(R, GP_T) * p.col_tiles));
  const bool plus = (flags & PG_GP_PLUS) != 0;
  if (bt) {
    if (plus)
      hipLaunchKernelGGL((gp_gemm_kernel<false, false>), grid, dim3(GP_THREADS), 0, st, p);
    else
      hipLaunchKernelGGL((gp_gemm_kernel<false, true>), grid, dim3(GP_THREADS), 0, st, p);
  } else {
    if (plus)
      hipLaunchKernelGGL((gp_gemm_kernel<true, false>), grid, dim3(GP_THREADS), 0, st, p);
    else
      hipLaunchKernelGGL((gp_gemm_kernel<true, true>), grid, dim3(GP_THREADS), 0, st, p);
  }
  PG_LAUNCH_CHECK(name);
  return 0;
}

int gp_potrf_diag(float* a, long ld, int jb, int done, int base, int* info, hipStream_t st, const char* name) {
  hipLaunchKernelGGL(gp_potrf_diag_kernel, dim3(1), dim3(GP_THREADS), 0, st, a, ld, jb, done, base, info);
  PG_LAUNCH_CHECK(name);
  return 0;
}

int gp_trsm_diag(const float* l, long ld, float* x, long ldx, int rows, int jb, int done, int back, hipStream_t st, const char* name) {
  const dim3 grid((unsigned)pg_cdiv(rows, GP_T));
  if (back)
    hipLaunchKernelGGL((gp_subst_diag_kernel<true, false>), grid, dim3(GP_THREADS), 0, st, l, ld, x, ldx, rows, jb, 0);
  else
    hipLaunchKernelGGL((gp_subst_diag_kernel<false, false>), grid, dim3(GP_THREADS), 0, st, l, ld, x, ldx, rows, jb, done);
  PG_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace

PG_EXPORT int pg_gp_plan(int n, int m, int d, int p, long long* out, int out_len) {
  PG_REQUIRE(out && out_len >= PG_GP_PLAN_INTS, PG_EINVAL, "pg_gp_plan: null pointer or short output array");
  GP_PLAN_OR_RETURN(pl, n, m, d, p, "pg_gp_plan");
  out[0] = GP_T;
  out[1] = GP_KC;
  out[2] = pl.panels;
  out[3] = pl.row_tiles;
  out[4] = pl.se_route;
  out[5] = GP_SE_DIRECT_D;
  out[6] = pl.se_sym_tiles;
  out[7] = pl.se_cross_tiles;
  out[8] = pl.potrf_launches;
  out[9] = pl.trsm_launches;
  out[10] = pl.trailing_groups;
  out[11] = GP_MAX_N;
  out[12] = GP_MAX_D;
  out[13] = GP_MAX_P;
  out[14] = pg_cdiv(p, GP_T);
  out[15] = GP_SE_DIRECT_MAX_D;
  return 0;
}

namespace {

template <int KIND, bool ARD>
void gp_stat_launch(int route, dim3 grid, hipStream_t st, const GpSeArgs& p) {
  if (route == 0)
    hipLaunchKernelGGL((gp_se_direct_kernel<KIND, ARD>), grid, dim3(GP_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((gp_se_mfma_kernel<KIND, ARD>), grid, dim3(GP_THREADS), 0, st, p);
}

// the one launch path of pg_gp_se_kernel (kind SE, inv_ls NULL) and pg_gp_stat_kernel
int gp_stat_kernel(const char* name, int kind, const float* a, long lda, int n, const float* b, long ldb, int m, int d, float std,
                   float lengthscale, const float* inv_ls, float noise_var, float* k, long ldk, int diag_off, int flags, void* stream) {
  GP_PLAN_OR_RETURN(pl, n, m, d, 1, name);
  PG_REQUIRE(gp_kind_known(kind), PG_EINVAL, "%s: kind %d is none of PG_GP_KIND_*", name, kind);
  PG_REQUIRE(a && b && k, PG_EINVAL, "%s: null pointer", name);
  PG_REQUIRE(lda >= d && ldb >= d && ldk >= m, PG_EINVAL, "%s: a row stride below its row length", name);
  PG_REQUIRE((inv_ls || lengthscale > 0.f) && std == std && noise_var == noise_var, PG_EINVAL,
             "%s: lengthscale = %g must be > 0, std and noise_var no NaN", name, (double)lengthscale);
  const int known = PG_GP_LOWER | PG_GP_MIRROR | PG_GP_DIAG | PG_GP_SE_DIRECT | PG_GP_SE_MFMA;
  PG_REQUIRE((flags & ~known) == 0 && (flags & (PG_GP_SE_DIRECT | PG_GP_SE_MFMA)) != (PG_GP_SE_DIRECT | PG_GP_SE_MFMA), PG_EINVAL,
             "%s: flags %d", name, flags);
  PG_REQUIRE(diag_off > -GP_MAX_N && diag_off < GP_MAX_N, PG_EINVAL, "%s: diag_off = %d", name, diag_off);
  PG_REQUIRE(!(flags & PG_GP_MIRROR) || ((flags & PG_GP_LOWER) && a == b && lda == ldb && n == m && diag_off == 0), PG_EINVAL,
             "%s: the mirror takes the symmetric form (a is b, lower, diag_off = 0)", name);
  int route = pl.se_route;
  if (flags & PG_GP_SE_MFMA) route = 1;
  if (flags & PG_GP_SE_DIRECT) {
    PG_REQUIRE(d <= GP_SE_DIRECT_MAX_D, PG_ESHAPE, "%s: the exact-difference route holds d <= %d, got %d", name, GP_SE_DIRECT_MAX_D, d);
    route = 0;
  }
  GP_TRY(gp_device(name));
  GpSeArgs p;
  p.a = a;
  p.b = b;
  p.k = k;
  p.lda = lda;
  p.ldb = ldb;
  p.ldk = ldk;
  p.n = n;
  p.m = m;
  p.d = d;
  p.diag_off = diag_off;
  p.lower = (flags & PG_GP_LOWER) != 0;
  p.mirror = (flags & PG_GP_MIRROR) != 0;
  p.diag = (flags & PG_GP_DIAG) != 0;
  p.col_tiles = pg_cdiv(m, GP_T);
  p.std2 = std * std;
  p.neg_inv = inv_ls ? -0.5f : -0.5f / (lengthscale * lengthscale);
  p.diag_val = p.std2 + noise_var;
  p.w = inv_ls;
  p.inv_l2 = inv_ls ? 1.f : 1.f / (lengthscale * lengthscale);
  const dim3 grid((unsigned)((long)pg_cdiv(n, GP_T) * p.col_tiles));
  const hipStream_t st = (hipStream_t)stream;
  gp_with_kind(kind, [&](auto K) {
    if (inv_ls)
      gp_stat_launch<decltype(K)::value, true>(route, grid, st, p);
    else
      gp_stat_launch<decltype(K)::value, false>(route, grid, st, p);
  });
  PG_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace

PG_EXPORT int pg_gp_se_kernel(const float* a, long lda, int n, const float* b, long ldb, int m, int d, float std, float lengthscale,
                              float noise_var, float* k, long ldk, int diag_off, int flags, void* stream) {
  return gp_stat_kernel("pg_gp_se_kernel", PG_GP_KIND_SE, a, lda, n, b, ldb, m, d, std, lengthscale, nullptr, noise_var, k, ldk, diag_off, flags,
                        stream);
}

PG_EXPORT int pg_gp_stat_kernel(int kind, const float* a, long lda, int n, const float* b, long ldb, int m, int d, float std, float lengthscale,
                                const float* inv_ls, float noise_var, float* k, long ldk, int diag_off, int flags, void* stream) {
  return gp_stat_kernel("pg_gp_stat_kernel", kind, a, lda, n, b, ldb, m, d, std, lengthscale, inv_ls, noise_var, k, ldk, diag_off, flags, stream);
}

PG_EXPORT int pg_gp_add_diag(float* a, long ld, int n, float value, void* stream) {
  GP_PLAN_OR_RETURN(pl, n, 1, 1, 1, "pg_gp_add_diag");
  PG_REQUIRE(a && ld >= n, PG_EINVAL, "pg_gp_add_diag: null pointer or a row stride below the row length");
  GP_TRY(gp_device("pg_gp_add_diag"));
  hipLaunchKernelGGL(gp_add_diag_kernel, dim3((unsigned)pg_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a, ld, n, value);
  PG_LAUNCH_CHECK("pg_gp_add_diag");
  return 0;
}

PG_EXPORT int pg_gp_gemm_nt(const float* a, long lda, const float* b, long ldb, float* c, long ldc, int R, int C, int K, int diag_off,
                            int flags, void* stream) {
  GP_PLAN_OR_RETURN(pl, R, C, 1, 1, "pg_gp_gemm_nt");
  PG_REQUIRE(K >= 1 && K <= GP_MAX_N, PG_ESHAPE, "pg_gp_gemm_nt: K = %d outside 1 .. %d", K, GP_MAX_N);
  PG_REQUIRE(a && b && c, PG_EINVAL, "pg_gp_gemm_nt: null pointer");
  const int known = PG_GP_LOWER | PG_GP_MIRROR | PG_GP_PLUS | PG_GP_B_TRANS;
  PG_REQUIRE((flags & ~known) == 0, PG_EINVAL, "pg_gp_gemm_nt: flags %d", flags);
  PG_REQUIRE(lda >= K && ldb >= ((flags & PG_GP_B_TRANS) ? C : K) && ldc >= C, PG_EINVAL, "pg_gp_gemm_nt: a row stride below its row length");
  PG_REQUIRE(diag_off > -GP_MAX_N && diag_off < GP_MAX_N, PG_EINVAL, "pg_gp_gemm_nt: diag_off = %d", diag_off);
  PG_REQUIRE(!(flags & PG_GP_MIRROR) || ((flags & PG_GP_LOWER) && R == C && diag_off == 0), PG_EINVAL,
             "pg_gp_gemm_nt: the mirror takes a square lower update with diag_off = 0");
  GP_TRY(gp_device("pg_gp_gemm_nt"));
  return gp_gemm(a, lda, b, ldb, c, ldc, R, C, K, diag_off, flags, (hipStream_t)stream, "pg_gp_gemm_nt");
}

PG_EXPORT int pg_gp_potrf_diag(float* a, long ld, int jb, int done, int base, int* info, void* stream) {
  PG_REQUIRE(jb >= 1 && jb <= GP_T && done >= 0 && done <= jb && base >= 0, PG_ESHAPE,
             "pg_gp_potrf_diag: jb = %d (1 .. %d), done = %d (0 .. jb), base = %d (>= 0)", jb, GP_T, done, base);
  GP_PLAN_OR_RETURN(pl, (int)std::min<long>((long)base + jb, 1L << 30), 1, 1, 1, "pg_gp_potrf_diag");  // the block ends inside n <= 16384
  PG_REQUIRE(a && info && ld >= jb, PG_EINVAL, "pg_gp_potrf_diag: null pointer or a row stride below the row length");
  GP_TRY(gp_device("pg_gp_potrf_diag"));
  return gp_potrf_diag(a, ld, jb, done, base, info, (hipStream_t)stream, "pg_gp_potrf_diag");
}

PG_EXPORT int pg_gp_trsm_diag(const float* l, long ld, float* x, long ldx, int rows, int jb, int done, int transposed, void* stream) {
  GP_PLAN_OR_RETURN(pl, 1, rows, 1, 1, "pg_gp_trsm_diag");
  PG_REQUIRE(jb >= 1 && jb <= GP_T && done >= 0 && done <= jb, PG_ESHAPE, "pg_gp_trsm_diag: jb = %d (1 .. %d), done = %d (0 .. jb)", jb, GP_T,
             done);
  PG_REQUIRE(l && x && ld >= jb && ldx >= jb, PG_EINVAL, "pg_gp_trsm_diag: null pointer or a row stride below the row length");
  PG_REQUIRE(!transposed || done == 0, PG_EINVAL, "pg_gp_trsm_diag: the X L = B form completes no columns (done = %d)", done);
  GP_TRY(gp_device("pg_gp_trsm_diag"));
  return gp_trsm_diag(l, ld, x, ldx, rows, jb, done, transposed != 0, (hipStream_t)stream, "pg_gp_trsm_diag");
}

PG_EXPORT int pg_gp_potrf(float* a, long ld, int n, int n_done, int* info, void* stream) {
  GP_PLAN_OR_RETURN(pl, n, 1, 1, 1, "pg_gp_potrf");
  PG_REQUIRE(n_done >= 0 && n_done <= n, PG_ESHAPE, "pg_gp_potrf: n_done = %d outside 0 .. n = %d", n_done, n);
  PG_REQUIRE(a && info && ld >= n, PG_EINVAL, "pg_gp_potrf: null pointer or a row stride below the row length");
  GP_TRY(gp_device("pg_gp_potrf"));
  if (n_done == n) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const char* name = "pg_gp_potrf";
  const int first = n_done / GP_T;  // the first panel with unfinished columns
  // the new rows through the finished whole panels: solve against the panel's diagonal block, update the columns to its right
  for (int k = 0; k < first; ++k) {
    const int j0 = k * GP_T, rows = n - n_done, right = n - (j0 + GP_T);
    float* x = a + (size_t)n_done * ld + j0;
    GP_TRY(gp_trsm_diag(a + (size_t)j0 * ld + j0, ld, x, ld, rows, GP_T, 0, 0, st, name));
    GP_TRY(gp_gemm(x, ld, a + (size_t)(j0 + GP_T) * ld + j0, ld, x + GP_T, ld, rows, right, GP_T, n_done - (j0 + GP_T), PG_GP_LOWER, st, name));
  }
  for (int k = first; k < pl.panels; ++k) {
    const int j0 = k * GP_T, jb = std::min(GP_T, n - j0), below = n - j0 - jb;
    float* diag = a + (size_t)j0 * ld + j0;
    GP_TRY(gp_potrf_diag(diag, ld, jb, std::max(0, n_done - j0), j0, info, st, name));
    if (below > 0) {
      float* x = diag + (size_t)GP_T * ld;
      GP_TRY(gp_trsm_diag(diag, ld, x, ld, below, GP_T, 0, 0, st, name));
      GP_TRY(gp_gemm(x, ld, x, ld, x + GP_T, ld, below, below, GP_T, 0, PG_GP_LOWER, st, name));
    }
  }
  return 0;
}

PG_EXPORT int pg_gp_trsm_right(const float* l, long ld, int n, float* x, long ldx, int rows, int col_done, int transposed, void* stream) {
  GP_PLAN_OR_RETURN(pl, n, rows, 1, 1, "pg_gp_trsm_right");
  PG_REQUIRE(col_done >= 0 && col_done <= n, PG_ESHAPE, "pg_gp_trsm_right: col_done = %d outside 0 .. n = %d", col_done, n);
  PG_REQUIRE(l && x && ld >= n && ldx >= n, PG_EINVAL, "pg_gp_trsm_right: null pointer or a row stride below the row length");
  PG_REQUIRE(!transposed || col_done == 0, PG_EINVAL, "pg_gp_trsm_right: the X L = B form completes no columns (col_done = %d)", col_done);
  GP_TRY(gp_device("pg_gp_trsm_right"));
  if (col_done == n) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const char* name = "pg_gp_trsm_right";
  if (transposed) {
    for (int k = pl.panels - 1; k >= 0; --k) {
      const int j0 = k * GP_T, jb = std::min(GP_T, n - j0);
      GP_TRY(gp_trsm_diag(l + (size_t)j0 * ld + j0, ld, x + j0, ldx, rows, jb, 0, 1, st, name));
      if (j0 > 0) GP_TRY(gp_gemm(x + j0, ldx, l + (size_t)j0 * ld, ld, x, ldx, rows, j0, jb, 0, PG_GP_B_TRANS, st, name));
    }
    return 0;
  }
  const int first = col_done / GP_T;
  // the finished whole panels act on the new columns as one product: the same chain as panel after panel
  if (first > 0) GP_TRY(gp_gemm(x, ldx, l + (size_t)col_done * ld, ld, x + col_done, ldx, rows, n - col_done, first * GP_T, 0, 0, st, name));
  for (int k = first; k < pl.panels; ++k) {
    const int j0 = k * GP_T, jb = std::min(GP_T, n - j0), right = n - j0 - jb;
    GP_TRY(gp_trsm_diag(l + (size_t)j0 * ld + j0, ld, x + j0, ldx, rows, jb, std::max(0, col_done - j0), 0, st, name));
    if (right > 0) GP_TRY(gp_gemm(x + j0, ldx, l + (size_t)(j0 + GP_T) * ld + j0, ld, x + j0 + GP_T, ldx, rows, right, GP_T, 0, 0, st, name));
  }
  return 0;
}
