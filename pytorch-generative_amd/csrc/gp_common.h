// gp_common.h — what gp.hip and gp_mll.hip share: the tile constants, the stationary kinds and their host-side dispatch, the
// 64 x 64 x K product of one workgroup on mfma_tile.h, the staging of rows into LDS and the exact differences behind a lane's
// MFMA outputs, the substitution against a diagonal block (gp.hip's panel solves and gp_mll.hip's triangular inverse are
// instantiations of one kernel), and the one function that decides the domain and the geometry of the Gaussian-process
// kernels. Every name keeps internal linkage (one copy per translation unit).
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int GP_V = pg_tile::SMALL;  // the MFMA products run on the small tile of mfma_tile.h
using GpTile = pg_tile::Tile<GP_V>;
constexpr int GP_T = GpTile::BM;   // panel width, tile edge
constexpr int GP_KC = GpTile::KC;  // k per LDS chunk
constexpr int GP_LD = GpTile::LD;  // LDS row stride of an operand chunk
constexpr int GP_THREADS = pg_tile::THREADS;
constexpr int GP_BLK_LD = 68;    // LDS row stride of the diagonal block in gp_potrf_diag_kernel
constexpr int GP_TRI_LD = 65;    // LDS row stride of the diagonal block in gp_subst_diag_kernel and of the rows in gp_se_direct_kernel
constexpr int GP_MAX_N = 16384;  // n, m: element offsets of an (n, n) matrix fit 32 bits
constexpr int GP_MAX_D = 4096;
constexpr int GP_MAX_P = 4096;
constexpr int GP_SE_DIRECT_D = 16;      // largest d of the exact-difference route: measured faster up to 16, slower from 32 (profiles/gp.json)
constexpr int GP_SE_DIRECT_MAX_D = 64;  // largest d the exact-difference kernel holds in LDS when the route is forced
constexpr int GP_ARD_MAX_D = 256;       // largest d of the per-dimension gradient reduction: n^2 d / 2 terms on the VALU
constexpr int GP_ARD_CHUNK = 64;        // columns of x it stages per pass

// ---------------------------------------------------------------------------------------------------------------------------
// The stationary kernels k = std^2 phi(r) (PG_GP_KIND_*): phi and omega = -phi'(r) / r, both finite at r = 0.
//   SE          phi = exp(-r^2 / 2)                                omega = phi
//   Matern 3/2  phi = (1 + s) exp(-s), s = sqrt(3) r               omega = 3 exp(-s)
//   Matern 5/2  phi = (1 + s + s^2 / 3) exp(-s), s = sqrt(5) r     omega = (5 / 3)(1 + s) exp(-s)
// r2 is the squared scaled distance, >= 0.
template <int KIND>
__device__ __forceinline__ void gp_stat_phi_omega(float r2, float& phi, float& omega) {
  if (KIND == PG_GP_KIND_SE) {
    phi = omega = expf(-0.5f * r2);
  } else if (KIND == PG_GP_KIND_MATERN32) {
    const float s = 1.7320508075688772f * sqrtf(r2), e = expf(-s);
    phi = (1.f + s) * e;
    omega = 3.f * e;
  } else {
    const float s = 2.2360679774997897f * sqrtf(r2), e = expf(-s);
    phi = (1.f + s + s * s * (1.f / 3.f)) * e;
    omega = (5.f / 3.f) * (1.f + s) * e;
  }
}

inline bool gp_kind_known(int kind) { return kind == PG_GP_KIND_SE || kind == PG_GP_KIND_MATERN32 || kind == PG_GP_KIND_MATERN52; }

// Calls f(std::integral_constant<int, kind>()) for a known kind: the one place where a run-time kind picks an instantiation.
template <class F>
void gp_with_kind(int kind, F&& f) {
  if (kind == PG_GP_KIND_SE) f(std::integral_constant<int, PG_GP_KIND_SE>());
  if (kind == PG_GP_KIND_MATERN32) f(std::integral_constant<int, PG_GP_KIND_MATERN32>());
  if (kind == PG_GP_KIND_MATERN52) f(std::integral_constant<int, PG_GP_KIND_MATERN52>());
}

// ---------------------------------------------------------------------------------------------------------------------------
// The 64 x 64 x K product of one workgroup: acc += (NEG ? -A : A) B^T with A(r, k) = a[r * a_rs + k] and
// B(c, k) = b[c * b_rs + k * b_ks], on mfma_tile.h's pipeline (BK: B is k-contiguous). Ragged edges are zero-filled. NORMS:
// thread t < 64 also sums A(r0 + t, k)^2, thread 64 + t B(c0 + t, k)^2, in k order. SCALE (BK only): both operands are
// multiplied by w[k] on the way into LDS (a thread's elements of a chunk share k), so the product and the norms are those of
// the scaled rows; without it w is not read and nothing changes.
struct GpMma {
  const float* a;
  const float* b;
  long a_rs, b_rs, b_ks;
  int R, C, K;
  const float* w = nullptr;
};

template <bool BK, bool NEG, bool NORMS, bool SCALE = false>
__device__ __forceinline__ void gp_mma_tile(const GpMma& p, int r0, int c0, float* s_a, float* s_b, const pg_tile::Lanes<GP_V>& ln,
                                            pg_tile::Acc<GP_V>& acc, float& norm) {
  const int tid = ln.tid;
  pg_tile::Regs<GP_V> ra, rb;
  auto load = [&](int ch) {
    pg_tile::load_operand<GP_V, true, NEG>(ra, p.a, p.a_rs, 1, r0, p.R, ch * GP_KC, p.K, tid);
    pg_tile::load_operand<GP_V, BK>(rb, p.b, p.b_rs, p.b_ks, c0, p.C, ch * GP_KC, p.K, tid);
    if (SCALE) {
      static_assert(!SCALE || BK, "the scaled walk is k-contiguous");
      const int gk = ch * GP_KC + tid % GP_KC;
      const float wk = gk < p.K ? p.w[gk] : 0.f;
#pragma unroll
      for (int j = 0; j < GP_T * GP_KC / GP_THREADS; ++j) {
        ra[j] *= wk;
        rb[j] *= wk;
      }
    }
  };
  auto store = [&]() {
    pg_tile::store_operand<GP_V, true>(s_a, ra, tid);
    pg_tile::store_operand<GP_V, BK>(s_b, rb, tid);
  };
  auto norms = [&](int) {
    if (NORMS && tid < 2 * GP_T) {
      const float* row = (tid < GP_T ? s_a + tid * GP_LD : s_b + (tid - GP_T) * GP_LD);
#pragma unroll
      for (int k = 0; k < GP_KC; ++k) norm = fmaf(row[k], row[k], norm);  // zero beyond K
    }
  };
  PG_TILE_PIPELINE(GP_V, false, 0, (p.K + GP_KC - 1) / GP_KC, load, store, acc, s_a, s_b, ln, norms);  // every caller has K >= 1
}

// ---------------------------------------------------------------------------------------------------------------------------
// GP_STAGE_ROWS: columns k0 .. k0 + kc of the rows ra0 .. ra0 + 63 of a and rb0 .. rb0 + 63 of b into LDS at row stride LD, zero
// from row na (nb) on; the caller synchronises. A macro, so that the loop reaches the kernel as source: as a force-inlined
// function it changed the code of gp_se_direct_kernel (tools/same_code_as.py), as a macro it does not.
#define GP_STAGE_ROWS(LD, s_a, s_b, a, lda, ra0, na, b, ldb, rb0, nb, k0, kc, tid)                        \
  for (int e_ = (tid); e_ < GP_T * (kc); e_ += GP_THREADS) {                                              \
    const int r_ = e_ / (kc), k_ = e_ % (kc);                                                             \
    (s_a)[r_ * (LD) + k_] = (ra0) + r_ < (na) ? (a)[(size_t)((ra0) + r_) * (lda) + (k0) + k_] : 0.f;      \
    (s_b)[r_ * (LD) + k_] = (rb0) + r_ < (nb) ? (b)[(size_t)((rb0) + r_) * (ldb) + (k0) + k_] : 0.f;      \
  }

// The exact differences behind a lane's 16 MFMA outputs (the layout of PG_TILE_FOR_EACH_OUTPUT: 2 x 4 rows of a against 2 rows
// of b, staged at row stride LD), scaled per column. fetch reads column k of those rows; diff is (a - b) wk, the difference
// first; add_squares adds diff^2 to each output by one fmaf, so a sum over k is one chain in the order of the calls. Both passes
// of the ARD reduction use it; the shared-lengthscale reduction keeps its unscaled loop written out (gp_mll.hip says why).
template <int LD>
struct GpLaneDiffs {
  int ra[2][4], rb[2];
  float av[2][4], bv[2];
  __device__ __forceinline__ explicit GpLaneDiffs(const pg_tile::Lanes<GP_V>& ln) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) ra[i][q] = pg_tile::out_row<GP_V>(ln, i, q) * LD;
      rb[i] = pg_tile::out_col<GP_V>(ln, i) * LD;
    }
  }
  __device__ __forceinline__ void fetch(const float* s_a, const float* s_b, int k) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) av[i][q] = s_a[ra[i][q] + k];
      bv[i] = s_b[rb[i] + k];
    }
  }
  __device__ __forceinline__ float diff(int i, int j, int q, float wk) const {
    return (av[i][q] - bv[j]) * wk;
  }
  __device__ __forceinline__ void add_squares(pg_tile::Acc<GP_V>& sq, float wk) const {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float df = diff(i, j, q, wk);
          sq[i][j][q] = fmaf(df, df, sq[i][j][q]);
        }
  }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The substitution against one diagonal block l (jb, jb), 64 rows of X per workgroup, four lanes per row, each with the columns
// j = 4 q + (lane & 3) of its row in registers; x_k goes to the row's lanes by a shuffle. One fmaf chain per element, then one
// IEEE division (no explicit inverse of the block).
//   forward (BACK = false): X L^T = B, x_ij = (b_ij - sum_{k < j} x_ik l_jk) / l_jj, k ascending; columns < done are final.
//   backward (BACK = true): X L = B,   x_ij = (b_ij - sum_{k > j} x_ik l_kj) / l_jj, k descending; done = 0.
//   UNIT (forward, done = 0): a panel of X L^T = I. x points at column j0 = rows - jb of row 0; the workgroup of the diagonal
//   block (rows j0 ..) starts from the identity instead of reading x and writes the columns on or right of the diagonal only;
//   the others continue from the values the updates left.
template <bool BACK, bool UNIT>
__global__ void __launch_bounds__(GP_THREADS) gp_subst_diag_kernel(const float* __restrict__ l, long ld, float* __restrict__ x, long ldx,
                                                                   int rows, int jb, int done_columns) {
  static_assert(!(BACK && UNIT), "the identity right-hand side belongs to the forward form");
  __shared__ float s_l[GP_T * GP_TRI_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < GP_T * GP_T; e += GP_THREADS) {
    const int j = e >> 6, k = e & 63;
    float v = j == k ? 1.f : 0.f;  // rows beyond jb: the identity
    if (j < jb && k <= j) v = l[(size_t)j * ld + k];
    s_l[j * GP_TRI_LD + k] = v;
  }
  const int done = UNIT ? 0 : done_columns;
  const int row = blockIdx.x * GP_T + (tid >> 2), c = tid & 3;
  const bool unit = UNIT && (int)blockIdx.x * GP_T == rows - jb;
  const int first = unit ? row - (rows - jb) : done;  // the first column this row writes
  float v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int j = 4 * q + c;
    float b = 0.f;
    if (row < rows && j < jb) b = unit ? (j == first ? 1.f : 0.f) : x[(size_t)row * ldx + j];
    v[q] = b;
  }
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < GP_T; ++kk) {
    const int k = BACK ? GP_T - 1 - kk : kk;
    if (k < jb) {  // the same in every lane
      const int qk = k >> 2, ck = k & 3;
      float cand = v[qk];
      if (BACK || k >= done) cand = cand / s_l[k * GP_TRI_LD + k];
      const float xk = __shfl(cand, (lane & ~3) | ck);
      if (c == ck) v[qk] = xk;
      if (BACK) {
#pragma unroll
        for (int q = 0; q <= qk; ++q) {
          const int j = 4 * q + c;
          if (j < k) v[q] = fmaf(-xk, s_l[k * GP_TRI_LD + j], v[q]);
        }
      } else {
#pragma unroll
        for (int q = qk; q < 16; ++q) {
          const int j = 4 * q + c;
          if (j > k && j >= done) v[q] = fmaf(-xk, s_l[j * GP_TRI_LD + k], v[q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int j = 4 * q + c;
    if (row < rows && j < jb && j >= first) x[(size_t)row * ldx + j] = v[q];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The one function that decides the domain and the geometry: pg_gp_plan reports it, every entry point goes by it.
struct GpPlan {
  int n, m, d, p, panels, row_tiles, se_route;
  long se_sym_tiles, se_cross_tiles, potrf_launches, trsm_launches, trailing_groups;
};

int gp_plan(int n, int m, int d, int p, GpPlan& pl, const char* name) {
  PG_REQUIRE(n >= 1 && m >= 1 && d >= 1 && p >= 1, PG_ESHAPE, "%s: n = %d, m = %d, d = %d, p = %d must all be >= 1", name, n, m, d, p);
  PG_REQUIRE(n <= GP_MAX_N && m <= GP_MAX_N, PG_ESHAPE, "%s: n = %d, m = %d: at most %d rows (element offsets stay inside 32 bits)", name, n, m,
             GP_MAX_N);
  PG_REQUIRE(d <= GP_MAX_D && p <= GP_MAX_P, PG_ESHAPE, "%s: d = %d (at most %d), p = %d (at most %d)", name, d, GP_MAX_D, p, GP_MAX_P);
  pl.n = n;
  pl.m = m;
  pl.d = d;
  pl.p = p;
  pl.panels = pg_cdiv(n, GP_T);
  pl.row_tiles = pg_cdiv(m, GP_T);
  pl.se_route = d <= GP_SE_DIRECT_D ? 0 : 1;
  pl.se_sym_tiles = (long)pl.panels * (pl.panels + 1) / 2;
  pl.se_cross_tiles = (long)pl.row_tiles * pl.panels;
  pl.potrf_launches = 3L * pl.panels - 2;  // diagonal block, panel solve, trailing update; the last panel has no rows below
  pl.trsm_launches = 2L * pl.panels - 1;   // panel solve, update of the columns to the right
  pl.trailing_groups = (long)(pl.panels - 1) * (pl.panels - 1);
  return 0;
}

#define GP_PLAN_OR_RETURN(pl, n, m, d, p, name)        \
  GpPlan pl;                                           \
  {                                                    \
    const int rc__ = gp_plan(n, m, d, p, pl, name);    \
    if (rc__) return rc__;                             \
  }                                                    \
  (void)pl;

// a missing device is reported once the plan and the argument checks accepted the call
int gp_device(const char* name) {
  static bool seen = false;
  if (seen) return 0;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    (void)hipGetLastError();
    pg_set_error("%s: no HIP device", name);
    return (int)hipErrorNoDevice;
  }
  seen = true;
  return 0;
}

#define GP_TRY(call)           \
  do {                         \
    const int rc__ = (call);   \
    if (rc__) return rc__;     \
  } while (0)

}  // namespace
