// mfma_tile.h — the one fp32-MFMA workgroup tile behind dense_linear.hip, fvbn.hip and gp.hip.
//
// Geometry. A workgroup of 256 threads = 4 waves arranged 2 x 2 computes one BM x BN tile of C[r][c] = sum_k A(r, k) B(c, k); a
// wave owns 2 x 2 MFMA tiles of MT x MT. Both operands are staged in LDS as rows of KC k values, LD floats apart; the next chunk
// waits in registers while the current one multiplies out of LDS.
//     variant  BM x BN    KC  LD  MT  KS  instruction              accumulator
//     SMALL     64 x  64  32  34  16   4  v_mfma_f32_16x16x4_f32   f32x4
//     LARGE    128 x 128  16  17  32   2  v_mfma_f32_32x32x2_f32   f32x16
// Banks. LDS banks a 4-byte access as (address / 4) % 32 within a half-wave. The 16x16x4 operand read of a half-wave is 16 rows
// x 2 k: (34 row + k) % 32 = (2 row + k) % 32, 32 distinct banks (a stride of 36 = KC + 4 gives 4 row + k: 16 banks, two-way).
// The 32x32x2 read is 32 rows at one k: 17 row % 32, 32 distinct banks; so are staging stores along rows. Only those reads are
// conflict free: at 34 the staging stores of a row-contiguous operand and a thread's walk along one row are two-way, at 17 a
// k-contiguous store shares one bank of 32.
// Chain order. An fp32 MFMA is, per output element, an fmaf chain over its KS products in ascending k. multiply_chunk issues the
// MFMAs in ascending k and pipeline the chunks in ascending order, so every output is ONE chain v = fmaf(a_k, b_k, v) in k order
// that starts from whatever the accumulator held: zero, or a value the caller seeded. The result therefore does not depend on
// KC, on where a chunk or a launch boundary falls, or on the zero fill beyond a ragged edge (it adds exact zeros): fp32-exact,
// deterministic, and continuing a sum in a later launch gives the bits of one launch.
#pragma once
#include <hip/hip_runtime.h>

namespace pg_tile {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

enum { SMALL = 0, LARGE = 1 };
constexpr int THREADS = 256;

template <int V>
struct Tile;
template <>
struct Tile<SMALL> {
  static constexpr int BM = 64, BN = 64, KC = 32, LD = 34, MT = 16, KS = 4;
  typedef f32x4 acc_t;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return mfma16(a, b, c); }
};
template <>
struct Tile<LARGE> {
  static constexpr int BM = 128, BN = 128, KC = 16, LD = 17, MT = 32, KS = 2;
  typedef f32x16 acc_t;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return mfma32(a, b, c); }
};
template <int V>
using Acc = typename Tile<V>::acc_t[2][2];  // a wave's 2 x 2 MFMA tiles

// Where a thread sits: lane row lr and k group lk inside an MFMA operand, wave row wr and wave column wc inside the tile.
template <int V>
struct Lanes {
  int tid, lr, lk, wr, wc;
  __device__ __forceinline__ Lanes() : tid(threadIdx.x) {
    const int lane = tid & 63, wave = tid >> 6;
    lr = lane & (Tile<V>::MT - 1), lk = lane / Tile<V>::MT;
    wr = wave >> 1, wc = wave & 1;
  }
};

template <int V>
__device__ __forceinline__ void zero(Acc<V>& acc) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = typename Tile<V>::acc_t{};
}

// Row and column, inside the tile, of element q of a lane's MFMA tile (i, j): the D layouts. Column = lane % MT;
// 16x16: row = 4 (lane >> 4) + reg; 32x32: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
template <int V>
__device__ __forceinline__ int out_row(const Lanes<V>& ln, int i, int q) {
  return (ln.wr * 2 + i) * Tile<V>::MT + (V == LARGE ? (q & 3) + 8 * (q >> 2) + 4 * ln.lk : 4 * ln.lk + q);
}
template <int V>
__device__ __forceinline__ int out_col(const Lanes<V>& ln, int j) {
  return (ln.wc * 2 + j) * Tile<V>::MT + ln.lr;
}

// PG_TILE_FOR_EACH_OUTPUT(V, ln, li, lj) { ... } runs the block once for every element a lane owns, fully unrolled, with
// li, lj the element's place inside the tile and PG_TILE_OUTPUT(acc) the element itself (readable and assignable; `continue`
// goes to the next element). A loop header and not a function taking a lambda for the reason given at PG_TILE_PIPELINE: seed
// and epilogue bodies optimised ahead of the kernel cost gp_gemm_kernel 190 instructions of repeated address arithmetic.
#define PG_TILE_FOR_EACH_OUTPUT(V, ln, li, lj)                                                                             \
  _Pragma("unroll") for (int pg_i_ = 0; pg_i_ < 2; ++pg_i_)                                                                \
  _Pragma("unroll") for (int pg_j_ = 0; pg_j_ < 2; ++pg_j_)                                                                \
  _Pragma("unroll") for (int pg_q_ = 0; pg_q_ < pg_tile::Tile<V>::MT * pg_tile::Tile<V>::MT / 64; ++pg_q_)                 \
    if (const int li = pg_tile::out_row<V>(ln, pg_i_, pg_q_), lj = pg_tile::out_col<V>(ln, pg_j_); true)
#define PG_TILE_OUTPUT(acc) acc[pg_i_][pg_j_][pg_q_]

// acc += A B^T of the chunk in LDS, k ascending
template <int V>
__device__ __forceinline__ void multiply_chunk(const Lanes<V>& ln, const float* s_a, const float* s_b, Acc<V>& acc) {
  using T = Tile<V>;
  const float* ap = s_a + (ln.wr * 2 * T::MT + ln.lr) * T::LD + ln.lk;
  const float* bp = s_b + (ln.wc * 2 * T::MT + ln.lr) * T::LD + ln.lk;
#pragma unroll
  for (int kk = 0; kk < T::KC; kk += T::KS) {
    const float a0 = ap[kk], a1 = ap[T::MT * T::LD + kk];
    const float b0 = bp[kk], b1 = bp[T::MT * T::LD + kk];
    acc[0][0] = T::mfma(a0, b0, acc[0][0]);
    acc[0][1] = T::mfma(a0, b1, acc[0][1]);
    acc[1][0] = T::mfma(a1, b0, acc[1][0]);
    acc[1][1] = T::mfma(a1, b1, acc[1][1]);
  }
}

// Chunks ch_beg .. ch_end - 1: load(ch) fetches chunk ch into the caller's registers, store() puts them into s_a / s_b, hook(ch)
// runs while the chunk is still in LDS; load, store and hook are the caller's named lambdas. MAY_BE_EMPTY = false where the
// caller's plan guarantees a chunk: the first load is then unguarded.
// A macro: the loop has to reach the kernel as source. As a force-inlined function template it is
// optimised once on its own, with the accumulators and staging registers behind pointers, before it is inlined, and the kernels
// come out with other registers than the same loop written in place (fv_wgrad_kernel: 78 instead of 70, a wave per SIMD less).
#define PG_TILE_PIPELINE(V, MAY_BE_EMPTY, ch_beg, ch_end, load, store, acc, s_a, s_b, ln, hook) \
  do {                                                                                          \
    const int pg_beg_ = (ch_beg), pg_end_ = (ch_end);                                           \
    if (!(MAY_BE_EMPTY) || pg_beg_ < pg_end_) load(pg_beg_);                                    \
    for (int pg_ch_ = pg_beg_; pg_ch_ < pg_end_; ++pg_ch_) {                                    \
      store();                                                                                  \
      __syncthreads();                                                                          \
      if (pg_ch_ + 1 < pg_end_) load(pg_ch_ + 1); /* in flight while this chunk multiplies */   \
      pg_tile::multiply_chunk<V>(ln, s_a, s_b, acc);                                            \
      hook(pg_ch_);                                                                             \
      __syncthreads();                                                                          \
    }                                                                                           \
  } while (0)

// Element e of a thread's share of a ROWS x KC chunk: k-contiguous operands walk k fastest, row-contiguous ones rows fastest.
template <int ROWS, int KC, bool KCONTIG>
__device__ __forceinline__ void coord(int e, int& r, int& k) {
  if (KCONTIG) {
    r = e / KC;
    k = e % KC;
  } else {
    r = e % ROWS;
    k = e / ROWS;
  }
}

// A thread's share of the chunk at k0 of a strided operand X(r, k) = x[r * rs + k * ks], rows row0 .. row0 + BM - 1: zero from
// row R and from k = kend on, negated on the way in if NEG.
template <int V>
using Regs = float[Tile<V>::BM * Tile<V>::KC / THREADS];

template <int V, bool KCONTIG, bool NEG = false>
__device__ __forceinline__ void load_operand(Regs<V>& reg, const float* x, long rs, long ks, int row0, int R, int k0, int kend, int tid) {
  using T = Tile<V>;
  static_assert(THREADS % T::KC == 0, "the elements of a thread share k in a k-contiguous walk");
  // k-contiguous: THREADS is a multiple of KC, every element tid + j THREADS of a thread has k = tid % KC, and its offset is
  // taken once. Left inside the loop, the compiler repeats the 64-bit product for every element.
  const size_t koff = (size_t)(k0 + tid % T::KC) * ks;
#pragma unroll
  for (int j = 0; j < T::BM * T::KC / THREADS; ++j) {
    int r, k;
    coord<T::BM, T::KC, KCONTIG>(tid + j * THREADS, r, k);
    const int gr = row0 + r, gk = k0 + k;
    const float v = (gr < R && gk < kend) ? x[(size_t)gr * rs + (KCONTIG ? koff : (size_t)gk * ks)] : 0.f;
    reg[j] = NEG ? -v : v;
  }
}

template <int V, bool KCONTIG>
__device__ __forceinline__ void store_operand(float* s, const Regs<V>& reg, int tid) {
#pragma unroll
  for (int j = 0; j < Tile<V>::BM * Tile<V>::KC / THREADS; ++j) {
    int r, k;
    coord<Tile<V>::BM, Tile<V>::KC, KCONTIG>(tid + j * THREADS, r, k);
    s[r * Tile<V>::LD + k] = reg[j];
  }
}

}  // namespace pg_tile
