// masked_linear.hip — MADE's MaskedLinear (reference models/autoregressive/made.py:21-33) as masked fp32-MFMA GEMMs.
//
// One tiled kernel computes C[r][c] = sum_k A(r, k) B(c, k) for the three products of a masked linear layer
// (X: (N, in), W: (out, in), Y / dY: (N, out), M[o][i] = deg_in[i] <= deg_out[o], or < for MADE's output layer):
//   forward   Y  = X (W o M)^T + b  [relu]   rows n, cols o, k = i   (A = X,    B = W o M: both k-contiguous)
//   data grad dX = dY (W o M) [* (x > 0)]   rows n, cols i, k = o   (A = dY k-contiguous, B = W o M row-contiguous)
//   wgrad     dW += dY^T X, db += sum_n dY   rows o, cols i, k = n   (A = dY^T, B = X^T: both row-contiguous)
// The mask is never read from memory: it is evaluated from the two int degree vectors while W is staged. The forward
// writes W o M back into `weight` (the reference's in-place `weight.data *= mask`) from the workgroups of the first
// row tile only: exactly one workgroup writes each weight element. Workgroups of later row tiles read W or W o M there,
// and multiply by the same 0 / 1 mask, so what they compute does not depend on the order.
// The weight gradient is UNMASKED, as the reference's (its mask is applied outside autograd).
//
// Tiles: 64 rows x 32 columns per workgroup of 4 waves (wave w owns rows 16w .. 16w + 15 and both 16-column MFMA
// tiles), k in chunks of 64 through LDS, the next chunk loaded into registers while the current one is multiplied.
// At the recipe's batch (64) one workgroup holds every batch row, so every weight byte is read once per GEMM.
// Products are v_mfma_f32_16x16x4_f32 (an fp32 fmaf chain per output in k order: deterministic, fp32-exact). Each
// output element is owned by one lane of one workgroup. A forward or data gradient with too few output tiles to fill
// the chip (the recipe's 8000 -> 784 layer: 25) is split along k into slices (blockIdx.z); the slices write raw partial
// sums to a caller-provided workspace and ml_splitk_reduce_kernel adds them in slice order and applies the epilogue.
// The weight gradient always sums its whole k range (the batch) in one workgroup. No atomics anywhere:
// bit-reproducible. Ragged edges are zero-filled on load and guarded on store.
#include <algorithm>

#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int ML_BM = 64;             // rows per workgroup
constexpr int ML_BN = 32;             // columns per workgroup
constexpr int ML_KC = 64;             // k per LDS chunk
constexpr int ML_LD = ML_KC + 4;      // LDS row stride (floats): the MFMA operand reads (16 rows x 4 k) are conflict free
constexpr int ML_THREADS = 256;
constexpr int ML_A_PER = ML_BM * ML_KC / ML_THREADS;  // 16 staged A elements per thread
constexpr int ML_B_PER = ML_BN * ML_KC / ML_THREADS;  // 8 staged B elements per thread

using pg_tile::f32x4;

enum { ML_FWD = 0, ML_DGRAD = 1, ML_WGRAD = 2 };

struct MlArgs {
  const float* a;       // A(r, k) = a[r * a_rs + k * a_ks]
  const float* b;       // B(c, k) = b[c * b_rs + k * b_ks]
  float* wb;            // forward: W o M written back (b's storage), first row tile only
  const float* bias;    // forward epilogue (may be NULL)
  const float* relu_src;  // data grad epilogue: multiply by (relu_src[r][c] > 0) (may be NULL)
  const int* deg_in;    // mask degrees (both NULL: unmasked)
  const int* deg_out;
  float* c;             // C[r * ldc + c]
  float* db;            // weight grad: db[r] += sum_k A(r, k) (may be NULL)
  float* part;          // split-K (forward / data grad): raw partial sums of slice z at part + z * R * ldc
  long a_rs, a_ks, b_rs, b_ks, ldc;
  int R, C, K, strict, relu, kper;  // kper: k per slice (blockIdx.z), a multiple of ML_KC
};

__device__ __forceinline__ bool ml_keep(const MlArgs& p, int o, int i) {
  const int di = p.deg_in[i], dout = p.deg_out[o];
  return p.strict ? di < dout : di <= dout;
}

// Element e (0 .. ROWS * ML_KC) of a thread's share of a ROWS x ML_KC chunk: k-contiguous operands walk k fastest
// (coalesced along k), row-contiguous operands walk rows fastest.
template <int ROWS, bool KCONTIG>
__device__ __forceinline__ void ml_coord(int e, int& r, int& k) {
  if (KCONTIG) {
    r = e / ML_KC;
    k = e % ML_KC;
  } else {
    r = e % ROWS;
    k = e / ROWS;
  }
}

template <int MODE, bool AK, bool BK>
__global__ void __launch_bounds__(ML_THREADS) ml_gemm_kernel(const MlArgs p) {
  __shared__ float s_a[ML_BM * ML_LD];
  __shared__ float s_b[ML_BN * ML_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int c0 = blockIdx.x * ML_BN, r0 = blockIdx.y * ML_BM;
  const bool masked = p.deg_in != nullptr;
  // forward: the first row tile writes W o M back; the data gradient has W in B with o = k, i = c
  const bool write_back = MODE == ML_FWD && p.wb != nullptr && blockIdx.y == 0;
  const int kbeg = blockIdx.z * p.kper;
  const int kend = min(p.K, kbeg + p.kper);

  float ra[ML_A_PER], rb[ML_B_PER];
  auto load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < ML_A_PER; ++j) {
      int r, k;
      ml_coord<ML_BM, AK>(tid + j * ML_THREADS, r, k);
      const int gr = r0 + r, gk = k0 + k;
      ra[j] = (gr < p.R && gk < kend) ? p.a[(size_t)gr * p.a_rs + (size_t)gk * p.a_ks] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < ML_B_PER; ++j) {
      int c, k;
      ml_coord<ML_BN, BK>(tid + j * ML_THREADS, c, k);
      const int gc = c0 + c, gk = k0 + k;
      rb[j] = (gc < p.C && gk < kend) ? p.b[(size_t)gc * p.b_rs + (size_t)gk * p.b_ks] : 0.f;
    }
  };
  auto store = [&](int k0) {
#pragma unroll
    for (int j = 0; j < ML_A_PER; ++j) {
      int r, k;
      ml_coord<ML_BM, AK>(tid + j * ML_THREADS, r, k);
      s_a[r * ML_LD + k] = ra[j];
    }
#pragma unroll
    for (int j = 0; j < ML_B_PER; ++j) {
      int c, k;
      ml_coord<ML_BN, BK>(tid + j * ML_THREADS, c, k);
      float v = rb[j];
      const int gc = c0 + c, gk = k0 + k;
      if (MODE != ML_WGRAD && masked && gc < p.C && gk < kend) {
        const bool keep = MODE == ML_FWD ? ml_keep(p, gc, gk) : ml_keep(p, gk, gc);
        v *= keep ? 1.f : 0.f;  // the reference's `weight.data *= mask` (w * 0 keeps the sign of a zero)
        if (write_back) p.wb[(size_t)gc * p.b_rs + gk] = v;
      }
      s_b[c * ML_LD + k] = v;
    }
  };

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.f;  // weight grad: row tid of the tile (tid < ML_BM) sums its dY entries in k order
  const bool do_db = MODE == ML_WGRAD && p.db != nullptr && blockIdx.x == 0;
  const int nch = (kend - kbeg + ML_KC - 1) / ML_KC;
  load(kbeg);
  for (int ch = 0; ch < nch; ++ch) {
    const int k0 = kbeg + ch * ML_KC;
    store(k0);
    __syncthreads();
    if (ch + 1 < nch) load(k0 + ML_KC);  // in flight while this chunk is multiplied
    const float* ap = s_a + (wave * 16 + lr) * ML_LD + lk;
    const float* bp0 = s_b + lr * ML_LD + lk;
    const float* bp1 = s_b + (16 + lr) * ML_LD + lk;
#pragma unroll
    for (int kk = 0; kk < ML_KC; kk += 4) {
      const float av = ap[kk];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp0[kk], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp1[kk], acc1, 0, 0, 0);
    }
    if (do_db && tid < ML_BM) {
      const float* row = s_a + tid * ML_LD;
      for (int k = 0; k < ML_KC; ++k) dbsum += row[k];  // zero beyond K
    }
    __syncthreads();
  }
  if (do_db && tid < ML_BM && r0 + tid < p.R) p.db[r0 + tid] += dbsum;

  // D layout: column = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const f32x4 acc = t ? acc1 : acc0;
    const int gc = c0 + t * 16 + lr;
    if (gc >= p.C) continue;
    const float bv = (MODE == ML_FWD && p.bias) ? p.bias[gc] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gr = r0 + wave * 16 + lk * 4 + q;
      if (gr >= p.R) continue;
      float* dst = p.c + (size_t)gr * p.ldc + gc;
      if (MODE != ML_WGRAD && p.part) {  // split-K: the epilogue runs in ml_splitk_reduce_kernel
        p.part[(size_t)blockIdx.z * p.R * p.ldc + (size_t)gr * p.ldc + gc] = acc[q];
      } else if (MODE == ML_FWD) {
        const float v = acc[q] + bv;
        *dst = (p.relu && v < 0.f) ? 0.f : v;
      } else if (MODE == ML_DGRAD) {
        float v = acc[q];
        if (p.relu_src && !(p.relu_src[(size_t)gr * p.ldc + gc] > 0.f)) v = 0.f;
        *dst = v;
      } else {
        *dst += acc[q];
      }
    }
  }
}

// Split-K epilogue: c[r][col] = sum of the slices' partial sums in slice order (deterministic), then the forward's bias +
// ReLU or the data gradient's ReLU' gate.
__global__ void __launch_bounds__(256) ml_splitk_reduce_kernel(const MlArgs p, int slices) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)p.R * p.ldc;
  if (e >= total) return;
  const int col = (int)(e % p.ldc);
  float v = 0.f;
  for (int z = 0; z < slices; ++z) v += p.part[(size_t)z * total + e];
  if (p.bias) v += p.bias[col];
  if (p.relu && v < 0.f) v = 0.f;
  if (p.relu_src && !(p.relu_src[e] > 0.f)) v = 0.f;
  p.c[e] = v;
}

// mask[o][i] = deg_in[i] <= deg_out[o] (strict: <) as 0. / 1.
__global__ void __launch_bounds__(256) ml_mask_kernel(float* __restrict__ mask, const int* __restrict__ deg_in,
                                                      const int* __restrict__ deg_out, int strict, int in, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int o = (int)(e / in), i = (int)(e % in);
  const int di = deg_in[i], dout = deg_out[o];
  mask[e] = (strict ? di < dout : di <= dout) ? 1.f : 0.f;
}

constexpr int ML_MAX_ROW_TILES = 65535;  // gridDim.y

int ml_check(const char* name, int N, int in, int out, const int* deg_in, const int* deg_out) {
  PG_REQUIRE(N >= 1 && in >= 1 && out >= 1, PG_ESHAPE, "%s: N = %d, in = %d, out = %d must all be >= 1", name, N, in,
             out);
  PG_REQUIRE(pg_cdiv(N, ML_BM) <= ML_MAX_ROW_TILES && pg_cdiv(out, ML_BM) <= ML_MAX_ROW_TILES, PG_ESHAPE,
             "%s: N = %d or out = %d above %d", name, N, out, ML_MAX_ROW_TILES * ML_BM);
  PG_REQUIRE((deg_in == nullptr) == (deg_out == nullptr), PG_EINVAL,
             "%s: pass both degree vectors (masked) or neither (unmasked)", name);
  return 0;
}

// K slices of the forward / data gradient: a problem with fewer than 128 output tiles (e.g. the recipe's 8000 -> 784
// layer: 25 tiles, K = 8000) is split along k until it fills about 256 workgroups, at least ML_KC per slice.
int ml_slices(int R, int C, int K, int& kper) {
  const long tiles = (long)pg_cdiv(C, ML_BN) * pg_cdiv(R, ML_BM);
  const int chunks = pg_cdiv(K, ML_KC);
  int ks = 1;
  if (tiles < 128 && chunks > 2) ks = (int)std::min<long>((256 + tiles - 1) / tiles, chunks);
  kper = pg_cdiv(chunks, ks) * ML_KC;
  return pg_cdiv(K, kper);
}

size_t ml_ws_floats(int R, int C, int K) {
  int kper;
  const int ks = ml_slices(R, C, K, kper);
  return ks > 1 ? (size_t)ks * R * C : 0;
}

template <int MODE, bool AK, bool BK>
int ml_launch(MlArgs p, float* ws, size_t ws_floats, hipStream_t st, const char* name) {
  int ks = 1;
  p.kper = p.K;
  if (MODE != ML_WGRAD) {
    ks = ml_slices(p.R, p.C, p.K, p.kper);
    if (ks > 1) {
      const size_t need = (size_t)ks * p.R * p.C;
      PG_REQUIRE(ws != nullptr && ws_floats >= need, PG_EINVAL, "%s: workspace of %zu floats < %zu (_workspace_floats)",
                 name, ws_floats, need);
      p.part = ws;
    }
  }
  dim3 grid((unsigned)pg_cdiv(p.C, ML_BN), (unsigned)pg_cdiv(p.R, ML_BM), (unsigned)ks);
  hipLaunchKernelGGL((ml_gemm_kernel<MODE, AK, BK>), grid, dim3(ML_THREADS), 0, st, p);
  PG_LAUNCH_CHECK(name);
  if (ks > 1) {
    hipLaunchKernelGGL(ml_splitk_reduce_kernel, dim3((unsigned)pg_cdiv((long)p.R * p.C, 256)), dim3(256), 0, st, p, ks);
    PG_LAUNCH_CHECK(name);
  }
  return 0;
}

MlArgs ml_args() {
  MlArgs p;
  p.a = p.b = p.bias = p.relu_src = nullptr;
  p.wb = p.c = p.db = p.part = nullptr;
  p.deg_in = p.deg_out = nullptr;
  p.a_rs = p.a_ks = p.b_rs = p.b_ks = p.ldc = 0;
  p.R = p.C = p.K = p.strict = p.relu = p.kper = 0;
  return p;
}

}  // namespace

PG_EXPORT size_t pg_masked_linear_workspace_floats(int N, int in, int out, int dgrad) {
  if (N < 1 || in < 1 || out < 1) return 0;
  return dgrad ? ml_ws_floats(N, in, out) : ml_ws_floats(N, out, in);
}

PG_EXPORT int pg_masked_linear_fwd(const float* x, float* w, const float* b, const int* deg_in, const int* deg_out,
                                   int strict, float* y, int N, int in, int out, int relu, float* ws, size_t ws_floats,
                                   void* stream) {
  const int rc = ml_check("pg_masked_linear_fwd", N, in, out, deg_in, deg_out);
  if (rc) return rc;
  PG_REQUIRE(x && w && y, PG_EINVAL, "pg_masked_linear_fwd: null pointer");
  MlArgs p = ml_args();
  p.a = x;
  p.a_rs = in;
  p.a_ks = 1;
  p.b = w;
  p.b_rs = in;
  p.b_ks = 1;
  p.wb = deg_in ? w : nullptr;
  p.bias = b;
  p.deg_in = deg_in;
  p.deg_out = deg_out;
  p.strict = strict != 0;
  p.relu = relu != 0;
  p.c = y;
  p.ldc = out;
  p.R = N;
  p.C = out;
  p.K = in;
  return ml_launch<ML_FWD, true, true>(p, ws, ws_floats, (hipStream_t)stream, "pg_masked_linear_fwd");
}

PG_EXPORT int pg_masked_linear_dgrad(const float* dy, const float* w, const int* deg_in, const int* deg_out, int strict,
                                     const float* relu_out, float* dx, int N, int in, int out, float* ws,
                                     size_t ws_floats, void* stream) {
  const int rc = ml_check("pg_masked_linear_dgrad", N, in, out, deg_in, deg_out);
  if (rc) return rc;
  PG_REQUIRE(dy && w && dx, PG_EINVAL, "pg_masked_linear_dgrad: null pointer");
  MlArgs p = ml_args();
  p.a = dy;
  p.a_rs = out;
  p.a_ks = 1;
  p.b = w;  // B(c = i, k = o) = w[o * in + i]
  p.b_rs = 1;
  p.b_ks = in;
  p.deg_in = deg_in;
  p.deg_out = deg_out;
  p.strict = strict != 0;
  p.relu_src = relu_out;
  p.c = dx;
  p.ldc = in;
  p.R = N;
  p.C = in;
  p.K = out;
  return ml_launch<ML_DGRAD, true, false>(p, ws, ws_floats, (hipStream_t)stream, "pg_masked_linear_dgrad");
}

PG_EXPORT int pg_masked_linear_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int in, int out,
                                     void* stream) {
  const int rc = ml_check("pg_masked_linear_wgrad", N, in, out, nullptr, nullptr);
  if (rc) return rc;
  PG_REQUIRE(x && dy && dw, PG_EINVAL, "pg_masked_linear_wgrad: null pointer");
  MlArgs p = ml_args();
  p.a = dy;  // A(r = o, k = n) = dy[n * out + o]
  p.a_rs = 1;
  p.a_ks = out;
  p.b = x;  // B(c = i, k = n) = x[n * in + i]
  p.b_rs = 1;
  p.b_ks = in;
  p.c = dw;
  p.db = db;
  p.ldc = in;
  p.R = out;
  p.C = in;
  p.K = N;
  return ml_launch<ML_WGRAD, false, false>(p, nullptr, 0, (hipStream_t)stream, "pg_masked_linear_wgrad");
}

PG_EXPORT int pg_masked_linear_mask(float* mask, const int* deg_in, const int* deg_out, int strict, int in, int out,
                                    void* stream) {
  PG_REQUIRE(in >= 1 && out >= 1, PG_ESHAPE, "pg_masked_linear_mask: in = %d, out = %d must be >= 1", in, out);
  PG_REQUIRE(mask && deg_in && deg_out, PG_EINVAL, "pg_masked_linear_mask: null pointer");
  const long total = (long)in * out;
  ml_mask_kernel<<<pg_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(mask, deg_in, deg_out, strict != 0, in, total);
  PG_LAUNCH_CHECK("pg_masked_linear_mask");
  return 0;
}
