// vq_mfma.hip — vector quantisation for any embedding width, and the codebook's gradient (reference nn/utils.py:53-96).
//
// vq_tiled_assign_kernel: the assignment as a pairwise-distance GEMM with a running argmin, the structure of density.hip
// with (best, index) in place of the running logsumexp. A workgroup owns 64 positions (p = n * L + l, read from the NCHW
// planes: consecutive lanes read consecutive l), walks the codes in tiles of 32 in ascending order, and walks D in chunks
// of 64 through LDS (4 waves, v_mfma_f32_16x16x4_f32, the next chunk prefetched into registers), so any D >= 1 works and
// nothing of size P x K leaves the chip. The distance has the reference's form (|x|^2 + |e|^2) - 2 x.e; |e|^2 and |x|^2 are
// summed from the staged operands. Every lane compares with a strict '<' over ascending codes, and the 16 lanes of a row
// merge with "smaller distance, then smaller index": the FIRST minimum wins, as in torch.argmin and vq_assign_kernel.
// Outputs are those of vq_assign_kernel (idx, q, the straight-through value x + (q - x), the commitment-loss sum).
//
// vq_cbgrad_kernel: dE[k][d] = g (2 / numel) sum_{p : idx[p] = k} (q[p][d] - x[p][d]), the gradient of the embedding loss
// mse(q, x.detach()) of a codebook trained by gradient descent (:93). It is the GEMM onehot^T (q - x): the one-hot operand
// is generated from idx in the MFMA operand read (exact 0 / 1, so the products are exact), the differences themselves are
// accumulated (count E - sum x cancels once the codebook fits the data). Ranges of positions go to separate workgroups,
// each WRITES its whole (codes x dims) tile of the workspace (no zero fill needed, none is assumed), and
// vq_cbgrad_finish_kernel adds the ranges in order: no float atomics, bit-reproducible in both determinism modes.
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int VT_THREADS = 256;
constexpr int VT_BM = 64;            // positions per workgroup / per chunk
constexpr int VT_BN = 32;            // codes per tile
constexpr int VT_DC = 64;            // dims per LDS chunk
constexpr int VT_LDA = VT_BM + 16;   // x chunk [d][position]: stores along positions, MFMA reads 16 positions x 4 dims
constexpr int VT_LDB = VT_DC + 4;    // code chunk [code][d] (density.hip's stride)
constexpr int VT_A_PER = VT_BM * VT_DC / VT_THREADS;  // 16
constexpr int VT_B_PER = VT_BN * VT_DC / VT_THREADS;  // 8

constexpr int CG_BK = 64;            // codes per workgroup (16 per wave)
constexpr int CG_BD = 32;            // dims per workgroup
constexpr int CG_LD = VT_BM + 4;     // difference chunk [d][position]
constexpr int CG_PER = CG_BD * VT_BM / VT_THREADS;    // 8
constexpr int CG_MAX_SPLITS = 32;

constexpr int VT_MAX_D = 1 << 20;
constexpr int VT_MAX_K = 65535 * CG_BK;               // gridDim.y of the gradient kernel
constexpr long VT_MAX_P = (1L << 31) - 1 - VT_BM;     // idx and block offsets stay in int range

using pg_tile::f32x4;

__global__ void __launch_bounds__(VT_THREADS) vq_tiled_assign_kernel(
    const float* __restrict__ x, const float* __restrict__ emb, int* __restrict__ idx, float* __restrict__ q,
    float* __restrict__ st, float* __restrict__ loss, int N, int D, int L, int K, float inv_numel) {
  __shared__ float s_a[VT_DC * VT_LDA];
  __shared__ float s_b[VT_BN * VT_LDB];
  __shared__ float s_x2[4 * VT_BM];
  __shared__ float s_e2[VT_BN];
  __shared__ int s_idx[VT_BM];
  __shared__ float s_part[VT_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const long P = (long)N * L;
  const long pr = (long)blockIdx.x * VT_BM + lane;  // the position this thread stages and writes
  const bool pvalid = pr < P;
  const int n = pvalid ? (int)(pr / L) : 0;
  const int l = pvalid ? (int)(pr - (long)n * L) : 0;
  const size_t xoff = (size_t)n * D * L + l;  // element d of the position: xoff + d * L
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int nch = (D + VT_DC - 1) / VT_DC;

  float x2r[4] = {0.f, 0.f, 0.f, 0.f};
  float best[4];
  int bi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) best[r] = 3.0e38f, bi[r] = 0;

  for (int c0 = 0; c0 < K; c0 += VT_BN) {
    const bool first = c0 == 0;
    float ra[VT_A_PER], rb[VT_B_PER], sq[VT_B_PER];
    float x2p = 0.f;
#pragma unroll
    for (int j = 0; j < VT_B_PER; ++j) sq[j] = 0.f;
    auto load = [&](int d0) {
#pragma unroll
      for (int j = 0; j < VT_A_PER; ++j) {  // dim wave + 4 j of the chunk, position `lane`
        const int gd = d0 + wave + 4 * j;
        ra[j] = (pvalid && gd < D) ? x[xoff + (size_t)gd * L] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < VT_B_PER; ++j) {  // code wave + 4 j of the tile, dim `lane`
        const int gc = c0 + wave + 4 * j, gd = d0 + lane;
        rb[j] = (gc < K && gd < D) ? emb[(size_t)gc * D + gd] : 0.f;
      }
    };
    f32x4 t0 = zero, t1 = zero;
    load(0);
    for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
      for (int j = 0; j < VT_A_PER; ++j) {
        s_a[(wave + 4 * j) * VT_LDA + lane] = ra[j];
        if (first) x2p = fmaf(ra[j], ra[j], x2p);
      }
#pragma unroll
      for (int j = 0; j < VT_B_PER; ++j) {
        s_b[(wave + 4 * j) * VT_LDB + lane] = rb[j];
        sq[j] = fmaf(rb[j], rb[j], sq[j]);
      }
      __syncthreads();
      if (ch + 1 < nch) load((ch + 1) * VT_DC);  // in flight while this chunk is multiplied
      const float* ap = s_a + lk * VT_LDA + wave * 16 + lr;
      const float* bp0 = s_b + lr * VT_LDB + lk;
      const float* bp1 = s_b + (16 + lr) * VT_LDB + lk;
      f32x4 a0 = zero, a1 = zero;  // this chunk alone, summed from zero (density.hip: error grows with chunks, not terms)
#pragma unroll
      for (int kk = 0; kk < VT_DC; kk += 4) {
        const float av = ap[kk * VT_LDA];
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp0[kk], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp1[kk], a1, 0, 0, 0);
      }
      t0 += a0;
      t1 += a1;
      __syncthreads();
    }
    // |e|^2 of the tile's codes (a wave holds code wave + 4 j across its lanes), |x|^2 once
#pragma unroll
    for (int j = 0; j < VT_B_PER; ++j) {
      const float v = pg_wave_sum(sq[j]);
      if (lane == 0) s_e2[wave + 4 * j] = v;
    }
    if (first) s_x2[wave * VT_BM + lane] = x2p;
    __syncthreads();
    if (first) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + lk * 4 + r;
        x2r[r] = (s_x2[row] + s_x2[VT_BM + row]) + (s_x2[2 * VT_BM + row] + s_x2[3 * VT_BM + row]);
      }
    }
    // accumulator element r of tile t: position wave * 16 + lk * 4 + r, code c0 + 16 t + lr — ascending per lane
    if (c0 + lr < K) {
      const float e2 = s_e2[lr];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dist = (x2r[r] + e2) - 2.f * t0[r];
        if (dist < best[r]) best[r] = dist, bi[r] = c0 + lr;
      }
    }
    if (c0 + 16 + lr < K) {
      const float e2 = s_e2[16 + lr];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dist = (x2r[r] + e2) - 2.f * t1[r];
        if (dist < best[r]) best[r] = dist, bi[r] = c0 + 16 + lr;
      }
    }
    // s_e2 is rewritten only after the next tile's chunk barriers
  }
  // the 16 lanes of a position merge: smaller distance, then smaller index
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ob = __shfl_xor(best[r], off, 64);
      const int oi = __shfl_xor(bi[r], off, 64);
      if (ob < best[r] || (ob == best[r] && oi < bi[r])) best[r] = ob, bi[r] = oi;
    }
  }
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s_idx[wave * 16 + lk * 4 + r] = bi[r];
  }
  __syncthreads();
  // outputs: thread = (position `lane`, dims wave, wave + 4, ...)
  float s = 0.f;
  if (pvalid) {
    const int code = s_idx[lane];
    if (wave == 0) idx[pr] = code;
    const float* ep = emb + (size_t)code * D;
    for (int d = wave; d < D; d += 4) {
      const size_t o = xoff + (size_t)d * L;
      const float xv = x[o], qv = ep[d];
      q[o] = qv;
      st[o] = xv + (qv - xv);  // the straight-through VALUE of nn/utils.py:95
      const float df = xv - qv;
      s += df * df;
    }
  }
  // commitment loss mse(x, q): block sum, one atomic per block (as vq_assign_kernel)
  s = pg_wave_sum(s);
  if (lane == 0) s_part[wave] = s;
  __syncthreads();
  if (tid == 0) atomicAdd(loss, ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) * inv_numel);
}

// part[(z K + k) D + d] = sum over the positions of range z with idx[p] = k of (q[p][d] - x[p][d]).
// grid (dim tiles of 32, code tiles of 64, ranges of `cper` 64-position chunks)
__global__ void __launch_bounds__(VT_THREADS) vq_cbgrad_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                               const int* __restrict__ idx, float* __restrict__ part,
                                                               int N, int D, int L, int K, int cper) {
  __shared__ float s_d[CG_BD * CG_LD];
  __shared__ int s_i[VT_BM];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const long P = (long)N * L;
  const int d0 = blockIdx.x * CG_BD, k0 = blockIdx.y * CG_BK;
  const int chunks = (int)((P + VT_BM - 1) / VT_BM);
  const int cbeg = blockIdx.z * cper, cend = min(chunks, cbeg + cper);
  const int mycode = k0 + wave * 16 + lr;  // the A-operand row of this lane
  float rd[CG_PER];
  int ri = -1;
  auto load = [&](int ch) {
    const long pr = (long)ch * VT_BM + lane;
    const bool pvalid = pr < P;
    const int n = pvalid ? (int)(pr / L) : 0;
    const int l = pvalid ? (int)(pr - (long)n * L) : 0;
    const size_t off = (size_t)n * D * L + l;
#pragma unroll
    for (int j = 0; j < CG_PER; ++j) {
      const int gd = d0 + wave + 4 * j;
      const size_t o = off + (size_t)gd * L;
      rd[j] = (pvalid && gd < D) ? q[o] - x[o] : 0.f;
    }
    ri = pvalid ? idx[pr] : -1;  // -1 matches no code
  };
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 a0 = zero, a1 = zero;
  if (cbeg < cend) load(cbeg);
  for (int ch = cbeg; ch < cend; ++ch) {
#pragma unroll
    for (int j = 0; j < CG_PER; ++j) s_d[(wave + 4 * j) * CG_LD + lane] = rd[j];
    if (wave == 0) s_i[lane] = ri;
    __syncthreads();
    if (ch + 1 < cend) load(ch + 1);
    const float* bp0 = s_d + lr * CG_LD + lk;
    const float* bp1 = s_d + (16 + lr) * CG_LD + lk;
#pragma unroll
    for (int pp = 0; pp < VT_BM; pp += 4) {
      const float oh = s_i[pp + lk] == mycode ? 1.f : 0.f;  // onehot^T[code][position]
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(oh, bp0[pp], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(oh, bp1[pp], a1, 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int code = k0 + wave * 16 + lk * 4 + r;
    if (code >= K) continue;
    float* row = part + ((size_t)blockIdx.z * K + code) * D;
    if (d0 + lr < D) row[d0 + lr] = a0[r];
    if (d0 + 16 + lr < D) row[d0 + 16 + lr] = a1[r];
  }
}

// dE (+)= g (2 / numel) * (the ranges added in order)
__global__ void __launch_bounds__(256) vq_cbgrad_finish_kernel(const float* __restrict__ part,
                                                               const float* __restrict__ g_loss, float* __restrict__ dE,
                                                               long total, int ns, float two_inv_numel, int accumulate) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float s = 0.f;
  for (int z = 0; z < ns; ++z) s += part[(size_t)z * total + e];
  const float v = (g_loss[0] * two_inv_numel) * s;
  dE[e] = accumulate ? dE[e] + v : v;
}

int vt_check(const char* name, int N, int D, int L, int K) {
  PG_REQUIRE(N >= 1 && D >= 1 && L >= 1 && K >= 1, PG_ESHAPE, "%s: N = %d, D = %d, L = %d, K = %d must all be >= 1", name,
             N, D, L, K);
  PG_REQUIRE(D <= VT_MAX_D && K <= VT_MAX_K, PG_ESHAPE, "%s: D = %d above %d or K = %d above %d", name, D, VT_MAX_D, K,
             VT_MAX_K);
  PG_REQUIRE((long)N * L <= VT_MAX_P && (long)N * L * D < (1L << 40) && (long)K * D < (1L << 31), PG_ESHAPE,
             "%s: N * L = %ld, N * L * D or K * D too large", name, (long)N * L);
  return 0;
}

// Ranges of positions of the gradient: whole 64-position chunks, until about 512 workgroups run.
int cg_splits(int N, int D, int L, int K, int& cper) {
  const long wgs = (long)pg_cdiv(D, CG_BD) * pg_cdiv(K, CG_BK);
  const int chunks = pg_cdiv((long)N * L, VT_BM);
  long ns = (512 + wgs - 1) / wgs;
  if (ns > chunks) ns = chunks;
  if (ns > CG_MAX_SPLITS) ns = CG_MAX_SPLITS;
  cper = pg_cdiv(chunks, ns);
  return pg_cdiv(chunks, cper);  // every range holds at least one chunk
}

}  // namespace

PG_EXPORT int pg_vq_assign_tiled(const float* x, const float* embedding, int* idx, float* q, float* st, float* loss,
                                 int N, int D, int L, int K, void* stream) {
  const char* name = "pg_vq_assign_tiled";
  const int rc = vt_check(name, N, D, L, K);
  if (rc) return rc;
  PG_REQUIRE(x && embedding && idx && q && st && loss, PG_EINVAL, "%s: null pointer", name);
  const long P = (long)N * L;
  const float inv_numel = 1.f / ((float)P * (float)D);
  hipLaunchKernelGGL(vq_tiled_assign_kernel, dim3((unsigned)pg_cdiv(P, VT_BM)), dim3(VT_THREADS), 0, (hipStream_t)stream,
                     x, embedding, idx, q, st, loss, N, D, L, K, inv_numel);
  PG_LAUNCH_CHECK(name);
  return 0;
}

PG_EXPORT size_t pg_vq_codebook_grad_workspace_floats(int N, int D, int L, int K) {
  if (N < 1 || D < 1 || L < 1 || K < 1 || D > VT_MAX_D || K > VT_MAX_K || (long)N * L > VT_MAX_P ||
      (long)K * D >= (1L << 31))
    return 0;
  int cper;
  return (size_t)cg_splits(N, D, L, K, cper) * (size_t)K * (size_t)D;
}

PG_EXPORT int pg_vq_codebook_grad(const float* x, const float* q, const int* idx, const float* g_loss, float* d_embedding,
                                  int accumulate, int N, int D, int L, int K, float* ws, size_t ws_floats, void* stream) {
  const char* name = "pg_vq_codebook_grad";
  const int rc = vt_check(name, N, D, L, K);
  if (rc) return rc;
  PG_REQUIRE(x && q && idx && g_loss && d_embedding, PG_EINVAL, "%s: null pointer", name);
  const size_t need = pg_vq_codebook_grad_workspace_floats(N, D, L, K);
  PG_REQUIRE(ws != nullptr && ws_floats >= need, PG_EINVAL,
             "%s: workspace of %zu floats < %zu (pg_vq_codebook_grad_workspace_floats)", name, ws_floats, need);
  hipStream_t s = (hipStream_t)stream;
  int cper;
  const int ns = cg_splits(N, D, L, K, cper);
  const dim3 grid((unsigned)pg_cdiv(D, CG_BD), (unsigned)pg_cdiv(K, CG_BK), (unsigned)ns);
  hipLaunchKernelGGL(vq_cbgrad_kernel, grid, dim3(VT_THREADS), 0, s, x, q, idx, ws, N, D, L, K, cper);
  PG_LAUNCH_CHECK(name);
  const long total = (long)K * D;
  const float two_inv_numel = 2.f / ((float)((long)N * L) * (float)D);
  hipLaunchKernelGGL(vq_cbgrad_finish_kernel, dim3((unsigned)pg_cdiv(total, 256)), dim3(256), 0, s, ws, g_loss, d_embedding,
                     total, ns, two_inv_numel, accumulate);
  PG_LAUNCH_CHECK(name);
  return 0;
}
