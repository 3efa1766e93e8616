// gpt_block.hip — everything of an ImageGPT transformer block that is not the attention core, as two
// forward and two backward kernels working on 16-pixel tiles held in registers, a fifth that runs
// a block's tail and the next block's head forward in one launch, a sixth that runs the next block's head and the block's tail
// backward in one launch, and the model's one segmented-reduce
// kernel, which adds the rows of partial weight-gradient sums that the backward kernels here and in
// gpt_ends.hip leave.
//
// Reference (models/autoregressive/image_gpt.py:21-52, :104-109), C = n_embedding_channels = 16:
//   head:  qkv   = [W_q; W_kv] LN1(x) + [b_q; b_kv]                  (nn/attention.py:134-143)
//   (attention core: attention*.hip)
//   tail:  x_mid = x + W_p o + b_p                                    (x + attn(ln1(x)),   :50)
//          b     = x_mid + W_2 gelu(W_1 LN2(x_mid) + b_1) + b_2       (x + mlp(ln2(x)),    :51-52)
//          x_new = x + b                                              (the model loop adds x again, :107)
// Unfused this is 2 LayerNorms, 5 1x1 convolutions, GELU and 3 adds forward and their 25-odd backward
// launches, each streaming (N, 16..64, L) tensors through HBM. Here a wave owns 16 pixels at a time:
// every [channels x 16 px] intermediate is an MFMA accumulator tile ("D layout": lane (pixel j,
// group g), register r <-> channel 4g + r), and a D-layout tile IS a valid B operand of the next
// v_mfma_f32_16x16x4_f32 (K-step r contracts channels {4g + r}), so the whole chain — projection,
// residual, LayerNorm, fc1, GELU, fc2, residuals — never leaves the register file. Per layer the
// kernels read x, o (resp. d x_new, d qkv) once and write qkv, x_new (resp. d o, d x) once.
// Weight gradients contract over pixels: both operands go through per-wave LDS transposes (the loaded ones,
// d qkv / d x_new / o, are written from the registers that already hold them instead of being read from
// global memory a second time in transposed order); partial sums live in registers for all the
// tiles of a wave, are reduced per workgroup in LDS to one row per workgroup, and seg_reduce_kernel adds the rows
// (deterministic: a fixed order, the same whether a kernel's rows are reduced at once, alone, or later in a launch
// shared with other blocks and the model's ends).
// Backward recomputes x_mid, both LayerNorms and the hidden activations instead of storing them.
// The tile loops are software-pipelined: a wave issues the global loads of its next tile before the
// MFMA/VALU chain of the tile in hand and touches them after its stores (see prefetch_fence below).
#include <stdlib.h>

#include "common.h"
#include "gpt_ends.h"
#include "mfma_tile.h"

namespace {

using pg_tile::f32x4;
using pg_tile::mfma16;

constexpr int C = 16, HD = 64, QKV = 48;
constexpr int GB_THREADS = 256;  // 4 waves
constexpr int TS = 20;           // LDS row stride (floats) of a transposed [channel][16 px] tile
constexpr float INV_C = 1.f / 16.f;

constexpr int TB_WAVE_ROWS = 6 * C;  // the tail backward chain's per-wave LDS tiles: G, dH of one hidden chunk, LN2, dx_mid, D, o; 16 rows of TS each
constexpr int TB_FRAGS = 64;         // its per-lane operands kept in LDS: w1f, w2t, w1t, b1r [4][4]
// partial-row layouts (floats)
constexpr int T_W1 = 0, T_B1 = T_W1 + HD * C, T_W2 = T_B1 + HD, T_B2 = T_W2 + C * HD, T_WP = T_B2 + C,
              T_BP = T_WP + C * C, T_G2 = T_BP + C, T_BE2 = T_G2 + C, T_PART = T_BE2 + C;          // 2432
constexpr int H_WQ = 0, H_WKV = H_WQ + C * C, H_BQ = H_WKV + 2 * C * C, H_BKV = H_BQ + C,
              H_G1 = H_BKV + 2 * C, H_BE1 = H_G1 + C, H_PART = H_BE1 + C;                            // 848

struct BlockArgs {
  // head
  const float* x; const float* g1; const float* be1; const float* wq; const float* bq;
  const float* wkv; const float* bkv; float* qkv; const float* dqkv; const float* gx; float* dx;
  // tail
  const float* o; const float* wp; const float* bp; const float* g2; const float* be2;
  const float* w1; const float* b1; const float* w2; const float* b2;
  float* xnew; const float* dxnew; float* d_o; float* gx_out;
  float* part;
  // head(i+1) + tail(i) backward: x of the tail's block (x is the head's), the tail's partial rows (part is the head's) and the
  // rows that the two reduce jobs count
  const float* tx; float* tpart; int head_rows, tail_rows;
  int N, L, tiles_per_img, total_tiles;
  float eps;
};

struct Ln { float mu, rs; f32x4 xhat; };

__device__ __forceinline__ float gsum4(float s) {  // over the four lane groups g
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  return s;
}
__device__ __forceinline__ float jsum16(float s) {  // over the 16 pixel lanes of a group
  s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
  return s;
}

// LayerNorm statistics of this lane's pixel: its 16 channels are 4 registers x 4 lane groups
// (biased variance, eps inside the square root, one Newton step on v_rsq_f32 — as layernorm.hip)
__device__ __forceinline__ Ln ln_stats(const f32x4& v, float eps) {
  Ln s;
  s.mu = gsum4((v[0] + v[1]) + (v[2] + v[3])) * INV_C;
  const f32x4 dd = {v[0] - s.mu, v[1] - s.mu, v[2] - s.mu, v[3] - s.mu};
  const float a = gsum4(fmaf(dd[0], dd[0], fmaf(dd[1], dd[1], fmaf(dd[2], dd[2], dd[3] * dd[3])))) * INV_C + eps;
  float rs = rsqrtf(a);
  rs = rs * (1.5f - 0.5f * a * rs * rs);
  s.rs = rs;
  s.xhat = f32x4{dd[0] * rs, dd[1] * rs, dd[2] * rs, dd[3] * rs};
  return s;
}

// D-layout tile of a 16-channel tensor: register r <-> channel ch0 + 4g + r of pixel `base`
__device__ __forceinline__ f32x4 load_tile(const float* __restrict__ base, int L, int g) {
  f32x4 t;
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = base[(size_t)(4 * g + r) * L];
  return t;
}
__device__ __forceinline__ void store_tile(float* __restrict__ base, int L, int g, const f32x4& t) {
#pragma unroll
  for (int r = 0; r < 4; ++r) base[(size_t)(4 * g + r) * L] = t[r];
}
// per-channel parameter vector in D layout: v[4g + r]
__device__ __forceinline__ f32x4 load_vec(const float* __restrict__ v, int g) {
  return f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
}

__device__ __forceinline__ float gelu_f(float x) { return pg_gelu(x); }

// A wave's walk over its tiles (wave, wave + nwaves, ...) as (image n, tile t within the image), all wave-uniform so
// that the address arithmetic stays on the scalar unit; one division before the loop, none inside it.
struct TileWalk {
  int n, t, dn, dt, tpi;
  __device__ __forceinline__ TileWalk(const BlockArgs& a, int wave, int nwaves)
      : n(wave / a.tiles_per_img), t(wave % a.tiles_per_img), dn(nwaves / a.tiles_per_img),
        dt(nwaves % a.tiles_per_img), tpi(a.tiles_per_img) {}
  __device__ __forceinline__ TileWalk next() const {
    TileWalk w = *this;
    w.n += dn; w.t += dt;
    if (w.t >= tpi) { w.t -= tpi; ++w.n; }
    return w;
  }
  // float offset of the tile's pixel 0 in an (N, chans, L) tensor
  __device__ __forceinline__ size_t base(int chans, int L) const { return ((size_t)n * chans) * L + t * 16; }
};
// Software pipeline of the tile loops: the loads of the wave's next tile are issued at the top of an iteration and
// first touched at its bottom, behind the whole MFMA chain and the stores. prefetch_fence() pins them there;
// wait_prologue_loads() lets the first tile land before the loop, so that the loop's own waits (which the compiler
// derives from every way into the loop) never cover loads that were issued a moment ago.
__device__ __forceinline__ void prefetch_fence() { __builtin_amdgcn_sched_barrier(0); }
// s_waitcnt immediate of gfx9 (gfx950 included): vmcnt = bits [15:14] and [3:0], expcnt [6:4], lgkmcnt [11:8]
constexpr int waitcnt_gfx9(int vm, int exp, int lgkm) { return ((vm & 0x30) << 10) | (vm & 0xF) | ((exp & 7) << 4) | ((lgkm & 0xF) << 8); }
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "wait_prologue_loads() encodes s_waitcnt for gfx9; re-derive the immediate for another target"
#endif
__device__ __forceinline__ void wait_prologue_loads() {
  constexpr int VMCNT0_ONLY = waitcnt_gfx9(/*vmcnt*/ 0, /*expcnt: no wait*/ 7, /*lgkmcnt: no wait*/ 15);
  static_assert(VMCNT0_ONLY == 0x0F70, "gfx9 s_waitcnt vmcnt(0)");
  __builtin_amdgcn_s_waitcnt(VMCNT0_ONLY);
}
// D-layout tile -> per-wave LDS tile [channel][TS] (conflict-free ds_write_b32), read back transposed with
// lds_row4: channel `row`, pixels 4g..4g+3 (one ds_read_b128)
__device__ __forceinline__ void lds_put_tile(float* t, int j, int g, const f32x4& v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) t[(4 * g + r) * TS + j] = v[r];
}
__device__ __forceinline__ f32x4 lds_row4(const float* t, int row, int g) {
  return *reinterpret_cast<const f32x4*>(t + row * TS + 4 * g);
}

// row `ch` of the merged [W_q; W_kv] matrix (each row has C entries)
__device__ __forceinline__ const float* qkv_row(const BlockArgs& a, int ch) {
  return ch < C ? a.wq + ch * C : a.wkv + (ch - C) * C;
}

// ---------------------------------------------------------------------------------- head, forward
// The per-lane operands of the head chain: A[i = out channel 16m+j][k = g <-> in channel 4g+r], bias / LN1 affine in D layout
struct HeadFrags {
  float wf[3][4]; f32x4 bias[3], gam, bet;
  __device__ __forceinline__ HeadFrags(const BlockArgs& a, int j, int g) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        wf[m][r] = qkv_row(a, 16 * m + j)[4 * g + r];
        const int ch = 16 * m + 4 * g + r;
        bias[m][r] = ch < C ? a.bq[ch] : a.bkv[ch - C];
      }
    }
    gam = load_vec(a.g1, g);
    bet = load_vec(a.be1, g);
  }
};
// head chain of one tile: q/kv tile m (channels 16m .. 16m+15) = [W_q; W_kv] LN1(x) + [b_q; b_kv]. The ONE copy of this arithmetic:
// head_fwd_kernel runs it on a loaded tile, tail_head_fwd_kernel on the x_new tile its tail chain left in registers.
__device__ __forceinline__ void head_chain(const f32x4& xv, const HeadFrags& f, float eps, f32x4 (&out)[3]) {
  const Ln s = ln_stats(xv, eps);
  f32x4 y;
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = fmaf(s.xhat[r], f.gam[r], f.bet[r]);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    out[m] = f.bias[m];
#pragma unroll
    for (int r = 0; r < 4; ++r) out[m] = mfma16(f.wf[m][r], y[r], out[m]);
  }
}
__device__ __forceinline__ void store_qkv_tiles(float* __restrict__ qb, int L, int g, const f32x4 (&q)[3]) {
#pragma unroll
  for (int m = 0; m < 3; ++m) store_tile(qb + (size_t)(16 * m) * L, L, g, q[m]);
}

__global__ void __launch_bounds__(GB_THREADS) head_fwd_kernel(const BlockArgs a) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wave = blockIdx.x * (GB_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  const HeadFrags hf(a, j, g);
  if (wave >= a.total_tiles) return;  // a wave without a tile loads nothing
  TileWalk tw(a, wave, nwaves);
  f32x4 xv = load_tile(a.x + tw.base(C, a.L) + j, a.L, g);
  wait_prologue_loads();
  for (;;) {
    // the last iteration re-reads its own tile instead of branching around the prefetch
    const TileWalk nx = tw.next();
    const bool more = nx.n < a.N;
    const f32x4 xn = load_tile(a.x + (more ? nx : tw).base(C, a.L) + j, a.L, g);
    prefetch_fence();
    f32x4 q[3];
    head_chain(xv, hf, a.eps, q);
    store_qkv_tiles(a.qkv + tw.base(QKV, a.L) + j, a.L, g, q);
    if (!more) break;
    xv = xn;
    tw = nx;
  }
}

// ---------------------------------------------------------------------------------- head, backward
// dx = LN1'(W^T dqkv) + gx ; dW += dqkv^T LN1(x) ; db += sum dqkv ; dgamma1, dbeta1
constexpr int HB_WAVE_ROWS = C + QKV;  // head backward's per-wave LDS tiles: LN1(x)^T [16] + dqkv^T [48] rows of TS
constexpr int HB_FRAGS = 20;           // per-lane operands of the head's backward chain: wt[3][4], gamma1[4], beta1[4]

__device__ __forceinline__ float sum4(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// The sums a wave keeps over all of its tiles. accb[m] belongs to channel 16m+j and holds the pixels 4g..4g+3 of every tile: it is
// summed from the transposed row that the weight-gradient MFMAs read anyway, one register per 16 channels where a D-layout sum
// takes four; the final cross-lane sum runs over the lane groups g.
struct HeadBwdAcc {
  f32x4 accw[3], dgam, dbet;
  float accb[3];
  __device__ __forceinline__ HeadBwdAcc() {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    dgam = zero4; dbet = zero4;
#pragma unroll
    for (int m = 0; m < 3; ++m) { accw[m] = zero4; accb[m] = 0.f; }
  }
};
// The chain's per-lane operands, wt(m, r) = A[i = in channel j][k = g <-> out channel 16m+4g+r] and LN1's affine in D layout:
// in registers (head_bwd_kernel) or in the workgroup's [fragment][lane] LDS copy (head_tail_bwd_kernel)
struct HeadBwdRegs {
  float w[3][4]; f32x4 gamv, betv;
  __device__ __forceinline__ HeadBwdRegs(const BlockArgs& a, int j, int g) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) w[m][r] = qkv_row(a, 16 * m + 4 * g + r)[j];
    }
    gamv = load_vec(a.g1, g);
    betv = load_vec(a.be1, g);
  }
  __device__ __forceinline__ float wt(int m, int r) const { return w[m][r]; }
  __device__ __forceinline__ float gam(int r) const { return gamv[r]; }
  __device__ __forceinline__ float bet(int r) const { return betv[r]; }
};
struct HeadBwdLds {
  const float* wlane;  // [HB_FRAGS fragments][64 lanes] + lane
  static __device__ __forceinline__ void fill(float* wl, const BlockArgs& a, int lane, int j, int g) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) wl[(4 * m + r) * 64 + lane] = qkv_row(a, 16 * m + 4 * g + r)[j];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wl[(12 + r) * 64 + lane] = a.g1[4 * g + r];
      wl[(16 + r) * 64 + lane] = a.be1[4 * g + r];
    }
  }
  __device__ __forceinline__ float wt(int m, int r) const { return wlane[(4 * m + r) * 64]; }
  __device__ __forceinline__ float gam(int r) const { return wlane[(12 + r) * 64]; }
  __device__ __forceinline__ float bet(int r) const { return wlane[(16 + r) * 64]; }
};
// head backward chain of one tile; returns dx. ty [16][TS] and tq [48][TS] are the wave's LDS tiles. The ONE copy of this
// arithmetic: head_bwd_kernel stores the dx tile, head_tail_bwd_kernel hands it to the previous block's tail chain as D.
template <class Ops>
__device__ __forceinline__ f32x4 head_bwd_chain(const f32x4& xv, const f32x4& gxv, const f32x4 (&dqv)[3], const Ops& f, float eps,
                                                float* ty, float* tq, int j, int g, HeadBwdAcc& acc) {
  // Every fused multiply-add of this chain is written out: left to itself the compiler contracts a product that has several uses
  // (gy) differently from one kernel to the next (scalar or packed, operands from registers or LDS), and dx would differ in
  // its last bit between head_bwd_kernel and head_tail_bwd_kernel. The forms below are the ones head_bwd_kernel was compiled to
  // before it shared this function (s1 and, except for element 0, gy - m1 take the unrounded product), so dx keeps its bits.
#pragma clang fp contract(off)
#pragma unroll
  for (int m = 0; m < 3; ++m) lds_put_tile(tq + 16 * m * TS, j, g, dqv[m]);
  const Ln s = ln_stats(xv, eps);
  f32x4 dy = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dy = mfma16(f.wt(m, r), dqv[m][r], dy);
  }
  // LayerNorm backward (dy is the gradient of y = xhat * gamma + beta)
  f32x4 gy;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gy[r] = dy[r] * f.gam(r);
    s1 = fmaf(dy[r], f.gam(r), s1);
    s2 = fmaf(gy[r], s.xhat[r], s2);
    acc.dgam[r] = fmaf(dy[r], s.xhat[r], acc.dgam[r]);
    acc.dbet[r] += dy[r];
    ty[(4 * g + r) * TS + j] = fmaf(s.xhat[r], f.gam(r), f.bet(r));
  }
  const float m1 = gsum4(s1) * INV_C, m2 = gsum4(s2) * INV_C;
  f32x4 dxv;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float c = r == 0 ? gy[0] - m1 : fmaf(dy[r], f.gam(r), -m1);  // element 0 from the rounded product: as compiled before
    dxv[r] = fmaf(s.rs, fmaf(-s.xhat[r], m2, c), gxv[r]);
  }
  // dW[ch][c] += sum_px dqkv[px][ch] y[px][c]
  const f32x4 yt = lds_row4(ty, j, g);  // B[k = px 4g+e][c = j]
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const f32x4 dqtm = lds_row4(tq, 16 * m + j, g);  // A[i = ch 16m+j][k = px 4g+e]
    acc.accb[m] += sum4(dqtm);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc.accw[m] = mfma16(dqtm[e], yt[e], acc.accw[m]);
  }
  return dxv;
}
// a wave's sums -> its H_PART floats of LDS staging
__device__ __forceinline__ void head_bwd_stage(float* mine, const HeadBwdAcc& acc, int j, int g) {
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) mine[H_WQ + (16 * m + 4 * g + r) * C + j] = acc.accw[m][r];  // rows 0..15 = W_q, 16..47 = W_kv
    const float b = gsum4(acc.accb[m]);
    if (g == 0) mine[H_BQ + 16 * m + j] = b;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float dg = jsum16(acc.dgam[r]), db = jsum16(acc.dbet[r]);
    if (j == 0) { mine[H_G1 + 4 * g + r] = dg; mine[H_BE1 + 4 * g + r] = db; }
  }
}
// the four waves' staged rows of n floats each, at the start of lds -> the workgroup's partial row
__device__ __forceinline__ void write_partial_row(float* __restrict__ prow, const float* lds, int n) {
  for (int i = threadIdx.x; i < n; i += GB_THREADS)
    prow[i] = (lds[i] + lds[n + i]) + (lds[2 * n + i] + lds[3 * n + i]);
}

// only x and gx of the next tile are prefetched (8 registers): with d qkv prefetched as well (12 more) the kernel leaves the
// four-waves-per-SIMD budget unless the allocator is forced, and measured within run-to-run spread of this form
__global__ void __launch_bounds__(GB_THREADS) head_bwd_kernel(const BlockArgs a) {
  extern __shared__ float4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave = blockIdx.x * (GB_THREADS / 64) + wv;
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  float* ty = lds + (size_t)wv * HB_WAVE_ROWS * TS;  // LN1(x)^T [16 c][TS]
  float* tq = ty + C * TS;                           // dqkv^T   [48 ch][TS]
  const HeadBwdRegs hf(a, j, g);
  HeadBwdAcc acc;

  if (wave < a.total_tiles) {  // a wave without a tile loads nothing
    TileWalk tw(a, wave, nwaves);
    size_t off = tw.base(C, a.L) + j;
    f32x4 xv = load_tile(a.x + off, a.L, g);
    f32x4 gxv = load_tile(a.gx + off, a.L, g);
    wait_prologue_loads();
    for (;;) {
      // d qkv of the tile in hand goes first, so that waiting for it leaves the prefetch behind it in flight
      f32x4 dqv[3];
      {
        const float* dqp = a.dqkv + tw.base(QKV, a.L) + j;
#pragma unroll
        for (int m = 0; m < 3; ++m) dqv[m] = load_tile(dqp + (size_t)(16 * m) * a.L, a.L, g);
      }
      // the last iteration re-reads its own tile instead of branching around the prefetch
      const TileWalk nx = tw.next();
      const bool more = nx.n < a.N;
      const size_t offn = (more ? nx : tw).base(C, a.L) + j;
      const f32x4 xn = load_tile(a.x + offn, a.L, g);
      const f32x4 gxn = load_tile(a.gx + offn, a.L, g);
      prefetch_fence();
      store_tile(a.dx + off, a.L, g, head_bwd_chain(xv, gxv, dqv, hf, a.eps, ty, tq, j, g, acc));
      if (!more) break;
      xv = xn;
      gxv = gxn;
      off = offn;
      tw = nx;
    }
  }

  __syncthreads();
  head_bwd_stage(lds + (size_t)wv * H_PART, acc, j, g);
  __syncthreads();
  write_partial_row(a.part + (size_t)blockIdx.x * H_PART, lds, H_PART);
}

// ---------------------------------------------------------------------------------- tail, forward
// The per-lane operands of the tail chain
struct TailFrags {
  float wpf[4];     // A[i = co j][k <-> ci 4g+r]
  float w1f[4][4];  // A[i = hidden 16m+j][k <-> c 4g+r]
  float w2f[4][4];  // A[i = co j][k <-> hidden 16m+4g+r]
  f32x4 b1r[4], bpv, b2v, gam, bet;
  __device__ __forceinline__ TailFrags(const BlockArgs& a, int j, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) wpf[r] = a.wp[j * C + 4 * g + r];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        w1f[m][r] = a.w1[(16 * m + j) * C + 4 * g + r];
        w2f[m][r] = a.w2[j * HD + 16 * m + 4 * g + r];
        b1r[m][r] = a.b1[16 * m + 4 * g + r];
      }
    }
    bpv = load_vec(a.bp, g);
    b2v = load_vec(a.b2, g);
    gam = load_vec(a.g2, g);
    bet = load_vec(a.be2, g);
  }
};
// tail chain of one tile: x_new = x + x_mid + W_2 gelu(W_1 LN2(x_mid) + b_1) + b_2, x_mid = x + W_p o + b_p. The ONE copy of this
// arithmetic, shared by tail_fwd_kernel and tail_head_fwd_kernel.
__device__ __forceinline__ f32x4 tail_chain(const f32x4& xv, const f32x4& ov, const TailFrags& f, float eps) {
  f32x4 xm = xv + f.bpv;
#pragma unroll
  for (int r = 0; r < 4; ++r) xm = mfma16(f.wpf[r], ov[r], xm);
  const Ln s = ln_stats(xm, eps);
  f32x4 y;
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = fmaf(s.xhat[r], f.gam[r], f.bet[r]);
  f32x4 h[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    h[m] = f.b1r[m];
#pragma unroll
    for (int r = 0; r < 4; ++r) h[m] = mfma16(f.w1f[m][r], y[r], h[m]);
  }
  f32x4 out = (xm + f.b2v) + xv;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out = mfma16(f.w2f[m][r], gelu_f(h[m][r]), out);
  }
  return out;
}

__global__ void __launch_bounds__(GB_THREADS) tail_fwd_kernel(const BlockArgs a) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wave = blockIdx.x * (GB_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  const TailFrags tf(a, j, g);
  if (wave >= a.total_tiles) return;  // a wave without a tile loads nothing
  TileWalk tw(a, wave, nwaves);
  size_t off = tw.base(C, a.L) + j;
  f32x4 xv = load_tile(a.x + off, a.L, g);
  f32x4 ov = load_tile(a.o + off, a.L, g);
  wait_prologue_loads();
  for (;;) {
    // the last iteration re-reads its own tile instead of branching around the prefetch
    const TileWalk nx = tw.next();
    const bool more = nx.n < a.N;
    const size_t offn = (more ? nx : tw).base(C, a.L) + j;
    const f32x4 xn = load_tile(a.x + offn, a.L, g);
    const f32x4 on = load_tile(a.o + offn, a.L, g);
    prefetch_fence();
    store_tile(a.xnew + off, a.L, g, tail_chain(xv, ov, tf, a.eps));
    if (!more) break;
    xv = xn;
    ov = on;
    off = offn;
    tw = nx;
  }
}

// ---------------------------------------------------------------------------------- tail(i) + head(i+1), forward
// A block boundary of the forward pass in one launch: the tail chain of block i, then LN1 and the q/kv projection of block i+1 on
// the x_new tile while it is still a register tile (D layout = the head's input layout). x_new is still written — the backward
// pass reads it — but never read back: 64 B per pixel and one launch less than tail_fwd + head_fwd. The tail chain is bound by
// issue (MFMA + VALU cycles add), the head by its 192 B per pixel of stores, which here drain under the next tile's chain.
// tail_fwd's registers plus the head's 12 + 12 + 8 operand registers: 164 VGPRs, three waves per SIMD (launch bounds). A form with
// those 32 and b_1's 16 operands as one [fragment][lane] copy in LDS (118 VGPRs, four waves) measured the same in the step at
// batch 1024 and slower at batch 64 (profiles/gpt_boundary.json, "other_form").
__global__ void __launch_bounds__(GB_THREADS, 3) tail_head_fwd_kernel(const BlockArgs a) {
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wave = blockIdx.x * (GB_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  const TailFrags tf(a, j, g);
  const HeadFrags hf(a, j, g);
  if (wave >= a.total_tiles) return;  // a wave without a tile loads nothing
  TileWalk tw(a, wave, nwaves);
  size_t off = tw.base(C, a.L) + j;
  f32x4 xv = load_tile(a.x + off, a.L, g);
  f32x4 ov = load_tile(a.o + off, a.L, g);
  wait_prologue_loads();
  for (;;) {
    // the last iteration re-reads its own tile instead of branching around the prefetch
    const TileWalk nx = tw.next();
    const bool more = nx.n < a.N;
    const size_t offn = (more ? nx : tw).base(C, a.L) + j;
    const f32x4 xn = load_tile(a.x + offn, a.L, g);
    const f32x4 on = load_tile(a.o + offn, a.L, g);
    prefetch_fence();
    const f32x4 out = tail_chain(xv, ov, tf, a.eps);
    store_tile(a.xnew + off, a.L, g, out);
    f32x4 q[3];
    head_chain(out, hf, a.eps, q);
    store_qkv_tiles(a.qkv + tw.base(QKV, a.L) + j, a.L, g, q);
    if (!more) break;
    xv = xn;
    ov = on;
    off = offn;
    tw = nx;
  }
}

// ---------------------------------------------------------------------------------- tail, backward
// D = d x_new. Outputs d_o = W_p^T d x_mid and gx = D + d x_mid (everything that reaches the block
// input x except through LN1), plus the gradients of W_p, b_p, LN2, fc1, fc2.
// The sums a wave keeps over all of its tiles. The bias sums db1[m] (hidden 16m+j), db2 and dbp (channel j) hold the pixels
// 4g..4g+3 of every tile, from the transposed rows that feed the weight-gradient MFMAs (as HeadBwdAcc::accb).
struct TailBwdAcc {
  f32x4 acc1[4], acc2[4], accp, dgam, dbet;
  float db1[4], db2, dbp;
  __device__ __forceinline__ TailBwdAcc() {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    accp = zero4; dgam = zero4; dbet = zero4; db2 = 0.f; dbp = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) { acc1[m] = zero4; acc2[m] = zero4; db1[m] = 0.f; }
  }
};
// Weight fragments depend on the lane only, not on the wave or the tile: the workgroup keeps ONE
// copy in LDS ([fragment][lane], conflict-free ds_read_b32) instead of 64 VGPRs per lane — with
// them in registers the kernel needs 316 registers (one wave per SIMD, measured 196 us per launch).
//   w1f(m, r) = W1[16m+j][4g+r]      A[i = hidden 16m+j][k <-> c 4g+r]       (H recompute)
//   w2t(m, r) = W2[4g+r][16m+j]      A[i = hidden 16m+j][k <-> co 4g+r]      (dG = W_2^T D)
//   w1t(m, r) = W1[16m+4g+r][j]      A[i = c j][k <-> hidden 16m+4g+r]       (dY = W_1^T dH)
//   b1r(m, r) = b1[16m+4g+r]
// The projection's two fragments and the per-channel vectors stay in registers.
struct TailBwdOps {
  const float* wlane;  // [TB_FRAGS fragments][64 lanes] + lane
  float wpf[4], wpt[4];
  f32x4 bpv, gam, bet;
  static __device__ __forceinline__ void fill(float* wl, const BlockArgs& a, int lane, int j, int g) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        wl[(0 + 4 * m + r) * 64 + lane] = a.w1[(16 * m + j) * C + 4 * g + r];
        wl[(16 + 4 * m + r) * 64 + lane] = a.w2[(4 * g + r) * HD + 16 * m + j];
        wl[(32 + 4 * m + r) * 64 + lane] = a.w1[(16 * m + 4 * g + r) * C + j];
        wl[(48 + 4 * m + r) * 64 + lane] = a.b1[16 * m + 4 * g + r];
      }
    }
  }
  __device__ __forceinline__ TailBwdOps(const float* wl, const BlockArgs& a, int lane, int j, int g) : wlane(wl + lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wpf[r] = a.wp[j * C + 4 * g + r];    // A[i = co j][k <-> ci 4g+r]      (x_mid recompute)
      wpt[r] = a.wp[(4 * g + r) * C + j];  // A[i = ci j][k <-> co 4g+r]      (d_o = W_p^T d x_mid)
    }
    bpv = load_vec(a.bp, g);
    gam = load_vec(a.g2, g);
    bet = load_vec(a.be2, g);
  }
  __device__ __forceinline__ float w1f(int m, int r) const { return wlane[(0 + 4 * m + r) * 64]; }
  __device__ __forceinline__ float w2t(int m, int r) const { return wlane[(16 + 4 * m + r) * 64]; }
  __device__ __forceinline__ float w1t(int m, int r) const { return wlane[(32 + 4 * m + r) * 64]; }
  __device__ __forceinline__ float b1r(int m, int r) const { return wlane[(48 + 4 * m + r) * 64]; }
};
// tail backward chain of one tile: x, o, D = d x_new in, d_o and gx out. tiles: the wave's TB_WAVE_ROWS rows of LDS. The ONE copy of
// this arithmetic, shared by tail_bwd_kernel (D loaded) and head_tail_bwd_kernel (D = the dx tile of the next block's head chain).
// The 64 hidden channels go through in four chunks of 16: h, dG, GELU, GELU', the chunk's share of dY and its dW1 / dW2 MFMAs, then
// the next chunk into the same 16-row G / dH tiles. A wave's LDS operations execute in order, so the rewrite needs no barrier (the
// fused attention backward relies on the same). dY accumulates over (m, r) ascending in either form.
__device__ __forceinline__ void tail_bwd_chain(const f32x4& xv, const f32x4& ov, const f32x4& dv, const TailBwdOps& f, float eps,
                                               float* tiles, int j, int g, TailBwdAcc& acc, f32x4& dov, f32x4& gxv) {
  // as head_bwd_chain: every fused multiply-add is written out, in the forms tail_bwd_kernel was compiled to before it shared this
  // function (here s1 sums the rounded products gy and only gy - m1 takes the unrounded one)
#pragma clang fp contract(off)
  float* tg = tiles;        // G^T      [16][TS], one hidden chunk
  float* th = tg + C * TS;  // dH^T     [16][TS], one hidden chunk
  float* ty = th + C * TS;  // LN2^T    [16][TS]
  float* tx = ty + C * TS;  // dx_mid^T [16][TS]
  float* td = tx + C * TS;  // D^T      [16][TS]
  float* to = td + C * TS;  // o^T      [16][TS]
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  lds_put_tile(td, j, g, dv);
  lds_put_tile(to, j, g, ov);

  // ---- recompute the forward: x_mid, LN2
  f32x4 xm = xv + f.bpv;
#pragma unroll
  for (int r = 0; r < 4; ++r) xm = mfma16(f.wpf[r], ov[r], xm);
  const Ln s = ln_stats(xm, eps);
  f32x4 y;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    y[r] = fmaf(s.xhat[r], f.gam[r], f.bet[r]);
    ty[(4 * g + r) * TS + j] = y[r];
  }
  // the contraction over the tile's pixels takes pixel 4g+e in K-step e
  const f32x4 yt = lds_row4(ty, j, g);   // B[k = px][c = j]
  const f32x4 dvt = lds_row4(td, j, g);  // A[i = co j][k = px]
  acc.db2 += sum4(dvt);
  // ---- per hidden chunk: H, dG = W_2^T D; G, dH = dG * gelu'(H); dY += W_1^T dH; dW2 += D^T G, dW1 += dH^T y
  f32x4 dy = zero4;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    f32x4 h = {f.b1r(m, 0), f.b1r(m, 1), f.b1r(m, 2), f.b1r(m, 3)}, dg = zero4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h = mfma16(f.w1f(m, r), y[r], h);
      dg = mfma16(f.w2t(m, r), dv[r], dg);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float hv = h[r];
      float cdf, ee;
      pg_gelu_parts(hv, cdf, ee);
      const float pdf = 0.39894228040143267794f * ee;
      const float dh = dg[r] * fmaf(hv, pdf, cdf);
      tg[(4 * g + r) * TS + j] = hv * cdf;
      th[(4 * g + r) * TS + j] = dh;
      dy = mfma16(f.w1t(m, r), dh, dy);
    }
    const f32x4 gt = lds_row4(tg, j, g);  // B[k = px][hidden 16m+j]
    const f32x4 ht = lds_row4(th, j, g);  // A[i = hidden 16m+j][k = px]
    acc.db1[m] += sum4(ht);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc.acc2[m] = mfma16(dvt[e], gt[e], acc.acc2[m]);  // dW2[co][hidden] += D[px][co] G[px][hidden]
      acc.acc1[m] = mfma16(ht[e], yt[e], acc.acc1[m]);   // dW1[hidden][c]  += dH[px][hidden] y[px][c]
    }
  }
  // ---- LN2 backward, d x_mid = D + LN2'(dY)
  f32x4 gy, dxm;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gy[r] = dy[r] * f.gam[r];
    s1 += gy[r];
    s2 = fmaf(gy[r], s.xhat[r], s2);
    acc.dgam[r] = fmaf(dy[r], s.xhat[r], acc.dgam[r]);
    acc.dbet[r] += dy[r];
  }
  const float m1 = gsum4(s1) * INV_C, m2 = gsum4(s2) * INV_C;
  dov = zero4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dxm[r] = fmaf(s.rs, fmaf(-s.xhat[r], m2, fmaf(dy[r], f.gam[r], -m1)), dv[r]);
    tx[(4 * g + r) * TS + j] = dxm[r];
    gxv[r] = dv[r] + dxm[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) dov = mfma16(f.wpt[r], dxm[r], dov);
  // ---- dWp[co][ci] += dx_mid[px][co] o[px][ci]
  const f32x4 xt = lds_row4(tx, j, g);  // A[i = co j][k = px]
  const f32x4 ot = lds_row4(to, j, g);  // B[k = px][ci = j]
  acc.dbp += sum4(xt);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc.accp = mfma16(xt[e], ot[e], acc.accp);
}
// a wave's sums -> its T_PART floats of LDS staging
__device__ __forceinline__ void tail_bwd_stage(float* mine, const TailBwdAcc& acc, int j, int g) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mine[T_W1 + (16 * m + 4 * g + r) * C + j] = acc.acc1[m][r];    // D: lane c = j, rows hidden 16m+4g+r
      mine[T_W2 + (4 * g + r) * HD + 16 * m + j] = acc.acc2[m][r];   // D: lane hidden 16m+j, rows co 4g+r
    }
    const float v = gsum4(acc.db1[m]);
    if (g == 0) mine[T_B1 + 16 * m + j] = v;
  }
  const float v2 = gsum4(acc.db2), vp = gsum4(acc.dbp);
  if (g == 0) { mine[T_B2 + j] = v2; mine[T_BP + j] = vp; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mine[T_WP + (4 * g + r) * C + j] = acc.accp[r];                  // D: lane ci = j, rows co 4g+r
    const float vg = jsum16(acc.dgam[r]), vb = jsum16(acc.dbet[r]);
    if (j == 0) { mine[T_G2 + 4 * g + r] = vg; mine[T_BE2 + 4 * g + r] = vb; }
  }
}

__global__ void __launch_bounds__(GB_THREADS) tail_bwd_kernel(const BlockArgs a) {
  extern __shared__ float4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave = blockIdx.x * (GB_THREADS / 64) + wv;
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  float* tiles = lds + (size_t)wv * TB_WAVE_ROWS * TS;
  float* wl = lds + (size_t)4 * TB_WAVE_ROWS * TS;  // [TB_FRAGS fragments][64 lanes]
  if (wv == 0) TailBwdOps::fill(wl, a, lane, j, g);
  __syncthreads();
  const TailBwdOps tf(wl, a, lane, j, g);
  TailBwdAcc acc;

  if (wave < a.total_tiles) {  // a wave without a tile loads nothing
    TileWalk tw(a, wave, nwaves);
    size_t off = tw.base(C, a.L) + j;
    f32x4 xv = load_tile(a.x + off, a.L, g);
    f32x4 ov = load_tile(a.o + off, a.L, g);
    f32x4 dv = load_tile(a.dxnew + off, a.L, g);
    wait_prologue_loads();
    for (;;) {
      // the last iteration re-reads its own tile instead of branching around the prefetch
      const TileWalk nx = tw.next();
      const bool more = nx.n < a.N;
      const size_t offn = (more ? nx : tw).base(C, a.L) + j;
      const f32x4 xn = load_tile(a.x + offn, a.L, g);
      const f32x4 on = load_tile(a.o + offn, a.L, g);
      const f32x4 dn = load_tile(a.dxnew + offn, a.L, g);
      prefetch_fence();
      f32x4 dov, gxv;
      tail_bwd_chain(xv, ov, dv, tf, a.eps, tiles, j, g, acc, dov, gxv);
      store_tile(a.d_o + off, a.L, g, dov);
      store_tile(a.gx_out + off, a.L, g, gxv);
      if (!more) break;
      xv = xn;
      ov = on;
      dv = dn;
      off = offn;
      tw = nx;
    }
  }

  // ---- one partial row per workgroup
  __syncthreads();
  tail_bwd_stage(lds + (size_t)wv * T_PART, acc, j, g);
  __syncthreads();
  write_partial_row(a.part + (size_t)blockIdx.x * T_PART, lds, T_PART);
}

// ---------------------------------------------------------------------------------- head(i+1) + tail(i), backward
// A block boundary of the backward pass in one launch: the head chain of block i+1 on x_{i+1}, gx_{i+1}, d qkv_{i+1}, then the tail
// chain of block i on x_i, o_i with the head's dx tile as D while it is still a register tile. dx (64 B per pixel written by
// head_bwd_kernel and read back by tail_bwd_kernel) never exists in memory, and the head's loads run under the tail's issue-bound
// chain. Here a.x, a.gx, a.dqkv, a.part are the head's and a.tx, a.o, a.tpart the tail's. The head's operands join the tail's
// fragments in LDS; the partial rows of the two jobs are staged in the tile space after the loop. One row per workgroup and job;
// the reduce jobs count rows by the grids of head_bwd_kernel and tail_bwd_kernel (head_rows, tail_rows >= this grid), so the
// workgroups leave the rows beyond this grid as zeros, which add nothing.
__device__ __forceinline__ void zero_rows_beyond_grid(float* __restrict__ part, int stride, int rows) {
  for (int row = blockIdx.x + gridDim.x; row < rows; row += gridDim.x)
    for (int i = threadIdx.x; i < stride; i += GB_THREADS) part[(size_t)row * stride + i] = 0.f;
}
__global__ void __launch_bounds__(GB_THREADS, 2) head_tail_bwd_kernel(const BlockArgs a) {
  extern __shared__ float4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave = blockIdx.x * (GB_THREADS / 64) + wv;
  const int nwaves = gridDim.x * (GB_THREADS / 64);
  float* tiles = lds + (size_t)wv * (TB_WAVE_ROWS + HB_WAVE_ROWS) * TS;  // the tail chain's rows, then the head chain's
  float* ty = tiles + TB_WAVE_ROWS * TS;                                  // LN1(x)^T [16 c][TS]
  float* tq = ty + C * TS;                                                // dqkv^T   [48 ch][TS]
  float* wl = lds + (size_t)4 * (TB_WAVE_ROWS + HB_WAVE_ROWS) * TS;       // [TB_FRAGS + HB_FRAGS fragments][64 lanes]
  if (wv == 0) TailBwdOps::fill(wl, a, lane, j, g);
  if (wv == 1) HeadBwdLds::fill(wl + TB_FRAGS * 64, a, lane, j, g);
  __syncthreads();
  const TailBwdOps tf(wl, a, lane, j, g);
  const HeadBwdLds hf = {wl + TB_FRAGS * 64 + lane};
  TailBwdAcc tacc;
  HeadBwdAcc hacc;

  if (wave < a.total_tiles) {  // a wave without a tile loads nothing
    TileWalk tw(a, wave, nwaves);
    size_t off = tw.base(C, a.L) + j;
    f32x4 xh = load_tile(a.x + off, a.L, g);
    f32x4 gxh = load_tile(a.gx + off, a.L, g);
    f32x4 xv = load_tile(a.tx + off, a.L, g);
    f32x4 ov = load_tile(a.o + off, a.L, g);
    wait_prologue_loads();
    for (;;) {
      // d qkv of the tile in hand goes first, so that waiting for it leaves the prefetch behind it in flight
      f32x4 dqv[3];
      {
        const float* dqp = a.dqkv + tw.base(QKV, a.L) + j;
#pragma unroll
        for (int m = 0; m < 3; ++m) dqv[m] = load_tile(dqp + (size_t)(16 * m) * a.L, a.L, g);
      }
      // the last iteration re-reads its own tile instead of branching around the prefetch
      const TileWalk nx = tw.next();
      const bool more = nx.n < a.N;
      const size_t offn = (more ? nx : tw).base(C, a.L) + j;
      const f32x4 xhn = load_tile(a.x + offn, a.L, g);
      const f32x4 gxhn = load_tile(a.gx + offn, a.L, g);
      const f32x4 xn = load_tile(a.tx + offn, a.L, g);
      const f32x4 on = load_tile(a.o + offn, a.L, g);
      prefetch_fence();
      const f32x4 dv = head_bwd_chain(xh, gxh, dqv, hf, a.eps, ty, tq, j, g, hacc);
      f32x4 dov, gxv;
      tail_bwd_chain(xv, ov, dv, tf, a.eps, tiles, j, g, tacc, dov, gxv);
      store_tile(a.d_o + off, a.L, g, dov);
      store_tile(a.gx_out + off, a.L, g, gxv);
      if (!more) break;
      xh = xhn;
      gxh = gxhn;
      xv = xn;
      ov = on;
      off = offn;
      tw = nx;
    }
  }

  // ---- one partial row per workgroup and job: the four tail rows, then the four head rows
  __syncthreads();
  float* hstage = lds + 4 * T_PART;
  tail_bwd_stage(lds + (size_t)wv * T_PART, tacc, j, g);
  head_bwd_stage(hstage + (size_t)wv * H_PART, hacc, j, g);
  __syncthreads();
  write_partial_row(a.tpart + (size_t)blockIdx.x * T_PART, lds, T_PART);
  write_partial_row(a.part + (size_t)blockIdx.x * H_PART, hstage, H_PART);
  zero_rows_beyond_grid(a.tpart, T_PART, a.tail_rows);
  zero_rows_beyond_grid(a.part, H_PART, a.head_rows);
}

// ---- second stage: the segmented reduce, the one kernel that turns rows of partial sums into gradients
// A job is a [rows x stride] matrix of partial sums, one row per workgroup of the kernel that left it, and up to 8 destination
// tensors that tile its columns: dst_k[i] += sum_rows part[row][begin_k + i]. Jobs are independent; a launch runs any mix of them.
struct SegArgs {
  const float* part; int rows, stride, nseg;
  int end[8]; float* dst[8];
};
// Up to 8 blocks (a head and a tail job each) and the model's two ends (gpt_ends.hip): the output head's rows, the stem's
// d weight / d bias rows, and the stem's d pos — the one job that is not a plain column sum: column q gathers the position-wise
// sums G[tap][q - off(tap)] of the four active taps (gpt_ends.h, region B). Job k owns workgroups first[k] .. first[k + 1] - 1,
// eight columns each.
constexpr int SEG_MAX_BLOCKS = 8;
constexpr int SEG_MAX_JOBS = 2 * SEG_MAX_BLOCKS + 3;
struct SegJobs { SegArgs j[SEG_MAX_JOBS]; int first[SEG_MAX_JOBS + 1]; int n, pos_job, H, W; };
__global__ void __launch_bounds__(256) seg_reduce_kernel(const SegJobs an) {
  __shared__ float red[32][9];
  int job = 0;
  while (job + 1 < an.n && (int)blockIdx.x >= an.first[job + 1]) ++job;
  const SegArgs& a = an.j[job];
  const int blk = blockIdx.x - an.first[job];
  const int sl = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int s = blk * 8 + sl;
  const int ncol = a.end[a.nseg - 1];  // columns this job writes
  int col[4] = {s, -1, -1, -1};
  if (job == an.pos_job && s < ncol) {
    // forward: x0[.., (r, c)] += w[.., tap] in(r + dr, c + dc), (dr, dc) = (-1,-1) (-1,0) (-1,1) (0,-1); so d pos[(r, c)]
    // takes G[tap] at (r - dr, c - dc) where that pixel exists
    const int L = an.H * an.W, r = s / an.W, c = s - r * an.W;
    col[0] = (r + 1 < an.H && c + 1 < an.W) ? 0 * L + s + an.W + 1 : -1;
    col[1] = (r + 1 < an.H) ? 1 * L + s + an.W : -1;
    col[2] = (r + 1 < an.H && c >= 1) ? 2 * L + s + an.W - 1 : -1;
    col[3] = (c + 1 < an.W) ? 3 * L + s + 1 : -1;
  }
  float a0 = 0.f, a1 = 0.f;
  if (s < ncol) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (col[k] < 0) continue;
      const float* p = a.part + col[k];
      int r = rg;
      for (; r + 32 < a.rows; r += 64) {
        a0 += p[(size_t)r * a.stride];
        a1 += p[(size_t)(r + 32) * a.stride];
      }
      if (r < a.rows) a0 += p[(size_t)r * a.stride];
    }
  }
  red[rg][sl] = a0 + a1;
  __syncthreads();
  if (rg != 0 || s >= ncol) return;
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 32; ++r) acc += red[r][sl];
  int begin = 0;
  for (int k = 0; k < a.nseg; ++k) {
    if (s < a.end[k]) { a.dst[k][s - begin] += acc; return; }
    begin = a.end[k];
  }
}

// Workgroups per launch, at least `min_tiles` tiles per wave. which: 0 head fwd, 1 head bwd, 2 tail fwd, 3 tail bwd,
// 4 tail + head fwd, 5 head + tail bwd. Resident waves per SIMD by register count (75 / 118 / 125 / 166 / 164 / 233 VGPRs):
// 6 / 4 / 4 / 3 / 3 / 2; head + tail bwd is also held at two workgroups per CU by its 71 KiB of LDS. Tail bwd fits three waves
// since its chain runs the hidden dimension in chunks, but keeps the cap of two: 768 workgroups measured 136 us against 144
// back to back, and every row it adds is read again by the reduce. Head + tail bwd at 384 / 256 workgroups leaves SIMDs idle
// (234 / 240 us against 191), at 768 / 1024 adds part of a second round (198 / 195): profiles/gpt_boundary_bwd.json,
// "grid_sweep_us_per_launch". PG_BLOCK_GRID="a,b,c,d[,e[,f]]" overrides the caps (tuning).
// A backward kernel's workgroup count is also its number of partial rows (the *_bwd_workspace_floats and the reduce jobs use it).
int grid_blocks(int which, int N, int L) {
  // immutable init-once tables (function-local static with an initialiser: thread-safe; the library
  // is entered from the main thread and from the autograd thread)
  struct Cfg { int cap[6]; int mt[2]; };
  static const Cfg cfg = []() {
    Cfg c = {{2048, 1024, 2048, 512,  // the backward caps are one full round of resident waves; the re-sweep with the pipelined
                                      // loops moved nothing beyond spread (profiles/gpt_block_pipeline.json, "grid_sweep_us_per_launch")
              1536,                   // tail + head fwd: two whole rounds like tail fwd's 2048, but of 3 waves per SIMD
                                      // (256 CUs x 4 SIMDs x 3 waves / 4 waves per workgroup = 768 workgroups per round)
              512},                   // head + tail bwd: one round of two waves per SIMD, as tail bwd
             {1, 2}};                 // tiles per wave below which the grid shrinks (forward, backward);
                                      // measured at batch 64: (4, 8) 1.82 ms/step, (2, 4) 1.59, (1, 2) 1.53, (1, 1) 1.56
    if (const char* e = PG_AB_ENV("PG_BLOCK_GRID")) {
      int v[6];
      const int got = sscanf(e, "%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
      bool ok = got >= 4;
      for (int i = 0; i < got; ++i) ok = ok && v[i] > 0;
      if (ok)
        for (int i = 0; i < got; ++i) c.cap[i] = v[i];
    }
    if (const char* e = PG_AB_ENV("PG_BLOCK_MINTILES")) {
      int f = 0, b = 0;
      if (sscanf(e, "%d,%d", &f, &b) == 2 && f > 0 && b > 0) { c.mt[0] = f; c.mt[1] = b; }
    }
    return c;
  }();
  const int* cap = cfg.cap;
  const int* mt_cfg = cfg.mt;
  const int min_tiles = (which & 1) ? mt_cfg[1] : mt_cfg[0];
  const long tiles = (long)N * (L / 16);
  long b = (tiles + 4 * min_tiles - 1) / (4 * min_tiles);
  if (b > cap[which]) b = cap[which];
  if (which == 5) {  // its rows are reduced as the rows of head bwd and tail bwd: never more workgroups than either
    if (b > cap[1]) b = cap[1];
    if (b > cap[3]) b = cap[3];
  }
  return b < 1 ? 1 : (int)b;
}

int check_shape(const char* who, int N, int Cc, int L) {
  PG_REQUIRE(N > 0 && L > 0, PG_EINVAL, "%s: non-positive dimension", who);
  PG_REQUIRE(Cc == C, PG_ESHAPE, "%s: only C = 16 is instantiated (got %d)", who, Cc);
  PG_REQUIRE(L % 16 == 0, PG_ESHAPE, "%s: L=%d is not a multiple of 16", who, L);
  return 0;
}

void set_geometry(BlockArgs& a, int N, int L, float eps) {
  a.N = N; a.L = L; a.tiles_per_img = L / 16; a.total_tiles = N * a.tiles_per_img; a.eps = eps;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

PG_EXPORT size_t pg_gpt_block_head_bwd_workspace_floats(int N, int L) {
  if (N <= 0 || L < 16) return 0;
  return (size_t)grid_blocks(1, N, L) * H_PART;
}
PG_EXPORT size_t pg_gpt_block_tail_bwd_workspace_floats(int N, int L) {
  if (N <= 0 || L < 16) return 0;
  return (size_t)grid_blocks(3, N, L) * T_PART;
}

PG_EXPORT int pg_gpt_block_head_fwd(const float* x, const float* ln_w, const float* ln_b, const float* wq,
                                    const float* bq, const float* wkv, const float* bkv, float* qkv,
                                    int N, int Cc, int L, float eps, void* stream) {
  PG_REQUIRE(x && ln_w && ln_b && wq && bq && wkv && bkv && qkv, PG_EINVAL, "pg_gpt_block_head_fwd: null pointer");
  int rc = check_shape("pg_gpt_block_head_fwd", N, Cc, L);
  if (rc) return rc;
  BlockArgs a = {};
  a.x = x; a.g1 = ln_w; a.be1 = ln_b; a.wq = wq; a.bq = bq; a.wkv = wkv; a.bkv = bkv; a.qkv = qkv;
  set_geometry(a, N, L, eps);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)grid_blocks(0, N, L)), dim3(GB_THREADS), 0, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_block_head_fwd");
  return 0;
}

namespace {
SegArgs tail_seg_args(const float* workspace, int rows, float* dw1, float* db1, float* dw2, float* db2,
                      float* dwp, float* dbp, float* dln_w, float* dln_b) {
  SegArgs r = {};
  r.part = workspace; r.rows = rows; r.stride = T_PART; r.nseg = 8;
  r.end[0] = T_B1; r.dst[0] = dw1;
  r.end[1] = T_W2; r.dst[1] = db1;
  r.end[2] = T_B2; r.dst[2] = dw2;
  r.end[3] = T_WP; r.dst[3] = db2;
  r.end[4] = T_BP; r.dst[4] = dwp;
  r.end[5] = T_G2; r.dst[5] = dbp;
  r.end[6] = T_BE2; r.dst[6] = dln_w;
  r.end[7] = T_PART; r.dst[7] = dln_b;
  return r;
}

SegArgs head_seg_args(const float* workspace, int rows, float* dln_w, float* dln_b, float* dwq, float* dbq, float* dwkv,
                      float* dbkv) {
  SegArgs r = {};
  r.part = workspace; r.rows = rows; r.stride = H_PART; r.nseg = 6;
  r.end[0] = H_WKV; r.dst[0] = dwq;
  r.end[1] = H_BQ; r.dst[1] = dwkv;
  r.end[2] = H_BKV; r.dst[2] = dbq;
  r.end[3] = H_G1; r.dst[3] = dbkv;
  r.end[4] = H_BE1; r.dst[4] = dln_w;
  r.end[5] = H_PART; r.dst[5] = dln_b;
  return r;
}

// The one way to seg_reduce_kernel: jobs[0 .. n) in ONE launch, job k on (its columns + 7) / 8 workgroups behind those of
// job k - 1. pos_job: the index of the stem's d pos job (over an H x W image), -1 without one.
int seg_reduce(const SegArgs* jobs, int n, const char* who, hipStream_t st, int pos_job = -1, int H = 0, int W = 0) {
  SegJobs an = {};
  for (int k = 0; k < n; ++k) {
    an.j[k] = jobs[k];
    an.first[k + 1] = an.first[k] + (jobs[k].end[jobs[k].nseg - 1] + 7) / 8;
  }
  an.n = n; an.pos_job = pos_job; an.H = H; an.W = W;
  hipLaunchKernelGGL(seg_reduce_kernel, dim3((unsigned)an.first[n]), dim3(256), 0, st, an);
  PG_LAUNCH_CHECK(who);
  return 0;
}

// reduce_now == false: the partial rows stay in `workspace` for pg_gpt_model_reduce; the six gradient pointers are then unused
int head_bwd_impl(const float* x, const float* ln_w, const float* ln_b, const float* wq, const float* wkv,
                  const float* dqkv, const float* gx, float* dx, float* dln_w, float* dln_b, float* dwq,
                  float* dbq, float* dwkv, float* dbkv, int N, int Cc, int L, float eps, float* workspace,
                  size_t workspace_floats, bool reduce_now, void* stream) {
  PG_REQUIRE(x && ln_w && ln_b && wq && wkv && dqkv && gx && dx && workspace &&
                 (!reduce_now || (dln_w && dln_b && dwq && dbq && dwkv && dbkv)), PG_EINVAL, "pg_gpt_block_head_bwd: null pointer");
  int rc = check_shape("pg_gpt_block_head_bwd", N, Cc, L);
  if (rc) return rc;
  PG_REQUIRE(workspace_floats >= pg_gpt_block_head_bwd_workspace_floats(N, L), PG_EINVAL,
             "pg_gpt_block_head_bwd: workspace too small");
  PG_REQUIRE(al16(dqkv), PG_EINVAL, "pg_gpt_block_head_bwd: dqkv must be 16-byte aligned");
  BlockArgs a = {};
  a.x = x; a.g1 = ln_w; a.be1 = ln_b; a.wq = wq; a.wkv = wkv; a.dqkv = dqkv; a.gx = gx; a.dx = dx;
  a.part = workspace;
  set_geometry(a, N, L, eps);
  const int blocks = grid_blocks(1, N, L);
  hipStream_t st = (hipStream_t)stream;
  const size_t tr = (size_t)4 * (C + QKV) * TS, rd = (size_t)4 * H_PART;
  hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)blocks), dim3(GB_THREADS), (tr > rd ? tr : rd) * sizeof(float), st, a);
  PG_LAUNCH_CHECK("pg_gpt_block_head_bwd");
  if (!reduce_now) return 0;
  const SegArgs r = head_seg_args(workspace, blocks, dln_w, dln_b, dwq, dbq, dwkv, dbkv);
  return seg_reduce(&r, 1, "pg_gpt_block_head_bwd(reduce)", st);
}
}  // namespace

PG_EXPORT int pg_gpt_block_head_bwd(const float* x, const float* ln_w, const float* ln_b, const float* wq,
                                    const float* wkv, const float* dqkv, const float* gx, float* dx,
                                    float* dln_w, float* dln_b, float* dwq, float* dbq, float* dwkv,
                                    float* dbkv, int N, int Cc, int L, float eps, float* workspace,
                                    size_t workspace_floats, void* stream) {
  return head_bwd_impl(x, ln_w, ln_b, wq, wkv, dqkv, gx, dx, dln_w, dln_b, dwq, dbq, dwkv, dbkv, N, Cc, L, eps,
                       workspace, workspace_floats, true, stream);
}

// the head kernel only: its rows of partial weight-gradient sums stay in `workspace` (which must stay alive) until
// pg_gpt_model_reduce adds them
PG_EXPORT int pg_gpt_block_head_bwd_partial(const float* x, const float* ln_w, const float* ln_b, const float* wq,
                                            const float* wkv, const float* dqkv, const float* gx, float* dx, int N, int Cc,
                                            int L, float eps, float* workspace, size_t workspace_floats, void* stream) {
  return head_bwd_impl(x, ln_w, ln_b, wq, wkv, dqkv, gx, dx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, Cc, L,
                       eps, workspace, workspace_floats, false, stream);
}

// ONE launch adds the partial rows of n_blocks (0..8) blocks whose head (pg_gpt_block_head_bwd_partial) and tail
// (pg_gpt_block_tail_bwd_partial) kernels left them, of the output head (out_ws: out_rows rows left by pg_gpt_out_head_bwd;
// out_grads = d ln.weight, d ln.bias, d conv.weight, d conv.bias) and of the stem (stem_ws as left by pg_gpt_stem_bwd with
// stem_rows / stem_slices of pg_gpt_stem_bwd_plan; stem_grads = d weight (16, 1, 3, 3), d bias, d pos (H x W)). grads: n_blocks x 14
// destinations, per block in the order dln1_w, dln1_b, dwq, dbq, dwkv, dbkv (head) | t_dw1, t_db1, t_dw2, t_db2, t_dwp, t_dbp,
// t_dln_w, t_dln_b (tail). A null out_ws / stem_ws leaves that end out. Everything is added to.
PG_EXPORT int pg_gpt_model_reduce(int n_blocks, const float* const* head_ws, const float* const* tail_ws, float* const* grads,
                                  int N, int Cc, int L, const float* out_ws, int out_rows, int Cout, float* const* out_grads,
                                  const float* stem_ws, int stem_rows, int stem_slices, int H, int W,
                                  float* const* stem_grads, void* stream) {
  PG_REQUIRE(n_blocks >= 0 && n_blocks <= SEG_MAX_BLOCKS, PG_ESHAPE, "pg_gpt_model_reduce: 0..8 blocks per launch, got %d", n_blocks);
  PG_REQUIRE(n_blocks == 0 || (head_ws && tail_ws && grads), PG_EINVAL, "pg_gpt_model_reduce: null pointer");
  PG_REQUIRE(n_blocks > 0 || out_ws || stem_ws, PG_EINVAL, "pg_gpt_model_reduce: nothing to reduce");
  if (n_blocks > 0)
    if (int rc = check_shape("pg_gpt_model_reduce", N, Cc, L)) return rc;
  SegArgs jobs[SEG_MAX_JOBS];
  int nj = 0, pos_job = -1;
  for (int b = 0; b < n_blocks; ++b) {
    float* const* g = grads + 14 * b;
    PG_REQUIRE(head_ws[b] && tail_ws[b], PG_EINVAL, "pg_gpt_model_reduce: null workspace of block %d", b);
    for (int k = 0; k < 14; ++k) PG_REQUIRE(g[k], PG_EINVAL, "pg_gpt_model_reduce: null gradient %d of block %d", k, b);
    jobs[nj++] = head_seg_args(head_ws[b], grid_blocks(1, N, L), g[0], g[1], g[2], g[3], g[4], g[5]);
    jobs[nj++] = tail_seg_args(tail_ws[b], grid_blocks(3, N, L), g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13]);
  }
  if (out_ws) {
    PG_REQUIRE(out_rows >= 1 && Cout >= 1 && Cout <= pg_ends::MAX_COUT && out_grads && out_grads[0] && out_grads[1] &&
                   out_grads[2] && out_grads[3], PG_EINVAL, "pg_gpt_model_reduce: bad output-head arguments");
    SegArgs r = {};
    r.part = out_ws; r.rows = out_rows; r.stride = pg_ends::out_row_floats(Cout); r.nseg = 4;
    r.end[0] = pg_ends::O_BE; r.dst[0] = out_grads[0];
    r.end[1] = pg_ends::O_W; r.dst[1] = out_grads[1];
    r.end[2] = pg_ends::O_W + Cout * pg_ends::C; r.dst[2] = out_grads[2];
    r.end[3] = r.stride; r.dst[3] = out_grads[3];
    jobs[nj++] = r;
  }
  if (stem_ws) {
    PG_REQUIRE(stem_rows >= 1 && stem_slices >= 1 && H >= 1 && W >= 1 && stem_grads && stem_grads[0] && stem_grads[1] &&
                   stem_grads[2], PG_EINVAL, "pg_gpt_model_reduce: bad stem arguments");
    SegArgs r = {};
    r.part = stem_ws; r.rows = stem_rows; r.stride = pg_ends::S_PART; r.nseg = 2;
    r.end[0] = pg_ends::S_B; r.dst[0] = stem_grads[0];
    r.end[1] = pg_ends::S_PART; r.dst[1] = stem_grads[1];
    jobs[nj++] = r;
    SegArgs q = {};  // d pos: H x W columns gathered from ACTIVE x H x W position-wise sums per slice
    q.part = stem_ws + (size_t)stem_rows * pg_ends::S_PART; q.rows = stem_slices; q.stride = pg_ends::ACTIVE * H * W; q.nseg = 1;
    q.end[0] = H * W; q.dst[0] = stem_grads[2];
    pos_job = nj;
    jobs[nj++] = q;
  }
  return seg_reduce(jobs, nj, "pg_gpt_model_reduce", (hipStream_t)stream, pos_job, H, W);
}

PG_EXPORT int pg_gpt_block_tail_fwd(const float* o, const float* x, const float* wp, const float* bp,
                                    const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* x_new, int N, int Cc, int Hd,
                                    int L, float eps, void* stream) {
  PG_REQUIRE(o && x && wp && bp && ln_w && ln_b && w1 && b1 && w2 && b2 && x_new, PG_EINVAL,
             "pg_gpt_block_tail_fwd: null pointer");
  int rc = check_shape("pg_gpt_block_tail_fwd", N, Cc, L);
  if (rc) return rc;
  PG_REQUIRE(Hd == HD, PG_ESHAPE, "pg_gpt_block_tail_fwd: only hidden = 64 is instantiated (got %d)", Hd);
  BlockArgs a = {};
  a.o = o; a.x = x; a.wp = wp; a.bp = bp; a.g2 = ln_w; a.be2 = ln_b; a.w1 = w1; a.b1 = b1; a.w2 = w2;
  a.b2 = b2; a.xnew = x_new;
  set_geometry(a, N, L, eps);
  hipLaunchKernelGGL(tail_fwd_kernel, dim3((unsigned)grid_blocks(2, N, L)), dim3(GB_THREADS), 0, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_block_tail_fwd");
  return 0;
}

// tail_fwd of block i and head_fwd of block i+1 in one launch (tail_head_fwd_kernel): writes x_new (N, 16, L) and the NEXT block's
// qkv (N, 48, L), bit for bit what pg_gpt_block_tail_fwd followed by pg_gpt_block_head_fwd(x_new, ...) write. eps serves both
// LayerNorms (the caller fuses only blocks whose ln2 / next ln1 share it).
PG_EXPORT int pg_gpt_block_tail_head_fwd(const float* o, const float* x, const float* wp, const float* bp,
                                         const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                         const float* w2, const float* b2, float* x_new, const float* next_ln_w,
                                         const float* next_ln_b, const float* next_wq, const float* next_bq,
                                         const float* next_wkv, const float* next_bkv, float* next_qkv, int N, int Cc,
                                         int Hd, int L, float eps, void* stream) {
  PG_REQUIRE(o && x && wp && bp && ln_w && ln_b && w1 && b1 && w2 && b2 && x_new && next_ln_w && next_ln_b && next_wq &&
                 next_bq && next_wkv && next_bkv && next_qkv, PG_EINVAL, "pg_gpt_block_tail_head_fwd: null pointer");
  int rc = check_shape("pg_gpt_block_tail_head_fwd", N, Cc, L);
  if (rc) return rc;
  PG_REQUIRE(Hd == HD, PG_ESHAPE, "pg_gpt_block_tail_head_fwd: only hidden = 64 is instantiated (got %d)", Hd);
  BlockArgs a = {};
  a.o = o; a.x = x; a.wp = wp; a.bp = bp; a.g2 = ln_w; a.be2 = ln_b; a.w1 = w1; a.b1 = b1; a.w2 = w2;
  a.b2 = b2; a.xnew = x_new;
  a.g1 = next_ln_w; a.be1 = next_ln_b; a.wq = next_wq; a.bq = next_bq; a.wkv = next_wkv; a.bkv = next_bkv; a.qkv = next_qkv;
  set_geometry(a, N, L, eps);
  hipLaunchKernelGGL(tail_head_fwd_kernel, dim3((unsigned)grid_blocks(4, N, L)), dim3(GB_THREADS), 0, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_block_tail_head_fwd");
  return 0;
}

namespace {
int tail_bwd_impl(const float* o, const float* x, const float* wp, const float* bp,
                                    const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                    const float* w2, const float* dx_new, float* d_o, float* gx,
                                    float* dwp, float* dbp, float* dln_w, float* dln_b, float* dw1,
                                    float* db1, float* dw2, float* db2, int N, int Cc, int Hd, int L,
                                    float eps, float* workspace, size_t workspace_floats, bool reduce_now, void* stream) {
  PG_REQUIRE(o && x && wp && bp && ln_w && ln_b && w1 && b1 && w2 && dx_new && d_o && gx && workspace &&
                 (!reduce_now || (dwp && dbp && dln_w && dln_b && dw1 && db1 && dw2 && db2)), PG_EINVAL,
             "pg_gpt_block_tail_bwd: null pointer");
  int rc = check_shape("pg_gpt_block_tail_bwd", N, Cc, L);
  if (rc) return rc;
  PG_REQUIRE(Hd == HD, PG_ESHAPE, "pg_gpt_block_tail_bwd: only hidden = 64 is instantiated (got %d)", Hd);
  PG_REQUIRE(workspace_floats >= pg_gpt_block_tail_bwd_workspace_floats(N, L), PG_EINVAL,
             "pg_gpt_block_tail_bwd: workspace too small");
  PG_REQUIRE(al16(o) && al16(dx_new), PG_EINVAL, "pg_gpt_block_tail_bwd: o / dx_new must be 16-byte aligned");
  BlockArgs a = {};
  a.o = o; a.x = x; a.wp = wp; a.bp = bp; a.g2 = ln_w; a.be2 = ln_b; a.w1 = w1; a.b1 = b1; a.w2 = w2;
  a.dxnew = dx_new; a.d_o = d_o; a.gx_out = gx; a.part = workspace;
  set_geometry(a, N, L, eps);
  const int blocks = grid_blocks(3, N, L);
  hipStream_t st = (hipStream_t)stream;
  const size_t tr = (size_t)4 * TB_WAVE_ROWS * TS + TB_FRAGS * 64, rd = (size_t)4 * T_PART;
  const size_t shmem = (tr > rd ? tr : rd) * sizeof(float);  // 46 KiB
  hipLaunchKernelGGL(tail_bwd_kernel, dim3((unsigned)blocks), dim3(GB_THREADS), shmem, st, a);
  PG_LAUNCH_CHECK("pg_gpt_block_tail_bwd");
  if (!reduce_now) return 0;
  const SegArgs r = tail_seg_args(workspace, blocks, dw1, db1, dw2, db2, dwp, dbp, dln_w, dln_b);
  return seg_reduce(&r, 1, "pg_gpt_block_tail_bwd(reduce)", st);
}
}  // namespace

PG_EXPORT int pg_gpt_block_tail_bwd(const float* o, const float* x, const float* wp, const float* bp,
                                    const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                    const float* w2, const float* dx_new, float* d_o, float* gx,
                                    float* dwp, float* dbp, float* dln_w, float* dln_b, float* dw1,
                                    float* db1, float* dw2, float* db2, int N, int Cc, int Hd, int L,
                                    float eps, float* workspace, size_t workspace_floats, void* stream) {
  return tail_bwd_impl(o, x, wp, bp, ln_w, ln_b, w1, b1, w2, dx_new, d_o, gx, dwp, dbp, dln_w, dln_b, dw1, db1, dw2,
                       db2, N, Cc, Hd, L, eps, workspace, workspace_floats, true, stream);
}

// the tail kernel only: its rows of partial weight-gradient sums stay in `workspace` (which must stay alive) until
// pg_gpt_model_reduce adds them
PG_EXPORT int pg_gpt_block_tail_bwd_partial(const float* o, const float* x, const float* wp, const float* bp,
                                            const float* ln_w, const float* ln_b, const float* w1, const float* b1,
                                            const float* w2, const float* dx_new, float* d_o, float* gx, int N,
                                            int Cc, int Hd, int L, float eps, float* workspace,
                                            size_t workspace_floats, void* stream) {
  return tail_bwd_impl(o, x, wp, bp, ln_w, ln_b, w1, b1, w2, dx_new, d_o, gx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, N, Cc, Hd, L, eps, workspace, workspace_floats, false, stream);
}

// head_bwd of block i+1 and tail_bwd of block i in one launch (head_tail_bwd_kernel). next_* are pg_gpt_block_head_bwd_partial's
// inputs of block i+1 (its dx is not written: it is the tail's dx_new and stays in registers), the rest pg_gpt_block_tail_bwd_partial's
// of block i. d_o and gx are bit for bit what the two launches write; the partial rows land in the two workspaces as those launches
// leave them for pg_gpt_model_reduce, fewer of them non-zero. eps serves both LayerNorms.
PG_EXPORT int pg_gpt_block_head_tail_bwd_partial(const float* next_x, const float* next_ln_w, const float* next_ln_b,
                                                 const float* next_wq, const float* next_wkv, const float* next_dqkv,
                                                 const float* next_gx, const float* o, const float* x, const float* wp,
                                                 const float* bp, const float* ln_w, const float* ln_b, const float* w1,
                                                 const float* b1, const float* w2, float* d_o, float* gx, int N, int Cc, int Hd,
                                                 int L, float eps, float* head_workspace, size_t head_workspace_floats,
                                                 float* tail_workspace, size_t tail_workspace_floats, void* stream) {
  PG_REQUIRE(next_x && next_ln_w && next_ln_b && next_wq && next_wkv && next_dqkv && next_gx && o && x && wp && bp && ln_w &&
                 ln_b && w1 && b1 && w2 && d_o && gx && head_workspace && tail_workspace, PG_EINVAL,
             "pg_gpt_block_head_tail_bwd_partial: null pointer");
  int rc = check_shape("pg_gpt_block_head_tail_bwd_partial", N, Cc, L);
  if (rc) return rc;
  PG_REQUIRE(Hd == HD, PG_ESHAPE, "pg_gpt_block_head_tail_bwd_partial: only hidden = 64 is instantiated (got %d)", Hd);
  PG_REQUIRE(head_workspace_floats >= pg_gpt_block_head_bwd_workspace_floats(N, L) &&
                 tail_workspace_floats >= pg_gpt_block_tail_bwd_workspace_floats(N, L), PG_EINVAL,
             "pg_gpt_block_head_tail_bwd_partial: workspace too small");
  PG_REQUIRE(al16(next_dqkv) && al16(o), PG_EINVAL, "pg_gpt_block_head_tail_bwd_partial: o / next_dqkv must be 16-byte aligned");
  BlockArgs a = {};
  a.x = next_x; a.g1 = next_ln_w; a.be1 = next_ln_b; a.wq = next_wq; a.wkv = next_wkv; a.dqkv = next_dqkv; a.gx = next_gx;
  a.part = head_workspace; a.head_rows = grid_blocks(1, N, L);
  a.o = o; a.tx = x; a.wp = wp; a.bp = bp; a.g2 = ln_w; a.be2 = ln_b; a.w1 = w1; a.b1 = b1; a.w2 = w2;
  a.d_o = d_o; a.gx_out = gx; a.tpart = tail_workspace; a.tail_rows = grid_blocks(3, N, L);
  set_geometry(a, N, L, eps);
  const size_t tr = (size_t)4 * (TB_WAVE_ROWS + HB_WAVE_ROWS) * TS + (TB_FRAGS + HB_FRAGS) * 64, rd = (size_t)4 * (T_PART + H_PART);
  const size_t shmem = (tr > rd ? tr : rd) * sizeof(float);  // 71 KiB: above the 64 KB default, two workgroups per CU (160 KB)
  static_assert(((size_t)4 * (TB_WAVE_ROWS + HB_WAVE_ROWS) * TS + (TB_FRAGS + HB_FRAGS) * 64) * sizeof(float) <= 80 * 1024 &&
                    (size_t)4 * (T_PART + H_PART) * sizeof(float) <= 80 * 1024, "two workgroups per CU");
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(head_tail_bwd_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
  (void)attr;  // thread-safe one-time opt-in
  hipLaunchKernelGGL(head_tail_bwd_kernel, dim3((unsigned)grid_blocks(5, N, L)), dim3(GB_THREADS), shmem, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_block_head_tail_bwd_partial");
  return 0;
}
