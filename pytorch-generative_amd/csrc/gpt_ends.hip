// gpt_ends.hip — the two ends of ImageGPT (models/autoregressive/image_gpt.py: forward's first and last line) as four kernels.
//
//   stem:  x0     = CausalConv2d_A_3x3(img + pos)            1 -> 16 channels, zero padding applied to the SUM
//   head:  logits = Conv1x1(LayerNorm_C(x))                  16 -> Cout channels (Cout <= 4)
//
// Through the generic operators these two lines were 18 launches that streamed a 16-channel tensor about a dozen times
// (add_bcast, mask multiply, weight packing, tap convolution, its two gradients, LayerNorm each way, 1x1 convolution each
// way, four reductions). Here every (N, 16, L) tensor is read or written once per kernel:
//   stem forward    reads img, pos                writes x0
//   head forward    reads x                       writes logits        (the normalised tensor stays in registers)
//   head backward   reads x, dlogits              writes dx            (LayerNorm statistics recomputed)
//   stem backward   reads dx0, img, pos                                (d weight for all nine taps, d bias, d pos)
// A thread owns four pixels and walks the 16 channels: consecutive lanes hold consecutive pixels, so every channel row is
// one coalesced float4 (or, where L % 4 != 0 or a pointer is not 16-byte aligned, four scalar) accesses per lane; the
// stem's backward, whose sums run over the batch at a fixed position, gives a lane one position instead (see there). The
// kernels are memory-bound; a thread issues its 16 independent row loads of a tile up front, and the stem's backward
// prefetches the next image's d x0 rows under the accumulation of the one in hand.
// Reductions are deterministic: one partial row per workgroup (layouts: gpt_ends.h), added by pg_gpt_model_reduce
// (gpt_block.hip) — together with the blocks' rows when the model queues them. No floating-point atomics.
#include "common.h"
#include "gpt_ends.h"

namespace {

using namespace pg_ends;

constexpr int THREADS = 256;
constexpr int TILE_PX = 4 * THREADS;  // pixels per tile of the head kernels and the stem forward
constexpr float INV_C = 1.f / 16.f;

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// Four pixels of one thread. VEC = 4: pixels o, o+1, o+2, o+3 of one image (one float4 per channel row);
// VEC = 1: four pixels THREADS apart, each with its own image / position and validity.
template <int VEC>
struct Px4 {
  size_t img_off[4];  // n * L + p: offset in a (N, 1, L) tensor; x (N, ch, L) offset = (img_off - p) * ch + p
  int p[4];
  bool ok[4];
  __device__ __forceinline__ Px4(long tile, long total, int L) {
    if (VEC == 4) {  // L % 4 == 0: the four pixels share the image; one division
      const long px = tile * TILE_PX + (long)threadIdx.x * 4;
      const bool in = px < total;
      const long n = in ? px / L : 0;
      const int p0 = in ? (int)(px - n * L) : 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) { ok[v] = in; p[v] = p0 + (in ? v : 0); img_off[v] = (size_t)n * L + p[v]; }
      return;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long px = tile * TILE_PX + (long)v * THREADS + threadIdx.x;
      ok[v] = px < total;
      const long n = ok[v] ? px / L : 0;
      p[v] = ok[v] ? (int)(px - n * L) : 0;
      img_off[v] = (size_t)n * L + p[v];
    }
  }
  __device__ __forceinline__ size_t off(int v, int chans, int L) const { return (img_off[v] - p[v]) * chans + p[v]; }
};

template <int VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ t, const Px4<VEC>& q, int chans, int ch, int L, float out[4]) {
  if (VEC == 4) {
    if (q.ok[0]) {
      const float4 f = *reinterpret_cast<const float4*>(t + q.off(0, chans, L) + (size_t)ch * L);
      out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = f.w;
    } else {
      out[0] = out[1] = out[2] = out[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v) out[v] = q.ok[v] ? t[q.off(v, chans, L) + (size_t)ch * L] : 0.f;
  }
}
template <int VEC>
__device__ __forceinline__ void store_row(float* __restrict__ t, const Px4<VEC>& q, int chans, int ch, int L, const float in[4]) {
  if (VEC == 4) {
    if (q.ok[0]) *reinterpret_cast<float4*>(t + q.off(0, chans, L) + (size_t)ch * L) = make_float4(in[0], in[1], in[2], in[3]);
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (q.ok[v]) t[q.off(v, chans, L) + (size_t)ch * L] = in[v];
  }
}

// ---------------------------------------------------------------------------------- stem, forward
struct StemArgs {
  const float* img; const float* pos; const float* w; const float* b; float* wmut; float* x0;
  const float* dx0; float* part;
  int N, H, W, L;
  long total; int tiles;                                   // forward
  int nchunks, chunk_px, slices, btiles;                   // backward
};

// in(n, r + dr, c + dc) of the padded sum img + pos; the type A taps are (dr, dc) = (-1,-1) (-1,0) (-1,1) (0,-1),
// weight[c][0][kh][kw] with kh*3 + kw = 0..3
__device__ __forceinline__ float stem_in(const StemArgs& a, size_t img_base, int r, int c) {
  if (r < 0 || r >= a.H || c < 0 || c >= a.W) return 0.f;
  const int o = r * a.W + c;
  return a.img[img_base + o] + a.pos[o];
}

template <int VEC>
__global__ void __launch_bounds__(THREADS) stem_fwd_kernel(const StemArgs a) {
  float w[C][ACTIVE], bb[C];  // wave-uniform: scalar registers
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    bb[ch] = a.b[ch];
#pragma unroll
    for (int t = 0; t < ACTIVE; ++t) w[ch][t] = a.w[ch * TAPS + t];
  }
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const Px4<VEC> q(tile, a.total, a.L);
    float in[ACTIVE][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = q.p[v] / a.W, c = q.p[v] - r * a.W;
      const size_t base = q.img_off[v] - q.p[v];
      in[0][v] = q.ok[v] ? stem_in(a, base, r - 1, c - 1) : 0.f;
      in[1][v] = q.ok[v] ? stem_in(a, base, r - 1, c) : 0.f;
      in[2][v] = q.ok[v] ? stem_in(a, base, r - 1, c + 1) : 0.f;
      in[3][v] = q.ok[v] ? stem_in(a, base, r, c - 1) : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      float out[4];
#pragma unroll
      for (int v = 0; v < 4; ++v)
        out[v] = fmaf(w[ch][3], in[3][v], fmaf(w[ch][2], in[2][v], fmaf(w[ch][1], in[1][v], fmaf(w[ch][0], in[0][v], bb[ch]))));
      store_row<VEC>(a.x0, q, C, ch, a.L, out);
    }
  }
  // nn/convolution.py:42 of the reference: the masked entries of the weight are zeroed in place on every forward.
  // Nothing here reads them (taps 4..8 of each output channel); the store comes last so that the weights above are
  // loaded through the scalar cache, ahead of any store of the kernel.
  if (blockIdx.x == 0 && threadIdx.x < C * (TAPS - ACTIVE))
    a.wmut[(threadIdx.x / (TAPS - ACTIVE)) * TAPS + ACTIVE + threadIdx.x % (TAPS - ACTIVE)] = 0.f;
}

// ---------------------------------------------------------------------------------- stem, backward
// Tile = (chunk of <= 128 pixel positions, slice of the images n = s, s + slices, ...). A lane owns ONE position of the
// chunk and 8 of the 16 channels (waves 0 / 1: channels 0..7 / 8..15 of positions 0..63, waves 2 / 3: of positions
// 64..127), so a row of d x0 is one coalesced dword load per wave and the 3 x 3 neighbourhood of the image is read once
// per 8 channels. in = img + pos and every sum is linear, so over the images of a slice a lane accumulates only
//   D[c] = sum_n d[n][c][p]   and   aw[c][t] = sum_n d[n][c][p] img[n][p + off(t)];
// pos (aw[c][t] += D[c] pos[p + off(t)]), d bias (sum of D) and G[t][p] = sum_c w[c][t] D[c] follow once per tile.
// d weight / d bias stay in registers over all tiles of the workgroup.
constexpr int SB_PX = 128, SB_CH = 8;
__global__ void __launch_bounds__(THREADS) stem_bwd_kernel(const StemArgs a) {
  __shared__ float gs[2][ACTIVE][SB_PX];
  __shared__ float red[4][SB_CH * (TAPS + 1)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cg = wv & 1, q = (wv >> 1) * 64 + lane;  // channel group, position within the chunk
  const int L = a.L;
  float aw[SB_CH][TAPS], ab[SB_CH];
#pragma unroll
  for (int cc = 0; cc < SB_CH; ++cc) {
    ab[cc] = 0.f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) aw[cc][t] = 0.f;
  }
  float* part_b = a.part + (size_t)gridDim.x * S_PART;
  for (int tile = blockIdx.x; tile < a.btiles; tile += gridDim.x) {
    const int k = tile % a.nchunks, s = tile / a.nchunks;
    const int start = k * a.chunk_px;
    const int p = start + q;
    const bool ok = q < a.chunk_px && p < L;
    const int r = p / a.W, c = p - r * a.W;
    // tap t: offset in an (H, W) plane — the pixel itself where the tap is outside the image, so never out of bounds
    int off[TAPS];
    bool valid[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int rr = r + t / 3 - 1, cc = c + t % 3 - 1;
      valid[t] = ok && rr >= 0 && rr < a.H && cc >= 0 && cc < a.W;
      off[t] = valid[t] ? rr * a.W + cc : (ok ? p : 0);
    }
    const float* dbase = a.dx0 + (size_t)(SB_CH * cg) * L + (ok ? p : 0);
    auto load_d = [&](int n, float d[SB_CH]) {
      const float* b = dbase + (size_t)n * C * L;
#pragma unroll
      for (int cc = 0; cc < SB_CH; ++cc) d[cc] = ok ? b[(size_t)cc * L] : 0.f;
    };
    float D[SB_CH], d[SB_CH], dn[SB_CH];
#pragma unroll
    for (int cc = 0; cc < SB_CH; ++cc) D[cc] = 0.f;
    load_d(s, d);  // s < slices <= N
    for (int n = s; n < a.N; n += a.slices) {
      const int nn = n + a.slices;
      load_d(nn < a.N ? nn : n, dn);  // the last image of the slice re-reads its own rows instead of branching
      const float* im = a.img + (size_t)n * L;
      float in[TAPS];
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const float x = im[off[t]];
        in[t] = valid[t] ? x : 0.f;
      }
#pragma unroll
      for (int cc = 0; cc < SB_CH; ++cc) {
        D[cc] += d[cc];  // 0 for a lane without a pixel
#pragma unroll
        for (int t = 0; t < TAPS; ++t) aw[cc][t] = fmaf(d[cc], in[t], aw[cc][t]);
        d[cc] = dn[cc];
      }
    }
    float G[ACTIVE] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const float x = a.pos[off[t]];
      const float pv = valid[t] ? x : 0.f;
#pragma unroll
      for (int cc = 0; cc < SB_CH; ++cc) aw[cc][t] = fmaf(D[cc], pv, aw[cc][t]);
    }
#pragma unroll
    for (int cc = 0; cc < SB_CH; ++cc) {
      ab[cc] += D[cc];
#pragma unroll
      for (int t = 0; t < ACTIVE; ++t) G[t] = fmaf(a.w[(SB_CH * cg + cc) * TAPS + t], D[cc], G[t]);
    }
    // G of the two channel groups -> row s of region B
#pragma unroll
    for (int t = 0; t < ACTIVE; ++t) gs[cg][t][q] = G[t];
    __syncthreads();
    for (int i = threadIdx.x; i < ACTIVE * SB_PX; i += THREADS) {
      const int t = i / SB_PX, qq = i % SB_PX;
      if (qq < a.chunk_px && start + qq < L) part_b[((size_t)s * ACTIVE + t) * L + start + qq] = gs[0][t][qq] + gs[1][t][qq];
    }
    __syncthreads();
  }
  // one row of region A per workgroup: waves w and w + 2 hold the same channels of the two halves of the chunk
#pragma unroll
  for (int cc = 0; cc < SB_CH; ++cc) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const float v = wave_sum(aw[cc][t]);
      if (lane == 0) red[wv][cc * TAPS + t] = v;
    }
    const float v = wave_sum(ab[cc]);
    if (lane == 0) red[wv][SB_CH * TAPS + cc] = v;
  }
  __syncthreads();
  float* row = a.part + (size_t)blockIdx.x * S_PART;
  if (threadIdx.x < 2 * SB_CH * (TAPS + 1)) {
    const int g = threadIdx.x / (SB_CH * (TAPS + 1)), j = threadIdx.x % (SB_CH * (TAPS + 1));
    const float v = red[g][j] + red[g + 2][j];
    if (j < SB_CH * TAPS) row[S_W + SB_CH * TAPS * g + j] = v;
    else row[S_B + SB_CH * g + (j - SB_CH * TAPS)] = v;
  }
}

// ---------------------------------------------------------------------------------- output head
struct OutArgs {
  const float* x; const float* g; const float* be; const float* cw; const float* cb; float* logits;
  const float* dl; float* dx; float* part;
  int N, L; long total; int tiles; float eps;
};

// LayerNorm statistics as ln_stats of gpt_block.hip: biased variance, eps inside the root, one Newton step on v_rsq_f32.
// x[c] becomes xhat[c]; returns rs.
__device__ __forceinline__ float ln_normalise(float x[C], float eps) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) s += x[c];
  const float mu = s * INV_C;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { x[c] -= mu; q = fmaf(x[c], x[c], q); }
  const float var = q * INV_C + eps;
  float rs = rsqrtf(var);
  rs = rs * (1.5f - 0.5f * var * rs * rs);
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] *= rs;
  return rs;
}

template <int VEC, int COUT>
__global__ void __launch_bounds__(THREADS) out_fwd_kernel(const OutArgs a) {
  float g[C], be[C], cw[COUT][C];  // wave-uniform: scalar registers
#pragma unroll
  for (int c = 0; c < C; ++c) {
    g[c] = a.g[c]; be[c] = a.be[c];
#pragma unroll
    for (int co = 0; co < COUT; ++co) cw[co][c] = a.cw[co * C + c];
  }
  float cb[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) cb[co] = a.cb[co];
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const Px4<VEC> q(tile, a.total, a.L);
    float x[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) load_row<VEC>(a.x, q, C, c, a.L, x[c]);
    float out[COUT][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float xv[C];
#pragma unroll
      for (int c = 0; c < C; ++c) xv[c] = x[c][v];
      ln_normalise(xv, a.eps);
#pragma unroll
      for (int c = 0; c < C; ++c) xv[c] = fmaf(xv[c], g[c], be[c]);
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        float o = cb[co];
#pragma unroll
        for (int c = 0; c < C; ++c) o = fmaf(cw[co][c], xv[c], o);
        out[co][v] = o;
      }
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) store_row<VEC>(a.logits, q, COUT, co, a.L, out[co]);
  }
}

// dx = LN'(W^T dlogits). The four parameter gradients all follow from S[co][c] = sum_px dl[co] xhat[c] and
// T[co] = sum_px dl[co]:  d gamma[c] = sum_co w[co][c] S[co][c],  d beta[c] = sum_co w[co][c] T[co],
// d w[co][c] = gamma[c] S[co][c] + beta[c] T[co],  d b[co] = T[co]  — 17 Cout accumulators per thread.
template <int VEC, int COUT>
__global__ void __launch_bounds__(THREADS) out_bwd_kernel(const OutArgs a) {
  __shared__ float red[4][COUT * (C + 1)];
  float g[C], be[C], cw[COUT][C];  // wave-uniform: scalar registers
#pragma unroll
  for (int c = 0; c < C; ++c) {
    g[c] = a.g[c]; be[c] = a.be[c];
#pragma unroll
    for (int co = 0; co < COUT; ++co) cw[co][c] = a.cw[co * C + c];
  }
  float S[COUT][C], T[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    T[co] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) S[co][c] = 0.f;
  }
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const Px4<VEC> q(tile, a.total, a.L);
    float x[C][4], dl[COUT][4];
#pragma unroll
    for (int c = 0; c < C; ++c) load_row<VEC>(a.x, q, C, c, a.L, x[c]);
#pragma unroll
    for (int co = 0; co < COUT; ++co) load_row<VEC>(a.dl, q, COUT, co, a.L, dl[co]);  // 0 for a lane without a pixel
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float xh[C], dxh[C];
#pragma unroll
      for (int c = 0; c < C; ++c) xh[c] = x[c][v];
      const float rs = ln_normalise(xh, a.eps);
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float dy = 0.f;
#pragma unroll
        for (int co = 0; co < COUT; ++co) dy = fmaf(cw[co][c], dl[co][v], dy);
        dxh[c] = dy * g[c];
        m1 += dxh[c];
        m2 = fmaf(dxh[c], xh[c], m2);
      }
      m1 *= INV_C; m2 *= INV_C;
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        T[co] += dl[co][v];
#pragma unroll
        for (int c = 0; c < C; ++c) S[co][c] = fmaf(dl[co][v], xh[c], S[co][c]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) x[c][v] = rs * (dxh[c] - m1 - xh[c] * m2);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) store_row<VEC>(a.dx, q, C, c, a.L, x[c]);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = wave_sum(S[co][c]);
      if (lane == 0) red[wv][co * (C + 1) + c] = v;
    }
    const float v = wave_sum(T[co]);
    if (lane == 0) red[wv][co * (C + 1) + C] = v;
  }
  __syncthreads();
  float* row = a.part + (size_t)blockIdx.x * out_row_floats(COUT);
  auto tot = [&](int i) { return (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]); };
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    float dg = 0.f, db = 0.f;
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const float s = tot(co * (C + 1) + c), t = tot(co * (C + 1) + C), w = a.cw[co * C + c];
      dg = fmaf(w, s, dg);
      db = fmaf(w, t, db);
      row[O_W + co * C + c] = fmaf(a.g[c], s, a.be[c] * t);
    }
    row[O_G + c] = dg;
    row[O_BE + c] = db;
  } else if (threadIdx.x < C + COUT) {
    const int co = threadIdx.x - C;
    row[O_W + COUT * C + co] = tot(co * (C + 1) + C);
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int tile_grid(long total_px, int grid_cap, int* tiles) {
  const long t = (total_px + TILE_PX - 1) / TILE_PX;
  *tiles = (int)t;
  const long cap = grid_cap > 0 ? grid_cap : 2048;
  return (int)(t < cap ? t : cap);
}

struct StemPlan { int nchunks, chunk_px, slices, tiles, grid; };
StemPlan stem_plan(int N, int L, int grid_cap) {
  StemPlan p;
  p.nchunks = (L + SB_PX - 1) / SB_PX;
  p.chunk_px = (L + p.nchunks - 1) / p.nchunks;  // balanced chunks
  int s = 512 / p.nchunks;  // about two workgroups per CU
  if (s < 1) s = 1;
  p.slices = N < s ? N : s;
  p.tiles = p.nchunks * p.slices;
  const int cap = grid_cap > 0 ? grid_cap : 1024;
  p.grid = p.tiles < cap ? p.tiles : cap;
  return p;
}

int check_dims(const char* who, int N, long L) {
  PG_REQUIRE(N > 0 && L > 0, PG_EINVAL, "%s: non-positive dimension", who);
  PG_REQUIRE((long)N * L * C < (1L << 40) && L < (1L << 30), PG_ESHAPE, "%s: tensor too large", who);
  return 0;
}

}  // namespace

// ---- stem
PG_EXPORT int pg_gpt_stem_fwd(const float* img, const float* pos, float* weight, const float* bias, float* x0, int N,
                              int H, int W, int grid_cap, void* stream) {
  PG_REQUIRE(img && pos && weight && bias && x0, PG_EINVAL, "pg_gpt_stem_fwd: null pointer");
  PG_REQUIRE(H > 0 && W > 0 && grid_cap >= 0, PG_EINVAL, "pg_gpt_stem_fwd: bad argument");
  const long L = (long)H * W;
  if (int rc = check_dims("pg_gpt_stem_fwd", N, L)) return rc;
  StemArgs a = {};
  a.img = img; a.pos = pos; a.w = weight; a.wmut = weight; a.b = bias; a.x0 = x0;
  a.N = N; a.H = H; a.W = W; a.L = (int)L; a.total = (long)N * L;
  const int grid = tile_grid(a.total, grid_cap, &a.tiles);
  if (L % 4 == 0 && al16(x0))
    hipLaunchKernelGGL(stem_fwd_kernel<4>, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(stem_fwd_kernel<1>, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_stem_fwd");
  return 0;
}

PG_EXPORT int pg_gpt_stem_bwd_plan(int N, int H, int W, int grid_cap, int* rows, int* slices) {
  PG_REQUIRE(N > 0 && H > 0 && W > 0 && grid_cap >= 0 && rows && slices, PG_EINVAL, "pg_gpt_stem_bwd_plan: bad argument");
  const StemPlan p = stem_plan(N, H * W, grid_cap);
  *rows = p.grid; *slices = p.slices;
  return 0;
}
PG_EXPORT size_t pg_gpt_stem_bwd_workspace_floats(int N, int H, int W, int grid_cap) {
  if (N <= 0 || H <= 0 || W <= 0 || grid_cap < 0) return 0;
  const StemPlan p = stem_plan(N, H * W, grid_cap);
  return (size_t)stem_workspace_floats(p.grid, p.slices, H * W);
}

PG_EXPORT int pg_gpt_stem_bwd(const float* dx0, const float* img, const float* pos, const float* weight, int N, int H,
                              int W, int grid_cap, float* workspace, size_t workspace_floats, void* stream) {
  PG_REQUIRE(dx0 && img && pos && weight && workspace, PG_EINVAL, "pg_gpt_stem_bwd: null pointer");
  PG_REQUIRE(H > 0 && W > 0 && grid_cap >= 0, PG_EINVAL, "pg_gpt_stem_bwd: bad argument");
  const long L = (long)H * W;
  if (int rc = check_dims("pg_gpt_stem_bwd", N, L)) return rc;
  PG_REQUIRE(workspace_floats >= pg_gpt_stem_bwd_workspace_floats(N, H, W, grid_cap), PG_EINVAL,
             "pg_gpt_stem_bwd: workspace too small");
  const StemPlan p = stem_plan(N, (int)L, grid_cap);
  StemArgs a = {};
  a.dx0 = dx0; a.img = img; a.pos = pos; a.w = weight; a.part = workspace;
  a.N = N; a.H = H; a.W = W; a.L = (int)L;
  a.nchunks = p.nchunks; a.chunk_px = p.chunk_px; a.slices = p.slices; a.btiles = p.tiles;
  hipLaunchKernelGGL(stem_bwd_kernel, dim3((unsigned)p.grid), dim3(THREADS), 0, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_stem_bwd");
  return 0;
}

// ---- output head
namespace {
template <int VEC>
int launch_out(bool bwd, int cout, int grid, hipStream_t st, const OutArgs& a) {
#define PG_OUT_CASE(K)                                                                                   \
  case K:                                                                                                \
    if (bwd) hipLaunchKernelGGL((out_bwd_kernel<VEC, K>), dim3((unsigned)grid), dim3(THREADS), 0, st, a); \
    else hipLaunchKernelGGL((out_fwd_kernel<VEC, K>), dim3((unsigned)grid), dim3(THREADS), 0, st, a);     \
    return 0;
  switch (cout) {
    PG_OUT_CASE(1) PG_OUT_CASE(2) PG_OUT_CASE(3) PG_OUT_CASE(4)
  }
#undef PG_OUT_CASE
  return PG_ESHAPE;
}
}  // namespace

PG_EXPORT int pg_gpt_out_head_fwd(const float* x, const float* ln_w, const float* ln_b, const float* conv_w,
                                  const float* conv_b, float* logits, int N, int Cc, int Cout, int L, float eps,
                                  int grid_cap, void* stream) {
  PG_REQUIRE(x && ln_w && ln_b && conv_w && conv_b && logits && grid_cap >= 0, PG_EINVAL, "pg_gpt_out_head_fwd: bad argument");
  PG_REQUIRE(Cc == C, PG_ESHAPE, "pg_gpt_out_head_fwd: only C = 16 is instantiated (got %d)", Cc);
  PG_REQUIRE(Cout >= 1 && Cout <= MAX_COUT, PG_ESHAPE, "pg_gpt_out_head_fwd: 1..%d output channels (got %d)", MAX_COUT, Cout);
  if (int rc = check_dims("pg_gpt_out_head_fwd", N, L)) return rc;
  OutArgs a = {};
  a.x = x; a.g = ln_w; a.be = ln_b; a.cw = conv_w; a.cb = conv_b; a.logits = logits;
  a.N = N; a.L = L; a.total = (long)N * L; a.eps = eps;
  const int grid = tile_grid(a.total, grid_cap, &a.tiles);
  if (L % 4 == 0 && al16(x) && al16(logits)) launch_out<4>(false, Cout, grid, (hipStream_t)stream, a);
  else launch_out<1>(false, Cout, grid, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_out_head_fwd");
  return 0;
}

PG_EXPORT int pg_gpt_out_head_bwd_rows(int N, int L, int grid_cap) {
  if (N <= 0 || L <= 0 || grid_cap < 0) return 0;
  int tiles;
  return tile_grid((long)N * L, grid_cap, &tiles);
}

// dx and one partial row per workgroup (pg_gpt_out_head_bwd_rows of them, out_row_floats(Cout) = 32 + 17 Cout floats each)
PG_EXPORT int pg_gpt_out_head_bwd(const float* x, const float* ln_w, const float* ln_b, const float* conv_w,
                                  const float* dlogits, float* dx, int N, int Cc, int Cout, int L, float eps, int grid_cap,
                                  float* workspace, size_t workspace_floats, void* stream) {
  PG_REQUIRE(x && ln_w && ln_b && conv_w && dlogits && dx && workspace && grid_cap >= 0, PG_EINVAL,
             "pg_gpt_out_head_bwd: bad argument");
  PG_REQUIRE(Cc == C, PG_ESHAPE, "pg_gpt_out_head_bwd: only C = 16 is instantiated (got %d)", Cc);
  PG_REQUIRE(Cout >= 1 && Cout <= MAX_COUT, PG_ESHAPE, "pg_gpt_out_head_bwd: 1..%d output channels (got %d)", MAX_COUT, Cout);
  if (int rc = check_dims("pg_gpt_out_head_bwd", N, L)) return rc;
  OutArgs a = {};
  a.x = x; a.g = ln_w; a.be = ln_b; a.cw = conv_w; a.dl = dlogits; a.dx = dx; a.part = workspace;
  a.N = N; a.L = L; a.total = (long)N * L; a.eps = eps;
  const int grid = tile_grid(a.total, grid_cap, &a.tiles);
  PG_REQUIRE(workspace_floats >= (size_t)grid * out_row_floats(Cout), PG_EINVAL, "pg_gpt_out_head_bwd: workspace too small");
  if (L % 4 == 0 && al16(x) && al16(dlogits) && al16(dx)) launch_out<4>(true, Cout, grid, (hipStream_t)stream, a);
  else launch_out<1>(true, Cout, grid, (hipStream_t)stream, a);
  PG_LAUNCH_CHECK("pg_gpt_out_head_bwd");
  return 0;
}
