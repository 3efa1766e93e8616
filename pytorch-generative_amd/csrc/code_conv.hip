// code_conv.hip — a masked convolution whose input is an image of code indices (a one-hot convolution is a table lookup):
//   out[n, :, y, x] = b + sum over taps of W[:, code(n, y + u - ph, x + v - pw), u, v]
// and its weight / bias gradient, for autoregressive priors over VQ-VAE codes (ImageGPT, PixelCNN with `input_codes`).
// The input is a LEVEL image (N, 1, H, W) at the levels j / (K - 1) (csrc/categorical.h: cat_class); a negative level is
// an undrawn canvas position and stands for the all-zero one-hot vector. Nothing of the size N K H W is formed.
//   pg_code_conv_fwd:       pack the admitted taps into a (taps, K, Cout) table, gather contiguous Cout rows
//   pg_code_conv_wgrad:     store-and-sum: inverted index (per code the ascending list of its positions, a stable counting
//                           sort on integer counters), one wave sums one (list chunk, channel group), chunks added in order
//   pg_sample_embed_codes:  one raster position of the stem for the incremental sampler
//   pg_vq_lookup:           codebook rows by code image (the VQ-VAE decoder's input)
#include "code_index.h"

namespace {

constexpr int CC_POS = 64;        // output positions per workgroup of the forward
constexpr int CC_THREADS = 256;
constexpr int CC_ACC = 8;         // accumulators (output channels) per lane of the sum kernel

// table[(tp * K + k) * Cout + co] = w[co][k][u][v] for the tp-th set bit g = u * KW + v of `mask`
__global__ void code_pack_kernel(const float* __restrict__ w, float* __restrict__ table, int Cout, int K, int KH, int KW,
                                 unsigned long long mask, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int co = (int)(e % Cout);
  const long r = e / Cout;
  const int k = (int)(r % K);
  int tp = (int)(r / K);
  int g = 0;
  for (int i = 0; i < KH * KW; ++i) {  // the tp-th admitted tap
    if ((mask >> i) & 1ull) {
      if (tp == 0) {
        g = i;
        break;
      }
      --tp;
    }
  }
  table[e] = w[((size_t)co * K + k) * (size_t)(KH * KW) + g];
}

// One workgroup: CC_POS consecutive output positions (of the sequence (n OH + y) OW + x) x all output channels.
// Phase 1 turns the levels under every tap into codes in LDS; phase 2 gathers with the lanes along the channels (contiguous
// table rows) into a transposing LDS tile, which is written with the lanes along the positions (contiguous NCHW planes).
__global__ void __launch_bounds__(CC_THREADS) code_conv_fwd_kernel(
    const float* __restrict__ levels, const float* __restrict__ table, const float* __restrict__ bias,
    float* __restrict__ out, int N, int K, int Hin, int Win, int Cout, int KH, int KW, int OH, int OW, int ph, int pw,
    unsigned long long mask, long P) {
  __shared__ short codes[PG_MAX_TAPS][CC_POS];
  __shared__ float tile[64][CC_POS + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = (long)blockIdx.x * CC_POS;
  const int T = KH * KW;
  const int OHW = OH * OW;
  for (int i = tid; i < T * CC_POS; i += CC_THREADS) {
    const int g = i / CC_POS, pl = i - g * CC_POS;
    const long p = p0 + pl;
    int code = -1;
    if (p < P && ((mask >> g) & 1ull)) {
      const int n = (int)(p / OHW);
      const int rem = (int)(p - (long)n * OHW);
      const int y = rem / OW, x = rem - y * OW;
      const int u = g / KW, v = g - u * KW;
      const int iy = y + u - ph, ix = x + v - pw;
      if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win)
        code = code_of(levels[((size_t)n * Hin + iy) * Win + ix], K);
    }
    codes[g][pl] = (short)code;
  }
  __syncthreads();
  for (int c0 = 0; c0 < Cout; c0 += 64) {
    const int co = c0 + lane;
    const bool cok = co < Cout;
    const float b = (cok && bias) ? bias[co] : 0.f;
    const float* trow = table + (cok ? co : 0);
    for (int pp = wave * 4; pp < CC_POS; pp += (CC_THREADS / 64) * 4) {
      float acc[4] = {b, b, b, b};  // bias first, then the admitted taps in ascending order
      int tp = 0;
      for (int g = 0; g < T; ++g) {
        if (!((mask >> g) & 1ull)) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = codes[g][pp + j];
          if (k >= 0 && cok) acc[j] += trow[((size_t)tp * K + k) * Cout];
        }
        ++tp;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[lane][pp + j] = acc[j];
    }
    __syncthreads();
    for (int i = tid; i < 64 * CC_POS; i += CC_THREADS) {
      const int cl = i / CC_POS, pl = i - cl * CC_POS;
      const long p = p0 + pl;
      if (c0 + cl < Cout && p < P) {
        const long n = p / OHW;
        const long rem = p - n * OHW;
        out[((size_t)n * Cout + (c0 + cl)) * OHW + rem] = tile[cl][pl];
      }
    }
    __syncthreads();
  }
}

// ---- weight gradient: the inverted index is built by code_index.h -----------------------------------------------------
// One wave: one work item (a chunk of at most CC_CHUNK entries of one code's list) x one group of output channels.
// lane = (channel sub-index, tap): a list entry's KH x KW window of dY is read once per channel; CC_ACC channels per lane.
// part[(item * Cout + co) * T + tap] = the chunk's sum in list order.
__global__ void __launch_bounds__(64) code_sum_kernel(const float* __restrict__ dy, const int* __restrict__ total,
                                                      const int* __restrict__ start, const int* __restrict__ cstart,
                                                      const int* __restrict__ list, float* __restrict__ part, int K,
                                                      int Hin, int Win, int Cout, int KH, int KW, int OH, int OW, int ph,
                                                      int pw, int P) {
  const int item = blockIdx.x;
  if (item >= cstart[K]) return;
  int lo = 0, hi = K;  // the code k with cstart[k] <= item < cstart[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= item) lo = mid;
    else hi = mid;
  }
  const int k = lo;
  const int j = item - cstart[k];
  const int len = total[k];
  const int i0 = j * CC_CHUNK;
  const int i1 = i0 + CC_CHUNK < len ? i0 + CC_CHUNK : len;
  const int* lp = list + start[k];
  const int lane = threadIdx.x;
  const int T = KH * KW;
  const int cpl = 64 / T;  // channels per pass
  const int tap = lane % T, cs = lane / T;
  const int u = tap / KW, v = tap - u * KW;
  const bool active = cs < cpl;
  const int co0 = blockIdx.y * (cpl * CC_ACC) + cs;
  const int HW = Hin * Win;
  const size_t OHW = (size_t)OH * OW;
  float acc[CC_ACC];
#pragma unroll
  for (int a = 0; a < CC_ACC; ++a) acc[a] = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int q = lp[i];
    if ((unsigned)q >= (unsigned)P) continue;  // (never taken: the lists hold positions; keeps every read inside dY)
    const int n = q / HW;
    const int rem = q - n * HW;
    const int iy = rem / Win, ix = rem - iy * Win;
    const int y = iy + ph - u, x = ix + pw - v;
    const bool ok = active && y >= 0 && y < OH && x >= 0 && x < OW;
    const float* src = dy + (size_t)n * Cout * OHW + (size_t)(ok ? y * OW + x : 0);
#pragma unroll
    for (int a = 0; a < CC_ACC; ++a) {
      const int co = co0 + a * cpl;
      if (ok && co < Cout) acc[a] += src[(size_t)co * OHW];
    }
  }
#pragma unroll
  for (int a = 0; a < CC_ACC; ++a) {
    const int co = co0 + a * cpl;
    if (active && co < Cout) part[((size_t)item * Cout + co) * T + tap] = acc[a];
  }
}

// dW[co][k][tap] (+)= the chunks of code k in chunk order; a code without a chunk receives an exact zero.
__global__ void code_merge_kernel(const float* __restrict__ part, const int* __restrict__ cstart, float* __restrict__ dw,
                                  int K, int Cout, int T, int accumulate, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int tap = (int)(e % T);
  const long r = e / T;
  const int k = (int)(r % K);
  const int co = (int)(r / K);
  float s = 0.f;
  for (int it = cstart[k]; it < cstart[k + 1]; ++it) s += part[((size_t)it * Cout + co) * T + tap];
  dw[e] = accumulate ? dw[e] + s : s;
}

// db[co] (+)= sum of dY[:, co, :, :]: one workgroup per channel, a fixed strided order and a fixed tree.
__global__ void __launch_bounds__(CC_THREADS) code_bias_grad_kernel(const float* __restrict__ dy, float* __restrict__ db,
                                                                    int Cout, long OHW, long total, int accumulate) {
  __shared__ float red[CC_THREADS];
  const int co = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (long i = tid; i < total; i += CC_THREADS) {
    const long n = i / OHW;
    s += dy[((size_t)n * Cout + co) * OHW + (i - n * OHW)];
  }
  red[tid] = s;
  __syncthreads();
  for (int off = CC_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) db[co] = accumulate ? db[co] + red[0] : red[0];
}

// out[co * ld + n] = b[co] + pos_term[co][r][c] + sum_{u,v} w[co][code(n, r + u - KH/2, c + v - KW/2)][u][v]
// (the weight is already masked in place, so every tap is read: a masked tap adds zero)
__global__ void sample_embed_codes_kernel(const float* __restrict__ canvas, const float* __restrict__ w,
                                          const float* __restrict__ b, const float* __restrict__ pos_term,
                                          float* __restrict__ out, int N, int K, int H, int W, int Cout, int KH, int KW,
                                          int r, int c, int ld, const int* __restrict__ pos_dev) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int co = blockIdx.y;
  if (n >= N) return;
  if (pos_dev) {
    const int p = min(max(*pos_dev, 0), H * W - 1);
    r = p / W;
    c = p - r * W;
  }
  float acc = b ? b[co] : 0.f;
  for (int u = 0; u < KH; ++u) {
    const int rr = r + u - KH / 2;
    if (rr < 0 || rr >= H) continue;
    for (int v = 0; v < KW; ++v) {
      const int cc = c + v - KW / 2;
      if (cc < 0 || cc >= W) continue;
      const int k = code_of(canvas[((size_t)n * H + rr) * W + cc], K);
      if (k >= 0) acc += w[(((size_t)co * K + k) * KH + u) * KW + v];
    }
  }
  if (pos_term) acc += pos_term[((size_t)co * H + r) * W + c];
  out[(size_t)co * ld + n] = acc;
}

// out[n][d][l] = embedding[code(n, l)][d] (a negative level reads code 0, as cat_class clamps it)
__global__ void vq_lookup_kernel(const float* __restrict__ levels, const float* __restrict__ emb, float* __restrict__ out,
                                 int D, int L, int K, long P) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const long n = p / L;
  const long l = p - n * L;
  const float* e = emb + (size_t)cat_class(levels[p], K) * D;
  float* o = out + (size_t)n * D * L + l;
  for (int d = 0; d < D; ++d) o[(size_t)d * L] = e[d];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
inline bool taps_to_mask(int KH, int KW, int n_taps, const int* u, const int* v, unsigned long long* mask) {
  if (!u || !v || n_taps < 1 || n_taps > KH * KW) return false;
  unsigned long long m = 0;
  int prev = -1;
  for (int t = 0; t < n_taps; ++t) {
    if (u[t] < 0 || u[t] >= KH || v[t] < 0 || v[t] >= KW) return false;
    const int g = u[t] * KW + v[t];
    if (g <= prev) return false;  // ascending, no duplicates: the summation order is the tap order
    prev = g;
    m |= 1ull << g;
  }
  *mask = m;
  return true;
}

}  // namespace

PG_EXPORT size_t pg_code_conv_fwd_workspace_floats(int Cout, int K, int n_taps) {
  if (Cout < 1 || K < 2 || K > 4096 || n_taps < 1 || n_taps > PG_MAX_TAPS) return 0;
  return (size_t)n_taps * K * Cout;
}

PG_EXPORT int pg_code_conv_fwd(const float* levels, const float* w, const float* b, float* out, int N, int K, int Hin,
                               int Win, int Cout, int KH, int KW, int OH, int OW, int n_taps, const int* u, const int* v,
                               int pad_h, int pad_w, float* ws, size_t ws_floats, void* stream) {
  PG_REQUIRE(levels && w && out && ws, PG_EINVAL, "pg_code_conv_fwd: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_conv_fwd: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(N > 0 && Hin > 0 && Win > 0 && Cout > 0 && KH > 0 && KW > 0 && OH > 0 && OW > 0, PG_ESHAPE,
             "pg_code_conv_fwd: non-positive dimension");
  PG_REQUIRE(KH * KW <= PG_MAX_TAPS, PG_ESHAPE, "pg_code_conv_fwd: more than %d taps", PG_MAX_TAPS);
  unsigned long long mask = 0;
  PG_REQUIRE(taps_to_mask(KH, KW, n_taps, u, v, &mask), PG_EINVAL,
             "pg_code_conv_fwd: the tap list must be non-empty, inside the kernel and ascending");
  const long P = (long)N * OH * OW;
  PG_REQUIRE(P < 2147483647L - CC_POS && (long)N * Hin * Win < 2147483647L, PG_ESHAPE,
             "pg_code_conv_fwd: more than 2^31 positions");
  const size_t need = pg_code_conv_fwd_workspace_floats(Cout, K, n_taps);
  PG_REQUIRE((long)need > 0 && need < 2147483647UL, PG_ESHAPE, "pg_code_conv_fwd: table of %zu floats", need);
  PG_REQUIRE(ws_floats >= need, PG_EINVAL, "pg_code_conv_fwd: workspace of %zu floats, %zu needed", ws_floats, need);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(code_pack_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, st, w, ws, Cout, K, KH, KW,
                     mask, (long)need);
  PG_LAUNCH_CHECK("pg_code_conv_fwd(pack)");
  hipLaunchKernelGGL(code_conv_fwd_kernel, dim3((unsigned)((P + CC_POS - 1) / CC_POS)), dim3(CC_THREADS), 0, st, levels,
                     ws, b, out, N, K, Hin, Win, Cout, KH, KW, OH, OW, pad_h, pad_w, mask, P);
  PG_LAUNCH_CHECK("pg_code_conv_fwd");
  return 0;
}

PG_EXPORT int pg_code_conv_wgrad_plan(int N, int K, int Hin, int Win, int* max_chunks, int* items) {
  WgradPlan pl;
  PG_REQUIRE(max_chunks && items, PG_EINVAL, "pg_code_conv_wgrad_plan: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_conv_wgrad_plan: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(wgrad_plan(N, K, Hin, Win, 0, 0, &pl), PG_ESHAPE, "pg_code_conv_wgrad_plan: shape outside the kernels' range");
  *max_chunks = pl.max_chunks;
  *items = pl.items;
  return 0;
}

PG_EXPORT size_t pg_code_conv_wgrad_workspace_floats(int N, int K, int Hin, int Win, int Cout, int KH, int KW) {
  WgradPlan pl;
  if (Cout < 1 || KH < 1 || KW < 1 || KH * KW > PG_MAX_TAPS) return 0;
  if (!wgrad_plan(N, K, Hin, Win, Cout, KH * KW, &pl)) return 0;
  return pl.words;
}

PG_EXPORT int pg_code_conv_wgrad(const float* levels, const float* dy, float* dw, float* db, int accumulate, int N, int K,
                                 int Hin, int Win, int Cout, int KH, int KW, int OH, int OW, int pad_h, int pad_w,
                                 float* ws, size_t ws_floats, void* stream) {
  PG_REQUIRE(levels && dy && (dw || db) && ws, PG_EINVAL, "pg_code_conv_wgrad: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_conv_wgrad: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(N > 0 && Hin > 0 && Win > 0 && Cout > 0 && KH > 0 && KW > 0 && OH > 0 && OW > 0, PG_ESHAPE,
             "pg_code_conv_wgrad: non-positive dimension");
  const int T = KH * KW;
  PG_REQUIRE(T <= PG_MAX_TAPS, PG_ESHAPE, "pg_code_conv_wgrad: more than %d taps", PG_MAX_TAPS);
  WgradPlan pl;
  PG_REQUIRE(wgrad_plan(N, K, Hin, Win, Cout, T, &pl), PG_ESHAPE, "pg_code_conv_wgrad: shape outside the kernels' range");
  PG_REQUIRE((long)K * Cout * T < 2147483647L && (long)N * OH * OW < 2147483647L, PG_ESHAPE,
             "pg_code_conv_wgrad: more than 2^31 weights or output positions");
  const int cpl = 64 / T;  // channels per pass of the sum kernel
  const int groups = (Cout + cpl * CC_ACC - 1) / (cpl * CC_ACC);
  PG_REQUIRE(groups <= 65535, PG_ESHAPE, "pg_code_conv_wgrad: too many output channels");
  PG_REQUIRE(ws_floats >= pl.words, PG_EINVAL, "pg_code_conv_wgrad: workspace of %zu floats, %zu needed", ws_floats,
             pl.words);
  hipStream_t st = (hipStream_t)stream;
  if (dw) {
    int* wi = reinterpret_cast<int*>(ws);
    int *hist = wi + pl.hist, *total = wi + pl.total, *start = wi + pl.start, *cstart = wi + pl.cstart, *list = wi + pl.list;
    float* part = ws + pl.part;
    const size_t lds = (size_t)K * sizeof(int);
    hipLaunchKernelGGL(code_hist_kernel, dim3((unsigned)pl.nb), dim3(64), lds, st, levels, hist, K, pl.P, pl.B);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(hist)");
    hipLaunchKernelGGL(code_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, hist, total, start, cstart, K, pl.nb);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(scan)");
    hipLaunchKernelGGL(code_fill_kernel, dim3((unsigned)pl.nb), dim3(64), lds, st, levels, hist, start, list, K, pl.P,
                       pl.B);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(fill)");
    hipLaunchKernelGGL(code_sum_kernel, dim3((unsigned)pl.items, (unsigned)groups), dim3(64), 0, st, dy, total, start,
                       cstart, list, part, K, Hin, Win, Cout, KH, KW, OH, OW, pad_h, pad_w, (int)pl.P);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(sum)");
    const long nw = (long)K * Cout * T;
    hipLaunchKernelGGL(code_merge_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, part, cstart, dw, K, Cout,
                       T, accumulate, nw);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(merge)");
  }
  if (db) {
    hipLaunchKernelGGL(code_bias_grad_kernel, dim3((unsigned)Cout), dim3(CC_THREADS), 0, st, dy, db, Cout, (long)OH * OW,
                       (long)N * OH * OW, accumulate);
    PG_LAUNCH_CHECK("pg_code_conv_wgrad(bias)");
  }
  return 0;
}

PG_EXPORT int pg_sample_embed_codes(const float* canvas, const float* w, const float* b, const float* pos_term, float* out,
                                    int N, int K, int H, int W, int Cout, int KH, int KW, int r, int c, int ld,
                                    const int* pos_dev, void* stream) {
  PG_REQUIRE(canvas && w && out, PG_EINVAL, "pg_sample_embed_codes: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_sample_embed_codes: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && Cout <= 65535 && KH > 0 && KW > 0 && ld >= N &&
                 (long)H * W < 2147483647L,
             PG_ESHAPE, "pg_sample_embed_codes: dimensions outside the kernel's range (or ld < N)");
  PG_REQUIRE(r >= 0 && r < H && c >= 0 && c < W, PG_EINVAL, "pg_sample_embed_codes: pixel outside the image");
  hipLaunchKernelGGL(sample_embed_codes_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)Cout), dim3(64), 0,
                     (hipStream_t)stream, canvas, w, b, pos_term, out, N, K, H, W, Cout, KH, KW, r, c, ld, pos_dev);
  PG_LAUNCH_CHECK("pg_sample_embed_codes");
  return 0;
}

PG_EXPORT int pg_vq_lookup(const float* levels, const float* embedding, float* out, int N, int D, int L, int K,
                           void* stream) {
  PG_REQUIRE(levels && embedding && out, PG_EINVAL, "pg_vq_lookup: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_vq_lookup: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(N > 0 && D > 0 && L > 0 && (long)N * L < 2147483647L - 256, PG_ESHAPE, "pg_vq_lookup: bad dims");
  const long P = (long)N * L;
  hipLaunchKernelGGL(vq_lookup_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, levels,
                     embedding, out, D, L, K, P);
  PG_LAUNCH_CHECK("pg_vq_lookup");
  return 0;
}
