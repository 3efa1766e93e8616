// code_up.hip — a transposed convolution with kernel = stride = f over an image of code indices: a table lookup with a phase,
//   out[n, co, i f + a, j f + b] = base[n, co, i f + a, j f + b] + w[code(n, i, j), co, a, b]        w (K, Cout, f, f)
// (F.conv_transpose2d(one_hot(codes), w, stride = f) added to `base`), its weight gradient, and one raster position of it for
// the incremental sampler: how an autoregressive prior over the bottom codes of a two-level VQ-VAE takes the top codes as
// context. The code image is a LEVEL image (N, 1, h, w) at the levels j / (K - 1), decoded as code_conv.hip decodes it; a
// negative level adds nothing. Nothing of the size N K h w or N Cout f^2 h w is formed.
//   pg_code_up_fwd:        pack the weight into (f^2, K, Cout) rows, gather contiguous Cout rows, one pass over base / out
//   pg_code_up_wgrad:      store-and-sum over the inverted index of the (N, h, w) top positions (code_index.h)
//   pg_sample_cond_codes:  x[co ld + n] += w[code(n, r / f, c / f), co, r % f, c % f]
#include "code_index.h"

namespace {

constexpr int CU_POS = 64;      // output positions per workgroup of the forward
constexpr int CU_THREADS = 256;
constexpr int CU_ACC = 8;       // accumulators (output channels) per lane of the sum kernel
constexpr int CU_FLIGHT = 4;   // list entries whose dY reads are in flight together in the sum kernel (divides 64)
constexpr int CU_MAX_F = 4;

// table[((a f + b) K + k) Cout + co] = w[k][co][a][b]
__global__ void code_up_pack_kernel(const float* __restrict__ w, float* __restrict__ table, int K, int Cout, int T,
                                    long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int co = (int)(e % Cout);
  const long r = e / Cout;
  const int k = (int)(r % K);
  const int ph = (int)(r / K);
  table[e] = w[((size_t)k * Cout + co) * T + ph];
}

// One workgroup: CU_POS consecutive output positions (of the sequence (n H + y) W + x, H = h f, W = w f) x all channels.
// Phase 1 turns every position into its table row (phase K + code, or -1); phase 2 gathers with the lanes along the channels
// (contiguous table rows) into a transposing LDS tile, which is added to `base` and written with the lanes along the positions
// (contiguous NCHW planes). `out` may be `base`: an element is read and written by the same thread, once.
__global__ void __launch_bounds__(CU_THREADS) code_up_fwd_kernel(const float* __restrict__ levels,
                                                                 const float* __restrict__ table, const float* base,
                                                                 float* out, int K, int h, int w, int Cout, int f, long P) {
  __shared__ int rows[CU_POS];
  __shared__ float tile[64][CU_POS + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = (long)blockIdx.x * CU_POS;
  const int W = w * f;
  const long HW = (long)h * f * W;
  if (tid < CU_POS) {
    const long p = p0 + tid;
    int row = -1;
    if (p < P) {
      const long n = p / HW;
      const int rem = (int)(p - n * HW);
      const int y = rem / W, x = rem - y * W;
      const int i = y / f, j = x / f;
      const int k = code_of(levels[((size_t)n * h + i) * w + j], K);
      if (k >= 0) row = ((y - i * f) * f + (x - j * f)) * K + k;
    }
    rows[tid] = row;
  }
  __syncthreads();
  for (int c0 = 0; c0 < Cout; c0 += 64) {
    const int co = c0 + lane;
    const bool cok = co < Cout;
    for (int pp = wave; pp < CU_POS; pp += CU_THREADS / 64) {
      const int row = rows[pp];
      tile[lane][pp] = (row >= 0 && cok) ? table[(size_t)row * Cout + co] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < 64 * CU_POS; i += CU_THREADS) {
      const int cl = i / CU_POS, pl = i - cl * CU_POS;
      const long p = p0 + pl;
      if (c0 + cl < Cout && p < P) {
        const long n = p / HW;
        const long rem = p - n * HW;
        const size_t o = ((size_t)n * Cout + (c0 + cl)) * HW + rem;
        const float t = tile[cl][pl];
        // a position without a code keeps `base` as it is (no addition); without `base` the row itself is the result
        out[o] = base ? (rows[pl] >= 0 ? base[o] + t : base[o]) : t;
      }
    }
    __syncthreads();
  }
}

// One wave: one work item (a chunk of at most CC_CHUNK entries of one code's list of TOP positions) x one group of output
// channels. lane = (channel sub-index, phase): a list entry's f x f block of dY is read once per channel; CU_ACC channels per
// lane. part[(item * Cout + co) * T + phase] = the chunk's sum in list order.
__global__ void __launch_bounds__(64) code_up_sum_kernel(const float* __restrict__ dy, const int* __restrict__ total,
                                                         const int* __restrict__ start, const int* __restrict__ cstart,
                                                         const int* __restrict__ list, float* __restrict__ part, int K,
                                                         int h, int w, int Cout, int f, int P) {
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
  const int T = f * f;
  const int cpl = 64 / T;  // channels per pass
  const int phase = lane % T, cs = lane / T;
  const int a = phase / f, b = phase - a * f;
  const bool active = cs < cpl;
  const int co0 = blockIdx.y * (cpl * CU_ACC) + cs;
  const int hw = h * w;
  const int W = w * f;
  const size_t HW = (size_t)h * f * W;
  float acc[CU_ACC];
#pragma unroll
  for (int c = 0; c < CU_ACC; ++c) acc[c] = 0.f;
  // The walk is a chain of memory latencies (list entry -> address -> dY), so 64 entries are fetched with one coalesced load
  // and handed round by lane broadcast, and the dY reads of CU_FLIGHT entries are issued before the first of them is added.
  // The additions keep the list order (an absent entry adds 0): the same sum as the entry-by-entry walk.
  for (int ib = i0; ib < i1; ib += 64) {
    const int mine = ib + lane < i1 ? lp[ib + lane] : -1;
    const int cnt = i1 - ib < 64 ? i1 - ib : 64;
    for (int e = 0; e < cnt; e += CU_FLIGHT) {
      float v[CU_FLIGHT][CU_ACC];
#pragma unroll
      for (int u = 0; u < CU_FLIGHT; ++u) {
        const int q = __shfl(mine, e + u);  // e + u <= 63; lanes past cnt hold -1
        const bool okq = active && (unsigned)q < (unsigned)P;  // (keeps every read inside dY)
        const int qq = okq ? q : 0;
        const int n = qq / hw;
        const int rem = qq - n * hw;
        const int ty = rem / w, tx = rem - ty * w;
        const float* src = dy + (size_t)n * Cout * HW + (size_t)(ty * f + a) * W + (size_t)(tx * f + b);
#pragma unroll
        for (int c = 0; c < CU_ACC; ++c) {
          const int co = co0 + c * cpl;
          v[u][c] = (okq && co < Cout) ? src[(size_t)co * HW] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < CU_FLIGHT; ++u)
#pragma unroll
        for (int c = 0; c < CU_ACC; ++c) acc[c] += v[u][c];
    }
  }
#pragma unroll
  for (int c = 0; c < CU_ACC; ++c) {
    const int co = co0 + c * cpl;
    if (active && co < Cout) part[((size_t)item * Cout + co) * T + phase] = acc[c];
  }
}

// dW[k][co][phase] (+)= the chunks of code k in chunk order; a code without a chunk receives an exact zero.
__global__ void code_up_merge_kernel(const float* __restrict__ part, const int* __restrict__ cstart, float* __restrict__ dw,
                                     int Cout, int T, int accumulate, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int phase = (int)(e % T);
  const long r = e / T;
  const int co = (int)(r % Cout);
  const int k = (int)(r / Cout);
  float s = 0.f;
  for (int it = cstart[k]; it < cstart[k + 1]; ++it) s += part[((size_t)it * Cout + co) * T + phase];
  dw[e] = accumulate ? dw[e] + s : s;
}

__global__ void sample_cond_codes_kernel(const float* __restrict__ cond, const float* __restrict__ wt, float* __restrict__ x,
                                         int N, int K, int h, int w, int Cout, int f, int r, int c, int ld,
                                         const int* __restrict__ pos_dev) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int co = blockIdx.y;
  if (n >= N) return;
  const int W = w * f;
  if (pos_dev) {
    const int p = min(max(*pos_dev, 0), h * f * W - 1);
    r = p / W;
    c = p - r * W;
  }
  const int i = r / f, j = c / f;
  const int k = code_of(cond[((size_t)n * h + i) * w + j], K);
  if (k >= 0) x[(size_t)co * ld + n] += wt[(((size_t)k * Cout + co) * f + (r - i * f)) * f + (c - j * f)];
}

// the shape rules every entry point shares; the output image is (h f, w f)
inline bool code_up_dims_ok(int N, int h, int w, int Cout, int f) {
  if (N < 1 || h < 1 || w < 1 || Cout < 1 || f < 1 || f > CU_MAX_F) return false;
  const long top = (long)N * h * w;
  return top < 2147483647L / (CU_MAX_F * CU_MAX_F) && top * f * f < 2147483647L - CU_POS;
}

}  // namespace

PG_EXPORT size_t pg_code_up_fwd_workspace_floats(int K, int Cout, int f) {
  if (K < 2 || K > 4096 || Cout < 1 || f < 1 || f > CU_MAX_F) return 0;
  const size_t need = (size_t)f * f * K * Cout;
  return need < 2147483647UL ? need : 0;
}

PG_EXPORT int pg_code_up_fwd(const float* levels, const float* wt, const float* base, float* out, int N, int K, int h, int w,
                             int Cout, int f, float* ws, size_t ws_floats, void* stream) {
  PG_REQUIRE(levels && wt && out && ws, PG_EINVAL, "pg_code_up_fwd: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_up_fwd: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(f >= 1 && f <= CU_MAX_F, PG_ESHAPE, "pg_code_up_fwd: factor = %d outside 1..%d", f, CU_MAX_F);
  PG_REQUIRE(code_up_dims_ok(N, h, w, Cout, f), PG_ESHAPE, "pg_code_up_fwd: non-positive dimension or 2^31 positions");
  const size_t need = pg_code_up_fwd_workspace_floats(K, Cout, f);
  PG_REQUIRE(need > 0, PG_ESHAPE, "pg_code_up_fwd: table of more than 2^31 floats");
  PG_REQUIRE(ws_floats >= need, PG_EINVAL, "pg_code_up_fwd: workspace of %zu floats, %zu needed", ws_floats, need);
  const long P = (long)N * h * w * f * f;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(code_up_pack_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, st, wt, ws, K, Cout, f * f,
                     (long)need);
  PG_LAUNCH_CHECK("pg_code_up_fwd(pack)");
  hipLaunchKernelGGL(code_up_fwd_kernel, dim3((unsigned)((P + CU_POS - 1) / CU_POS)), dim3(CU_THREADS), 0, st, levels, ws,
                     base, out, K, h, w, Cout, f, P);
  PG_LAUNCH_CHECK("pg_code_up_fwd");
  return 0;
}

PG_EXPORT int pg_code_up_plan(int N, int K, int h, int w, int* max_chunks, int* items) {
  WgradPlan pl;
  PG_REQUIRE(max_chunks && items, PG_EINVAL, "pg_code_up_plan: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_up_plan: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(code_up_dims_ok(N, h, w, 1, 1) && wgrad_plan(N, K, h, w, 0, 0, &pl), PG_ESHAPE,
             "pg_code_up_plan: shape outside the kernels' range");
  *max_chunks = pl.max_chunks;
  *items = pl.items;
  return 0;
}

PG_EXPORT size_t pg_code_up_wgrad_workspace_floats(int N, int K, int h, int w, int Cout, int f) {
  WgradPlan pl;
  if (!code_up_dims_ok(N, h, w, Cout, f) || (long)K * Cout * f * f >= 2147483647L) return 0;
  if (!wgrad_plan(N, K, h, w, Cout, f * f, &pl)) return 0;
  return pl.words;
}

PG_EXPORT int pg_code_up_wgrad(const float* levels, const float* dy, float* dw, int accumulate, int N, int K, int h, int w,
                               int Cout, int f, float* ws, size_t ws_floats, void* stream) {
  PG_REQUIRE(levels && dy && dw && ws, PG_EINVAL, "pg_code_up_wgrad: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_code_up_wgrad: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(f >= 1 && f <= CU_MAX_F, PG_ESHAPE, "pg_code_up_wgrad: factor = %d outside 1..%d", f, CU_MAX_F);
  PG_REQUIRE(code_up_dims_ok(N, h, w, Cout, f), PG_ESHAPE, "pg_code_up_wgrad: non-positive dimension or 2^31 positions");
  const int T = f * f;
  WgradPlan pl;
  PG_REQUIRE(wgrad_plan(N, K, h, w, Cout, T, &pl), PG_ESHAPE, "pg_code_up_wgrad: shape outside the kernels' range");
  const long nw = (long)K * Cout * T;
  PG_REQUIRE(nw < 2147483647L, PG_ESHAPE, "pg_code_up_wgrad: more than 2^31 weights");
  const int cpl = 64 / T;  // channels per pass of the sum kernel
  const int groups = (Cout + cpl * CU_ACC - 1) / (cpl * CU_ACC);
  PG_REQUIRE(groups <= 65535, PG_ESHAPE, "pg_code_up_wgrad: too many output channels");
  PG_REQUIRE(ws_floats >= pl.words, PG_EINVAL, "pg_code_up_wgrad: workspace of %zu floats, %zu needed", ws_floats, pl.words);
  hipStream_t st = (hipStream_t)stream;
  int* wi = reinterpret_cast<int*>(ws);
  int *hist = wi + pl.hist, *total = wi + pl.total, *start = wi + pl.start, *cstart = wi + pl.cstart, *list = wi + pl.list;
  float* part = ws + pl.part;
  const size_t lds = (size_t)K * sizeof(int);
  hipLaunchKernelGGL(code_hist_kernel, dim3((unsigned)pl.nb), dim3(64), lds, st, levels, hist, K, pl.P, pl.B);
  PG_LAUNCH_CHECK("pg_code_up_wgrad(hist)");
  hipLaunchKernelGGL(code_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, hist, total, start, cstart, K, pl.nb);
  PG_LAUNCH_CHECK("pg_code_up_wgrad(scan)");
  hipLaunchKernelGGL(code_fill_kernel, dim3((unsigned)pl.nb), dim3(64), lds, st, levels, hist, start, list, K, pl.P, pl.B);
  PG_LAUNCH_CHECK("pg_code_up_wgrad(fill)");
  hipLaunchKernelGGL(code_up_sum_kernel, dim3((unsigned)pl.items, (unsigned)groups), dim3(64), 0, st, dy, total, start,
                     cstart, list, part, K, h, w, Cout, f, (int)pl.P);
  PG_LAUNCH_CHECK("pg_code_up_wgrad(sum)");
  hipLaunchKernelGGL(code_up_merge_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, part, cstart, dw, Cout, T,
                     accumulate, nw);
  PG_LAUNCH_CHECK("pg_code_up_wgrad(merge)");
  return 0;
}

PG_EXPORT int pg_sample_cond_codes(const float* cond_levels, const float* wt, float* x, int N, int K, int h, int w, int Cout,
                                   int f, int r, int c, int ld, const int* pos_dev, void* stream) {
  PG_REQUIRE(cond_levels && wt && x, PG_EINVAL, "pg_sample_cond_codes: null pointer");
  PG_REQUIRE(K >= 2 && K <= 4096, PG_ESHAPE, "pg_sample_cond_codes: n_codes = %d outside 2..4096", K);
  PG_REQUIRE(f >= 1 && f <= CU_MAX_F, PG_ESHAPE, "pg_sample_cond_codes: factor = %d outside 1..%d", f, CU_MAX_F);
  PG_REQUIRE(code_up_dims_ok(N, h, w, Cout, f) && Cout <= 65535 && ld >= N && (long)K * Cout * f * f < 2147483647L, PG_ESHAPE,
             "pg_sample_cond_codes: dimensions outside the kernel's range (or ld < N)");
  PG_REQUIRE(r >= 0 && r < h * f && c >= 0 && c < w * f, PG_EINVAL, "pg_sample_cond_codes: pixel outside the image");
  hipLaunchKernelGGL(sample_cond_codes_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)Cout), dim3(64), 0,
                     (hipStream_t)stream, cond_levels, wt, x, N, K, h, w, Cout, f, r, c, ld, pos_dev);
  PG_LAUNCH_CHECK("pg_sample_cond_codes");
  return 0;
}
