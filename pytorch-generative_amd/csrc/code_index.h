// code_index.h — the inverted index over a code image that the store-and-sum weight gradients share (code_conv.hip,
// code_up.hip): per code the ascending list of the positions that hold it, a stable counting sort on integer counters.
// Every kernel has internal linkage: each translation unit that includes this header carries its own copy.
#pragma once
#include "categorical.h"

namespace {

constexpr int CC_CHUNK = 512;     // list entries one wave sums; longer lists are split and merged in chunk order
constexpr int CC_SORT_MIN = 2048; // positions per sort block (at least; at most CC_SORT_BLOCKS blocks)
constexpr int CC_SORT_BLOCKS = 256;
constexpr int CC_SCAN_THREADS = 1024;

__device__ __forceinline__ int code_of(float level, int K) { return level < 0.f ? -1 : cat_class(level, K); }

// hist[b][k] = number of positions of sort block b (positions [b B, (b + 1) B)) that hold code k. Integer LDS atomics: exact.
__global__ void __launch_bounds__(64) code_hist_kernel(const float* __restrict__ levels, int* __restrict__ hist, int K,
                                                       long P, int B) {
  extern __shared__ int cnt[];
  const int lane = threadIdx.x;
  for (int k = lane; k < K; k += 64) cnt[k] = 0;
  __syncthreads();
  const long q0 = (long)blockIdx.x * B;
  const long q1 = q0 + B < P ? q0 + B : P;
  for (long q = q0 + lane; q < q1; q += 64) {
    const int k = code_of(levels[q], K);
    if (k >= 0) atomicAdd(&cnt[k], 1);
  }
  __syncthreads();
  for (int k = lane; k < K; k += 64) hist[(size_t)blockIdx.x * K + k] = cnt[k];
}

// One workgroup. hist[b][k] becomes the number of positions with code k in the blocks before b; total[k] the list length,
// start[k] the list's first slot (exclusive prefix, start[K] = all listed positions), cstart[k] the first work item of
// code k (exclusive prefix of ceil(total / CC_CHUNK), cstart[K] = all items).
__global__ void __launch_bounds__(CC_SCAN_THREADS) code_scan_kernel(int* __restrict__ hist, int* __restrict__ total,
                                                                    int* __restrict__ start, int* __restrict__ cstart,
                                                                    int K, int nb) {
  __shared__ int sa[2][CC_SCAN_THREADS], sb[2][CC_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int kpt = (K + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS;  // <= 4 consecutive codes per thread
  int tot[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = tid * kpt + i;
    if (i < kpt && k < K) {
      int run = 0;
      for (int b = 0; b < nb; ++b) {
        const int t = hist[(size_t)b * K + k];
        hist[(size_t)b * K + k] = run;
        run += t;
      }
      tot[i] = run;
      total[k] = run;
    }
  }
  int a = 0, c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a += tot[i];
    c += (tot[i] + CC_CHUNK - 1) / CC_CHUNK;
  }
  sa[0][tid] = a;
  sb[0][tid] = c;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < CC_SCAN_THREADS; off <<= 1) {  // inclusive scan over the threads
    int va = sa[cur][tid], vb = sb[cur][tid];
    if (tid >= off) {
      va += sa[cur][tid - off];
      vb += sb[cur][tid - off];
    }
    sa[cur ^ 1][tid] = va;
    sb[cur ^ 1][tid] = vb;
    cur ^= 1;
    __syncthreads();
  }
  int ra = sa[cur][tid] - a, rc = sb[cur][tid] - c;  // exclusive
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = tid * kpt + i;
    if (i < kpt && k < K) {
      start[k] = ra;
      cstart[k] = rc;
      ra += tot[i];
      rc += (tot[i] + CC_CHUNK - 1) / CC_CHUNK;
    }
  }
  if (tid == CC_SCAN_THREADS - 1) {
    start[K] = sa[cur][tid];
    cstart[K] = sb[cur][tid];
  }
}

// list[start[k] + rank] = q, rank = the number of positions before q that hold the same code: every list is ascending.
// One wave per sort block walks its positions 64 at a time; lanes that share a code are found with ballots.
__global__ void __launch_bounds__(64) code_fill_kernel(const float* __restrict__ levels, const int* __restrict__ hist,
                                                       const int* __restrict__ start, int* __restrict__ list, int K,
                                                       long P, int B) {
  extern __shared__ int cnt[];
  const int lane = threadIdx.x;
  for (int k = lane; k < K; k += 64) cnt[k] = start[k] + hist[(size_t)blockIdx.x * K + k];
  __syncthreads();
  const long q0 = (long)blockIdx.x * B;
  const long q1 = q0 + B < P ? q0 + B : P;
  for (long qb = q0; qb < q1; qb += 64) {  // uniform trip count: the barriers below are reached by every lane
    const long q = qb + lane;
    const int k = q < q1 ? code_of(levels[q], K) : -1;
    const bool valid = k >= 0;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 12; ++bit) {  // K <= 4096: 12 bits
      const bool set = (k >> bit) & 1;
      const unsigned long long bm = __ballot(valid && set);
      peers &= set ? bm : ~bm;
    }
    const int lower = __popcll(peers & ((1ull << lane) - 1ull));
    const bool last = ((peers >> lane) >> 1) == 0ull;
    const int base = valid ? cnt[k] : 0;
    __syncthreads();
    if (valid) {
      const int slot = base + lower;
      if (slot >= 0 && slot < P) list[slot] = (int)q;
      if (last) cnt[k] = slot + 1;
    }
    __syncthreads();
  }
}

// The workspace of a store-and-sum weight gradient over P = N Hin Win indexed positions, Cout x T sums per work item.
struct WgradPlan {
  long P;
  int B, nb, items, max_chunks;
  size_t hist, total, start, cstart, list, part, words;  // offsets in 4-byte words
};

inline bool wgrad_plan(int N, int K, int Hin, int Win, int Cout, int T, WgradPlan* pl) {
  if (N < 1 || Hin < 1 || Win < 1 || K < 2 || K > 4096) return false;
  const long P = (long)N * Hin * Win;
  if (P >= 2147483647L - 64) return false;
  pl->P = P;
  long B = (P + CC_SORT_BLOCKS - 1) / CC_SORT_BLOCKS;
  if (B < CC_SORT_MIN) B = CC_SORT_MIN;
  B = (B + 63) / 64 * 64;
  pl->B = (int)B;
  pl->nb = (int)((P + B - 1) / B);
  pl->max_chunks = (int)((P + CC_CHUNK - 1) / CC_CHUNK);  // the longest possible list
  const long items = (long)K + P / CC_CHUNK;              // sum_k ceil(c_k / CHUNK) <= P / CHUNK + K
  if (items > 2147483647L) return false;
  pl->items = (int)items;
  size_t o = 0;
  pl->hist = o, o += (size_t)pl->nb * K;
  pl->total = o, o += (size_t)K;
  pl->start = o, o += (size_t)K + 1;
  pl->cstart = o, o += (size_t)K + 1;
  pl->list = o, o += (size_t)P;
  o = (o + 3) / 4 * 4;
  pl->part = o, o += (size_t)items * (size_t)(Cout > 0 ? Cout : 0) * (size_t)(T > 0 ? T : 0);
  pl->words = o;
  return true;
}

}  // namespace
