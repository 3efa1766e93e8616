// linear_attention.hip — LinearCausalAttention (reference nn/attention.py:168-275) as chunked prefix-state scans.
//
// Per image n and head h (L = H*W positions, phi = elu + 1 or the identity):
//   num[l] = phi(q[l]) . sum_{j <= l} phi(k[j])^T v[j]                     (_UnnormalizedLinearCausalAttention)
//   den[n, h, l] = 1 / (sum_i phi(q)[n,h,l,i] * sum_{h' <= h} phi(k)[n,h',l,i] + 1e-10)
//   out = num * den
// The denominator keeps the reference's cumsum over the HEADS axis (`einsum("nlhi,nlhi->nlh", Q, K.cumsum(1))` on
// (N, heads, L, d) tensors): head h reads the k of heads 0..h at the same pixel; it is not causal over positions.
//
// Every product of the forward and the backward is one instance of the generic scan
//   y[p] = rowscale[p] * sum_{p' <= p} (a[p] . b[p']) c[p']      (p in logical order: forward, or reversed for
//                                                                  the anti-causal products of the backward)
// on three launches (two-pass, so that few (n, head) sequences still fill the chip):
//   la_state_kernel   chunk states  S_c = B_c^T C_c  (da x dc) of every chunk of LA_T positions but the last
//   la_prefix_kernel  exclusive prefix over chunks, in place (fixed order: deterministic, no atomics)
//   la_out_kernel     y_c = A_c P_c + tril(A_c B_c^T) C_c
// All products are v_mfma_f32_16x16x4_f32: fp32 inputs, an fp32 fmaf chain per product (bit-for-bit), so the results
// are fp32-exact without the bf16x3 split. The matrix pipe is not what bounds these kernels: at every measured shape
// both the FLOP bound and the byte bound are 6-14 % of the measured time (profiles/linear_attention.json; staging,
// the chunk-state round trips and the launch chain take the rest), so the split's higher rate (six bf16 MFMAs per
// product, ~2.7x fp32) would buy nothing here. phi is applied while staging the
// operands (the backward recomputes it from the raw q and k); nothing L x L is ever formed.
//
// Backward (g = upstream gradient, gn = g * den, gs = -den * (g . out) = dLoss / d(den's sum)):
//   dphi(q)[l] = sum_{j <= l} (gn[l] . v[j]) phi(k)[j]          scan(a = gn, b = v,  c = phi k), forward
//   dphi(k)[j] = sum_{l >= j} (v[j] . gn[l]) phi(q)[l]          scan(a = v,  b = gn, c = phi q), reversed
//   dv[j]      = sum_{l >= j} (phi(k)[j] . phi(q)[l]) gn[l]     scan(a = phi k, b = phi q, c = gn), reversed
// then la_den_bwd_kernel adds the denominator's terms per pixel (dphi(q)[h] += gs[h] Kc[h], dphi(k)[h'] +=
// sum_{h >= h'} gs[h] phi(q)[h]: the cross-head term of the cumsum) and multiplies by phi'(t) = t > 0 ? 1 : phi(t).
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int LA_T = 64;           // positions per chunk
constexpr int LA_D = 64;           // largest head dim (PG_ESHAPE above)
constexpr int LA_LD = LA_T + 1;    // LDS row stride in floats: the column reads of the MFMA operands are conflict free
constexpr int LA_THREADS = 256;    // 4 waves

using pg_tile::f32x4;

#define LA_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)

__device__ __forceinline__ float la_phi(float x) { return x > 0.f ? x + 1.f : expf(x); }
__device__ __forceinline__ float la_dphi(float x) { return x > 0.f ? 1.f : expf(x); }

// One operand of a scan: element (n, h, comp, pos) at p + n * bs + (h * d + comp) * L + pos (the NCHW planes of q,
// k, v, g as the 1x1 projections write them); `scale` (optional) multiplies position pos of sequence n * heads + h.
struct LaOperand {
  const float* p;
  const float* scale;
  long bs;
  int d;
  int phi;
};

struct LaScan {
  LaOperand a, b, c;      // a.d == b.d == da, c.d == dc
  float* out;             // y (n, h, e, pos) at out + n * obs + (h * dc + e) * L + pos
  const float* oscale;    // optional row scale of y, (N * heads, L)
  float* ws;              // chunk states (N * heads, nch, da * dc)
  long obs;
  int heads, L, nch, reverse;
};

// Stages rows [0, round16(d)) x LA_T positions of chunk p0 into s[row][pos] (zero outside d and L; phi applied to real
// elements only — phi(0) = 1 must not leak into the padding).
__device__ __forceinline__ void la_stage(float* __restrict__ s, const LaOperand& op, int n, int nh, int h, int L,
                                         int p0, int reverse, int tid) {
  const int rows = (op.d + 15) & ~15;
  const float* base = op.p + (size_t)n * op.bs + (size_t)h * op.d * L;
  const float* sc = op.scale ? op.scale + (size_t)nh * L : nullptr;
  for (int idx = tid; idx < rows * LA_T; idx += LA_THREADS) {
    const int r = idx / LA_T, p = idx % LA_T;
    const int pos = p0 + p;
    float v = 0.f;
    if (r < op.d && pos < L) {
      const int l = reverse ? L - 1 - pos : pos;
      v = base[(size_t)r * L + l];
      if (op.phi) v = la_phi(v);
      if (sc) v *= sc[l];
    }
    s[r * LA_LD + p] = v;
  }
}

// S_c[i][e] = sum_{p in chunk} b[i][p] c[e][p] for every chunk but the last (the prefix is exclusive).
__global__ void __launch_bounds__(LA_THREADS) la_state_kernel(LaScan s) {
  __shared__ float b_s[LA_D * LA_LD];
  __shared__ float c_s[LA_D * LA_LD];
  const int chunk = blockIdx.x % s.nch, nh = blockIdx.x / s.nch;
  if (chunk == s.nch - 1) return;
  const int n = nh / s.heads, h = nh % s.heads;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  la_stage(b_s, s.b, n, nh, h, s.L, chunk * LA_T, s.reverse, tid);
  la_stage(c_s, s.c, n, nh, h, s.L, chunk * LA_T, s.reverse, tid);
  __syncthreads();
  const int da = s.b.d, dc = s.c.d;
  const int ti = (da + 15) >> 4, te = (dc + 15) >> 4;
  float* w = s.ws + ((size_t)nh * s.nch + chunk) * da * dc;
  const int lr = lane & 15, lk = lane >> 4;
  for (int t = wave; t < ti * te; t += LA_THREADS / 64) {
    const int i0 = (t / te) * 16, e0 = (t % te) * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int k0 = 0; k0 < LA_T; k0 += 4)
      acc = LA_MFMA(b_s[(i0 + lr) * LA_LD + k0 + lk], c_s[(e0 + lr) * LA_LD + k0 + lk], acc);
    const int e = e0 + lr;  // D: column = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + lk * 4 + r;
      if (i < da && e < dc) w[i * dc + e] = acc[r];
    }
  }
}

// In place: ws[nh][c] <- sum_{c' < c} ws[nh][c'], one thread per (sequence, state element), chunks in order.
__global__ void __launch_bounds__(LA_THREADS) la_prefix_kernel(float* __restrict__ ws, int nch, int sz, int blocks_per_seq) {
  const int nh = blockIdx.x / blocks_per_seq;
  const int e = (blockIdx.x % blocks_per_seq) * LA_THREADS + threadIdx.x;
  if (e >= sz) return;
  float* p = ws + (size_t)nh * nch * sz + e;
  float run = 0.f;
  for (int c0 = 0; c0 < nch; c0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = c0 + k < nch - 1 ? p[(size_t)(c0 + k) * sz] : 0.f;  // 8 loads in flight
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (c0 + k < nch) p[(size_t)(c0 + k) * sz] = run;
      run += v[k];
    }
  }
}

// y^T[e][l] = rowscale[l] * (sum_i P[i][e] a[i][l] + sum_{j <= l} c[e][j] (sum_i b[i][j] a[i][l])) over one chunk.
__global__ void __launch_bounds__(LA_THREADS) la_out_kernel(LaScan s) {
  __shared__ float a_s[LA_D * LA_LD];
  __shared__ float b_s[LA_D * LA_LD];  // b, then the masked score tile Sm^T[j][l]
  __shared__ float c_s[LA_D * LA_LD];
  const int chunk = blockIdx.x % s.nch, nh = blockIdx.x / s.nch;
  const int n = nh / s.heads, h = nh % s.heads;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int p0 = chunk * LA_T;
  la_stage(a_s, s.a, n, nh, h, s.L, p0, s.reverse, tid);
  la_stage(b_s, s.b, n, nh, h, s.L, p0, s.reverse, tid);
  la_stage(c_s, s.c, n, nh, h, s.L, p0, s.reverse, tid);
  __syncthreads();
  const int da = s.a.d, dc = s.c.d;
  const int da4 = (da + 3) & ~3;
  // Sm^T[j][l] = sum_i b[i][j] a[i][l]: 4 x 4 tiles of 16 x 16, wave w owns key block j0 = 16 w; tiles above the
  // diagonal (j0 > l0) are zero and skipped
  f32x4 sm[4];
  const int j0 = wave * 16;
#pragma unroll
  for (int tl = 0; tl < 4; ++tl) {
    const int l0 = tl * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (j0 <= l0) {
      for (int k0 = 0; k0 < da4; k0 += 4)
        acc = LA_MFMA(b_s[(k0 + lk) * LA_LD + j0 + lr], a_s[(k0 + lk) * LA_LD + l0 + lr], acc);
    }
    sm[tl] = acc;
  }
  __syncthreads();  // every wave is done reading b
#pragma unroll
  for (int tl = 0; tl < 4; ++tl) {
    const int l = tl * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + lk * 4 + r;
      b_s[j * LA_LD + l] = j <= l ? sm[tl][r] : 0.f;  // causal mask, inclusive of j = l
    }
  }
  __syncthreads();
  const float* P = s.ws + ((size_t)nh * s.nch + chunk) * da * dc;
  const int te = (dc + 15) >> 4;
  for (int t = wave; t < te * 4; t += LA_THREADS / 64) {
    const int e0 = (t >> 2) * 16, l0 = (t & 3) * 16;
    const int ea = e0 + lr;  // the A operand's row
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (chunk > 0) {  // the state before chunk 0 is zero
      for (int k0 = 0; k0 < da4; k0 += 4) {
        const int i = k0 + lk;
        const float pv = (i < da && ea < dc) ? P[i * dc + ea] : 0.f;
        acc = LA_MFMA(pv, a_s[i * LA_LD + l0 + lr], acc);
      }
    }
    for (int k0 = 0; k0 < l0 + 16; k0 += 4)  // keys j <= l < l0 + 16
      acc = LA_MFMA(c_s[ea * LA_LD + k0 + lk], b_s[(k0 + lk) * LA_LD + l0 + lr], acc);
    const int pos = p0 + l0 + lr;  // D: column (position) = lane & 15, row (e) = (lane >> 4) * 4 + r
    if (pos < s.L) {
      const int l = s.reverse ? s.L - 1 - pos : pos;
      const float sc = s.oscale ? s.oscale[(size_t)nh * s.L + l] : 1.f;
      float* y = s.out + (size_t)n * s.obs + (size_t)h * dc * s.L + l;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = e0 + lk * 4 + r;
        if (e < dc) y[(size_t)e * s.L] = acc[r] * sc;
      }
    }
  }
}

// den[n, h, l] = 1 / (sum_i phi(q)[h, i] * Kc[h, i] + 1e-10), Kc[h] = sum_{h' <= h} phi(k)[h'] — one thread per pixel,
// Kc in registers (DKR = the instantiated bound of dk).
template <int DKR>
__global__ void __launch_bounds__(LA_THREADS)
la_den_kernel(const float* __restrict__ q, const float* __restrict__ k, float* __restrict__ den, int N, int heads, int L,
              int dk, long qbs, long kbs, int phi) {
  const long idx = (long)blockIdx.x * LA_THREADS + threadIdx.x;
  if (idx >= (long)N * L) return;
  const int n = (int)(idx / L), l = (int)(idx % L);
  const float* qp = q + (size_t)n * qbs + l;
  const float* kp = k + (size_t)n * kbs + l;
  float kc[DKR];
#pragma unroll
  for (int i = 0; i < DKR; ++i) kc[i] = 0.f;
  for (int h = 0; h < heads; ++h) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DKR; ++i) {
      if (i < dk) {
        const float kv = *kp, qv = *qp;
        kp += L;
        qp += L;
        kc[i] += phi ? la_phi(kv) : kv;
        s = fmaf(phi ? la_phi(qv) : qv, kc[i], s);
      }
    }
    den[((size_t)n * heads + h) * L + l] = 1.f / (s + 1e-10f);
  }
}

// gs[n, h, l] = -den * sum_e g[h, e] * out[h, e]   (out = num * den, so dLoss/d(den's sum) = -den^2 (g . num))
__global__ void __launch_bounds__(LA_THREADS)
la_gs_kernel(const float* __restrict__ g, const float* __restrict__ out, const float* __restrict__ den,
             float* __restrict__ gs, int N, int heads, int L, int dv, long obs) {
  const long idx = (long)blockIdx.x * LA_THREADS + threadIdx.x;
  if (idx >= (long)N * heads * L) return;
  const long nh = idx / L;
  const int l = (int)(idx % L);
  const int n = (int)(nh / heads), h = (int)(nh % heads);
  const size_t base = (size_t)n * obs + (size_t)h * dv * L + l;
  float s = 0.f;
  for (int e = 0; e < dv; ++e) s = fmaf(g[base + (size_t)e * L], out[base + (size_t)e * L], s);
  gs[idx] = -den[idx] * s;
}

// dq, dk hold the scans' dphi(q), dphi(k); adds the denominator's terms and applies phi'.
template <int DKR>
__global__ void __launch_bounds__(LA_THREADS)
la_den_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ gs,
                  float* __restrict__ dq, float* __restrict__ dk, int N, int heads, int L, int dkd, long qbs, long kbs,
                  int phi) {
  const long idx = (long)blockIdx.x * LA_THREADS + threadIdx.x;
  if (idx >= (long)N * L) return;
  const int n = (int)(idx / L), l = (int)(idx % L);
  const float* qp = q + (size_t)n * qbs + l;
  const float* kp = k + (size_t)n * kbs + l;
  float* dqp = dq + (size_t)n * qbs + l;
  float* dkp = dk + (size_t)n * kbs + l;
  const float* gsp = gs + (size_t)n * heads * L + l;
  float acc[DKR];
#pragma unroll
  for (int i = 0; i < DKR; ++i) acc[i] = 0.f;
  for (int h = 0; h < heads; ++h) {  // dphi(q)[h] += gs[h] * Kc[h]
    const float gh = gsp[(size_t)h * L];
    const size_t off0 = (size_t)h * dkd * L;
#pragma unroll
    for (int i = 0; i < DKR; ++i) {
      if (i < dkd) {
        const size_t off = off0 + (size_t)i * L;
        const float kv = kp[off], qv = qp[off];
        acc[i] += phi ? la_phi(kv) : kv;
        const float d = fmaf(gh, acc[i], dqp[off]);
        dqp[off] = phi ? d * la_dphi(qv) : d;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < DKR; ++i) acc[i] = 0.f;
  for (int h = heads - 1; h >= 0; --h) {  // dphi(k)[h] += sum_{h'' >= h} gs[h''] phi(q)[h'']
    const float gh = gsp[(size_t)h * L];
    const size_t off0 = (size_t)h * dkd * L;
#pragma unroll
    for (int i = 0; i < DKR; ++i) {
      if (i < dkd) {
        const size_t off = off0 + (size_t)i * L;
        const float kv = kp[off], qv = qp[off];
        acc[i] = fmaf(gh, phi ? la_phi(qv) : qv, acc[i]);
        const float d = dkp[off] + acc[i];
        dkp[off] = phi ? d * la_dphi(kv) : d;
      }
    }
  }
}

int la_nch(int L) { return (L + LA_T - 1) / LA_T; }

int la_check(const char* fn, int N, int heads, int L, int dk, int dv, int feature) {
  PG_REQUIRE(N >= 1 && heads >= 1 && L >= 1, PG_EINVAL, "%s: N, heads and L must be >= 1 (got %d, %d, %d)", fn, N,
             heads, L);
  PG_REQUIRE(feature == PG_FEATURE_IDENTITY || feature == PG_FEATURE_ELU1, PG_EINVAL, "%s: unknown feature id %d", fn,
             feature);
  PG_REQUIRE(dk >= 1 && dk <= LA_D && dv >= 1 && dv <= LA_D, PG_ESHAPE,
             "%s: head dims dk = %d, dv = %d outside [1, %d]", fn, dk, dv, LA_D);
  PG_REQUIRE((long)N * heads * la_nch(L) < (1L << 31) && (long)N * L * heads < (1L << 31), PG_ESHAPE,
             "%s: N * heads * L too large", fn);
  return 0;
}

size_t la_state_floats(int N, int heads, int L, int dk, int dv) {
  return la_nch(L) > 1 ? (size_t)N * heads * la_nch(L) * dk * dv : 0;
}

// the three launches of one scan; `name` for the error message
int la_scan(const LaScan& s, int NH, hipStream_t st, const char* name) {
  const int da = s.a.d, dc = s.c.d;
  if (s.nch > 1) {
    la_state_kernel<<<NH * s.nch, LA_THREADS, 0, st>>>(s);
    PG_LAUNCH_CHECK(name);
    const int sz = da * dc, bps = pg_cdiv(sz, LA_THREADS);
    la_prefix_kernel<<<NH * bps, LA_THREADS, 0, st>>>(s.ws, s.nch, sz, bps);
    PG_LAUNCH_CHECK(name);
  }
  la_out_kernel<<<NH * s.nch, LA_THREADS, 0, st>>>(s);
  PG_LAUNCH_CHECK(name);
  return 0;
}

LaOperand la_op(const float* p, const float* scale, long bs, int d, int phi) {
  LaOperand o;
  o.p = p;
  o.scale = scale;
  o.bs = bs;
  o.d = d;
  o.phi = phi;
  return o;
}

template <int DKR>
void la_den_launch(const float* q, const float* k, float* den, int N, int heads, int L, int dk, long qbs, long kbs,
                   int phi, hipStream_t st) {
  la_den_kernel<DKR><<<pg_cdiv((long)N * L, LA_THREADS), LA_THREADS, 0, st>>>(q, k, den, N, heads, L, dk, qbs, kbs, phi);
}

template <int DKR>
void la_den_bwd_launch(const float* q, const float* k, const float* gs, float* dq, float* dk, int N, int heads, int L,
                       int dkd, long qbs, long kbs, int phi, hipStream_t st) {
  la_den_bwd_kernel<DKR><<<pg_cdiv((long)N * L, LA_THREADS), LA_THREADS, 0, st>>>(q, k, gs, dq, dk, N, heads, L, dkd,
                                                                                   qbs, kbs, phi);
}

}  // namespace

PG_EXPORT size_t pg_linear_attn_workspace_floats(int N, int heads, int L, int dk, int dv, int backward) {
  if (N < 1 || heads < 1 || L < 1 || dk < 1 || dv < 1) return 0;
  return la_state_floats(N, heads, L, dk, dv) + (backward ? (size_t)N * heads * L : 0);
}

PG_EXPORT int pg_linear_attn_fwd(const float* q, const float* k, const float* v, float* out, float* den, float* ws,
                                 size_t ws_floats, int N, int heads, int L, int dk, int dv, long q_bs, long kv_bs,
                                 long o_bs, int feature, void* stream) {
  const int rc = la_check("pg_linear_attn_fwd", N, heads, L, dk, dv, feature);
  if (rc) return rc;
  PG_REQUIRE(q && k && v && out && den, PG_EINVAL, "pg_linear_attn_fwd: null pointer");
  const size_t need = pg_linear_attn_workspace_floats(N, heads, L, dk, dv, 0);
  PG_REQUIRE(ws_floats >= need && (need == 0 || ws), PG_EINVAL,
             "pg_linear_attn_fwd: workspace of %zu floats < %zu (pg_linear_attn_workspace_floats)", ws_floats, need);
  hipStream_t st = (hipStream_t)stream;
  const int phi = feature == PG_FEATURE_ELU1;
  if (dk <= 4)
    la_den_launch<4>(q, k, den, N, heads, L, dk, q_bs, kv_bs, phi, st);
  else if (dk <= 16)
    la_den_launch<16>(q, k, den, N, heads, L, dk, q_bs, kv_bs, phi, st);
  else
    la_den_launch<64>(q, k, den, N, heads, L, dk, q_bs, kv_bs, phi, st);
  PG_LAUNCH_CHECK("pg_linear_attn_fwd");
  LaScan s;
  s.a = la_op(q, nullptr, q_bs, dk, phi);
  s.b = la_op(k, nullptr, kv_bs, dk, phi);
  s.c = la_op(v, nullptr, kv_bs, dv, 0);
  s.out = out;
  s.oscale = den;
  s.ws = ws;
  s.obs = o_bs;
  s.heads = heads;
  s.L = L;
  s.nch = la_nch(L);
  s.reverse = 0;
  return la_scan(s, N * heads, st, "pg_linear_attn_fwd");
}

PG_EXPORT int pg_linear_attn_bwd(const float* q, const float* k, const float* v, const float* out, const float* den,
                                 const float* g, float* dq, float* dk, float* dv, float* ws, size_t ws_floats, int N,
                                 int heads, int L, int dkd, int dvd, long q_bs, long kv_bs, long o_bs, int feature,
                                 void* stream) {
  const int rc = la_check("pg_linear_attn_bwd", N, heads, L, dkd, dvd, feature);
  if (rc) return rc;
  PG_REQUIRE(q && k && v && out && den && g && dq && dk && dv && ws, PG_EINVAL, "pg_linear_attn_bwd: null pointer");
  const size_t need = pg_linear_attn_workspace_floats(N, heads, L, dkd, dvd, 1);
  PG_REQUIRE(ws_floats >= need, PG_EINVAL,
             "pg_linear_attn_bwd: workspace of %zu floats < %zu (pg_linear_attn_workspace_floats)", ws_floats, need);
  hipStream_t st = (hipStream_t)stream;
  const int phi = feature == PG_FEATURE_ELU1;
  const int NH = N * heads;
  float* gs = ws + la_state_floats(N, heads, L, dkd, dvd);
  la_gs_kernel<<<pg_cdiv((long)NH * L, LA_THREADS), LA_THREADS, 0, st>>>(g, out, den, gs, N, heads, L, dvd, o_bs);
  PG_LAUNCH_CHECK("pg_linear_attn_bwd");
  LaScan s;
  s.ws = ws;
  s.oscale = nullptr;
  s.heads = heads;
  s.L = L;
  s.nch = la_nch(L);
  // dphi(q)[l] = sum_{j <= l} (gn[l] . v[j]) phi(k)[j]
  s.a = la_op(g, den, o_bs, dvd, 0);
  s.b = la_op(v, nullptr, kv_bs, dvd, 0);
  s.c = la_op(k, nullptr, kv_bs, dkd, phi);
  s.out = dq;
  s.obs = q_bs;
  s.reverse = 0;
  int r = la_scan(s, NH, st, "pg_linear_attn_bwd");
  if (r) return r;
  // dphi(k)[j] = sum_{l >= j} (v[j] . gn[l]) phi(q)[l]
  s.a = la_op(v, nullptr, kv_bs, dvd, 0);
  s.b = la_op(g, den, o_bs, dvd, 0);
  s.c = la_op(q, nullptr, q_bs, dkd, phi);
  s.out = dk;
  s.obs = kv_bs;
  s.reverse = 1;
  r = la_scan(s, NH, st, "pg_linear_attn_bwd");
  if (r) return r;
  // dv[j] = sum_{l >= j} (phi(k)[j] . phi(q)[l]) gn[l]
  s.a = la_op(k, nullptr, kv_bs, dkd, phi);
  s.b = la_op(q, nullptr, q_bs, dkd, phi);
  s.c = la_op(g, den, o_bs, dvd, 0);
  s.out = dv;
  s.obs = kv_bs;
  s.reverse = 1;
  r = la_scan(s, NH, st, "pg_linear_attn_bwd");
  if (r) return r;
  if (dkd <= 4)
    la_den_bwd_launch<4>(q, k, gs, dq, dk, N, heads, L, dkd, q_bs, kv_bs, phi, st);
  else if (dkd <= 16)
    la_den_bwd_launch<16>(q, k, gs, dq, dk, N, heads, L, dkd, q_bs, kv_bs, phi, st);
  else
    la_den_bwd_launch<64>(q, k, gs, dq, dk, N, heads, L, dkd, q_bs, kv_bs, phi, st);
  PG_LAUNCH_CHECK("pg_linear_attn_bwd");
  return 0;
}
